"""GPU parity of ktup_train_transd_step (include/ktup_hip.h, csrc/ktup_transd_step.hip) through the C ABI against the reference's
goldens (tests/golden/transd.npz) and the fp64 reference of tests/_transd_step_ref.py (torch autograd on the CPU over the header's
closed forms, from the same fp32 inputs; its cases hold no knife edge, which tests/test_transd_step_ref_host.py checks on the CPU).

Bars (those of tests/test_hip_transd.py): loss slots rtol 1e-4 / atol 1e-5; gradients rtol 1e-4 with an atol of
max(3e-5, 2e-6 x the largest entry of the reference's gradient of that table).  The launch ADDS, so gradient buffers and loss slots
start non-zero; rows of a gradient that the step adds nothing to (tests/_transd_step_ref.py touched_rows) and the pitch gaps must
keep their pre-filled content bit for bit."""
import numpy as np
import pytest
import torch

from tests import _transd_step_ref as T
from tests import _train_step_ref as K

pytestmark = pytest.mark.gpu
DEV = 'cuda'
OK, INVALID, UNSUPPORTED = 0, -1, -3
LOSS0 = (0.25, 7.5, -0.5, 0.125)                 # the slots start non-zero: the launch accumulates
ZERO4 = (0.0, 0.0, 0.0, 0.0)


def lib():
    from jTransUP.hip import lib as L
    return L


def p(t):
    return None if t is None else t.data_ptr()


def prefill(c, zero=False, seed=5):
    """Gradient buffers with the tables' shapes (pitch gaps included), non-zero unless asked otherwise."""
    gen = torch.Generator().manual_seed(seed)
    return {k: (torch.zeros_like(c[k]) if zero else torch.randn(c[k].shape, generator=gen) * 0.1) for k in T.TABLES}


def to_device(c, pre, loss0=LOSS0):
    h2, t2, r2 = T.ids(c)
    dev = {k: c[k].to(DEV) for k in T.TABLES}
    dev.update({'g' + k: pre[k].to(DEV) for k in T.TABLES})
    dev.update(h=h2.to(DEV), t=t2.to(DEV), r=r2.to(DEV), loss=torch.tensor(loss0, dtype=torch.float32, device=DEV))
    return dev


def issue(c, dev, margin, gscale, regs, d=None, lde=None, E=None, gnorm=None, stream=None):
    return lib().load().ktup_train_transd_step(p(dev['E']) if E is None else E, c['lde'] if lde is None else lde, p(dev['R']), c['ldr'],
                                               p(dev['Ep']), c['ldep'], p(dev['Rp']), c['ldrp'], c['d'] if d is None else d, p(dev['h']),
                                               p(dev['t']), p(dev['r']), c['B'], int(c['l1']), float(margin), float(gscale), int(regs),
                                               p(dev['loss']), p(dev['gE']), p(dev['gR']), p(dev['gEp']), p(dev['gRp']), gnorm, stream)


def launch(c, margin, gscale, regs, pre, loss0=LOSS0, **kw):
    """-> (status, loss[4], {table: the gradient buffer afterwards}), everything back on the host."""
    dev = to_device(c, pre, loss0)
    rc = issue(c, dev, margin, gscale, regs, **kw)
    torch.cuda.synchronize()
    return rc, dev['loss'].cpu(), {k: dev['g' + k].cpu() for k in T.TABLES}


def check_grads(c, got, pre, want, touched=None, what=''):
    w = c['d']
    for name in T.TABLES:
        g, p0, ref = got[name], pre[name], torch.as_tensor(want[name]).double()
        total = p0[:, :w].double() + ref
        top = float(ref.abs().max())
        err = (g[:, :w].double() - total).abs()
        print('%s g%s: max |got - want| %.3g, max |want| %.3g' % (what, name, float(err.max()), top))
        assert bool((err <= max(3e-5, 2e-6 * top) + 1e-4 * total.abs()).all()), \
            '%s g%s: max error %.3g against a largest entry of %.3g' % (what, name, float(err.max()), top)
        assert torch.equal(g[:, w:], p0[:, w:]), 'g%s: something landed between the rows' % name
        if touched is not None:
            idle = ~touched[name]
            assert float(ref[idle].abs().max() if bool(idle.any()) else 0.0) == 0.0      # (the reference agrees that nothing lands there)
            assert torch.equal(g[idle], p0[idle]), 'g%s: a row that receives nothing was written' % name


def check_loss(loss, loss0, want, regs, what=''):
    print('%s loss got %s want %s' % (what, [float(x) - y for x, y in zip(loss, loss0)], want))
    np.testing.assert_allclose(loss.double().numpy() - np.asarray(loss0), np.asarray(want), rtol=1e-4, atol=1e-5, err_msg='loss slots')
    assert float(loss[1]) == loss0[1], 'slot 1 is never written'
    for slot, bit in ((2, 2), (3, 4)):
        if not regs & bit:
            assert float(loss[slot]) == np.float32(loss0[slot]), 'slot %d with its regulariser off' % slot


def check(key, c, margin, gscale, regs, zero=False, what=''):
    want_loss, want, touched = T.reference_of(key, c, margin, gscale, regs)
    pre = prefill(c, zero)
    rc, loss, got = launch(c, margin, gscale, regs, pre)
    assert rc == OK, lib().load().ktup_last_error()
    check_loss(loss, LOSS0, want_loss, regs, what)
    check_grads(c, got, pre, want, touched, what)
    return got


# ------------------------------------------------------------------------------------------------ goldens
@pytest.mark.parametrize('l1', [True, False])
@pytest.mark.parametrize('d', [36, 64, 100])
def test_goldens_from_zeroed_buffers(d, l1):
    c, want = T.golden_case(d, l1)
    pre = prefill(c, zero=True)
    rc, loss, got = launch(c, 1.0, 1.0, 6, pre, loss0=ZERO4)
    assert rc == OK, lib().load().ktup_last_error()
    total = float(loss[0]) + float(loss[2]) + float(loss[3])
    print('loss %.6g golden %.6g' % (total, want['loss']))
    np.testing.assert_allclose(total, want['loss'], rtol=1e-4, atol=1e-5)
    assert float(loss[1]) == 0.0
    check_grads(c, got, pre, want['grad'], T.touched_rows(c, 1.0, 6), 'golden d=%d' % d)


# ------------------------------------------------------------------------------------------------ the grid
@pytest.mark.parametrize('spec', T.grid_specs(), ids=T.spec_id)
def test_grid_matches_the_fp64_reference(spec):
    check(T.spec_id(spec), T.spec_case(spec), 1.0, spec['gscale'], spec['regs'])


@pytest.mark.parametrize('l1', [0, 1])
@pytest.mark.parametrize('d', [36, 100, 256])
def test_a_batch_without_an_active_example(d, l1):
    """Slot 0 keeps its value, only the regularisers' rows are touched, gEp and gRp not at all."""
    c = T.inactive_case(d, l1)
    key = 'inactive-%d-%d' % (d, l1)
    for regs in (6, 0):
        want_loss, want, touched = T.reference_of(key, c, T.INACTIVE_MARGIN, 1.0, regs)
        assert want_loss[0] == 0.0 and not bool(touched['Ep'].any()) and not bool(touched['Rp'].any())
        assert bool(touched['E'].any()) == (regs == 6) and bool(touched['R'].any()) == (regs == 6)
        pre = prefill(c)
        rc, loss, got = launch(c, T.INACTIVE_MARGIN, 1.0, regs, pre)
        assert rc == OK
        assert float(loss[0]) == np.float32(LOSS0[0])
        check_loss(loss, LOSS0, want_loss, regs)
        check_grads(c, got, pre, want, touched)
        assert torch.equal(got['Ep'], pre['Ep']) and torch.equal(got['Rp'], pre['Rp'])
        if regs == 0:
            assert all(torch.equal(got[k], pre[k]) for k in got) and torch.equal(loss, torch.tensor(LOSS0))


@pytest.mark.parametrize('l1', [0, 1])
@pytest.mark.parametrize('d', [36, 100, 256])
def test_a_batch_of_active_examples(d, l1):
    c = T.active_case(d, l1)
    check('active-%d-%d' % (d, l1), c, T.ACTIVE_MARGIN, 0.5, 6)


@pytest.mark.parametrize('l1', [0, 1])
@pytest.mark.parametrize('d', [36, 100, 256])
def test_examples_whose_twin_names_another_relation(d, l1):
    c = T.stray_case(d, l1)
    assert int((c['nr'] != c['r']).sum()) == 6
    check('stray-%d-%d' % (d, l1), c, 1.0, 0.5, 6)
    check('stray-%d-%d' % (d, l1), c, 1.0, 1.0, 0, zero=True)


@pytest.mark.parametrize('l1', [0, 1])
@pytest.mark.parametrize('d', [36, 100, 256])
def test_zero_projection_tables_make_the_step_transe(d, l1):
    """gEp and gRp receive exact zeros; gE and gR are what ktup_train_kg_step(transh = 0) gives on the same ids, within the bars."""
    c = T.zero_proj_case(d, l1)
    pre = prefill(c)
    rc, loss, got = launch(c, 1.0, 1.0, 6, pre)
    assert rc == OK
    assert torch.equal(got['Ep'], pre['Ep']) and torch.equal(got['Rp'], pre['Rp'])
    zero = prefill(c, zero=True)
    rc, loss_z, got_z = launch(c, 1.0, 1.0, 6, zero, loss0=ZERO4)
    assert rc == OK and float(got_z['Ep'].abs().max()) == 0.0 and float(got_z['Rp'].abs().max()) == 0.0
    dev = to_device(c, zero, ZERO4)
    rc = lib().load().ktup_train_kg_step(0, p(dev['E']), c['lde'], p(dev['R']), c['ldr'], None, 0, d, p(dev['h']), p(dev['t']), p(dev['r']),
                                         c['B'], int(c['l1']), 1.0, 1.0, 6, p(dev['loss']), p(dev['gE']), p(dev['gR']), None, None, None)
    torch.cuda.synchronize()
    assert rc == OK, lib().load().ktup_last_error()
    np.testing.assert_allclose(loss_z.numpy(), dev['loss'].cpu().numpy(), rtol=1e-4, atol=1e-5)
    for k in ('E', 'R'):
        want = dev['g' + k].cpu().double()
        top = float(want.abs().max())
        err = (got_z[k].double() - want).abs()
        assert bool((err <= max(3e-5, 2e-6 * top) + 1e-4 * want.abs()).all()), 'g%s differs from the TransE step by %.3g' % (k, float(err.max()))
    check('zero-%d-%d' % (d, l1), c, 1.0, 1.0, 6)


# ------------------------------------------------------------------------------------------------ refused calls
def test_refused_calls_return_their_codes_and_touch_nothing():
    c = T.case(64, 20, 0, 3, pitch=(4, 4, 4, 4))
    pre = prefill(c)

    def refused(code, regs=6, **kw):
        rc, loss, got = launch(c, 1.0, 1.0, regs, pre, **kw)
        assert rc == code, (rc, kw)
        assert torch.equal(loss, torch.tensor(LOSS0)) and all(torch.equal(got[k], pre[k]) for k in got), kw

    refused(INVALID, regs=7)
    refused(INVALID, regs=1)
    refused(INVALID, regs=8)
    refused(UNSUPPORTED, d=50)
    refused(UNSUPPORTED, d=260)
    refused(UNSUPPORTED, lde=c['lde'] + 2)                              # a pitch of d + 2: no multiple of 4 floats
    dev = to_device(c, pre)
    refused(UNSUPPORTED, E=p(dev['E']) + 4)                             # a table offset by 4 bytes
    assert 'ktup_train_transd_step' in str(lib().load().ktup_last_error())
    rc, _, _ = launch(c, 1.0, 1.0, 6, pre)
    assert rc == OK


# ------------------------------------------------------------------------------------------------ the tracked norm
@pytest.mark.parametrize('l1', [0, 1])
@pytest.mark.parametrize('d', [36, 100])
def test_tracked_norm_is_the_norm_pass(d, l1):
    """Buffers start from zero and `gnorm` is given: ktup_optim_clip_step with the workspace (no norm pass) and with its own norm pass
    over the same step's gradients see the same norm and leave the same tables, to 2e-5 relative (plus an ulp of an entry of size 1:
    the two launches' atomics land in different orders)."""
    from jTransUP.utils.fused_optim import FusedOptimizer
    c = T.case(d, 67, l1, 300 + d + l1)
    h2, t2, r2 = (x.to(DEV) for x in T.ids(c))
    MAXN = 0.05
    out = []
    for tracked in (True, False):
        params = [torch.nn.Parameter(c[k].clone().to(DEV)) for k in T.TABLES]
        for q in params:
            q.grad = torch.zeros_like(q)
        opt = FusedOptimizer(torch.optim.SGD(params, lr=0.05))
        ws = torch.zeros(64, dtype=torch.float64, device=DEV) if tracked else None
        loss = torch.zeros(4, device=DEV)
        E, R, Ep, Rp = params
        rc = lib().load().ktup_train_transd_step(p(E), d, p(R), d, p(Ep), d, p(Rp), d, d, p(h2), p(t2), p(r2), c['B'], l1, 1.0, 1.0, 6, p(loss),
                                                 p(E.grad), p(R.grad), p(Ep.grad), p(Rp.grad), p(ws), None)
        assert rc == OK, lib().load().ktup_last_error()
        torch.cuda.synchronize()
        direct = float(torch.sqrt(sum((q.grad.double() ** 2).sum() for q in params)))
        opt.clip_and_step(MAXN, zero_grads=True, gnorm=p(ws))
        torch.cuda.synchronize()
        out.append((opt.total_norm(), direct, [q.detach().cpu() for q in params]))
        assert all(float(q.grad.abs().max()) == 0.0 for q in params)
        if tracked:
            assert int(ws[:1].view(torch.int64).item()) == 1            # the workspace counted the step
    (n1, d1, t1), (n2, d2, t2_) = out
    print('norm tracked %.8g, norm pass %.8g, fp64 of the buffers %.8g / %.8g' % (n1, n2, d1, d2))
    assert n2 > MAXN, 'the step was not clipped: the test would not see a wrong norm'
    assert abs(n1 - n2) <= 2e-5 * n2 and abs(n1 - d1) <= 2e-5 * d1
    for a, b, k in zip(t1, t2_, T.TABLES):
        assert bool(((a - b).abs() <= 2e-5 * b.abs() + 1.2e-7).all()), k
        assert not torch.equal(b, c[k]), k + ': the step moved nothing'


# ------------------------------------------------------------------------------------------------ graph capture
@pytest.mark.parametrize('l1', [0, 1])
@pytest.mark.parametrize('d', [36, 100, 256])
def test_the_launch_replays_from_a_graph_with_new_ids(d, l1):
    """Captured once, replayed five times, the ids changed in place between replays: every replay equals the reference for its ids."""
    L = lib()
    cases = [T.case(d, 67, l1, 900 + 10 * d + l1, pitch=(4, 4, 4, 4))]
    for k in range(1, 5):                                               # the same tables, other batches
        nxt = T.case(d, 67, l1, 900 + 10 * d + l1, pitch=(4, 4, 4, 4))
        gen = torch.Generator().manual_seed(k)
        for attempt in range(K.MAX_DRAWS):
            nxt['r'] = torch.randint(0, nxt['n_rel'], (67,), generator=gen)
            nxt['nr'] = nxt['r'].clone()
            T._draw_entities(nxt, torch.arange(67), gen)
            for _ in range(K.MAX_DRAWS):
                bad, _, _ = T._state(nxt, (1.0,))
                if not bool(bad.any()):
                    break
                T._draw_entities(nxt, bad.nonzero().flatten(), gen)
            if T.conditions(nxt, (1.0,)) is None:
                break
        assert T.conditions(nxt, (1.0,)) is None
        assert all(torch.equal(nxt[t], cases[0][t]) for t in T.TABLES)
        cases.append(nxt)
    c = cases[0]
    zero = prefill(c, zero=True)
    dev = to_device(c, zero, ZERO4)
    graph = torch.cuda.CUDAGraph()
    with L.capture(graph):
        rc = issue(c, dev, 1.0, 1.0, 6, stream=torch.cuda.current_stream().cuda_stream)
    assert rc == OK
    torch.cuda.synchronize()
    for replay, cc in enumerate(cases):
        h2, t2, r2 = T.ids(cc)
        dev['h'].copy_(h2); dev['t'].copy_(t2); dev['r'].copy_(r2)      # in place: the graph keeps its pointers
        for k in ('gE', 'gR', 'gEp', 'gRp', 'loss'):
            dev[k].zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        want_loss, want = T.reference(cc, 1.0, 1.0, 6)
        check_loss(dev['loss'].cpu(), ZERO4, want_loss, 6, 'replay %d' % replay)
        check_grads(cc, {k: dev['g' + k].cpu() for k in T.TABLES}, zero, want, T.touched_rows(cc, 1.0, 6), 'replay %d' % replay)


# ------------------------------------------------------------------------------------------------ option `deterministic`
@pytest.mark.parametrize('l1', [0, 1])
@pytest.mark.parametrize('d', [36, 100, 256])
def test_deterministic_option_gives_the_same_bits_twice(d, l1):
    L = lib()
    spec = dict(d=d, l1=l1, B=67, pitch=(4, 4, 4, 4), regs=6, gscale=1.0, seed=700 + d + l1)
    c = T.spec_case(spec)
    old = L.set_option('deterministic', 1)
    try:
        assert L.load().ktup_train_transd_step_supported(d) == 1          # not refused
        a = check(T.spec_id(spec), c, 1.0, 1.0, 6)
        b = check(T.spec_id(spec), c, 1.0, 1.0, 6)
        pre = prefill(c)
        _, la, _ = launch(c, 1.0, 1.0, 6, pre)
        _, lb, _ = launch(c, 1.0, 1.0, 6, pre)
    finally:
        L.set_option('deterministic', old)
    assert all(torch.equal(a[k], b[k]) for k in T.TABLES) and torch.equal(la, lb)
