"""GPU parity of ktup_train_transr_step (include/ktup_hip.h, csrc/ktup_transr_step.hip) through the C ABI against the fp64 reference
of tests/_transr_step_ref.py (torch autograd on the CPU of oracle.cpu_ref.score_transr, margin_loss and norm_loss, from the same
fp32 inputs; its cases hold no knife edge, which tests/test_transr_step_ref_host.py checks on the CPU).

Bars (the project's TransR bars, tests/test_hip_score.py and DESIGN.md section 4): loss slots rtol 1e-4 / atol 1e-5; gradients rtol
1e-4 with an atol of 2e-4 of the largest entry of the reference's gradient of that table.  Rows of a gradient that the step adds
nothing to (tests/_transr_step_ref.py touched_rows: entities of no active example and of no regularised row, relations without an
active example, unused relations) and the pitch gaps must keep their pre-filled content bit for bit: the launch ADDS and skips what
receives nothing."""
import numpy as np
import pytest
import torch

from tests import _transr_step_ref as T

pytestmark = pytest.mark.gpu
DEV = 'cuda'
OK, INVALID, UNSUPPORTED = 0, -1, -3
LOSS0 = (0.25, 7.5, -0.5, 0.125)                 # the slots start non-zero: the launch accumulates


def lib():
    from jTransUP.hip import lib as L
    return L


def p(t):
    return None if t is None else t.data_ptr()


def prefill(c, zero=False, seed=5):
    """Gradient buffers with the tables' shapes (pitch gaps included), non-zero unless asked otherwise."""
    gen = torch.Generator().manual_seed(seed)
    return {k: (torch.zeros_like(c[k]) if zero else torch.randn(c[k].shape, generator=gen) * 0.1) for k in ('E', 'R', 'M')}


def launch(c, margin, gscale, regs, nsplit, pre, loss0=LOSS0, B=None, d=None, lde=None, stream=None, dev=None):
    """-> (status, loss[4], {'E','R','M'}: the gradient buffers afterwards), everything back on the host."""
    L = lib()
    if dev is None:
        dev = to_device(c, pre, loss0)
    rc = L.load().ktup_train_transr_step(p(dev['E']), c['lde'] if lde is None else lde, p(dev['R']), c['ldr'], p(dev['M']), c['ldm'], c['n_rel'],
                                         c['d'] if d is None else d, p(dev['h']), p(dev['t']), p(dev['r']), c['B'] if B is None else B,
                                         int(c['l1']), float(margin), float(gscale), int(regs), int(nsplit), p(dev['loss']), p(dev['gE']),
                                         p(dev['gR']), p(dev['gM']), stream)
    torch.cuda.synchronize()
    return rc, dev['loss'].cpu(), {k: dev['g' + k].cpu() for k in ('E', 'R', 'M')}


def to_device(c, pre, loss0=LOSS0):
    h2, t2, r2 = T.ids(c)
    dev = {k: c[k].to(DEV) for k in ('E', 'R', 'M')}
    dev.update({'g' + k: pre[k].to(DEV) for k in ('E', 'R', 'M')})
    dev.update(h=h2.to(DEV), t=t2.to(DEV), r=r2.to(DEV), loss=torch.tensor(loss0, dtype=torch.float32, device=DEV))
    return dev


def widths(c):
    return {'E': c['d'], 'R': c['d'], 'M': c['d'] * c['d']}


def check_grads(c, got, pre, want, touched, what=''):
    for name, w in widths(c).items():
        g, p0, ref = got[name], pre[name], want[name]
        total = p0[:, :w].double() + ref
        top = float(ref.abs().max())
        err = (g[:, :w].double() - total).abs()
        print('%s g%s: max |got - want| %.3g, max |want| %.3g' % (what, name, float(err.max()), top))
        assert bool((err <= 2e-4 * top + 1e-4 * total.abs()).all()), '%s g%s: max error %.3g against a largest entry of %.3g' % (what, name, float(err.max()), top)
        assert torch.equal(g[:, w:], p0[:, w:]), 'g%s: something landed between the rows' % name
        idle = ~touched[name]
        assert float(ref[idle].abs().max() if bool(idle.any()) else 0.0) == 0.0      # (the reference agrees that nothing lands there)
        assert torch.equal(g[idle], p0[idle]), 'g%s: a row that receives nothing was written' % name


def check(c, margin, gscale, regs, nsplit, zero=False, what=''):
    want_loss, want = T.reference(c, margin, gscale, regs)
    pre = prefill(c, zero)
    rc, loss, got = launch(c, margin, gscale, regs, nsplit, pre)
    assert rc == OK, lib().load().ktup_last_error()
    print('%s loss got %s want %s' % (what, [float(x) - y for x, y in zip(loss, LOSS0)], want_loss))
    np.testing.assert_allclose(loss.double().numpy() - np.asarray(LOSS0), np.asarray(want_loss), rtol=1e-4, atol=1e-5, err_msg='loss slots')
    assert float(loss[1]) == LOSS0[1], 'slot 1 belongs to TransH'
    for slot, bit in ((2, 2), (3, 4)):
        if not regs & bit:
            assert float(loss[slot]) == np.float32(LOSS0[slot]), 'slot %d with its regulariser off' % slot
    check_grads(c, got, pre, want, T.touched_rows(c, margin, regs), what)
    # the rows the header names: entities of no example, projection rows of relations without an example
    h2, t2, r2 = T.ids(c)
    used_e = torch.zeros(c['ne'], dtype=torch.bool); used_e[h2] = True; used_e[t2] = True
    used_r = torch.zeros(c['n_rel'], dtype=torch.bool); used_r[r2] = True
    assert torch.equal(got['E'][~used_e], pre['E'][~used_e]) and torch.equal(got['M'][~used_r], pre['M'][~used_r])
    assert torch.equal(got['R'][~used_r], pre['R'][~used_r])
    return got


@pytest.mark.parametrize('spec', T.grid_specs(), ids=T.spec_id)
def test_grid_matches_the_fp64_reference(spec):
    check(T.spec_case(spec), 1.0, spec['gscale'], spec['regs'], spec['nsplit'])


@pytest.mark.parametrize('spec', T.edge_specs(), ids=T.spec_id)
def test_tile_edges_and_a_dominant_relation(spec):
    c = T.spec_case(spec)
    counts = torch.bincount(c['r'], minlength=c['n_rel'])
    if spec['kind'] == 'edge':
        assert 16 in counts.tolist() and (17 in counts.tolist() or c['B'] == 33 and int(counts[0]) == 17)
    else:
        assert int(counts.max()) > c['B'] // 2
    check(c, 1.0, spec['gscale'], spec['regs'], spec['nsplit'])


@pytest.mark.parametrize('nsplit', [0, 3])
@pytest.mark.parametrize('l1', [0, 1])
@pytest.mark.parametrize('d', [64, 100, 128])
def test_examples_whose_twin_names_another_relation(d, l1, nsplit):
    c = T.stray_case(d, l1)
    assert int((c['nr'] != c['r']).sum()) == 3
    check(c, 1.0, 0.37, 6, nsplit)
    check(c, 1.0, 1.0, 0, nsplit, zero=True)


@pytest.mark.parametrize('l1', [0, 1])
@pytest.mark.parametrize('d', [64, 100, 128])
def test_a_batch_without_an_active_example_adds_exact_zeros(d, l1):
    c = T.inactive_case(d, l1)
    want_loss, want = T.reference(c, T.INACTIVE_MARGIN, 1.0, 0)
    assert want_loss[0] == 0.0 and all(float(g.abs().max()) == 0.0 for g in want.values())
    rc, loss, got = launch(c, T.INACTIVE_MARGIN, 1.0, 0, 0, prefill(c, zero=True), loss0=(0.0, 0.0, 0.0, 0.0))
    assert rc == OK
    assert float(loss.abs().max()) == 0.0
    for name, g in got.items():
        assert float(g.abs().max()) == 0.0, 'g' + name
    pre = prefill(c)                                                    # and onto non-zero buffers: nothing moves
    rc, loss, got = launch(c, T.INACTIVE_MARGIN, 1.0, 0, 3, pre)
    assert rc == OK and all(torch.equal(got[k], pre[k]) for k in got) and torch.equal(loss, torch.tensor(LOSS0))


def test_supported_widths():
    L = lib().load()
    assert [d for d in (20, 36, 50, 64, 100, 128, 256) if L.ktup_train_transr_step_supported(d)] == [64, 100, 128]


def test_refused_calls_return_their_codes_and_touch_nothing():
    L = lib()
    c = T.case(64, 20, 4, 0, 3, pitch=(4, 4, 4))
    pre = prefill(c)

    def refused(code, **kw):
        regs = kw.pop('regs', 6)
        rc, loss, got = launch(c, 1.0, 1.0, regs, 0, pre, **kw)
        assert rc == code, (rc, kw)
        assert torch.equal(loss, torch.tensor(LOSS0)) and all(torch.equal(got[k], pre[k]) for k in got), kw

    refused(INVALID, regs=7)
    refused(INVALID, regs=1)
    refused(UNSUPPORTED, B=0)
    refused(UNSUPPORTED, B=4097)
    refused(UNSUPPORTED, d=36)
    refused(UNSUPPORTED, lde=c['lde'] + 2)                              # a pitch that is no multiple of 4 floats
    old = L.set_option('deterministic', 1)
    try:
        assert L.load().ktup_train_transr_step_supported(64) == 0
        refused(UNSUPPORTED)
    finally:
        L.set_option('deterministic', old)
    assert L.load().ktup_train_transr_step_supported(64) == 1
    rc, _, _ = launch(c, 1.0, 1.0, 6, 0, pre)
    assert rc == OK


@pytest.mark.parametrize('l1', [0, 1])
@pytest.mark.parametrize('d', [64, 100, 128])
def test_the_launch_replays_from_a_graph(d, l1):
    """The hazard of the bucketed route was "from the second replay on": five replays onto freshly zeroed buffers, each equal to
    the eager result within the gradient bar (float atomics land in another order) and to the reference."""
    L = lib()
    spec = dict(d=d, l1=l1, B=67, n_rel=7, kind='random', nsplit=0, pitch=(4, 4, 4), regs=6, gscale=1.0, seed=900 + d + l1)
    c = T.spec_case(spec)
    want_loss, want = T.reference(c, 1.0, 1.0, 6)
    zero = prefill(c, zero=True)
    rc, eager_loss, eager = launch(c, 1.0, 1.0, 6, 0, zero, loss0=(0.0,) * 4)
    assert rc == OK
    dev = to_device(c, zero, (0.0,) * 4)
    graph = torch.cuda.CUDAGraph()
    with L.capture(graph):
        rc = L.load().ktup_train_transr_step(p(dev['E']), c['lde'], p(dev['R']), c['ldr'], p(dev['M']), c['ldm'], c['n_rel'], d, p(dev['h']),
                                             p(dev['t']), p(dev['r']), c['B'], int(c['l1']), 1.0, 1.0, 6, 0, p(dev['loss']), p(dev['gE']),
                                             p(dev['gR']), p(dev['gM']), torch.cuda.current_stream().cuda_stream)
    assert rc == OK
    torch.cuda.synchronize()
    for replay in range(5):
        for k in ('gE', 'gR', 'gM', 'loss'):
            dev[k].zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        got = {k: dev['g' + k].cpu() for k in ('E', 'R', 'M')}
        np.testing.assert_allclose(dev['loss'].cpu().double().numpy(), np.asarray(want_loss), rtol=1e-4, atol=1e-5, err_msg='replay %d' % replay)
        check_grads(c, got, zero, want, T.touched_rows(c, 1.0, 6), 'replay %d' % replay)
        for name, w in widths(c).items():
            top = float(want[name].abs().max())
            err = (got[name].double() - eager[name].double()).abs()
            assert bool((err <= 2e-4 * top + 1e-4 * eager[name].double().abs()).all()), 'replay %d differs from the eager launch in g%s' % (replay, name)

