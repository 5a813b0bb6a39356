"""GPU parity of ktup_train_cfkg_rec_step (include/ktup_hip.h) through the C ABI: against the vectors the imported reference
produced (tests/golden/baselines.npz, d{36,64}.cfkg.{L1,L2}.rec.*), and against oracle.cpu_ref.score_cfkg_rec + bpr_loss
differentiated in fp64 on the CPU from the same fp32 inputs.  The oracle's tables are small so that rows collide: 7 users, 11
entities.

Tolerances are those tests/test_hip_baselines.py::test_cfkg_golden uses for the multi-launch route: loss rtol 1e-4 / atol 1e-5,
gradients rtol 2e-4 / atol 3e-5."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NU, NE, NR = 7, 11, 5
L1_MARGIN = 1e-5        # under L1 every coordinate of every z is at least this far from zero (asserted in fp64): no sign is in doubt
# make_case seeds per (B, d), picked on the CPU with the oracle so that the L1 margin holds (they serve the other pitches and the
# larger relation table of the smaller tests too: `check` asserts the margin for every case it runs)
SEEDS = {(1, 20): 120, (1, 36): 136, (1, 50): 150, (1, 100): 200, (1, 256): 356,
         (63, 20): 6320, (63, 36): 6336, (63, 50): 6350, (63, 100): 6400, (63, 256): 6556,
         (64, 20): 6420, (64, 36): 6436, (64, 50): 6450, (64, 100): 6500, (64, 256): 6656,
         (257, 20): 25720, (257, 36): 25736, (257, 50): 25750, (257, 100): 25801, (257, 256): 25956}


def lib():
    from jTransUP.hip import lib as L
    return L


def p(t):
    return None if t is None else t.data_ptr()


def close(got, want, rtol, atol, what):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = want.detach().cpu().numpy() if isinstance(want, torch.Tensor) else np.asarray(want)
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol, err_msg=what)


def make_case(B, d, seed, pitch_extra=4, n_rel=NR):
    """fp32 tables with pitch d + pitch_extra (the gap holds garbage the kernel must not read into a sum), ids with collisions, and
    one example whose positive and negative item are the same row."""
    gen = torch.Generator().manual_seed(seed)
    ld = d + pitch_extra
    c = {'d': d, 'B': B, 'ld': ld}
    for name, rows in (('U', NU), ('E', NE), ('R', n_rel)):
        c[name] = torch.randn(rows, ld, generator=gen) * 0.4
    c['u'] = torch.randint(0, NU, (B,), generator=gen)
    c['pi'] = torch.randint(0, NE, (B,), generator=gen)
    c['ni'] = torch.randint(0, NE, (B,), generator=gen)
    if B > 1:
        c['ni'][B // 2] = c['pi'][B // 2]                           # pos == neg: the two entity-row adds cancel up to rounding
    for name, rows in (('gU', NU), ('gE', NE), ('gR', n_rel)):      # the launch ADDS: buffers start non-zero
        c[name] = torch.randn(rows, ld, generator=gen) * 0.1
    c['loss0'] = 0.25
    return c


def l1_margin(c, rel):
    """min |z| over every coordinate of every z+- of the case, in fp64."""
    d = c['d']
    U, E, R = (c[k].double()[:, :d] for k in ('U', 'E', 'R'))
    q = U[c['u']] + R[rel]
    return float(torch.minimum((q - E[c['pi']]).abs().min(), (q - E[c['ni']]).abs().min()))


def reference(c, l1, target, up, rel=None):
    """fp64 on the CPU: (loss, gU, gE, gR) of up * bpr_loss(score(pos), score(neg), target), the oracle differentiated by autograd.
    The oracle's buy relation is the LAST row of the table it is given: for another `rel` it gets the rows up to it."""
    from oracle import cpu_ref
    d = c['d']
    leaves = {k: c[k].double().clone().requires_grad_(True) for k in ('U', 'E', 'R')}
    U, E, R = (leaves[k][:, :d] for k in ('U', 'E', 'R'))
    if rel is not None:
        R = R[:rel + 1]
    pos = cpu_ref.score_cfkg_rec(U, E, R, c['u'], c['pi'], l1)
    neg = cpu_ref.score_cfkg_rec(U, E, R, c['u'], c['ni'], l1)
    loss = up * cpu_ref.bpr_loss(pos, neg, target)
    loss.backward()
    return float(loss.detach()), leaves['U'].grad, leaves['E'].grad, leaves['R'].grad


def launch(c, l1, target, up, rel):
    L = lib()
    dev = {k: c[k].to(DEV) for k in ('U', 'E', 'R', 'gU', 'gE', 'gR')}
    u2 = torch.cat([c['u'], c['u']]).to(DEV)
    i2 = torch.cat([c['pi'], c['ni']]).to(DEV)
    loss = torch.full((1,), c['loss0'], device=DEV)
    ld = c['ld']
    L.call('ktup_train_cfkg_rec_step', p(dev['U']), ld, p(dev['E']), ld, p(dev['R']), ld, rel, c['d'], p(u2), p(i2), c['B'], int(l1),
           float(target), float(up), p(loss), p(dev['gU']), p(dev['gE']), p(dev['gR']), None)
    torch.cuda.synchronize()
    return float(loss.item()), dev['gU'].cpu(), dev['gE'].cpu(), dev['gR'].cpu()


def check(c, l1, target, up, rel=None):
    n_rel = c['R'].shape[0]
    r = n_rel - 1 if rel is None else rel
    if l1:
        m = l1_margin(c, r)
        print('L1: min |z| = %.3g' % m)
        assert m >= L1_MARGIN, 'pick another seed: a coordinate of z is %.3g from zero' % m
    want_loss, wU, wE, wR = reference(c, l1, target, up, rel)
    got_loss, gU, gE, gR = launch(c, l1, target, up, r)
    print('loss got %.9g want %.9g' % (got_loss - c['loss0'], want_loss))
    close(got_loss, c['loss0'] + want_loss, 1e-4, 1e-5, 'loss')
    d = c['d']
    for name, got, want in (('gU', gU, wU), ('gE', gE, wE), ('gR', gR, wR)):
        total = c[name].double() + want
        print('%s: max |got - want| %.3g, max |want| %.3g' % (name, float((got.double() - total).abs().max()), float(want.abs().max())))
        close(got, total.float(), 2e-4, 3e-5, name)                # every element: nothing is exempt
        assert torch.equal(got[:, d:], c[name][:, d:]), name + ': something landed between the rows'
    others = [k for k in range(n_rel) if k != r]
    assert torch.equal(gR[others], c['gR'][others]), 'a relation row other than `rel` was written'
    assert float((gR[r, :d] - c['gR'][r, :d]).abs().max()) > 0.0


@pytest.mark.parametrize('target', [1.0, -1.0])
@pytest.mark.parametrize('l1', [True, False])
@pytest.mark.parametrize('d', [20, 36, 50, 100, 256])
@pytest.mark.parametrize('B', [1, 63, 64, 257])
def test_cfkg_step_against_the_oracle(B, d, l1, target):
    """B below one workgroup's four examples, one short of and exactly 16 workgroups, and 65 workgroups with a tail; d = 50 takes the
    element-wise path, the others float4 rows with a gap between them (pitch d + 4)."""
    check(make_case(B, d, SEEDS[(B, d)]), l1, target, 0.5)


@pytest.mark.parametrize('l1', [True, False])
def test_cfkg_step_pitches(l1):
    """Pitch d (no gap), and d + 1 (rows lose their 16-byte alignment: element-wise loads at a width that is a multiple of four)."""
    check(make_case(63, 36, SEEDS[(63, 36)], pitch_extra=0), l1, -1.0, 0.5)
    check(make_case(63, 36, SEEDS[(63, 36)], pitch_extra=1), l1, -1.0, 0.5)


@pytest.mark.parametrize('l1', [True, False])
def test_cfkg_step_writes_the_given_relation_row_only(l1):
    """rel in the middle of a larger table: that row takes the gradient, no other row of gR changes (checked exactly)."""
    check(make_case(64, 36, SEEDS[(64, 36)], n_rel=9), l1, -1.0, 0.5, rel=3)


@pytest.mark.parametrize('l1', [True, False])
def test_cfkg_step_large_batch_walks_several_examples_per_wave(l1):
    """More examples than the launch has waves (256 workgroups x 4): every wave sums several examples' relation gradients."""
    check(make_case(1500, 36, 150036), l1, -1.0, 1.0)


@pytest.mark.parametrize('d', [36, 64])
@pytest.mark.parametrize('l1', [False, True])
def test_cfkg_step_golden(golden, d, l1):
    """One launch on zeroed gradients reproduces the reference's loss and its three gradients (target = -1)."""
    L = lib()
    g = golden('baselines')
    pre = 'd%d.' % d
    tag = pre + 'cfkg.%s.' % ('L1' if l1 else 'L2')
    U, E, R = (torch.from_numpy(g[pre + 'cfkg.' + k]).to(DEV).contiguous()
               for k in ('user_embeddings.weight', 'ent_embeddings.weight', 'rel_embeddings.weight'))
    u, pi, ni = (torch.from_numpy(g[pre + k]).long().to(DEV) for k in ('u', 'pi', 'ni'))
    B = u.numel()
    u2, i2 = torch.cat([u, u]), torch.cat([pi, ni])
    loss = torch.zeros(1, device=DEV)
    gU, gE, gR = torch.zeros_like(U), torch.zeros_like(E), torch.zeros_like(R)
    L.call('ktup_train_cfkg_rec_step', p(U), d, p(E), d, p(R), d, R.shape[0] - 1, d, p(u2), p(i2), B, int(l1), -1.0, 1.0, p(loss), p(gU),
           p(gE), p(gR), None)
    torch.cuda.synchronize()
    print('loss got %.9g want %.9g' % (float(loss.item()), float(g[tag + 'rec.loss'])))
    close(loss[0], g[tag + 'rec.loss'], 1e-4, 1e-5, 'loss')
    for name, got in (('user_embeddings.weight', gU), ('ent_embeddings.weight', gE), ('rel_embeddings.weight', gR)):
        close(got, g[tag + 'rec.grad.' + name], 2e-4, 3e-5, name)


def test_the_option_deterministic_declines():
    L = lib()
    c = make_case(5, 36, 1)
    dev = {k: c[k].to(DEV) for k in ('U', 'E', 'R', 'gU', 'gE', 'gR')}
    ids = torch.zeros(10, dtype=torch.int64, device=DEV)
    loss = torch.zeros(1, device=DEV)
    before = dev['gU'].clone()
    old = L.set_option('deterministic', 1)
    try:
        with pytest.raises(L.KtupError) as e:
            L.call('ktup_train_cfkg_rec_step', p(dev['U']), c['ld'], p(dev['E']), c['ld'], p(dev['R']), c['ld'], NR - 1, 36, p(ids), p(ids), 5, 1,
                   -1.0, 1.0, p(loss), p(dev['gU']), p(dev['gE']), p(dev['gR']), None)
        assert e.value.code == L.ERR_UNSUPPORTED
    finally:
        L.set_option('deterministic', old)
    torch.cuda.synchronize()
    assert float(loss.item()) == 0.0 and torch.equal(dev['gU'], before)       # nothing ran
