"""The split stage 2 of the soft-gate K5-K7 forward (option fwd_split, ktup_score_pref_mc.hip): r = Ar^T g and n = Cn^T g as three bf16
pieces per operand and six products on v_mfma_f32_16x16x32_bf16 instead of fp32 MFMAs.

Checked on every (d, P, n) below, for KTUP and TUP and both distances:
  * fwd_split = 1 against the CPU oracle at the tolerances of tests/test_hip_score.py (rtol 1e-4 / atol 1e-5);
  * fwd_split = 1 against fwd_split = 0 on the same inputs at rtol 2e-5 / atol 2e-6 (the rule of the fwd_wide test);
  * two launches give the same bits;
  * an inf / nan row of one pair stays in that pair (the pairs of a tile are the columns of one MFMA).
Shapes: d in {64, 100, 128}, P in {3, 16, 20, 32}, n in {5 (ragged single tile), 512 (the small-batch wave count), 70,001 (many tiles per
wave, ragged end)}.  Geometries that keep the fp32 stage 2 under fwd_split = 1 (P <= 8: two fp32 MFMAs per tile are fewer clocks than six
bf16 ones; d = 100 / P = 32, d = 128 / P = 16 and P = 32: the bf16 planes would cost the workgroup four waves) run the same kernel
under both settings; SPLIT_SHAPES lists the ones that must take the split form, and the test requires their bits to differ from the
fp32 form's somewhere in a large batch -- an option that silently selected nothing would fail here."""
import numpy as np
import pytest
import torch

from oracle import cpu_ref as O

pytestmark = pytest.mark.gpu
DEV = 'cuda'
RT, AT = 1e-4, 1e-5                      # tests/test_hip_score.py
SPLIT_SHAPES = {(64, 16), (64, 20), (64, 32), (100, 16), (100, 20), (128, 20)}


def close(got, want, rtol=RT, atol=AT):
    np.testing.assert_allclose(got.detach().cpu().numpy(), want.detach().cpu().numpy(), rtol=rtol, atol=atol)


def rand_world(seed, nu, ni, ne, nr, d):
    gen = torch.Generator().manual_seed(seed)
    mk = lambda r: O.make_table(r, d, gen)
    W = dict(U=mk(nu), I=mk(ni), E=torch.cat([mk(ne), torch.zeros(1, d)]), P=mk(nr), Pn=mk(nr), R=mk(nr), Rn=mk(nr))
    i2e = torch.randint(0, ne, (ni,), generator=gen)
    i2e[torch.rand(ni, generator=gen) < 0.1] = ne          # ~10 % of items map to the pad row
    return W, i2e, gen


def scores(D, i2e_d, u, i, l1, split):
    """(KTUP, TUP) scores with option fwd_split set to `split` for the two launches."""
    from jTransUP.hip import lib as L
    from jTransUP.hip import ops
    old = L.set_option('fwd_split', split)
    try:
        return (ops.score_ktup(D['U'], D['I'], D['E'], D['P'], D['Pn'], D['R'], D['Rn'], i2e_d, u, i, l1).cpu(),
                ops.score_tup(D['U'], D['I'], D['P'], D['Pn'], u, i, l1).cpu())
    finally:
        L.set_option('fwd_split', old)


@pytest.mark.parametrize('n', [5, 512, 70001])
@pytest.mark.parametrize('P', [3, 16, 20, 32])
@pytest.mark.parametrize('d', [64, 100, 128])
def test_split_forward_vs_oracle_and_fp32_form(d, P, n):
    nu, ni, ne = 700, 400, 900
    W, i2e, gen = rand_world(7 + d + P, nu, ni, ne, P, d)
    u = torch.randint(0, nu, (n,), generator=gen); i = torch.randint(0, ni, (n,), generator=gen)
    D = {k: v.to(DEV) for k, v in W.items()}
    i2e_d, ud, idv = i2e.to(DEV, torch.int32), u.to(DEV), i.to(DEV)
    for l1 in (False, True):
        want_k = O.score_ktup_rec(W['U'], W['I'], W['E'], W['P'], W['Pn'], W['R'], W['Rn'], i2e, u, i, l1)
        want_t = O.score_tup(W['U'], W['I'], W['P'], W['Pn'], u, i, l1)
        split, again, plain = scores(D, i2e_d, ud, idv, l1, 1), scores(D, i2e_d, ud, idv, l1, 1), scores(D, i2e_d, ud, idv, l1, 0)
        for k, want in enumerate((want_k, want_t)):
            close(split[k], want)
            close(split[k], plain[k], rtol=2e-5, atol=2e-6)
            assert torch.equal(split[k], again[k]), 'two launches of the split form differ'
            if (d, P) in SPLIT_SHAPES and n == 70001:
                assert not torch.equal(split[k], plain[k]), 'fwd_split = 1 ran the fp32 stage 2 at d = %d, P = %d' % (d, P)


@pytest.mark.parametrize('P', [16, 20])
@pytest.mark.parametrize('d', [64, 100, 128])
def test_split_forward_keeps_inf_and_nan_inside_their_pair(d, P):
    """Pair 5 gathers a user row holding inf, pair 37 an item row holding nan (each row is used by that pair alone): every other pair
    of their 16-pair tiles -- and of the batch -- keeps the bits of the clean run, and the two pairs themselves are not finite."""
    nu, ni, ne, n = 300, 200, 400, 100
    W, i2e, gen = rand_world(23 + d + P, nu, ni, ne, P, d)
    u = torch.randint(1, nu, (n,), generator=gen); i = torch.randint(1, ni, (n,), generator=gen)
    u[5] = 0; i[37] = 0
    D = {k: v.to(DEV) for k, v in W.items()}
    i2e_d, ud, idv = i2e.to(DEV, torch.int32), u.to(DEV), i.to(DEV)
    bad = {k: v.clone() for k, v in D.items()}
    bad['U'][0, d // 3] = float('inf')
    bad['I'][0, :] = float('nan')
    keep = torch.ones(n, dtype=torch.bool); keep[5] = False; keep[37] = False
    for l1 in (False, True):
        clean, dirty = scores(D, i2e_d, ud, idv, l1, 1), scores(bad, i2e_d, ud, idv, l1, 1)
        for k in range(2):
            assert torch.equal(clean[k][keep], dirty[k][keep]), 'an inf / nan row leaked into another pair'
            assert not torch.isfinite(dirty[k][5]) and not torch.isfinite(dirty[k][37])
            assert torch.isfinite(clean[k]).all()
