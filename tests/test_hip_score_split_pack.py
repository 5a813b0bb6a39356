"""The packed split stage 2 of the soft-gate K5-K7 forward (option fwd_split_pack, ktup_score_pref_mc.hip + ktup_split_plan.h): a lane holds
at most five logits at P <= 20, so the six products of the three-way bf16 split are packed into four v_mfma_f32_16x16x32_bf16 per tile
and table (three at P <= 16) instead of six.

Random data, on every (d, P, n) below, for KTUP and TUP and both distances:
  * packed against the CPU oracle at the tolerances of tests/test_hip_score.py (rtol 1e-4 / atol 1e-5);
  * packed against fwd_split_pack = 0 (the six-product form) at rtol 2e-5 / atol 2e-6, the rule of tests/test_hip_score_split.py
    between stage-2 forms;
  * two launches give the same bits; fwd_buf_gather 0 and 1 give the same bits under the packed form;
  * at n = 70,001 the bits differ from the six-product form somewhere (the sums are taken in another order): an option that selected
    nothing would fail here.
Shapes: d in {64, 100} x P in {9, 12, 13, 16, 17, 19, 20} and d = 128 x P in {17, 20} -- three, four and five logits per lane with full
and partly filled last groups; n in {5 (ragged single tile), 512 (the small-batch wave count), 70,001 (several tiles per wave, ragged end)}.

One product class at a time (test_each_product_class_*): bounds like the above cannot see a lost mid.mid or lo.hi product (2^-18 to
2^-16 of a term).  For every preference p < P (P = 20, 16, 12; d = 100; TUP, L1) the tables' only non-zero preference row is p, its
values and the logit are V = 1 + 2^-8 - 2^-15 + 2^-18 + 2^-19 times a power of two, whose bf16 pieces are all full-sized
(hi = 1, mid = 2^-8 - 2^-15, lo = 0.75 x 2^-17), the logit is exact (x has one non-zero coordinate, a power of two) and the score is,
up to a share below 1 %, linear in the contraction under test:
  * r side (Ar): u = i, so q = 0 and n = 0 (zero norm table): score = sum over 5 coordinates of |g Ar_p[k]|;
  * n side (Cn): q has one non-zero coordinate k1, where Cn_p is a power of two, so s = q . n needs the logit's pieces only; Cn_p = 256 V
    at four more coordinates, where the score collects |s n_k|.
The non-zero coordinates differ mod 16, so each lands in its own accumulator element and the distance sum is at most four roundings.
The test restates the six-class sum in numpy and asserts on the CPU, before the GPU is asked, that deleting any ONE class moves the fp64
score by more than 4 x the bound, and that the six-class sum itself is within the bound; then |GPU - fp64| <= 2^-20 relative, a quarter
of the smallest class's effect at full-sized pieces.

The inf / nan containment case of tests/test_hip_score_split.py runs at (100, 20) and (64, 12) under the packed form."""
import functools

import numpy as np
import pytest
import torch

from oracle import cpu_ref as O

pytestmark = pytest.mark.gpu
DEV = 'cuda'
RT, AT = 1e-4, 1e-5                      # tests/test_hip_score.py
SHAPES = [(d, P) for d in (64, 100) for P in (9, 12, 13, 16, 17, 19, 20)] + [(128, 17), (128, 20)]


def close(got, want, rtol=RT, atol=AT):
    np.testing.assert_allclose(got.detach().cpu().numpy(), want.detach().cpu().numpy(), rtol=rtol, atol=atol)


def rand_world(seed, nu, ni, ne, nr, d):
    gen = torch.Generator().manual_seed(seed)
    mk = lambda r: O.make_table(r, d, gen)
    W = dict(U=mk(nu), I=mk(ni), E=torch.cat([mk(ne), torch.zeros(1, d)]), P=mk(nr), Pn=mk(nr), R=mk(nr), Rn=mk(nr))
    i2e = torch.randint(0, ne, (ni,), generator=gen)
    i2e[torch.rand(ni, generator=gen) < 0.1] = ne          # ~10 % of items map to the pad row
    return W, i2e, gen


@functools.lru_cache(maxsize=None)
def world(d, P):
    """The (d, P) world, its 70,001 pairs (smaller batches are prefixes) and the oracle's scores, computed once and never modified."""
    nu, ni, ne = 700, 400, 900
    W, i2e, gen = rand_world(5 + d + P, nu, ni, ne, P, d)
    u = torch.randint(0, nu, (70001,), generator=gen); i = torch.randint(0, ni, (70001,), generator=gen)
    want = {l1: (O.score_ktup_rec(W['U'], W['I'], W['E'], W['P'], W['Pn'], W['R'], W['Rn'], i2e, u, i, l1),
                 O.score_tup(W['U'], W['I'], W['P'], W['Pn'], u, i, l1)) for l1 in (False, True)}
    return W, i2e, u, i, want


def scores(D, i2e_d, u, i, l1, pack, buf=1):
    """(KTUP, TUP) scores with options fwd_split_pack = `pack` and fwd_buf_gather = `buf` for the two launches."""
    from jTransUP.hip import lib as L
    from jTransUP.hip import ops
    old_p, old_b = L.set_option('fwd_split_pack', pack), L.set_option('fwd_buf_gather', buf)
    try:
        with torch.no_grad():
            return (ops.score_ktup(D['U'], D['I'], D['E'], D['P'], D['Pn'], D['R'], D['Rn'], i2e_d, u, i, l1).cpu(),
                    ops.score_tup(D['U'], D['I'], D['P'], D['Pn'], u, i, l1).cpu())
    finally:
        L.set_option('fwd_split_pack', old_p)
        L.set_option('fwd_buf_gather', old_b)


def test_option_is_on_by_default_and_after_fwd_buf_gather():
    from jTransUP.hip import lib as L
    assert L.get_option('fwd_split_pack') == 1
    assert L.get_option('fwd_split') == 1 and L.get_option('fwd_buf_gather') == 1


@pytest.mark.parametrize('n', [5, 512, 70001])
@pytest.mark.parametrize('d,P', SHAPES)
def test_packed_forward_vs_oracle_and_six_product_form(d, P, n):
    W, i2e, u, i, want = world(d, P)
    D = {k: v.to(DEV) for k, v in W.items()}
    i2e_d, ud, idv = i2e.to(DEV, torch.int32), u[:n].to(DEV), i[:n].to(DEV)
    for l1 in (False, True):
        packed, again, six = scores(D, i2e_d, ud, idv, l1, 1), scores(D, i2e_d, ud, idv, l1, 1), scores(D, i2e_d, ud, idv, l1, 0)
        pointer = scores(D, i2e_d, ud, idv, l1, 1, buf=0)
        for k in range(2):
            what = 'd = %d, P = %d, n = %d, l1 = %s, %s' % (d, P, n, l1, ('KTUP', 'TUP')[k])
            close(packed[k], want[l1][k][:n])
            close(packed[k], six[k], rtol=2e-5, atol=2e-6)
            assert torch.equal(packed[k], again[k]), 'two launches of the packed form differ at ' + what
            assert torch.equal(packed[k], pointer[k]), 'fwd_buf_gather changes bits under the packed form at ' + what
            if n == 70001:
                assert not torch.equal(packed[k], six[k]), 'fwd_split_pack = 1 ran the six-product form at ' + what


@pytest.mark.parametrize('d,P', [(100, 20), (64, 12)])
def test_packed_forward_keeps_inf_and_nan_inside_their_pair(d, P):
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


# ---- one product class at a time ------------------------------------------------------------------------------------------------
BOUND = 2.0 ** -20
V = np.float32(1 + 2.0 ** -8 - 2.0 ** -15 + 2.0 ** -18 + 2.0 ** -19)
CLASSES = ('hi.hi', 'hi.mid', 'mid.hi', 'mid.mid', 'hi.lo', 'lo.hi')      # (table piece).(logit piece)
D_CLS, K0, K1 = 100, 37, 6                                               # the logit's coordinate; the coordinate q lives at (n side)
KR = (37, 2, 20, 57, 99)                                                 # r side: non-zero coordinates of Ar_p (K0 among them), distinct mod 16
KN = (17, 40, 63, 92)                                                    # n side: coordinates where Cn_p = 256 V; with K0, K1: distinct mod 16
SCALES = (1.0, 0.5, 2.0)                                                 # x[K0] per pair: the logit is SCALES[pair % 3] x V, exactly
N_CLS = 40                                                               # three tiles, the last one ragged


def bf16_round(x):
    """float32 -> the nearest bf16 (ties to even), as float32."""
    u = np.asarray(x, np.float32).view(np.uint32)
    return ((u + np.uint32(0x7fff) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xffff0000)).view(np.float32)


def pieces(x):
    """(hi, mid, lo) of the kernel's three-way split, in fp64; hi + mid + lo == x."""
    x = np.asarray(x, np.float32)
    hi = bf16_round(x)
    r1 = (x - hi).astype(np.float32)
    mid = bf16_round(r1)
    lo = bf16_round((r1 - mid).astype(np.float32))
    assert np.all(hi.astype(np.float64) + mid + lo == x.astype(np.float64))
    return hi.astype(np.float64), mid.astype(np.float64), lo.astype(np.float64)


def six_class_product(a, b, drop=None):
    """table value a x logit b as the kernel's six products, in fp64, optionally without one class."""
    (ah, am, al), (bh, bm, bl) = pieces(a), pieces(b)
    terms = {'hi.hi': ah * bh, 'hi.mid': ah * bm, 'mid.hi': am * bh, 'mid.mid': am * bm, 'hi.lo': ah * bl, 'lo.hi': al * bh}
    return sum(v for k, v in terms.items() if k != drop)


def class_inputs(side):
    """Pairs and the non-zero preference row's values for one side: (U, I, u, i, row of P, row of Pn, logit per pair)."""
    c = np.array([SCALES[k % 3] for k in range(N_CLS)], np.float32)
    U = np.zeros((N_CLS, D_CLS), np.float32); I = np.zeros((N_CLS, D_CLS), np.float32)
    U[:, K0] = c / 2; I[:, K0] = c / 2                                   # x[K0] = c, q[K0] = 0
    prow = np.zeros(D_CLS, np.float32); nrow = np.zeros(D_CLS, np.float32)
    if side == 'r':
        prow[list(KR)] = V                                               # Alog_p = P_p / 2, Ar_p = P_p (TUP); q = 0, n = 0
        g = (c * np.float32(0.5)) * V
    else:
        prow[K0] = 2 * V                                                 # logit = c V; r lives at K0 alone
        nrow[K1] = 0.25
        nrow[list(KN)] = 256 * V
        U[:, K1] = 1; I[:, K1] = -1                                      # x[K1] = 0, q[K1] = 2
        g = c * V
    assert np.all(g.astype(np.float64) == c.astype(np.float64) * (0.5 if side == 'r' else 1.0) * np.float64(V))   # the logit is exact
    return U, I, prow, nrow, g


def class_score(side, prow, nrow, g, product):
    """The L1 score per pair in fp64 with table x logit products taken by `product` in the contraction under test (exact elsewhere)."""
    g64 = g.astype(np.float64)
    if side == 'r':
        return sum(np.abs(product(np.full_like(g, prow[k]), g)) for k in KR)          # q = 0, n = 0: |r_k|
    n = {k: product(np.full_like(g, nrow[k]), g) for k in (K1,) + KN}
    s = 2.0 * n[K1]                                                                    # q . n, q = 2 at K1
    return np.abs(g64 * np.float64(prow[K0])) + np.abs(2.0 - s * n[K1]) + sum(np.abs(s * n[k]) for k in KN)


@pytest.mark.parametrize('side', ['r', 'n'])
@pytest.mark.parametrize('P', [20, 16, 12])
def test_each_product_class_is_there_for_every_preference(P, side):
    from jTransUP.hip import lib as L
    from jTransUP.hip import ops
    U, I, prow, nrow, g = class_inputs(side)
    exact = class_score(side, prow, nrow, g, lambda a, b: a.astype(np.float64) * b.astype(np.float64))
    six = class_score(side, prow, nrow, g, six_class_product)
    assert np.all(np.abs(six - exact) <= BOUND * exact), 'the six-class sum itself misses the bound'
    for cls in CLASSES:
        moved = np.abs(class_score(side, prow, nrow, g, lambda a, b: six_class_product(a, b, drop=cls)) - exact) / exact
        assert np.all(moved > 4 * BOUND), 'the inputs cannot see a lost %s product: it moves the score by %.3g' % (cls, moved.min())
    ids = torch.arange(N_CLS, device=DEV)
    Ud, Id = torch.from_numpy(U).to(DEV), torch.from_numpy(I).to(DEV)
    assert L.get_option('fwd_split_pack') == 1 and L.get_option('fwd_split') == 1
    worst = 0.0
    for p in range(P):
        Pt = torch.zeros(P, D_CLS); Pn = torch.zeros(P, D_CLS)
        Pt[p] = torch.from_numpy(prow); Pn[p] = torch.from_numpy(nrow)
        with torch.no_grad():
            got = ops.score_tup(Ud, Id, Pt.to(DEV), Pn.to(DEV), ids, ids, True).cpu().numpy().astype(np.float64)
        err = np.abs(got - exact) / exact
        worst = max(worst, float(err.max()))
        assert np.all(err <= BOUND), 'P = %d, %s side, preference %d: relative error %.3g > 2^-20 at pair %d' % (P, side, p, err.max(), int(err.argmax()))
    print('P = %d, %s side: worst relative error %.3g (bound %.3g)' % (P, side, worst, BOUND))
