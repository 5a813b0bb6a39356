"""The one-sweep gold-rank passes (ktup_eval_dot_ranks, ktup_eval_cfkg_ranks) on the GPU: the matrix route's integers (K11 + the two
adds + ktup_eval_gold_ranks), exact ties, pitched tables, consistency with the wide list pass place by place (the gold keys are the
sweep's bits), CFKG against its own listed scores and against the fp64 reference, the declines and errors, and a replayed graph.

Gold lists of every case (golds()): random sizes 0-12; user 0 has none; user 1 has a gold that is also in its filter list (-> -1); user
2 repeats an id; user 3 has 40 golds; the last user has the id n + 3 (-> -1); u_ids holds duplicates.  With a single user that user
carries the 40 golds, the repeated id and n + 3.  Filters are those of tests/test_hip_dot_pass.py / tests/test_hip_cfkg_pass.py."""
import ctypes

import numpy as np
import pytest
import torch

from tests.test_hip_cfkg_pass import filters as cfkg_filters, tol
from tests.test_hip_dot_pass import filters as dot_filters

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NR = 4


def ops():
    from jTransUP.hip import ops as o
    return o


def golds(rng, nq, n, f_off, f_ids):
    """-> (gold_off, gold_ids) on the device and the lists on the host."""
    f_off, f_ids = f_off.cpu().numpy(), f_ids.cpu().numpy()
    lists = []
    for b in range(nq):
        k = int(rng.randint(0, 13))
        lists.append(rng.choice(n, size=min(k, n), replace=False).astype(np.int32).tolist())
    big = 3 if nq > 3 else 0
    lists[big] = rng.randint(0, n, size=40).astype(np.int32).tolist() if n < 40 else rng.choice(n, size=40, replace=False).astype(np.int32).tolist()
    rep = 2 if nq > 2 else 0
    lists[rep] = lists[rep] + [int(rng.randint(0, n)), int(rng.randint(0, n))]
    lists[rep].append(lists[rep][-2])                                      # an id twice in one list
    if nq > 1:
        lists[0] = []
        mine = f_ids[f_off[1]:f_off[2]]
        lists[1] = lists[1] + [int(mine[len(mine) // 2])]                  # a gold in the user's own filter list
    lists[nq - 1] = lists[nq - 1] + [n + 3]                                # outside the catalogue
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    flat = np.asarray([i for x in lists for i in x], dtype=np.int32)
    return torch.from_numpy(off).to(DEV), torch.from_numpy(flat).to(DEV), lists


# (d, users in table, items, nq): two and three user blocks with a partial last one, catalogues that are no multiple of 16 or of a
# stage, d % 4 != 0, the widest row, the degenerate minimum
SHAPES = [(64, 90, 203, 70), (100, 90, 1000, 130), (50, 40, 37, 5), (256, 70, 300, 64), (4, 10, 16, 1)]
_CASES = {}


def dot_case(shape):
    """Inputs of a shape and the matrix route's ranks for its four variants, made once and left unchanged."""
    if shape in _CASES:
        return _CASES[shape]
    d, nu, ni, nq = shape
    gen = torch.Generator().manual_seed(d * 7 + ni)
    rng = np.random.RandomState(ni + nq)
    U = (torch.randn(nu, d, generator=gen) * 0.5).to(DEV)
    I = (torch.randn(ni, d, generator=gen) * 0.5).to(DEV)
    u = torch.randint(0, nu, (nq,), generator=gen)
    if nq > 4:
        u[4] = u[0]; u[nq - 1] = u[3]                                     # duplicates
    u = u.to(DEV)
    scale = 0.25 * d ** 0.5
    ua = (torch.randn(nq, generator=gen) * scale).to(DEV)
    ia = (torch.randn(ni, generator=gen) * scale).to(DEV)
    f_off, f_ids = dot_filters(rng, nq, ni, min(165, max(2, ni // 8)))
    g_off, g_ids, lists = golds(rng, nq, ni, f_off, f_ids)
    want = {}
    for terms in (False, True):
        mat = ops().eval_bprmf(U, I, u)                                    # (built as tests/test_hip_dot_pass.py matrix_route builds it)
        if terms:
            mat = mat + ua[:, None]
            mat = mat + ia[None, :]
        for filt in (False, True):
            want[terms, filt] = ops().gold_ranks(mat, True, g_off, g_ids, f_off if filt else None, f_ids if filt else None)
    _CASES[shape] = (U, I, u, ua, ia, f_off, f_ids, g_off, g_ids, lists, want)
    return _CASES[shape]


@pytest.mark.parametrize('nsplit', [0, 1, 3])
@pytest.mark.parametrize('filt', [True, False])
@pytest.mark.parametrize('terms', [False, True])
@pytest.mark.parametrize('shape', SHAPES)
def test_dot_ranks_are_the_matrix_routes_integers(shape, terms, filt, nsplit):
    d, nu, ni, nq = shape
    U, I, u, ua, ia, f_off, f_ids, g_off, g_ids, lists, want = dot_case(shape)
    got = ops().eval_dot_ranks(U, I, u, g_off, g_ids, f_off if filt else None, f_ids if filt else None, ua if terms else None,
                               ia if terms else None, nsplit=nsplit)
    assert got is not None and got.dtype == torch.int32 and got.numel() == g_ids.numel()
    assert torch.equal(got, want[terms, filt])
    assert int(got[-1]) == -1                                              # the id n + 3
    if nq > 1 and filt:
        assert int(got[int(g_off[2]) - 1]) == -1                           # user 1's filtered gold (its whole catalogue is filtered)
    if nq > 3:
        assert int((got[int(g_off[3]):int(g_off[4])] >= 0).sum()) > 0      # the 40-gold user is ranked


@pytest.mark.parametrize('nsplit', [0, 1, 3, 8])
def test_exact_ties_go_to_the_lower_id(nsplit):
    """Items 3, 17 and 150 share one row: before the gold 17 stands 3, not 150; the gold 3 is unaffected by 17."""
    d, nu, ni, nq = 64, 20, 203, 20
    gen = torch.Generator().manual_seed(5)
    U = (torch.randn(nu, d, generator=gen) * 0.5).to(DEV)
    I = torch.randn(ni, d, generator=gen) * 0.5
    I[17] = I[3]; I[150] = I[3]
    I = I.to(DEV)
    u = torch.arange(nq).to(DEV)
    lists = [[17] if b % 2 else [3] for b in range(nq)]
    lists[4] = [3, 17]                                                     # both golds: neither counts for the other
    g_off = torch.from_numpy(np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)).to(DEV)
    g_ids = torch.tensor([i for x in lists for i in x], dtype=torch.int32, device=DEV)
    got = ops().eval_dot_ranks(U, I, u, g_off, g_ids, nsplit=nsplit).cpu().numpy()
    mat = ops().eval_bprmf(U, I, u)
    assert torch.equal(torch.from_numpy(got).to(DEV), ops().gold_ranks(mat, True, g_off, g_ids))
    mat = mat.cpu().numpy()
    off = g_off.cpu().numpy()
    for b in range(nq):
        assert mat[b, 3] == mat[b, 17] == mat[b, 150]
        above = int((mat[b] > mat[b, 3]).sum())
        for e in range(off[b], off[b + 1]):
            g = int(g_ids[e])
            if b == 4:
                assert got[e] == above
            else:
                assert got[e] == above + (1 if g == 17 else 0), (b, g)


def test_user_table_with_a_pitch_and_unaligned_item_rows():
    d, nu, ni, nq = SHAPES[0]
    U, I, u, ua, ia, f_off, f_ids, g_off, g_ids, lists, want = dot_case(SHAPES[0])
    wide = torch.zeros(nu, d + 12, device=DEV)
    wide[:, 5:5 + d] = U
    wide_i = torch.zeros(ni, d + 3, device=DEV)
    wide_i[:, 1:1 + d] = I
    got = ops().eval_dot_ranks(wide[:, 5:5 + d], wide_i[:, 1:1 + d], u, g_off, g_ids, f_off, f_ids, ua, ia)
    assert torch.equal(got, want[True, True])


def _cfkg_tables(d, nu, ne, nq, seed):
    gen = torch.Generator().manual_seed(seed)
    U, E, R = ((torch.randn(n, d, generator=gen) * 0.5) for n in (nu, ne, NR))
    u = torch.randint(0, nu, (nq,), generator=gen)
    if nq > 4:
        u[4] = u[0]; u[nq - 1] = u[3]
    return U, E, R, u


@pytest.mark.parametrize('shape', [(64, 90, 203, 70), (100, 90, 500, 70)])
@pytest.mark.parametrize('model', ['dot', 'cfkg_l1', 'cfkg_l2'])
def test_lists_and_ranks_agree_place_by_place(model, shape):
    """Against the wide list pass at topn 64 with the same filter: a gold listed at place p has rank p - (golds listed before it); a
    gold with rank r and b golds ordered before it, r + b < 64, is listed at place r + b.  One differing score bit between the gold
    keys and the sweep's would misplace a gold."""
    d, nu, n, nq = shape
    rng = np.random.RandomState(n + nq + len(model))
    U, E, R, u = _cfkg_tables(d, nu, n, nq, d + n)
    U, E, R, u = U.to(DEV), E.to(DEV), R.to(DEV), u.to(DEV)
    f_off, f_ids = dot_filters(rng, nq, n, 20)
    g_off, g_ids, lists = golds(rng, nq, n, f_off, f_ids)
    if model == 'dot':
        top = ops().eval_dot_topk_wide(U, E, u, 64, f_off, f_ids)
        ranks = ops().eval_dot_ranks(U, E, u, g_off, g_ids, f_off, f_ids)
    else:
        l1 = model == 'cfkg_l1'
        top = ops().eval_cfkg_topk_wide(U, R, NR - 1, E, u, 64, l1, filt_off=f_off, filt_ids=f_ids)
        ranks = ops().eval_cfkg_ranks(U, R, NR - 1, E, u, l1, g_off, g_ids, filt_off=f_off, filt_ids=f_ids)
    top, ranks, off = top.cpu().numpy(), ranks.cpu().numpy(), g_off.cpu().numpy()
    seen = 0
    for b in range(nq):
        mine = {}                                                          # gold id -> rank (both entries of a repeated id agree)
        for e in range(off[b], off[b + 1]):
            g = lists[b][e - off[b]]
            assert mine.setdefault(g, int(ranks[e])) == int(ranks[e])
        row = top[b].tolist()
        before = 0
        for p, j in enumerate(row):
            if j in mine:
                assert mine[j] == p - before, (b, p, j, mine[j], before)
                before += 1
                seen += 1
        for g, r in mine.items():
            if r < 0:
                assert g not in row
                continue
            lo = sum(1 for o, ro in mine.items() if o != g and 0 <= ro < r)            # golds certainly before / possibly before
            hi = sum(1 for o, ro in mine.items() if o != g and 0 <= ro <= r)
            if r + hi < 64:
                assert g in row[r + lo:r + hi + 1], (b, g, r, lo, hi, row)
    assert seen > nq // 2                                                  # (the check saw golds inside the lists)


@pytest.mark.parametrize('l1', [True, False])
@pytest.mark.parametrize('nc', [16, 37, 64])
def test_cfkg_ranks_from_the_passes_own_listed_scores(nc, l1):
    """A catalogue the wide list shows whole (topn 64, no filter): the ranks computed on the host from those scores and the filter /
    gold sets, exactly."""
    d, nu, ne, nq = 100, 40, 120, 70
    rng = np.random.RandomState(nc + 2 * l1)
    U, E, R, u = _cfkg_tables(d, nu, ne, nq, 31 + nc)
    cand = torch.from_numpy(rng.permutation(ne)[:nc].astype(np.int64))
    cand[1] = cand[0]                                                      # one entity row twice: exactly equal scores
    bad = nc // 2
    cand[bad] = -3 if nc % 2 else ne + 5                                   # one entry without an entity row
    U, E, R, u, cand = U.to(DEV), E.to(DEV), R.to(DEV), u.to(DEV), cand.to(DEV)
    f_off, f_ids, banned = cfkg_filters(rng, nq, nc)
    g_off, g_ids, lists = golds(rng, nq, nc, f_off, f_ids)
    lists[5].append(bad)                                                   # a gold without a row (-> -1): rebuild the CSR with it
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    g_off = torch.from_numpy(off).to(DEV)
    g_ids = torch.tensor([i for x in lists for i in x], dtype=torch.int32, device=DEV)
    top, sc = ops().eval_cfkg_topk_wide(U, R, NR - 1, E, u, 64, l1, cand_ids=cand, with_scores=True)
    top, sc = top.cpu().numpy(), sc.cpu().numpy()
    for filt in (True, False):
        got = ops().eval_cfkg_ranks(U, R, NR - 1, E, u, l1, g_off, g_ids, cand_ids=cand, filt_off=f_off if filt else None,
                                    filt_ids=f_ids if filt else None).cpu().numpy()
        for b in range(nq):
            assert (top[b, :nc - 1] >= 0).all() and (top[b, nc - 1:] == -1).all()
            score = {int(j): float(s) for j, s in zip(top[b, :nc - 1], sc[b, :nc - 1])}
            out = (banned[b] if filt else set()) | set(lists[b])
            for e in range(off[b], off[b + 1]):
                g = lists[b][e - off[b]]
                if g not in score or (filt and g in banned[b]):
                    assert got[e] == -1, (b, g)
                    continue
                want = sum(1 for j, s in score.items() if j not in out and (s < score[g] or (s == score[g] and j < g)))
                assert got[e] == want, (nc, l1, filt, b, g, got[e], want)


@pytest.mark.parametrize('l1', [True, False])
def test_cfkg_ranks_against_fp64(l1):
    """Every rank lies in [#{c : s_c < s_g - tol}, #{c : s_c <= s_g + tol}] of the fp64 scores (oracle.cpu_ref.eval_cfkg_rec), counted
    over unfiltered non-gold candidates with a row; tol(s) = 1e-4 |s| + 1e-5, the rule of tests/test_hip_cfkg_pass.py."""
    from oracle import cpu_ref
    d, nu, ne, nc, nq = 100, 90, 500, 333, 70
    rng = np.random.RandomState(ne + nq)
    U, E, R, u = _cfkg_tables(d, nu, ne, nq, 77)
    full = cpu_ref.eval_cfkg_rec(U.double(), E.double(), R.double(), u, l1).numpy()
    cand = torch.from_numpy(rng.permutation(ne)[:nc].astype(np.int64))
    cand[1] = cand[0]
    bad = nc // 2
    cand[bad] = ne + 5
    valid = ((cand >= 0) & (cand < ne)).numpy()
    ref = np.full((nq, nc), np.inf)
    ref[:, valid] = full[:, cand[valid].numpy()]
    f_off, f_ids, banned = cfkg_filters(rng, nq, nc)
    g_off, g_ids, lists = golds(rng, nq, nc, f_off, f_ids)
    got = ops().eval_cfkg_ranks(U.to(DEV), R.to(DEV), NR - 1, E.to(DEV), u.to(DEV), l1, g_off, g_ids, cand_ids=cand.to(DEV), filt_off=f_off,
                                filt_ids=f_ids).cpu().numpy()
    off = g_off.cpu().numpy()
    ranked = 0
    for b in range(nq):
        counted = np.isfinite(ref[b])
        for j in banned[b] | set(g for g in lists[b] if g < nc):
            counted[j] = False
        for e in range(off[b], off[b + 1]):
            g = lists[b][e - off[b]]
            if g >= nc or g in banned[b] or not np.isfinite(ref[b, g]):
                assert got[e] == -1, (b, g)
                continue
            s = ref[b, g]
            lo = int((ref[b, counted] < s - tol(s)).sum())
            hi = int((ref[b, counted] <= s + tol(s)).sum())
            assert lo <= got[e] <= hi, (l1, b, g, got[e], lo, hi)
            ranked += 1
    assert ranked > 200


def test_declines_and_errors():
    from jTransUP.hip import lib as L
    o = ops()
    lib = L.load()
    d, nu, ni, nq = 64, 90, 203, 70
    gen = torch.Generator().manual_seed(3)
    rng = np.random.RandomState(3)
    U = (torch.randn(nu, d, generator=gen) * 0.5).to(DEV)
    I = (torch.randn(ni, d, generator=gen) * 0.5).to(DEV)
    u = torch.randint(0, nu, (nq,), generator=gen).to(DEV)
    cap = 3072                                                             # KTUP_RANK_BLOCK_GOLDS: per 64-user block at d <= 128
    assert lib.ktup_eval_dot_ranks_supported(d, ni, cap) == 1 and lib.ktup_eval_dot_ranks_supported(d, ni, cap + 1) == 0
    assert lib.ktup_eval_dot_ranks_supported(256, ni, 2048) == 1 and lib.ktup_eval_dot_ranks_supported(256, ni, 2049) == 0
    assert lib.ktup_eval_cfkg_ranks_supported(129, ni, 2049) == 0 and lib.ktup_eval_cfkg_ranks_supported(128, ni, 2049) == 1
    assert lib.ktup_eval_dot_ranks_workspace_bytes(d, nq, ni, cap + 10, cap + 1) == 0
    assert lib.ktup_eval_dot_ranks_workspace_bytes(d, nq, ni, cap + 10, cap) > 0
    for first, served in ((cap - 4, True), (cap - 3, False)):            # block 0 = user 0's list + four singles: cap, cap + 1 entries
        sizes = [first] + [1] * 4 + [0] * (nq - 5)
        sizes[-1] = 7                                                      # (block 1 is small either way)
        off = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)).to(DEV)
        g = torch.from_numpy(rng.randint(0, ni, size=int(off[-1])).astype(np.int32)).to(DEV)
        got = o.eval_dot_ranks(U, I, u, off, g)
        if served:
            assert torch.equal(got, o.gold_ranks(o.eval_bprmf(U, I, u), True, off, g))
        else:
            assert got is None
    off = torch.tensor([0, 2] + [2] * (nq - 1), dtype=torch.int64, device=DEV)
    g = torch.tensor([1, 2], dtype=torch.int32, device=DEV)
    U260 = torch.zeros(nu, 260, device=DEV)
    assert o.eval_dot_ranks(U260, torch.zeros(ni, 260, device=DEV), u, off, g) is None
    assert lib.ktup_eval_dot_ranks_supported(260, ni, 2) == 0 and lib.ktup_eval_dot_ranks_workspace_bytes(260, nq, ni, 2, 2) == 0
    ranks = torch.empty(2, dtype=torch.int32, device=DEV)
    ws = torch.empty(lib.ktup_eval_dot_ranks_workspace_bytes(d, nq, ni, 2, 2) // 4 + 8, dtype=torch.float32, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    args = lambda gi, w: (p(U), d, p(I), d, d, p(u), nq, ni, None, None, None, None, p(off), gi, 2, 2, 0, p(ranks), w, None)
    with pytest.raises(L.KtupError) as e:
        L.call('ktup_eval_dot_ranks', *args(None, p(ws)))
    assert 'gold_ids' in str(e.value)
    with pytest.raises(L.KtupError) as e:
        L.call('ktup_eval_dot_ranks', *args(p(g), ctypes.c_void_p(ws.data_ptr() + 8)))
    assert 'workspace' in str(e.value) and '16-byte' in str(e.value)
    L.call('ktup_eval_dot_ranks', *args(p(g), p(ws)))                      # (the same arguments, aligned: served)
    assert torch.equal(ranks, o.gold_ranks(o.eval_bprmf(U, I, u), True, off, g))


def test_a_captured_call_follows_the_tables():
    from jTransUP.hip.lib import capture
    U, I, u, ua, ia, f_off, f_ids, g_off, g_ids, lists, want = dot_case(SHAPES[0])
    U, I = U.clone(), I.clone()
    o = ops()
    eager = o.eval_dot_ranks(U, I, u, g_off, g_ids, f_off, f_ids, ua, ia)      # (also: the one host read of the CSR, before the capture)
    assert torch.equal(eager, want[True, True])
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with capture(graph):
            held = o.eval_dot_ranks(U, I, u, g_off, g_ids, f_off, f_ids, ua, ia)
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()
    assert torch.equal(held, eager)
    gen = torch.Generator().manual_seed(99)
    U.copy_((torch.randn(U.shape, generator=gen) * 0.5).to(DEV))           # new tables in place
    I.copy_((torch.randn(I.shape, generator=gen) * 0.5).to(DEV))
    graph.replay()
    again = o.eval_dot_ranks(U, I, u, g_off, g_ids, f_off, f_ids, ua, ia)
    assert torch.equal(held, again) and not torch.equal(again, eager)
