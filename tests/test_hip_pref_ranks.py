"""The one-sweep gold-rank pass of TUP / KTUP (ktup_eval_pref_ranks, ops.eval_pref_ranks) on the GPU: place by place against the wide
list pass (the gold keys are the list pass's score bits), a referee against the matrix route's fp32 scores of all pairs, the same
integers at every split count and user order, exact ties, pitched / unaligned tables, the declines and errors, a replayed graph and
the models' rank_items.

Worlds, filters and the matrix route's scores are those of tests/test_hip_pref_wide_topn.py (made once, shared, never modified);
gold lists are tests/test_hip_rank_pass.py's golds(): random sizes 0-12, user 0 has none, user 1 has a gold that is also in its
filter list (its whole catalogue is filtered), user 2 repeats an id, user 3 has 40 golds, the last user has the id n + 3."""
import ctypes

import numpy as np
import pytest
import torch

from jTransUP.hip import lib as L
from tests.test_hip_pref_wide_topn import Q_SHAPES, World, csr, ordered_world, tol, world
from tests.test_hip_rank_pass import golds

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NSPLITS = [0, 1, 3, 8]
CAP = 3072                                                  # KTUP_PREF_RANK_BLOCK_GOLDS
ERR_INVALID, ERR_UNSUPPORTED = -1, -3
_GOLDS = {}


def ops():
    from jTransUP.hip import ops as o
    return o


def gold_case(shape):
    """The gold CSR of a world, made once."""
    if shape not in _GOLDS:
        w = world(shape)
        _GOLDS[shape] = golds(np.random.RandomState(shape[1] + shape[2]), w.nq, w.ni, w.f_off, w.f_ids)
    return _GOLDS[shape]


def ranks_of(w, ktup, filt, g_off, g_ids, nsplit=0, U=None, u=None, items=None):
    fo, fi = (w.f_off, w.f_ids) if filt else (None, None)
    got = ops().eval_pref_ranks(w.U if U is None else U, w.u if u is None else u, w.items(ktup) if items is None else items, False, g_off,
                                g_ids, fo, fi, nsplit=nsplit)
    assert got is not None and got.dtype == torch.int32 and got.numel() == g_ids.numel()
    return got


# ------------------------------------------------------------------------------------------ 1. place by place against the list pass
@pytest.mark.parametrize('nsplit', NSPLITS)
@pytest.mark.parametrize('shape', Q_SHAPES)
def test_ranks_and_lists_agree_place_by_place(shape, nsplit):
    """Against eval_pref_topk_wide at topn 64 with the same filter: a gold listed at place p has rank p - (the user's other golds
    listed before it), exactly; a rank below 64 - (golds of the user) must be in the list.  In the 5- and 33-item worlds the list
    shows every unfiltered item, so every ranked gold is pinned."""
    w = world(shape)
    g_off, g_ids, lists = gold_case(shape)
    off = g_off.cpu().numpy()
    for ktup in (False, True):
        for filt in (True, False):
            fo, fi = (w.f_off, w.f_ids) if filt else (None, None)
            top = ops().eval_pref_topk_wide(w.U, w.u, w.items(ktup), False, 64, fo, fi, with_scores=True)[0].cpu().numpy()
            ranks = ranks_of(w, ktup, filt, g_off, g_ids, nsplit).cpu().numpy()
            seen = 0
            for b in range(w.nq):
                mine = {}                                                  # gold id -> rank (both entries of a repeated id agree)
                for e in range(off[b], off[b + 1]):
                    g = lists[b][e - off[b]]
                    assert mine.setdefault(g, int(ranks[e])) == int(ranks[e]), (ktup, filt, b, g)
                row = top[b].tolist()
                before = 0
                for p, j in enumerate(row):
                    if j in mine:
                        assert mine[j] == p - before, (ktup, filt, b, p, j, mine[j], before)
                        before += 1
                        seen += 1
                for g, r in mine.items():
                    if r < 0:
                        assert g not in row, (ktup, filt, b, g)
                    elif r < 64 - len(mine) or w.ni <= 64:
                        assert g in row, (ktup, filt, b, g, r)
            assert seen > 0


# ------------------------------------------------------------------------------------------ 2. the referee
def referee_share(w, ktup, filt, g_off, lists, ranks):
    """-> (ranked golds, those whose window [lo, hi] is one integer, the widest window); asserts lo <= rank <= hi and the -1s."""
    ref = w.matrix(ktup, False, ops().GUMBEL_OFF).cpu().numpy().astype(np.float64)
    off = g_off.cpu().numpy()
    ranked = decisive = widest = 0
    for b in range(w.nq):
        banned = set(w.filt[b].tolist()) if filt else set()
        counted = np.ones(w.ni, bool)
        for j in banned | set(g for g in lists[b] if g < w.ni):
            counted[j] = False
        mc = ref[b, counted]
        for e in range(off[b], off[b + 1]):
            g = lists[b][e - off[b]]
            if g >= w.ni or g in banned:
                assert ranks[e] == -1, (ktup, filt, b, g, ranks[e])
                continue
            mg = ref[b, g]
            t = tol(mg) + tol(mc)
            lo, hi = int((mc < mg - t).sum()), int((mc <= mg + t).sum())
            assert lo <= ranks[e] <= hi, (ktup, filt, b, g, ranks[e], lo, hi)
            ranked += 1
            decisive += lo == hi
            widest = max(widest, hi - lo)
    return ranked, decisive, widest


@pytest.mark.parametrize('shape', Q_SHAPES)
def test_ranks_lie_in_the_matrix_routes_windows(shape):
    """Every rank lies in [#{c : m_c < m_g - t}, #{c : m_c <= m_g + t}] of the matrix route's fp32 scores m (eval_tup / eval_ktup, all
    pairs), counted over unfiltered non-gold items, t = tol(m_g) + tol(m_c) with tests/test_hip_pref_wide_topn.py's tol; -1 exactly
    where the gold is filtered or outside the catalogue.  The bound is not vacuous: in every world at least 75 % of the ranked golds
    have a window of one integer (on the CPU oracle's scores of these worlds the share is 0.82 - 1.00 and the widest window is 2)."""
    w = world(shape)
    g_off, g_ids, lists = gold_case(shape)
    ranked = decisive = 0
    for ktup in (False, True):
        for filt in (True, False):
            ranks = ranks_of(w, ktup, filt, g_off, g_ids).cpu().numpy()
            r, dcs, widest = referee_share(w, ktup, filt, g_off, lists, ranks)
            print('referee %s ktup=%d filt=%d: %d ranked, decisive share %.3f, widest window %d' % (shape, ktup, filt, r, dcs / max(r, 1), widest))
            ranked += r
            decisive += dcs
    assert ranked > 0
    print('referee %s: decisive share %.3f over %d ranked golds' % (shape, decisive / ranked, ranked))
    assert decisive >= 0.75 * ranked, (shape, decisive, ranked)


# ------------------------------------------------------------------------------------------ 3. the same integers
@pytest.mark.parametrize('shape', Q_SHAPES)
def test_same_integers_at_every_split_and_user_order(shape):
    w = world(shape)
    g_off, g_ids, lists = gold_case(shape)
    perm = np.random.RandomState(5).permutation(w.nq)
    p_off, p_ids = csr([np.asarray(lists[b], np.int32) for b in perm])
    pf_off, pf_ids = csr([w.filt[b] for b in perm])
    off = g_off.cpu().numpy()
    back = torch.from_numpy(np.concatenate([np.arange(off[b], off[b + 1]) for b in perm] + [np.zeros(0, np.int64)])).to(DEV)
    for ktup in (False, True):
        for filt in (True, False):
            base = ranks_of(w, ktup, filt, g_off, g_ids)
            for nsplit in NSPLITS[1:]:
                assert torch.equal(ranks_of(w, ktup, filt, g_off, g_ids, nsplit), base), (ktup, filt, nsplit)
            got = ops().eval_pref_ranks(w.U, w.u[torch.from_numpy(perm).to(DEV)], w.items(ktup), False, p_off, p_ids,
                                        pf_off if filt else None, pf_ids if filt else None)
            assert torch.equal(got, base[back]), (ktup, filt)


# ------------------------------------------------------------------------------------------ 4. exact ties
@pytest.mark.parametrize('ktup', [False, True])
def test_exact_ties_go_to_the_lower_id(ktup):
    """ordered_world: 40 item rows (and their item2ent entries) stand a second time 150 ids further on.  The lower id stands before
    the higher one, the higher not before the lower, and two golds that tie do not count for each other."""
    w = ordered_world('rising', False, ktup)
    low = w.src[np.arange(w.nq) % len(w.src)].astype(np.int32)
    one = lambda ids: csr([np.asarray([i], np.int32) for i in ids])
    both_off, both_ids = csr([np.asarray([a, a + 150], np.int32) for a in low])
    for nsplit in NSPLITS:
        r_low = ranks_of(w, ktup, False, *one(low), nsplit=nsplit)
        r_high = ranks_of(w, ktup, False, *one(low + 150), nsplit=nsplit)
        r_both = ranks_of(w, ktup, False, both_off, both_ids, nsplit=nsplit)
        assert int(r_low.min()) >= 0
        assert torch.equal(r_high, r_low + 1), nsplit
        assert torch.equal(r_both.view(-1, 2), torch.stack([r_low, r_low], 1)), nsplit
    top = ops().eval_pref_topk_wide(w.U, w.u, w.items(ktup), False, 64, None, None, with_scores=True)[0].cpu().numpy()
    r_low = r_low.cpu().numpy()
    for b in range(w.nq):                                                  # (and the list pass puts them there)
        if r_low[b] < 63:
            assert top[b, r_low[b]] == low[b] and top[b, r_low[b] + 1] == low[b] + 150, b


# ------------------------------------------------------------------------------------------ 5. pitched and unaligned tables
@pytest.mark.parametrize('ktup', [False, True])
def test_pitched_user_table_and_unaligned_item_table(ktup):
    shape = Q_SHAPES[0]
    w = world(shape)
    g_off, g_ids, lists = gold_case(shape)
    d = w.d
    wide_u = torch.zeros(w.U.shape[0], d + 12, device=DEV)
    wide_u[:, 5:5 + d] = w.U
    wide_i = torch.zeros(w.ni, d + 3, device=DEV)
    wide_i[:, 1:1 + d] = w.I
    items = ops().eval_pref_items(wide_i[:, 1:1 + d], w.E if ktup else None, w.Pm, w.Pn, w.R if ktup else None, w.Rn if ktup else None,
                                  w.i2e if ktup else None)
    got = ranks_of(w, ktup, True, g_off, g_ids, U=wide_u[:, 5:5 + d], items=items)
    assert torch.equal(got, ranks_of(w, ktup, True, g_off, g_ids))


# ------------------------------------------------------------------------------------------ 6. declines and errors
def c_call(w, items, l1, g_off, g_ids, bg, ranks, ws, n_gold=None):
    o = ops()
    p = o._p
    I, E = items.I, items.E
    L.call('ktup_eval_pref_ranks', p(w.U), w.U.stride(0), p(I), I.stride(0), p(E), 0 if E is None else E.stride(0), p(items.item2ent),
           p(items.pws), items.P, items.d, p(w.u), w.nq, w.ni, int(l1), None, None, p(g_off), p(g_ids),
           g_ids.numel() if n_gold is None else n_gold, bg, 0, ranks, ws, o._stream(w.U.device))


def declined(w, ktup, l1, g_off, g_ids, bg):
    """ops answers None, _supported 0, workspace 0, and the C entry point KTUP_ERR_UNSUPPORTED."""
    lib = L.load()
    items = w.items(ktup)
    assert ops().eval_pref_ranks(w.U, w.u, items, l1, g_off, g_ids) is None
    assert lib.ktup_eval_pref_ranks_supported(items.d, items.P, int(l1), w.ni, bg) == 0
    assert lib.ktup_eval_pref_ranks_workspace_bytes(items.d, items.P, int(l1), w.nq, w.ni, g_ids.numel(), bg) == 0
    ranks = torch.empty(g_ids.numel(), dtype=torch.int32, device=DEV)
    ws = torch.empty(1 << 16, dtype=torch.float32, device=DEV)
    with pytest.raises(L.KtupError) as e:
        c_call(w, items, l1, g_off, g_ids, bg, ranks.data_ptr(), ws.data_ptr())
    assert e.value.code == ERR_UNSUPPORTED, str(e.value)


def small_golds(w):
    sizes = [2] + [0] * (w.nq - 1)
    return csr([np.asarray([1, 2][:s], np.int32) for s in sizes])


def test_declines():
    lib = L.load()
    w = world(Q_SHAPES[4])                                                 # (100, 90, 211, 37, 4)
    g_off, g_ids = small_golds(w)
    assert lib.ktup_eval_pref_ranks_supported(w.d, w.P, 0, w.ni, 2) == 1
    assert lib.ktup_eval_pref_ranks_workspace_bytes(w.d, w.P, 0, w.nq, w.ni, 2, 2) > 0
    declined(w, True, True, g_off, g_ids, 2)                               # L1
    w36 = world((36, 90, 177, 37, 20))                                     # a width without a preference-space pass
    declined(w36, False, False, *small_golds(w36), 2)
    w256 = world((256, 40, 130, 17, 20))                                   # d = 256, whatever eval_q256 says
    old = L.set_option('eval_q256', 1)
    try:
        declined(w256, True, False, *small_golds(w256), 2)
    finally:
        L.set_option('eval_q256', old)
    w33 = World(64, 40, 50, 10, 33)                                        # 33 preferences
    declined(w33, False, False, *small_golds(w33), 2)
    old = L.set_option('eval_mc', 0)
    try:
        declined(w, False, False, g_off, g_ids, 2)
    finally:
        L.set_option('eval_mc', old)
    assert lib.ktup_eval_pref_ranks_supported(w.d, w.P, 0, w.ni, CAP) == 1 and lib.ktup_eval_pref_ranks_supported(w.d, w.P, 0, w.ni, CAP + 1) == 0
    assert lib.ktup_eval_pref_ranks_supported(w.d, w.P, 0, 1 << 31, 2) == 0
    rng = np.random.RandomState(3)
    for first, served in ((CAP - 4, True), (CAP - 3, False)):              # block 0 = user 0's list + four singles: CAP, CAP + 1 entries
        sizes = [first] + [1] * 4 + [0] * (w.nq - 5)
        big_off, big_ids = csr([rng.randint(0, w.ni, size=s).astype(np.int32) for s in sizes])
        if served:
            got = ops().eval_pref_ranks(w.U, w.u, w.items(False), False, big_off, big_ids)
            m = w.matrix(False, False, ops().GUMBEL_OFF)
            lists = [big_ids[int(big_off[b]):int(big_off[b + 1])].cpu().tolist() for b in range(w.nq)]
            referee_share(w, False, False, big_off, lists, got.cpu().numpy())
            assert got.shape == (CAP,) and m.shape[0] == w.nq
        else:
            declined(w, False, False, big_off, big_ids, CAP + 1)


def test_errors_and_empty_calls():
    lib = L.load()
    w = world(Q_SHAPES[4])
    items = w.items(True)
    g_off, g_ids = small_golds(w)
    ranks = torch.empty(2, dtype=torch.int32, device=DEV)
    ws = torch.empty(lib.ktup_eval_pref_ranks_workspace_bytes(w.d, w.P, 0, w.nq, w.ni, 2, 2) // 4 + 8, dtype=torch.float32, device=DEV)
    for bad_ranks, bad_ws, word in ((None, ws.data_ptr(), 'ranks'), (ranks.data_ptr(), None, 'workspace'), (ranks.data_ptr(), ws.data_ptr() + 8, '16-byte')):
        with pytest.raises(L.KtupError) as e:
            c_call(w, items, False, g_off, g_ids, 2, bad_ranks, None if bad_ws is None else ctypes.c_void_p(bad_ws))
        assert e.value.code == ERR_INVALID and word in str(e.value), str(e.value)
    c_call(w, items, False, g_off, g_ids, 2, ranks.data_ptr(), ws.data_ptr())         # (the same arguments, aligned: served)
    assert torch.equal(ranks, ops().eval_pref_ranks(w.U, w.u, items, False, g_off, g_ids))
    assert int(ranks.min()) >= 0
    # no users / no golds: an empty result, nothing launched
    none = ops().eval_pref_ranks(w.U, w.u[:0], items, False, torch.zeros(1, dtype=torch.int64, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV))
    assert none.dtype == torch.int32 and none.numel() == 0
    none = ops().eval_pref_ranks(w.U, w.u, items, False, torch.zeros(w.nq + 1, dtype=torch.int64, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV))
    assert none.dtype == torch.int32 and none.numel() == 0


# ------------------------------------------------------------------------------------------ 7. a captured call
@pytest.mark.parametrize('ktup', [False, True])
def test_a_captured_call_follows_the_tables(ktup):
    from jTransUP.hip.lib import capture
    shape = Q_SHAPES[0]
    w0 = world(shape)
    g_off, g_ids, lists = gold_case(shape)
    o = ops()
    U, I = w0.U.clone(), w0.I.clone()
    items = o.eval_pref_items(I, w0.E if ktup else None, w0.Pm, w0.Pn, w0.R if ktup else None, w0.Rn if ktup else None, w0.i2e if ktup else None)

    def call():
        # (the prepared preference tables do not change here: the item side may be shared; the operand rows are rebuilt by every call)
        return o.eval_pref_ranks(U, w0.u, items, False, g_off, g_ids, w0.f_off, w0.f_ids)
    eager = call()                                                         # (also: the one host read of the CSR, before the capture)
    assert torch.equal(eager, ranks_of(w0, ktup, True, g_off, g_ids))
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with capture(graph):
            held = call()
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()
    assert torch.equal(held, eager)
    gen = torch.Generator().manual_seed(99)
    rows = torch.randperm(U.shape[0], generator=gen).to(DEV)
    U.copy_(U[rows])                                                       # new table rows in place
    I[7].copy_(I[11])
    graph.replay()
    first = held.clone()
    graph.replay()
    again = call()
    assert torch.equal(held, again) and torch.equal(first, again) and not torch.equal(again, eager)


# ------------------------------------------------------------------------------------------ 8. the models
@pytest.mark.parametrize('ktup', [False, True])
def test_models_rank_items(ktup):
    torch.manual_seed(11)
    rng = np.random.RandomState(11)
    NU, NI, NE, NR, Dm = 150, 177, 150, 7, 64
    users = torch.arange(NU, device=DEV)

    def make(l1, gumbel):
        if ktup:
            from jTransUP.models import jTransUP as jt
            i_map = {i: i for i in range(NI)}
            new_map = {i: ((i * 3) % NE if i % 5 else -1, i) for i in range(NI)}
            m = jt.jTransUPModel(l1, Dm, NU, NI, NE, NR, i_map, new_map, False, gumbel)
        else:
            from jTransUP.models import transUP as tu
            m = tu.TransUPModel(l1, Dm, NU, NI, NR, gumbel)
        m.eval(); m.disable_grad()
        return m
    g_off, g_ids = csr([rng.choice(NI, size=rng.randint(0, 9), replace=False).astype(np.int32) for _ in range(NU)])
    f_off, f_ids = csr([rng.choice(NI, size=25, replace=False).astype(np.int32) for _ in range(NU)])
    m = make(False, False)
    want = ops().eval_pref_ranks(m.user_embeddings.weight, users, m.prepare_items(), False, g_off, g_ids, f_off, f_ids)
    assert want is not None and int(want.max()) > 0
    assert torch.equal(m.rank_items(users, None, g_off, g_ids, f_off, f_ids), want)
    assert torch.equal(m.rank_items(users, m.prepare_items(), g_off, g_ids, f_off, f_ids), want)
    assert make(False, True).rank_items(users, None, g_off, g_ids, f_off, f_ids) is None
    assert make(True, False).rank_items(users, None, g_off, g_ids, f_off, f_ids) is None
