"""The preference-space evaluation pass of TUP / KTUP at embedding size 256 (ktup_eval_pref_topk / ktup_eval_pref_topk_wide with
d = 256; library option eval_q256) on the GPU: the C entry points themselves, a referee that judges every row and slot against the
matrix route's fp32 scores of all pairs, the list forms against each other with no tolerance (narrow = wide up to 16, prefixes, any
split count), item orders, ties and filters that drive the merge network to its corners, what the option does to the bare wrappers,
and both models through the driver (eager, captured, replayed, the option toggled between passes).

World, referee, judge and ordered_world are those of tests/test_hip_pref_wide_topn.py, restated for this width."""
import functools
import types

import numpy as np
import pytest
import torch

from oracle import cpu_ref as O
from jTransUP.hip import lib as L

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# (d, users, items, nq, P).  64-user workgroups, 16-user waves, 16-item tiles; QGeom<64, NP> with NP = 1 (P <= 4), 5 (P <= 20), 8 (P <= 32).
Q256_SHAPES = [(256, 300, 177, 65, 20),      # two user blocks, a last wave with one user, 11 tiles + 1 item
               (256, 70, 5, 63, 20),         # a catalogue shorter than every cut-off: tails of -1 / 0.f
               (256, 90, 33, 1, 4),          # one query, NP = 1 (the matrix-core row kernel), two tiles + 1 item
               (256, 90, 211, 37, 5),        # first P of NP = 5
               (256, 90, 211, 37, 21),       # first P of NP = 8
               (256, 90, 211, 37, 32)]       # last P of NP = 8
# the narrow list, both segment counts of the wide one, every segment boundary
TOPNS = [1, 10, 16, 17, 32, 33, 64]


def ops():
    from jTransUP.hip import ops as o
    return o


def dv(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def csr(filt):
    off = dv(np.concatenate([[0], np.cumsum([len(f) for f in filt])]).astype(np.int64))
    flat = np.concatenate(filt).astype(np.int32) if sum(len(f) for f in filt) else np.zeros(0, np.int32)
    return off, dv(flat)


class World(object):
    """Tables, queries and filter lists of a shape, with the item sides and the matrix route's scores computed once and shared."""

    def __init__(self, d, nu, ni, nq, P, seed=0):
        gen = torch.Generator().manual_seed(d + ni + P + seed)
        ne = 200
        mk = lambda r: O.make_table(r, d, gen).to(DEV)
        self.d, self.ni, self.nq, self.P = d, ni, nq, P
        self.U, self.I = mk(nu), mk(ni)
        self.E = torch.cat([O.make_table(ne, d, gen), torch.zeros(1, d)]).to(DEV)
        self.Pm, self.Pn, self.R, self.Rn = mk(P), mk(P), mk(P), mk(P)
        self.i2e = torch.randint(0, ne + 1, (ni,), generator=gen).to(DEV, torch.int32)
        self.u = torch.randperm(nu, generator=gen)[:nq].to(DEV)
        rng = np.random.RandomState(ni + seed)
        # random sizes, query 1 filtered completely, query 2 with an empty list
        self.filt = [np.sort(rng.choice(ni, size=min(ni, int(rng.randint(0, 170))), replace=False)).astype(np.int32) for _ in range(nq)]
        if nq > 2:
            self.filt[1] = np.arange(ni, dtype=np.int32)
            self.filt[2] = np.zeros(0, np.int32)
        self._items, self._mat = {}, {}
        self.set_filters(self.filt)

    def set_filters(self, filt):
        self.filt = filt
        self.f_off, self.f_ids = csr(filt)

    def items(self, ktup):
        if ktup not in self._items:
            self._items[ktup] = ops().eval_pref_items(self.I, self.E if ktup else None, self.Pm, self.Pn, self.R if ktup else None,
                                                      self.Rn if ktup else None, self.i2e if ktup else None)
        return self._items[ktup]

    def matrix(self, ktup):
        """The matrix route (soft gate, squared L2): eval_tup / eval_ktup over ALL users in one call (fp32, (nq, ni)); never modified."""
        if ktup not in self._mat:
            G = ops()
            if ktup:
                m = G.eval_ktup(self.U, self.I, self.E, self.Pm, self.Pn, self.R, self.Rn, self.i2e, self.u, False, G.GUMBEL_OFF, None, 0, 0,
                                items=self.items(True))
            else:
                m = G.eval_tup(self.U, self.I, self.Pm, self.Pn, self.u, False, G.GUMBEL_OFF, None, 0, 0, items=self.items(False))
            self._mat[ktup] = m
        return self._mat[ktup]


@functools.lru_cache(maxsize=None)
def world(shape):
    return World(*shape)


def same(got, want):
    assert got is not None
    assert got[0].dtype == torch.int32 and got[0].shape == want[0].shape
    assert torch.equal(got[0], want[0])
    assert torch.equal(got[1], want[1])


@pytest.fixture
def q256_option():
    old = L.get_option('eval_q256')
    yield lambda value: L.set_option('eval_q256', value)
    L.set_option('eval_q256', old)


@pytest.fixture
def nsplit_option():
    old = L.get_option('eval_nsplit')
    yield lambda value: L.set_option('eval_nsplit', value)
    L.set_option('eval_nsplit', old)


def c_entry(w, ktup, topn, wide, filt=True):
    """ktup_eval_pref_topk / ktup_eval_pref_topk_wide called directly; any status but KTUP_OK raises, by name."""
    G = ops()
    entry = 'ktup_eval_pref_topk_wide' if wide else 'ktup_eval_pref_topk'
    items = w.items(ktup)
    I, E = items.I, items.E
    fo, fi = G._no_empty_filter(w.f_off, w.f_ids) if filt else (None, None)
    top = torch.full((w.nq, topn), -7, dtype=torch.int32, device=DEV)
    ts = torch.full((w.nq, topn), -7.0, dtype=torch.float32, device=DEV)
    ws = G._scratch(getattr(L.load(), entry + '_workspace_bytes')(w.d, w.P, w.nq, w.ni, topn), w.U.device)
    p = G._p
    L.call(entry, p(w.U), w.U.stride(0), p(I), I.stride(0), p(E), 0 if E is None else E.stride(0), p(items.item2ent), p(items.pws), w.P,
           w.d, p(w.u), w.nq, w.ni, 0, p(fo), p(fi), topn, p(top), p(ts), p(ws), G._stream(w.U.device))
    return top, ts


def q_pass(w, ktup, topn, filt=True, wide=True):
    """The pass through the wrappers (option eval_q256 = 1 set by the caller)."""
    G = ops()
    fo, fi = (w.f_off, w.f_ids) if filt else (None, None)
    got = (G.eval_pref_topk_wide if wide else G.eval_pref_topk)(w.U, w.u, w.items(ktup), False, topn, fo, fi, with_scores=True)
    assert got is not None
    return got


# ------------------------------------------------------------------------------------------ the referee
def tol(s):
    """tests/test_hip_eval.py's _same_lists_up_to_rounding holds the pass to rtol = atol = 2e-5 against the matrix route at d <= 128.
    Twice that here: the longest product grows from K = 128 + 64 to 256 + 64, and the worst-case error of a fp32 dot grows linearly
    with its length.  The matrix route itself is within 4e-7 of an fp64 evaluation on these worlds (unit-norm rows, scores 1.4 .. 2.9)."""
    return 4e-5 * np.abs(s) + 4e-5


def referee(ids, scores, ref, banned, topn, what):
    """ids / scores: (nq, topn) of the pass; ref: (nq, ni) reference scores of ALL pairs; banned: per query the filtered item ids (or
    None).  Every row, every slot is judged; a near-tie swap passes on its own, nothing else does."""
    nq, ni = ref.shape
    assert ids.shape == (nq, topn) and ids.dtype == np.int32 and scores.shape == (nq, topn) and scores.dtype == np.float32, what
    for b in range(nq):
        ok = np.ones(ni, bool)
        if banned is not None and len(banned[b]):
            ok[banned[b]] = False
        n = min(topn, int(ok.sum()))
        row, sc = ids[b], scores[b]
        # the -1 / 0.f tail exactly where fewer than topn unfiltered items exist
        assert (row[n:] == -1).all() and (sc[n:] == 0.0).all() and (row[:n] >= 0).all() and (row[:n] < ni).all(), (what, b, row, n)
        got = row[:n].astype(np.int64)
        assert len(set(got.tolist())) == n, (what, b, 'repeated ids', row)
        assert ok[got].all(), (what, b, 'a filtered item', row)
        sc = sc[:n]
        assert (sc[1:] >= sc[:-1]).all(), (what, b, 'scores not ascending', sc)
        tie = sc[1:] == sc[:-1]
        assert (got[1:][tie] > got[:-1][tie]).all(), (what, b, 'equal scores: lower id first', row, sc)
        mine = ref[b, got].astype(np.float64)
        assert (np.abs(sc.astype(np.float64) - mine) <= tol(mine)).all(), (what, b, sc, mine)
        if n:
            out = ok.copy()
            out[got] = False
            last = float(sc[-1])
            better = out & (ref[b] < last - tol(last))
            assert not better.any(), (what, b, 'a better item was left out', np.nonzero(better)[0], last)


def judge_lists(w, ktup, got, topn, filt, what):
    ref = w.matrix(ktup).cpu().numpy()
    referee(got[0].cpu().numpy(), got[1].cpu().numpy(), ref, w.filt if filt else None, topn, what)


def judge(w, ktup, topn, filt, what):
    judge_lists(w, ktup, q_pass(w, ktup, topn, filt), topn, filt, what)


def largest_error_ratio(shape):
    """max |pass - matrix| / (2e-5 |s| + 2e-5) over every (user, item) score the unfiltered 64-key lists of TUP and KTUP hold: in
    units of the bound the pass is held to at d <= 128 (the referee's is 2 of them).  For tools/pref_q256_time.py's report."""
    w = world(shape)
    worst = 0.0
    for ktup in (False, True):
        ids, sc = c_entry(w, ktup, 64, True, filt=False)
        ids, sc = ids.cpu().numpy().astype(np.int64), sc.cpu().numpy().astype(np.float64)
        ref = w.matrix(ktup).cpu().numpy().astype(np.float64)
        for b in range(w.nq):
            live = ids[b] >= 0
            mine = ref[b, ids[b][live]]
            if live.any():
                worst = max(worst, float((np.abs(sc[b][live] - mine) / (2e-5 * np.abs(mine) + 2e-5)).max()))
    return worst


# ------------------------------------------------------------------------------------------ 1. the C entry points
@pytest.mark.parametrize('shape', Q256_SHAPES)
def test_c_entry_points_take_d_256(shape):
    """No option is involved: the entry points answer KTUP_OK at d = 256 (before this pass existed: KTUP_ERR_UNSUPPORTED, 'no fused
    pass kernel for d=256 ...') and their lists stand before the referee."""
    w = world(shape)
    for ktup in (False, True):
        for filt in (True, False):
            for wide, topn in ((False, 10), (False, 16), (True, 10), (True, 20), (True, 64)):
                judge_lists(w, ktup, c_entry(w, ktup, topn, wide, filt), topn, filt, (shape, ktup, filt, wide, topn))


# ------------------------------------------------------------------------------------------ 2. the referee, every cut-off
@pytest.mark.parametrize('topn', TOPNS)
@pytest.mark.parametrize('shape', Q256_SHAPES)
def test_lists_are_those_of_the_matrix_route_scores(shape, topn, q256_option):
    q256_option(1)
    w = world(shape)
    for ktup in (False, True):
        for filt in (True, False):
            judge(w, ktup, topn, filt, (shape, topn, ktup, filt, 'wide'))
            if topn <= 16:
                judge_lists(w, ktup, q_pass(w, ktup, topn, filt, wide=False), topn, filt, (shape, topn, ktup, filt, 'narrow'))
            if w.nq > 2 and filt:                               # query 1 is filtered completely
                got = q_pass(w, ktup, topn, True)
                assert got[0][1].tolist() == [-1] * topn and got[1][1].tolist() == [0.0] * topn


# ------------------------------------------------------------------------------------------ 3. no tolerance
@pytest.mark.parametrize('shape', Q256_SHAPES)
def test_wide_against_narrow_prefixes_and_splits(shape, q256_option, nsplit_option):
    q256_option(1)
    w = world(shape)
    for ktup in (False, True):
        for filt in (True, False):
            # (a) the wide list code against the narrow one: the same score bits, the same lists
            narrow16 = None
            for topn in (1, 10, 16):
                narrow16 = q_pass(w, ktup, topn, filt, wide=False)
                same(q_pass(w, ktup, topn, filt), narrow16)
                same(c_entry(w, ktup, topn, False, filt), narrow16)          # the wrapper did take the pass
            # (b) every topn < 64 is a prefix of the 64-key list
            full = q_pass(w, ktup, 64, filt)
            for k in (1, 10, 16, 17, 20, 32, 33, 48, 49, 63):
                same(q_pass(w, ktup, k, filt), (full[0][:, :k].contiguous(), full[1][:, :k].contiguous()))
            same((full[0][:, :16].contiguous(), full[1][:, :16].contiguous()), narrow16)
            # (c) any split count
            for n in (1, 3, 8, 0):
                nsplit_option(n)
                same(q_pass(w, ktup, 64, filt), full)
                same(q_pass(w, ktup, 20, filt), (full[0][:, :20].contiguous(), full[1][:, :20].contiguous()))
                same(q_pass(w, ktup, 16, filt, wide=False), narrow16)


# ------------------------------------------------------------------------------------------ 4. orders that corner the merge
ORDER_SHAPE = (256, 64, 300, 64, 20)                        # one user block; 300 items = 18 tiles + 12 items


@functools.lru_cache(maxsize=None)
def ordered_world(order, ktup):
    """A d = 256 world whose item rows are permuted by the FIRST query's matrix-route scores so that, for that user, they fall
    ('falling': every item is a candidate and every tile fills the pending row) or rise with the item id; then 40 item rows (and
    their item2ent entries) are duplicated 150 ids further on -- equal rows give equal score bits, so the lower id must come first,
    across a split boundary too."""
    w = World(*ORDER_SHAPE, seed=1)
    w.u = torch.arange(w.nq).to(DEV)
    first = w.matrix(ktup)[0]
    perm = torch.argsort(first, descending=(order == 'falling'), stable=True)
    w.I, w.i2e = w.I[perm].contiguous(), w.i2e[perm].contiguous()
    src = torch.from_numpy(np.random.RandomState(4).choice(150, size=40, replace=False)).to(DEV)
    w.I[src + 150] = w.I[src]
    w.i2e[src + 150] = w.i2e[src]
    w._items, w._mat = {}, {}
    w.src = src.cpu().numpy()
    return w


@pytest.mark.parametrize('ktup', [False, True])
@pytest.mark.parametrize('order', ['falling', 'rising'])
def test_orders_and_ties_that_corner_the_merge(order, ktup, q256_option, nsplit_option):
    q256_option(1)
    w = ordered_world(order, ktup)
    ref = w.matrix(ktup)
    assert torch.equal(ref[:, w.src], ref[:, w.src + 150])                      # the duplicated rows do score the same bits
    for n in (1, 8, 0):
        nsplit_option(n)
        for topn in (10, 20, 64):
            judge(w, ktup, topn, True, (order, ktup, n, topn, 'filtered'))
            judge(w, ktup, topn, False, (order, ktup, n, topn))
        # the pass's own scores of a duplicated pair are equal bits too, so the pair sits in the list lower id first (the referee's
        # tie rule then bites): seen from the 64-key lists
        ids, sc = (t.cpu().numpy() for t in q_pass(w, ktup, 64, False))
        pairs = 0
        for b in range(w.nq):
            pos = {int(i): k for k, i in enumerate(ids[b])}
            for s in w.src:
                if int(s) in pos and int(s) + 150 in pos:
                    assert pos[int(s) + 150] == pos[int(s)] + 1 and sc[b][pos[int(s)]] == sc[b][pos[int(s)] + 1], (order, ktup, n, b, s)
                    pairs += 1
        assert pairs > 0


@pytest.mark.parametrize('ktup', [False, True])
def test_a_flush_with_more_than_sixteen_pending(ktup, q256_option, nsplit_option):
    """The falling order with filters that ban every item except the last 40 (ids 260 .. 299).  Such a user's pending row stays
    empty while its neighbours fill and flush theirs at every tile; then tile 16 (items 256 .. 271) brings it 12 candidates and tile
    17 sixteen more.  User 22 -- alone with this filter in its register slot -- is merged early by its neighbours' flushes, while
    users 1, 5, 9 and 13 -- a whole slot of wave 0 -- reach their flush with 28 pending: the merge's second round (n > 16).  One
    split, so that a row sees all three tiles."""
    q256_option(1)
    w = ordered_world('falling', ktup)
    old = w.filt
    late = np.arange(260, dtype=np.int32)
    try:
        w.set_filters([late if b in (1, 5, 9, 13, 22) else f for b, f in enumerate(old)])
        for n in (1, 0):
            nsplit_option(n)
            for topn, wide in ((16, False), (20, True), (64, True)):
                got = q_pass(w, ktup, topn, True, wide=wide)
                judge_lists(w, ktup, got, topn, True, ('late rows', ktup, n, topn))
                ids = got[0].cpu().numpy()
                for b in (1, 5, 9, 13, 22):
                    live = ids[b][:min(topn, 40)]
                    assert (live >= 260).all() and (ids[b][40:] == -1).all(), (b, ids[b])
    finally:
        w.set_filters(old)


# ------------------------------------------------------------------------------------------ 5. what the option does
def test_option_picks_the_route_of_the_bare_wrappers(q256_option):
    G = ops()
    w = world(Q256_SHAPES[0])
    for ktup in (False, True):
        mat = w.matrix(ktup)
        for topn, fn, wide in ((10, G.eval_pref_topk, False), (10, G.eval_pref_topk_wide, True), (20, G.eval_pref_topk_wide, True)):
            want = G.topk_filtered(mat, False, topn, w.f_off, w.f_ids, with_scores=True)
            for value in (0, -1):                               # the pair kernel's sweep: the matrix route's bits, as before
                q256_option(value)
                same(fn(w.U, w.u, w.items(ktup), False, topn, w.f_off, w.f_ids, with_scores=True), want)
            q256_option(1)                                      # the pass: the C entry point's lists
            got = fn(w.U, w.u, w.items(ktup), False, topn, w.f_off, w.f_ids, with_scores=True)
            same(got, c_entry(w, ktup, topn, wide))
            ids = fn(w.U, w.u, w.items(ktup), False, topn, w.f_off, w.f_ids)                   # top_scores absent
            assert torch.is_tensor(ids) and torch.equal(ids, got[0])
            # (the two routes sum in another association: were every score bit equal, the option would show nothing here)
            assert not torch.equal(got[1], want[1])
    # no effect at another width
    w100 = World(100, 90, 211, 37, 20)
    for ktup in (False, True):
        for topn, fn in ((10, G.eval_pref_topk), (20, G.eval_pref_topk_wide)):
            lists = []
            for value in (-1, 0, 1):
                q256_option(value)
                lists.append(fn(w100.U, w100.u, w100.items(ktup), False, topn, w100.f_off, w100.f_ids, with_scores=True))
            same(lists[1], lists[0])
            same(lists[2], lists[0])
    # eval_mc = 0 keeps the pass off whatever eval_q256 says
    q256_option(1)
    old = L.set_option('eval_mc', 0)
    try:
        got = G.eval_pref_topk(w.U, w.u, w.items(False), False, 10, w.f_off, w.f_ids, with_scores=True)
    finally:
        L.set_option('eval_mc', old)
    same(got, G.topk_filtered(w.matrix(False), False, 10, w.f_off, w.f_ids, with_scores=True))


# ------------------------------------------------------------------------------------------ 6. through the driver
@pytest.mark.parametrize('ktup', [False, True])
def test_models_through_the_driver_eager_captured_replayed(ktup, q256_option, monkeypatch):
    """TUP and KTUP with the soft gate and squared L2 at embedding size 256, FLAGS.topn = 20 (the wide list) and 10 (the narrow one)."""
    from jTransUP.models import _driver as D
    monkeypatch.delenv('KTUP_EVAL_GRAPH', raising=False)
    monkeypatch.delenv('KTUP_EVAL_PASS', raising=False)
    old_wide = L.set_option('eval_wide_topn', 1)
    try:
        torch.manual_seed(11)
        rng = np.random.RandomState(11)
        NU, NI, NE, NR, Dm = 300, 177, 150, 7, 256
        if ktup:
            from jTransUP.models import jTransUP as jt
            i_map = {i: i for i in range(NI)}
            new_map = {i: ((i * 3) % NE if i % 5 else -1, i) for i in range(NI)}
            m = jt.jTransUPModel(False, Dm, NU, NI, NE, NR, i_map, new_map, False, False)
            score_fn = lambda u: m.evaluateRec(u)
        else:
            from jTransUP.models import transUP as tu
            m = tu.TransUPModel(False, Dm, NU, NI, NR, False)
            score_fn = lambda u: m.evaluate(u)
        m.eval(); m.disable_grad()
        users = list(range(NU))
        gold = {u: set(rng.choice(NI, size=rng.randint(1, 9), replace=False).tolist()) for u in users if u % 9}
        train = {u: set(rng.choice(NI, size=25, replace=False).tolist()) for u in users}
        batches = [users[s:s + 64] for s in range(0, NU, 64)]
        index = D.rank_index(batches, gold, [train])
        pass_fn = lambda u, fo, fi, n: m.evaluate_topk(u, m.prepare_items(), n, fo, fi)
        allu = D.ids(users)
        present = [u in gold for u in users]
        G = ops()

        def direct(topn, model_call):
            """The lists of a direct wrapper call under the option as it is set."""
            fn = G.eval_pref_topk if topn <= 16 else G.eval_pref_topk_wide
            return fn(m.user_embeddings.weight, allu, m.prepare_items(), False, topn, index.f_off, index.f_ids, model_call=model_call)

        for topn in (20, 10):
            FL = types.SimpleNamespace(topn=topn)
            walk = D.rec_eval_pass(FL, score_fn, batches, gold, [train], False, want_rows=False)
            D._EVAL_GRAPHS.clear()
            q256_option(1)
            key1 = D.model_graph_key(m)
            assert key1 is not None
            rows = []
            for step in range(3):
                got = D.rec_eval_pass(FL, score_fn, batches, gold, [train], False, want_rows=False, pass_fn=pass_fn, graph_key=key1,
                                      pass_descending=False)
                rows.append(np.array(got, copy=True))
                entry = D._EVAL_GRAPHS[(id(batches), id(index), topn, key1)]
                assert (entry[0] is None) == (step == 0)                          # eager once, then a graph: captured, then replayed
            np.testing.assert_array_equal(rows[1], rows[0])
            np.testing.assert_array_equal(rows[2], rows[0])
            lists = pass_fn(allu, index.f_off, index.f_ids, topn)
            assert lists.shape == (NU, topn) and int(lists.min()) >= 0 and int(lists.max()) < NI
            assert torch.equal(lists, direct(topn, False))                        # option 1: the bare wrapper takes the pass too
            np.testing.assert_array_equal(rows[0], G.rec_metrics(lists, index.g_off, index.g_ids).cpu().numpy()[present])
            # the option toggled: another key, so the first pass on the other route is eager -- the captured graph is not replayed
            q256_option(0)
            key0 = D.model_graph_key(m)
            assert key0 != key1 and (id(batches), id(index), topn, key0) not in D._EVAL_GRAPHS
            off = np.array(D.rec_eval_pass(FL, score_fn, batches, gold, [train], False, want_rows=False, pass_fn=pass_fn, graph_key=key0,
                                           pass_descending=False), copy=True)
            assert D._EVAL_GRAPHS[(id(batches), id(index), topn, key0)][0] is None
            sweep_lists = pass_fn(allu, index.f_off, index.f_ids, topn)
            assert torch.equal(sweep_lists, direct(topn, False))
            np.testing.assert_array_equal(off, G.rec_metrics(sweep_lists, index.g_off, index.g_ids).cpu().numpy()[present])
            np.testing.assert_array_equal(off, walk)                              # the pair kernel's sweep: the walk's bits
            # ... and back: the first route's graph, its rows
            q256_option(1)
            assert D.model_graph_key(m) == key1
            back = D.rec_eval_pass(FL, score_fn, batches, gold, [train], False, want_rows=False, pass_fn=pass_fn, graph_key=key1,
                                   pass_descending=False)
            np.testing.assert_array_equal(back, rows[0])
            # unset: the models follow PREF_Q256_DEFAULT, the bare wrappers keep the sweep
            q256_option(-1)
            unset = pass_fn(allu, index.f_off, index.f_ids, topn)
            assert torch.equal(unset, lists if G.PREF_Q256_DEFAULT else sweep_lists)
            assert torch.equal(direct(topn, False), sweep_lists)
    finally:
        L.set_option('eval_wide_topn', old_wide)
