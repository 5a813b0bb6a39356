"""The wide-list evaluation passes of TUP / KTUP (ktup_eval_pref_topk_wide, ktup_eval_pref_topk_hard_wide: cut-offs up to 64) on the
GPU: the soft / hard sweeps bit for bit against the matrix route, which has no cap; the preference-space pass against its narrow
form at topn <= 16, on prefixes and under any split count, and judged slot by slot by a referee against the matrix route's fp32
scores of all pairs; item orders, ties and filters that drive the merge network to its corners; the models through the drivers
(eager, captured, replayed) and the command line at -topn 20."""
import functools
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from oracle import cpu_ref as O
from jTransUP.hip import lib as L
from tests.synth import make_dataset

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'joint-kg-recommender_amd')
ERR_UNSUPPORTED = -3

# (d, users, items, nq, P).  The preference-space pass works in 64-user workgroups, 16-user waves and 16-item tiles; the soft sweep
# stages 64 items for 16 x 3 users, the hard sweep 64 items for 8 x 8 users.  A catalogue shorter than every cut-off (5 items: tails
# of -1 / 0.f), one query, two user blocks with a ragged last wave and 33 tiles + 3 items, the smallest and the largest preference
# geometry; the last two widths have no preference-space pass (soft / hard sweeps only, d = 256 through the hybrid stage).
Q_SHAPES = [(64, 300, 177, 65, 20), (100, 70, 5, 63, 20), (128, 90, 33, 1, 20), (100, 500, 531, 70, 20), (100, 90, 211, 37, 4),
            (100, 90, 211, 37, 32)]
SWEEP_ONLY = [(256, 40, 130, 17, 20), (36, 90, 177, 37, 20)]
# the first key of each further segment, every segment boundary, the full list
TOPNS = [17, 20, 32, 33, 48, 49, 64]
SEED, OFFSET = 0x1234567, 4 * 977 + 3                       # a Philox offset that is not a multiple of 4


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
        # as tests/test_hip_eval.py's _fused_pass_case: random sizes, query 1 filtered completely, query 2 with an empty list
        self.filt = [np.sort(rng.choice(ni, size=min(ni, int(rng.randint(0, 170))), replace=False)).astype(np.int32) for _ in range(nq)]
        if nq > 2:
            self.filt[1] = np.arange(ni, dtype=np.int32)
            self.filt[2] = np.zeros(0, np.int32)
        self.uniform = torch.rand(nq, ni, P, generator=gen).to(DEV) if ni <= 200 else None
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

    def noise(self, mode):
        G = ops()
        return (mode, self.uniform if mode == G.GUMBEL_INPUT else None, SEED, OFFSET) if mode != G.GUMBEL_OFF else (mode, None, 0, 0)

    def matrix(self, ktup, l1, mode, pair_kernel=False):
        """The matrix route: eval_tup / eval_ktup over ALL users in one call (fp32, (nq, ni)); never modified.  pair_kernel: with the
        library option eval_mc = 0 for this one call, i.e. the soft gate's squared-L2 scores from the pair kernel where the route
        would take its matrix-core GEMMs (d in {20, 36, 64, 100, 128})."""
        key = (ktup, l1, mode, pair_kernel)
        if key not in self._mat:
            G = ops()
            old = L.set_option('eval_mc', 0) if pair_kernel else None
            try:
                if ktup:
                    m = G.eval_ktup(self.U, self.I, self.E, self.Pm, self.Pn, self.R, self.Rn, self.i2e, self.u, l1, *self.noise(mode),
                                    items=self.items(True))
                else:
                    m = G.eval_tup(self.U, self.I, self.Pm, self.Pn, self.u, l1, *self.noise(mode), items=self.items(False))
            finally:
                if pair_kernel:
                    L.set_option('eval_mc', old)
            self._mat[key] = m
        return self._mat[key]


@functools.lru_cache(maxsize=None)
def world(shape):
    return World(*shape)


def same(got, want):
    assert got is not None
    assert got[0].dtype == torch.int32 and got[0].shape == want[0].shape
    assert torch.equal(got[0], want[0])
    assert torch.equal(got[1], want[1])


def sweep_wide(w, ktup, l1, mode, topn, filt=True, with_scores=True):
    """The soft gate through eval_pref_topk_wide (which routes L1 / other widths to the sweep), the ST-Gumbel gate through
    eval_pref_topk_hard_wide."""
    G = ops()
    fo, fi = (w.f_off, w.f_ids) if filt else (None, None)
    if mode == G.GUMBEL_OFF:
        return G.eval_pref_topk_wide(w.U, w.u, w.items(ktup), l1, topn, fo, fi, with_scores)
    return G.eval_pref_topk_hard_wide(w.U, w.u, w.items(ktup), l1, topn, *w.noise(mode), fo, fi, with_scores)


def c_status_of_the_sweep(w, ktup, l1, mode, topn):
    """The C entry point's own answer for a call the wrapper declined."""
    G = ops()
    items = w.items(ktup)
    I, E = items.I, items.E
    m, uni, seed, off = w.noise(mode)
    top = torch.empty(w.nq, topn, dtype=torch.int32, device=DEV)
    ws = G._scratch(L.load().ktup_eval_pref_topk_hard_wide_workspace_bytes(w.d, w.P, w.nq, w.ni, topn), w.U.device)
    p = G._p
    with pytest.raises(L.KtupError) as e:
        L.call('ktup_eval_pref_topk_hard_wide', p(w.U), w.U.stride(0), p(I), I.stride(0), p(E), 0 if E is None else E.stride(0),
               p(items.item2ent), p(items.pws), w.P, w.d, p(w.u), w.nq, w.ni, int(l1), int(m), p(uni), seed, off, p(w.f_off), p(w.f_ids),
               topn, p(top), None, p(ws), G._stream(w.U.device))
    return e.value.code


# ------------------------------------------------------------------------------------------ 1. soft / hard sweeps, bit for bit
def sweep_cases(shape):
    G = ops()
    d, ni = shape[0], shape[2]
    cases = [('soft L1', True, G.GUMBEL_OFF)]
    if d not in (64, 100, 128):
        cases.append(('soft L2', False, G.GUMBEL_OFF))
    cases += [('philox L1', True, G.GUMBEL_PHILOX), ('philox L2', False, G.GUMBEL_PHILOX)]
    if ni <= 200:
        cases += [('input L1', True, G.GUMBEL_INPUT), ('input L2', False, G.GUMBEL_INPUT)]
    return cases


@pytest.mark.parametrize('topn', TOPNS)
@pytest.mark.parametrize('shape', Q_SHAPES + SWEEP_ONLY)
def test_sweeps_are_the_matrix_route_bit_for_bit(shape, topn):
    """ids AND scores of eval_tup / eval_ktup over all users in one call + topk_filtered at the same topn (that route has no cap):
    the sweeps score with the pair kernels' arithmetic and the same noise positions, so nothing may differ.  One case needs the
    route told which of its two kernels to score with: the soft gate with squared L2 at d = 36, where eval_tup / eval_ktup take the
    matrix-core GEMMs (another association of the same sums; d in {20, 36, 64, 100, 128}) unless the library option eval_mc is 0.
    The sweep -- the narrow one of the parent commit too -- has the pair kernel's bits, so the reference of that case is computed
    with eval_mc = 0; the sweep itself runs under the default options like everything else here."""
    G = ops()
    w = world(shape)
    for ktup in (False, True):
        for what, l1, mode in sweep_cases(shape):
            got = sweep_wide(w, ktup, l1, mode, topn)
            if got is None:                                     # declined: never silently, and never at the widths up to 128
                assert shape[0] > 128, (what, ktup)
                assert c_status_of_the_sweep(w, ktup, l1, mode, topn) == ERR_UNSUPPORTED
                continue
            mat = w.matrix(ktup, l1, mode, pair_kernel=(what == 'soft L2' and shape[0] in (20, 36)))
            same(got, G.topk_filtered(mat, False, topn, w.f_off, w.f_ids, with_scores=True))
            if w.nq > 2:
                assert got[0][1].tolist() == [-1] * topn and got[1][1].tolist() == [0.0] * topn
            want = G.topk_filtered(mat, False, topn, with_scores=True)
            same(sweep_wide(w, ktup, l1, mode, topn, filt=False), want)
            ids = sweep_wide(w, ktup, l1, mode, topn, filt=False, with_scores=False)        # top_scores absent
            assert torch.is_tensor(ids) and torch.equal(ids, want[0])


# ------------------------------------------------------------------------------------------ 2. the preference-space pass, no tolerance
@pytest.fixture
def nsplit_option():
    old = L.get_option('eval_nsplit')
    yield lambda value: L.set_option('eval_nsplit', value)
    L.set_option('eval_nsplit', old)


def q_wide(w, ktup, topn, filt=True):
    fo, fi = (w.f_off, w.f_ids) if filt else (None, None)
    got = ops().eval_pref_topk_wide(w.U, w.u, w.items(ktup), False, topn, fo, fi, with_scores=True)
    assert got is not None
    return got


@pytest.mark.parametrize('shape', Q_SHAPES)
def test_pref_pass_wide_against_narrow_prefixes_and_splits(shape, nsplit_option):
    G = ops()
    w = world(shape)
    for ktup in (False, True):
        for filt in (True, False):
            fo, fi = (w.f_off, w.f_ids) if filt else (None, None)
            # (a) the wide list code against the narrow one: the same score bits, the same lists
            narrow16 = None
            for topn in (1, 10, 16):
                narrow16 = G.eval_pref_topk(w.U, w.u, w.items(ktup), False, topn, fo, fi, with_scores=True)
                same(q_wide(w, ktup, topn, filt), narrow16)
            # (b) prefixes of the full list
            full = q_wide(w, ktup, 64, filt)
            for k in (17, 20, 32, 33, 48, 49):
                same(q_wide(w, ktup, k, filt), (full[0][:, :k].contiguous(), full[1][:, :k].contiguous()))
            same((full[0][:, :16].contiguous(), full[1][:, :16].contiguous()), narrow16)
            # (c) any split count
            for n in (1, 3, 8):
                nsplit_option(n)
                same(q_wide(w, ktup, 64, filt), full)
                same(q_wide(w, ktup, 20, filt), (full[0][:, :20].contiguous(), full[1][:, :20].contiguous()))
            nsplit_option(0)


# ------------------------------------------------------------------------------------------ 3. the referee
def tol(s):
    """tests/test_hip_eval.py's _same_lists_up_to_rounding pins the preference-space pass's score bits against the matrix route's at
    topn <= 16 with rtol = atol = 2e-5; section 2 (a) ties the wide scores to those bits."""
    return 2e-5 * np.abs(s) + 2e-5


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


def judge(w, ktup, topn, filt, what):
    got = q_wide(w, ktup, topn, filt)
    ref = w.matrix(ktup, False, ops().GUMBEL_OFF).cpu().numpy()
    referee(got[0].cpu().numpy(), got[1].cpu().numpy(), ref, w.filt if filt else None, topn, what)


@pytest.mark.parametrize('topn', TOPNS)
@pytest.mark.parametrize('shape', Q_SHAPES)
def test_pref_pass_lists_are_those_of_the_matrix_route_scores(shape, topn):
    w = world(shape)
    for ktup in (False, True):
        for filt in (True, False):
            judge(w, ktup, topn, filt, (shape, topn, ktup, filt))


# ------------------------------------------------------------------------------------------ 4. orders that corner the merge
ORDER_SHAPE = (100, 64, 300, 64, 20)                        # one user block; 300 items = 18 tiles + 12 items


@functools.lru_cache(maxsize=None)
def ordered_world(order, l1, ktup):
    """A d = 100 world whose item rows are permuted by the FIRST query's matrix-route scores so that, for that user, they fall
    ('falling': every item is a candidate and every tile fills the pending row) or rise with the item id; then 40 item rows (and
    their item2ent entries) are duplicated 150 ids further on -- equal rows give equal score bits, so the lower id must come first,
    across a split boundary too."""
    w = World(*ORDER_SHAPE, seed=1)
    w.u = torch.arange(w.nq).to(DEV)
    first = w.matrix(ktup, l1, ops().GUMBEL_OFF)[0]
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
def test_orders_and_ties_that_corner_the_merge(order, ktup, nsplit_option):
    G = ops()
    w = ordered_world(order, False, ktup)
    ref = w.matrix(ktup, False, G.GUMBEL_OFF)
    assert torch.equal(ref[:, w.src], ref[:, w.src + 150])                      # the duplicated rows do score the same bits
    for n in (1, 8, 0):
        nsplit_option(n)
        for topn in (20, 64):
            judge(w, ktup, topn, True, (order, ktup, n, topn, 'filtered'))
            judge(w, ktup, topn, False, (order, ktup, n, topn))
    w1 = ordered_world(order, True, ktup)                                       # the L1 sweep: the matrix route's bits
    mat = w1.matrix(ktup, True, G.GUMBEL_OFF)
    for topn in (20, 64):
        same(sweep_wide(w1, ktup, True, G.GUMBEL_OFF, topn), G.topk_filtered(mat, False, topn, w1.f_off, w1.f_ids, with_scores=True))
        same(sweep_wide(w1, ktup, True, G.GUMBEL_OFF, topn, filt=False), G.topk_filtered(mat, False, topn, with_scores=True))


# ------------------------------------------------------------------------------------------ 5. a flush with more than 16 pending
@pytest.mark.parametrize('ktup', [False, True])
def test_a_flush_with_more_than_sixteen_pending(ktup, nsplit_option):
    """The falling order of section 4 with filters that ban every item except the last 40 (ids 260 .. 299).  Such a user's pending
    row stays empty while its neighbours fill and flush theirs at every tile; then tile 16 (items 256 .. 271) brings it 12
    candidates and tile 17 sixteen more.  A flush merges the four rows of a register slot (users j, j + 4, j + 8, j + 12 of a
    wave) whenever one of them holds 16, so user 22 -- alone with this filter in its slot -- is merged early by its neighbours'
    flushes, while users 1, 5, 9 and 13 -- a whole slot of wave 0 -- reach their flush with 28 pending: row_merge_pending_wide's
    second round (n > 16), with the first round's surplus keys still in the list.  One split, so that a row sees all three tiles."""
    w = ordered_world('falling', False, ktup)
    old = w.filt
    late = np.arange(260, dtype=np.int32)
    try:
        w.set_filters([late if b in (1, 5, 9, 13, 22) else f for b, f in enumerate(old)])
        for n in (1, 0):
            nsplit_option(n)
            for topn in (20, 64):
                judge(w, ktup, topn, True, ('late rows', ktup, n, topn))
                got = q_wide(w, ktup, topn)[0].cpu().numpy()
                for b in (1, 5, 9, 13, 22):
                    live = got[b][:min(topn, 40)]
                    assert (live >= 260).all() and (got[b][40:] == -1).all(), (b, got[b])
    finally:
        w.set_filters(old)


# ------------------------------------------------------------------------------------------ 6. through the drivers
@pytest.fixture
def wide_option():
    old = L.get_option('eval_wide_topn')
    yield lambda value: L.set_option('eval_wide_topn', value)
    L.set_option('eval_wide_topn', old)


@pytest.mark.parametrize('ktup', [False, True])
def test_models_through_the_driver_eager_captured_replayed(ktup, wide_option, monkeypatch):
    """TUP with the soft gate and squared L2 (the preference-space pass) and KTUP with L1 (the soft sweep) at FLAGS.topn = 20."""
    from jTransUP.models import _driver as D
    monkeypatch.delenv('KTUP_EVAL_GRAPH', raising=False)
    monkeypatch.delenv('KTUP_EVAL_PASS', raising=False)
    torch.manual_seed(11)
    rng = np.random.RandomState(11)
    NU, NI, NE, NR, Dm = 300, 177, 150, 7, 100
    if ktup:
        from jTransUP.models import jTransUP as jt
        i_map = {i: i for i in range(NI)}
        new_map = {i: ((i * 3) % NE if i % 5 else -1, i) for i in range(NI)}
        m = jt.jTransUPModel(True, Dm, NU, NI, NE, NR, i_map, new_map, False, False)
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
    FL = types.SimpleNamespace(topn=20)
    wide_option(0)
    assert pass_fn(allu, None, None, 20) is None                              # the walk stays above 16 ...
    assert pass_fn(allu, None, None, 10) is not None                          # ... and only there
    wide_option(1)
    walk = D.rec_eval_pass(FL, score_fn, batches, gold, [train], False, want_rows=False)
    assert walk.shape == (sum(1 for u in users if u % 9), 5)
    key = D.model_graph_key(m)
    assert key is not None
    D._EVAL_GRAPHS.clear()
    rows = []
    for step in range(3):
        got = D.rec_eval_pass(FL, score_fn, batches, gold, [train], False, want_rows=False, pass_fn=pass_fn, graph_key=key,
                              pass_descending=False)
        rows.append(np.array(got, copy=True))
        entry = D._EVAL_GRAPHS[(id(batches), id(index), 20, key)]
        assert (entry[0] is None) == (step == 0)                              # eager once, then a graph: captured, then replayed
    np.testing.assert_array_equal(rows[1], rows[0])
    np.testing.assert_array_equal(rows[2], rows[0])
    lists = pass_fn(allu, index.f_off, index.f_ids, 20)
    assert lists.shape == (NU, 20) and int(lists.min()) >= 0 and int(lists.max()) < NI
    again = ops().rec_metrics(lists, index.g_off, index.g_ids).cpu().numpy()
    np.testing.assert_array_equal(rows[0], again[[u in gold for u in users]])
    if ktup:                                                                  # L1: the sweep's scores are the walk's bits
        np.testing.assert_array_equal(rows[0], walk)
    # (squared L2: the preference-space pass's lists are judged by the referee above, not by the walk's means)


# ------------------------------------------------------------------------------------------ 7. command line
def _eval_lines(data, name, env):
    logs = os.path.join(data, 'log')
    os.makedirs(logs, exist_ok=True)
    cmd = [sys.executable, os.path.join(PKG, 'run_item_recommendation.py'), '-data_path', data, '-log_path', logs, '-dataset', 'ml1m',
           '-experiment_name', name, '-nohas_visualization', '-batch_size', '32', '-embedding_size', '36', '-seed', '3',
           '-eval_interval_steps', '6', '-training_steps', '12', '-early_stopping_steps_to_wait', '0', '-learning_rate', '0.05',
           '-topn', '20', '-model_type', 'transup', '-L1_flag', '-rec_test_files', 'valid.dat']
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    log = open(os.path.join(logs, name + '.log')).read()
    return re.findall(r'f1:\d\.\d+, p:\d\.\d+, r:\d\.\d+, hit:\d\.\d+, ndcg:\d\.\d+, topn:20', log)


def test_command_line_logs_the_same_metrics_at_topn_20(tmp_path):
    make_dataset(str(tmp_path))
    env = {k: v for k, v in os.environ.items() if k not in ('KTUP_EVAL_PASS', 'KTUP_EVAL_WIDE_TOPN')}
    on = _eval_lines(str(tmp_path), 'wide-on', dict(env, KTUP_EVAL_WIDE_TOPN='1'))
    off = _eval_lines(str(tmp_path), 'wide-off', dict(env, KTUP_EVAL_PASS='0'))
    assert len(on) >= 2
    assert on == off
