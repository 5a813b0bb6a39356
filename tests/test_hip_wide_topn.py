"""The wide-list evaluation passes (ktup_eval_dot_topk_wide, ktup_eval_cfkg_topk_wide: a user's top-n list as two or four 16-key
segments, cut-offs up to 64) on the GPU: the inner-product pass bit for bit against the matrix route, which has no cap; any split
request; the wide list code against the narrow one at topn <= 16; prefixes; orders and filters that drive the merge network to its
corners; CFKG judged by the fp64 referee of tests/test_hip_cfkg_pass.py; the models through the drivers (eager, captured, replayed)
and the command line at -topn 20."""
import logging
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from tests.synth import make_dataset
from tests.test_hip_cfkg_pass import NR, SHAPES as CFKG_SHAPES, case as cfkg_case, referee
from tests.test_hip_dot_pass import case as dot_case, matrix_route

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'joint-kg-recommender_amd')

# (d, users, items, nq): catalogues shorter than topn (5, 33 items: -1 / 0.f tails), a ragged last wave and two user blocks (70
# queries), a short last tile (531 = 33 tiles + 11), the element-wise load path (d = 37, 12), the widest geometry (d = 256)
SHAPES = [(64, 300, 177, 65), (37, 90, 33, 1), (100, 70, 5, 63), (256, 40, 130, 17), (12, 70, 531, 70)]
# the first key of each further segment, every segment boundary, the full list
TOPNS = [17, 20, 32, 33, 48, 49, 64]


def ops():
    from jTransUP.hip import ops as o
    return o


def inputs(shape):
    """(U, I, u, user_add, item_add, f_off, f_ids) of tests/test_hip_dot_pass.py's `case` for a (d, users, items, nq): they do not
    depend on the cut-off that rides in its shape tuples (15: none of its MANY_SPLITS shapes, so the filter lists are `filters`':
    query 1 filtered completely, query 2 with an empty list)."""
    return dot_case(shape + (15,))[:7]


def same(got, want):
    assert got[0].dtype == torch.int32 and got[0].shape == want[0].shape
    assert torch.equal(got[0], want[0])
    assert torch.equal(got[1], want[1])


# ------------------------------------------------------------------------------------------ 1. the matrix route, bit for bit
@pytest.mark.parametrize('topn', TOPNS)
@pytest.mark.parametrize('shape', SHAPES)
def test_dot_pass_is_the_matrix_route_bit_for_bit(shape, topn):
    d, nu, ni, nq = shape
    U, I, u, ua, ia, f_off, f_ids = inputs(shape)
    for terms in (False, True):
        for filt in (False, True):
            args = (f_off if filt else None, f_ids if filt else None, ua if terms else None, ia if terms else None)
            want = matrix_route(U, I, u, topn, *args)
            got = ops().eval_dot_topk_wide(U, I, u, topn, *args, with_scores=True)
            assert tuple(got[0].shape) == (nq, topn)
            same(got, want)
            if filt and nq > 2:
                assert bool((got[0][1] == -1).all())                          # query 1: everything filtered
            if ni < topn:
                assert bool((got[0][:, ni:] == -1).all()) and bool((got[1][:, ni:] == 0).all())
            only = ops().eval_dot_topk_wide(U, I, u, topn, *args)
            assert torch.equal(only, want[0])                                 # top_scores == NULL


# ------------------------------------------------------------------------------------------ 2. any split request
@pytest.mark.parametrize('nsplit', [0, 1, 3, 8, 17, 32])
@pytest.mark.parametrize('topn', [17, 64])
@pytest.mark.parametrize('ni', [531, 499])
def test_the_same_lists_whatever_the_split_request(ni, topn, nsplit):
    U, I, u, ua, ia, f_off, f_ids = dot_case((12, 70, ni, 70, 16))[:7]       # (a MANY_SPLITS shape there: filters_all_but_two)
    want = matrix_route(U, I, u, topn, f_off, f_ids, ua, ia)
    got = ops().eval_dot_topk_wide(U, I, u, topn, f_off, f_ids, ua, ia, with_scores=True, nsplit=nsplit)
    same(got, want)
    assert sorted(got[0][1].tolist()[:2]) == [7, ni - 2] and got[0][1].tolist()[2:] == [-1] * (topn - 2)   # query 1 keeps two items
    assert got[1][1].tolist()[2:] == [0.0] * (topn - 2)


# ------------------------------------------------------------------------------------------ 3. the wide list code against the narrow
@pytest.mark.parametrize('topn', [1, 10, 16])
def test_wide_lists_return_the_narrow_lists_bits(topn):
    for shape in (SHAPES[0], SHAPES[4]):
        U, I, u, ua, ia, f_off, f_ids = inputs(shape)
        for nsplit in (0, 3):
            narrow = ops().eval_dot_topk(U, I, u, topn, f_off, f_ids, ua, ia, with_scores=True, nsplit=nsplit)
            same(ops().eval_dot_topk_wide(U, I, u, topn, f_off, f_ids, ua, ia, with_scores=True, nsplit=nsplit), narrow)
    for l1 in (True, False):
        c = cfkg_case(CFKG_SHAPES[1], l1)
        f_off, f_ids, _ = c['filt']['sub']
        args = (c['U'], c['R'], NR - 1, c['E'], c['u'], topn, l1)
        kw = dict(cand_ids=c['cand'], filt_off=f_off, filt_ids=f_ids, with_scores=True)
        same(ops().eval_cfkg_topk_wide(*args, **kw), ops().eval_cfkg_topk(*args, **kw))


# ------------------------------------------------------------------------------------------ 4. prefixes
def test_a_shorter_list_is_the_prefix_of_the_full_one():
    for shape in (SHAPES[0], SHAPES[4]):
        U, I, u, ua, ia, f_off, f_ids = inputs(shape)
        full = ops().eval_dot_topk_wide(U, I, u, 64, f_off, f_ids, ua, ia, with_scores=True)
        for k in (17, 33, 50):
            part = ops().eval_dot_topk_wide(U, I, u, k, f_off, f_ids, ua, ia, with_scores=True)
            same(part, (full[0][:, :k], full[1][:, :k]))


# ------------------------------------------------------------------------------------------ 5. adversarial orders
NQ, NI, D = 70, 531, 12


def _ordered_world(kind):
    """70 users x 531 items, d = 12, all table entries positive, item row j = c_j x one base row: every user's score moves with c_j."""
    gen = torch.Generator().manual_seed(29)
    U = (torch.rand(NQ, D, generator=gen) + 0.5)
    base = torch.rand(48, D, generator=gen) + 0.5
    j = torch.arange(NI, dtype=torch.float32)
    if kind == 'rising':                       # every tile holds 16 candidates for every user: the maximum of merges
        I = base[:1] * (1.0 + j / 64.0)[:, None]
    elif kind == 'falling':                    # after the first topn items nothing is a candidate
        I = base[:1] * (1.0 + (NI - j) / 64.0)[:, None]
    else:                                      # row j = row j - 48: exact ties across tiles, segments and splits
        I = base[torch.arange(NI) % 48]
    u = torch.randperm(NQ, generator=gen)
    return U.to(DEV), I.contiguous().to(DEV), u.to(DEV)


@pytest.mark.parametrize('topn', [20, 64])
@pytest.mark.parametrize('kind,nsplits', [('rising', (0,)), ('falling', (0,)), ('ties', (1, 8))])
def test_orders_that_corner_the_merge(kind, nsplits, topn):
    U, I, u = _ordered_world(kind)
    want = matrix_route(U, I, u, topn, None, None, None, None)
    if kind == 'rising':
        assert want[0][0].tolist() == list(range(NI - 1, NI - 1 - topn, -1))
    elif kind == 'falling':
        assert want[0][0].tolist() == list(range(topn))
    else:
        assert int((want[1][:, 1:] == want[1][:, :-1]).sum()) >= NQ * topn // 2      # ties among the best of every row ...
        tied = want[1][:, 1:] == want[1][:, :-1]
        assert bool((want[0][:, 1:][tied] > want[0][:, :-1][tied]).all())             # ... the lower id first
    for nsplit in nsplits:
        same(ops().eval_dot_topk_wide(U, I, u, topn, None, None, None, None, with_scores=True, nsplit=nsplit), want)


@pytest.mark.parametrize('topn', [20, 64])
def test_a_flush_with_more_than_16_pending(topn):
    """Rising scores and a filter that removes 7 of each user's first 16 items: the first tile leaves 9 pending, the second adds 16 --
    the flush finds 25 and runs its second round."""
    U, I, u = _ordered_world('rising')
    rng = np.random.RandomState(5)
    flat = np.concatenate([np.sort(rng.choice(16, size=7, replace=False)) for _ in range(NQ)]).astype(np.int32)
    f_off = torch.arange(0, 7 * NQ + 1, 7, dtype=torch.int64, device=DEV)
    f_ids = torch.from_numpy(flat).to(DEV)
    for nsplit in (0, 1):
        want = matrix_route(U, I, u, topn, f_off, f_ids, None, None)
        same(ops().eval_dot_topk_wide(U, I, u, topn, f_off, f_ids, None, None, with_scores=True, nsplit=nsplit), want)
    # the same with falling scores: the 9 unfiltered items of the first tile stay in every list
    U, I, u = _ordered_world('falling')
    want = matrix_route(U, I, u, topn, f_off, f_ids, None, None)
    same(ops().eval_dot_topk_wide(U, I, u, topn, f_off, f_ids, None, None, with_scores=True, nsplit=1), want)


# ------------------------------------------------------------------------------------------ 6. CFKG
@pytest.mark.parametrize('topn', [17, 33, 64])
@pytest.mark.parametrize('l1', [True, False])
@pytest.mark.parametrize('shape', [CFKG_SHAPES[0], CFKG_SHAPES[1], CFKG_SHAPES[3], CFKG_SHAPES[5]])
def test_cfkg_lists_are_right_for_the_fp64_scores(shape, l1, topn):
    """The referee, the tolerance and the rules of tests/test_hip_cfkg_pass.py, on its cases, at the wide cut-offs."""
    assert [s[:5] for s in (CFKG_SHAPES[0], CFKG_SHAPES[1], CFKG_SHAPES[3], CFKG_SHAPES[5])] == \
        [(36, 70, 53, 53, 9), (64, 300, 177, 177, 65), (100, 70, 9, 5, 63), (256, 80, 211, 150, 37)]
    c = cfkg_case(shape, l1)
    for which in ('all', 'sub'):
        cand = None if which == 'all' else c['cand']
        ref = c['ref'][which]
        f_off, f_ids, banned = c['filt'][which]
        for nsplit, filt in ((0, True), (0, False), (3, True)):
            what = '%s %s cand=%s nsplit=%d filter=%s topn=%d' % (shape, 'L1' if l1 else 'L2', which, nsplit, filt, topn)
            got = ops().eval_cfkg_topk_wide(c['U'], c['R'], NR - 1, c['E'], c['u'], topn, l1, cand_ids=cand, filt_off=f_off if filt else None,
                                            filt_ids=f_ids if filt else None, with_scores=True, nsplit=nsplit)
            ids, sc = got[0].cpu().numpy(), got[1].cpu().numpy()
            referee(ids, sc, ref, banned if filt else None, topn, what)
            if which == 'sub':
                assert not (ids == c['bad']).any(), what + ': the candidate without an entity row was ranked'
            if filt and shape[4] > 2:
                assert (ids[1] == -1).all(), what                             # query 1: everything filtered
        only = ops().eval_cfkg_topk_wide(c['U'], c['R'], NR - 1, c['E'], c['u'], topn, l1, cand_ids=cand)
        assert only.dtype == torch.int32
        referee(only.cpu().numpy(), None, ref, None, topn, '%s %s ids only topn=%d' % (shape, which, topn))


# ------------------------------------------------------------------------------------------ 7. through the drivers
@pytest.fixture
def wide_option():
    """Sets the library option eval_wide_topn for the span of a test."""
    from jTransUP.hip import lib as L
    old = L.get_option('eval_wide_topn')
    yield lambda value: L.set_option('eval_wide_topn', value)
    L.set_option('eval_wide_topn', old)


def test_bprmf_through_the_driver_eager_captured_replayed(wide_option):
    """The criterion of tests/test_hip_dot_pass.py's driver tests: the metric columns are the batch walk's, exactly."""
    from jTransUP.models import _driver as D
    from tests.test_hip_dot_pass import _world_model, _world_pass
    m, nu, ni = _world_model('bprmf')
    gold, train, batches, score_fn, pass_fn = _world_pass(m, nu, ni, seed=8)
    index = D.rank_index(batches, gold, [train])
    FL = types.SimpleNamespace(topn=20)
    wide_option(0)
    assert pass_fn(D.ids([u for b in batches for u in b]), None, None, 20) is None      # the walk stays above 16 ...
    assert pass_fn(D.ids([u for b in batches for u in b]), None, None, 10) is not None  # ... and only there
    wide_option(1)
    walk = D.rec_eval_pass(FL, score_fn, batches, gold, [train], True, want_rows=False)
    assert walk.shape == (sum(1 for u in range(nu) if u % 9), 5)
    key = D.model_graph_key(m)
    for step in range(3):
        got = D.rec_eval_pass(FL, score_fn, batches, gold, [train], True, want_rows=False, pass_fn=pass_fn, graph_key=key,
                              pass_descending=True)
        np.testing.assert_array_equal(got, walk)
        entry = D._EVAL_GRAPHS[(id(batches), id(index), 20, key)]
        assert (entry[0] is None) == (step == 0)                              # eager once, then a graph: captured, then replayed
    first = entry[1]
    D.rec_eval_pass(FL, score_fn, batches, gold, [train], True, want_rows=False, pass_fn=pass_fn, graph_key=key, pass_descending=True)
    assert D._EVAL_GRAPHS[(id(batches), id(index), 20, key)][1] is first      # the same tensor on the next pass


@pytest.mark.parametrize('l1', [True, False])
def test_cfkg_through_the_driver_eager_captured_replayed(l1, monkeypatch, wide_option):
    """The criterion of tests/test_hip_cfkg_pass.py's driver test: rows = the metrics of the pass's own lists; means within 2 / nq of
    the batch walk's."""
    from jTransUP.models import _driver as Dr
    from jTransUP.models import knowledgable_recommendation as K
    from tests.test_hip_cfkg_pass import NI as WNI, NU as WNU, _spy, _world
    m, i_map, gold, train, batches = _world(l1, seed=19)
    seen = _spy(monkeypatch, m)
    FL = types.SimpleNamespace(topn=20, share_embeddings=True)
    log = logging.getLogger('cfkg-wide')
    monkeypatch.delenv('KTUP_EVAL_GRAPH', raising=False)
    monkeypatch.delenv('KTUP_EVAL_PASS', raising=False)
    wide_option(0)
    K.evaluateRec(FL, m, batches, gold, [train], i_map, log, eval_descending=False)
    assert seen['topk'] == 1 and seen['lists'] is None and seen['walk'] == len(batches)       # declined: the batch walk
    walk = seen['rows'].copy()
    wide_option(1)
    rows = []
    for k in range(3):
        K.evaluateRec(FL, m, batches, gold, [train], i_map, log, eval_descending=False)
        rows.append(seen['rows'].copy())
    assert seen['walk'] == len(batches) and seen['topk'] == 3                 # eager once, once under capture, then a replay
    lists = seen['lists'].cpu().numpy()
    assert lists.shape == (WNU, 20) and (lists >= 0).all() and (lists < WNI).all()
    idx = Dr.rank_index(batches, gold, [train])
    again = ops().rec_metrics(torch.from_numpy(lists.copy()).to(DEV), idx.g_off, idx.g_ids).cpu().numpy()
    np.testing.assert_array_equal(rows[0], again[[u in gold for u in range(WNU)]])
    np.testing.assert_array_equal(rows[1], rows[0])
    np.testing.assert_array_equal(rows[2], rows[0])
    nq = len(rows[0])
    assert walk.shape == rows[0].shape
    assert (np.abs(rows[0].mean(0) - walk.mean(0)) <= 2.0 / nq).all()         # one near-tie swap moves a mean by at most 1 / nq
    graphs = [v for v in Dr._EVAL_GRAPHS.values() if v[2] is batches]
    assert len(graphs) == 1 and graphs[0][0] is not None


# ------------------------------------------------------------------------------------------ 8. command line
def _eval_lines(data, name, env):
    logs = os.path.join(data, 'log')
    os.makedirs(logs, exist_ok=True)
    cmd = [sys.executable, os.path.join(PKG, 'run_item_recommendation.py'), '-data_path', data, '-log_path', logs, '-dataset', 'ml1m',
           '-experiment_name', name, '-nohas_visualization', '-batch_size', '32', '-embedding_size', '36', '-seed', '3',
           '-eval_interval_steps', '6', '-training_steps', '12', '-early_stopping_steps_to_wait', '0', '-learning_rate', '0.05',
           '-topn', '20', '-model_type', 'bprmf', '-rec_test_files', 'valid.dat']
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
