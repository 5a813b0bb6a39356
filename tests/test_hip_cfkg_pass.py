"""The one-sweep rec evaluation pass of CFKG (ktup_eval_cfkg_topk) on the GPU, judged by a referee on the fp64 scores of
oracle.cpu_ref.eval_cfkg_rec (gathered through cand_ids), the reference's own evaluation matrices, and the model through the joint
driver (eager, captured, replayed).

The pass's scores are the matrix route's up to fp32 rounding, not bit for bit (include/ktup_hip.h), so a list is not compared with
another list: the referee decides whether it is A right list for the fp64 scores.  With tol(s) = 1e-4 |s| + 1e-5 (the `close`
tolerance of tests/test_hip_baselines.py) a returned list is right if
  * it has the reference list's length and padding,
  * its ids are distinct, unfiltered candidates with an entity row,
  * its returned scores agree with the fp64 scores of its own ids within tol,
  * its scores are non-decreasing, equal scores ordered by lower j first,
  * no unfiltered candidate left out has an fp64 score below the list's last fp64 score by more than tol."""
import logging
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
# (d, users, entities, n_cand, nq, topn): one and several user blocks with ragged last waves, fewer candidates than topn, candidate
# counts that are no multiple of the 16-candidate tile or of a stage, d = 50 on the element-wise path, d = 256 at the widest geometry
SHAPES = [(36, 70, 53, 53, 9, 10), (64, 300, 177, 177, 65, 16), (100, 90, 16, 16, 1, 3), (100, 70, 9, 5, 63, 10),
          (100, 500, 1000, 1000, 129, 1), (256, 80, 211, 150, 37, 10), (50, 40, 60, 60, 20, 10), (20, 40, 53, 40, 9, 10),
          (128, 40, 70, 70, 17, 10), (192, 40, 70, 50, 17, 16)]
NR = 4
_CASES = {}


def ops():
    from jTransUP.hip import ops as o
    return o


def tol(s):
    return 1e-4 * np.abs(s) + 1e-5


def referee(ids, scores, ref, banned, topn, what):
    """ids / scores: (nq, topn) of the pass (scores may be None); ref: (nq, n_cand) fp64 scores, +inf where the candidate has no
    entity row; banned: per query the set of filtered j.  Every row, every slot is judged."""
    nq, n_cand = ref.shape
    assert ids.shape == (nq, topn) and ids.dtype == np.int32, what
    for b in range(nq):
        ok = np.isfinite(ref[b])
        if banned is not None and len(banned[b]):
            ok[np.fromiter(banned[b], dtype=np.int64)] = False
        n = min(topn, int(ok.sum()))
        row = ids[b]
        assert (row[n:] == -1).all() and (row[:n] >= 0).all() and (row[:n] < n_cand).all(), (what, b, row, n)
        got = row[:n].astype(np.int64)
        assert len(set(got.tolist())) == n, (what, b, 'repeated ids', row)
        assert ok[got].all(), (what, b, 'a filtered candidate or one without an entity row', row)
        mine = ref[b, got]
        if scores is not None:
            assert (scores[b, n:] == 0.0).all(), (what, b, 'padding scores')
            sc = scores[b, :n]
            assert (np.abs(sc.astype(np.float64) - mine) <= tol(mine)).all(), (what, b, sc, mine)
            assert (sc[1:] >= sc[:-1]).all(), (what, b, 'scores not ascending', sc)
            same = sc[1:] == sc[:-1]
            assert (got[1:][same] > got[:-1][same]).all(), (what, b, 'equal scores: lower j first', row, sc)
        else:
            assert (mine[1:] >= mine[:-1] - tol(mine[:-1])).all(), (what, b, 'fp64 scores of the list not ascending', mine)
        if n:
            out = ok.copy()
            out[got] = False
            last = mine[-1]
            assert not (ref[b, out] < last - tol(last)).any(), (what, b, 'a better candidate was left out', np.nonzero(out & (ref[b] < last - tol(last)))[0])


def filters(rng, nq, n_cand):
    """CSR filter lists per query in j space: random sizes, query 0 without a list entry, query 1 filtered completely, query 2 a row
    of -1 (nothing is filtered by it)."""
    sizes = rng.randint(0, max(2, n_cand // 4) + 1, size=nq)
    sizes[0] = 0
    if nq > 1:
        sizes[1] = n_cand
    if nq > 2:
        sizes[2] = 3
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    flat = rng.randint(0, n_cand, size=int(off[-1])).astype(np.int32)
    if nq > 1:
        flat[off[1]:off[2]] = np.arange(n_cand, dtype=np.int32)
    if nq > 2:
        flat[off[2]:off[3]] = -1
    banned = [set(int(x) for x in flat[off[b]:off[b + 1]] if x >= 0) for b in range(nq)]
    return torch.from_numpy(off).to(DEV), torch.from_numpy(flat).to(DEV), banned


def case(shape, l1):
    """Inputs of a shape and its fp64 reference scores, made once and left unchanged."""
    key = (shape, l1)
    if key in _CASES:
        return _CASES[key]
    from oracle import cpu_ref
    d, nu, ne, nc, nq, topn = shape
    gen = torch.Generator().manual_seed(d * 7 + ne + nq)
    rng = np.random.RandomState(ne + nq)
    U, E, R = (torch.randn(n, d, generator=gen) * 0.5 for n in (nu, ne, NR))
    u = torch.randint(0, nu, (nq,), generator=gen)
    if nq > 4:
        u[4] = u[0]; u[nq - 1] = u[3]                                     # duplicate users
    full = cpu_ref.eval_cfkg_rec(U.double(), E.double(), R.double(), u, l1).numpy()          # (nq, ne), the buy relation = last row
    cand = torch.from_numpy(rng.permutation(ne)[:nc].astype(np.int64))    # a permuted subset
    if nc >= 3:
        cand[1] = cand[0]                                                 # the same entity row twice: exactly equal scores
    bad = nc // 2                                                          # one entry without an entity row, alternately below and above
    cand[bad] = -3 if nc % 2 else ne + 5
    valid = (cand >= 0) & (cand < ne)
    sub = np.full((nq, nc), np.inf)
    sub[:, valid.numpy()] = full[:, cand[valid].numpy()]
    c = {'U': U.to(DEV), 'E': E.to(DEV), 'R': R.to(DEV), 'u': u.to(DEV), 'cand': cand.to(DEV), 'bad': bad,
         'ref': {'all': full, 'sub': sub}, 'filt': {'all': filters(rng, nq, ne), 'sub': filters(rng, nq, nc)}}
    _CASES[key] = c
    return c


@pytest.mark.parametrize('l1', [True, False])
@pytest.mark.parametrize('shape', SHAPES)
def test_pass_lists_are_right_for_the_fp64_scores(shape, l1):
    d, nu, ne, nc, nq, topn = shape
    c = case(shape, l1)
    for which in ('all', 'sub'):
        cand = None if which == 'all' else c['cand']
        ref = c['ref'][which]
        f_off, f_ids, banned = c['filt'][which]
        for nsplit in (0, 1, 3):
            for filt in (True, False):
                what = '%s %s cand=%s nsplit=%d filter=%s' % (shape, 'L1' if l1 else 'L2', which, nsplit, filt)
                got = ops().eval_cfkg_topk(c['U'], c['R'], NR - 1, c['E'], c['u'], topn, l1, cand_ids=cand, filt_off=f_off if filt else None,
                                           filt_ids=f_ids if filt else None, with_scores=True, nsplit=nsplit)
                ids, sc = got[0].cpu().numpy(), got[1].cpu().numpy()
                referee(ids, sc, ref, banned if filt else None, topn, what)
                if which == 'sub':
                    assert not (ids == c['bad']).any(), what + ': the candidate without an entity row was ranked'
                if filt and nq > 2:
                    assert (ids[1] == -1).all(), what                     # query 1: everything filtered
                    assert (ids[2, :min(topn, int(np.isfinite(ref[2]).sum()))] >= 0).all(), what       # query 2: a row of -1 filters nothing
        only = ops().eval_cfkg_topk(c['U'], c['R'], NR - 1, c['E'], c['u'], topn, l1, cand_ids=cand)         # no filter argument, no scores
        assert only.dtype == torch.int32
        referee(only.cpu().numpy(), None, ref, None, topn, '%s %s ids only' % (shape, which))
    if nc < topn:
        assert (only.cpu().numpy()[:, nc - 1:] == -1).all()               # fewer candidates (one without a row) than topn: padding


def test_an_empty_filter_id_list_means_no_filter():
    c = case(SHAPES[0], True)
    off = torch.zeros(SHAPES[0][4] + 1, dtype=torch.int64, device=DEV)
    got = ops().eval_cfkg_topk(c['U'], c['R'], NR - 1, c['E'], c['u'], 10, True, filt_off=off, filt_ids=torch.zeros(0, dtype=torch.int32, device=DEV))
    referee(got.cpu().numpy(), None, c['ref']['all'], None, 10, 'empty filter')


def test_tables_with_a_pitch_and_unaligned_entity_rows():
    """Column slices as tables: pitches > d, entity rows off a 16-byte boundary (element-wise loads at d % 4 == 0)."""
    shape = SHAPES[0]
    d, nu, ne, nc, nq, topn = shape
    for l1 in (True, False):
        c = case(shape, l1)
        wide_u = torch.zeros(nu, d + 12, device=DEV); wide_u[:, 5:5 + d] = c['U']
        wide_e = torch.zeros(ne, d + 3, device=DEV); wide_e[:, 1:1 + d] = c['E']
        wide_r = torch.zeros(NR, d + 8, device=DEV); wide_r[:, 8:8 + d] = c['R']
        f_off, f_ids, banned = c['filt']['sub']
        got = ops().eval_cfkg_topk(wide_u[:, 5:5 + d], wide_r[:, 8:8 + d], NR - 1, wide_e[:, 1:1 + d], c['u'], topn, l1, cand_ids=c['cand'],
                                   filt_off=f_off, filt_ids=f_ids, with_scores=True)
        referee(got[0].cpu().numpy(), got[1].cpu().numpy(), c['ref']['sub'], banned, topn, 'pitched tables')


def test_declined_shapes_return_none():
    c = case(SHAPES[0], True)
    assert ops().eval_cfkg_topk(c['U'], c['R'], NR - 1, c['E'], c['u'], 17, True) is None
    assert ops().eval_cfkg_topk(c['U'], c['R'], NR - 1, c['E'], c['u'][:0], 10, True) is None
    wide = torch.zeros(8, 260, device=DEV)
    assert ops().eval_cfkg_topk(wide, wide, 0, wide, c['u'][:3] % 8, 10, False) is None


# ------------------------------------------------------------------------------------------ the reference's own matrices
GNU, GNI, GNE, GNR = 37, 45, 53, 7


@pytest.mark.parametrize('d', [36, 64])
@pytest.mark.parametrize('l1', [False, True])
def test_reference_goldens(golden, d, l1):
    """The users `uq` of baselines.npz: the pass's top-10 lists are right lists for the reference's own evalRec matrix."""
    from jTransUP.models import CFKG
    g = golden('baselines')
    pre = 'd%d.' % d
    m = CFKG.CFKG(l1, d, GNU, GNI, GNE, GNR)
    m.load_state_dict({k: torch.from_numpy(g[pre + 'cfkg.' + k]).to(DEV) for k in ('user_embeddings.weight', 'ent_embeddings.weight',
                                                                                 'rel_embeddings.weight')}, strict=False)
    m.eval()
    u = torch.from_numpy(g[pre + 'uq']).long().to(DEV)
    ref = g[pre + 'cfkg.%s.evalRec' % ('L1' if l1 else 'L2')].astype(np.float64)
    assert ref.shape == (u.numel(), GNE)
    ids, sc = ops().eval_cfkg_topk(m.user_embeddings.weight, m.rel_embeddings.weight, m.rel_total - 1, m.ent_embeddings.weight, u, 10, l1,
                                   with_scores=True)
    referee(ids.cpu().numpy(), sc.cpu().numpy(), ref, None, 10, 'golden d=%d' % d)
    assert torch.equal(m.evaluate_topk(u, None, 10), ids)                 # the model's own entry: the same call


# ------------------------------------------------------------------------------------------ the model through the joint driver
NU, NE, NI, D = 90, 230, 120, 36


def _world(l1, seed=13):
    from jTransUP.models import CFKG
    torch.manual_seed(seed)
    m = CFKG.CFKG(l1, D, NU, NE, NE, 6)
    with torch.no_grad():
        for prm in m.parameters():
            prm.add_(torch.randn_like(prm) * 0.3)
    i_map = {i: (i * 7) % NE for i in range(NI)}                          # item -> entity row, distinct rows
    rng = np.random.RandomState(4)
    users = list(range(NU))
    gold = {u: set(rng.choice(NI, size=rng.randint(1, 9), replace=False).tolist()) for u in users if u % 9}
    train = {u: set(rng.choice(sorted(set(range(NI)) - gold.get(u, set())), size=25, replace=False).tolist()) for u in users}
    batches = [users[s:s + 32] for s in range(0, NU, 32)]
    return m, i_map, gold, train, batches


def _spy(monkeypatch, m):
    """Counters on the model's two evaluation entries, the lists of the last pass, the rows of the last rec_eval_pass."""
    from jTransUP.models import _driver as Dr
    seen = {'topk': 0, 'walk': 0, 'lists': None, 'rows': None}
    topk, walk, rec_pass = m.evaluate_topk, m.evaluateRec, Dr.rec_eval_pass

    def evaluate_topk(*a, **k):
        seen['topk'] += 1
        seen['lists'] = topk(*a, **k)
        return seen['lists']

    def evaluateRec(*a, **k):
        seen['walk'] += 1
        return walk(*a, **k)

    def rec_eval_pass(*a, **k):
        seen['rows'] = rec_pass(*a, **k)
        return seen['rows']
    monkeypatch.setattr(m, 'evaluate_topk', evaluate_topk)
    monkeypatch.setattr(m, 'evaluateRec', evaluateRec)
    monkeypatch.setattr(Dr, 'rec_eval_pass', rec_eval_pass)
    return seen


@pytest.mark.parametrize('l1', [True, False])
def test_driver_pass_against_its_own_lists_and_the_batch_walk(l1, monkeypatch):
    from jTransUP.models import _driver as Dr
    from jTransUP.models import knowledgable_recommendation as K
    from jTransUP.utils import ranking as RK
    m, i_map, gold, train, batches = _world(l1)
    seen = _spy(monkeypatch, m)
    FL = types.SimpleNamespace(topn=10, share_embeddings=True)
    log = logging.getLogger('cfkg-pass')
    monkeypatch.setenv('KTUP_EVAL_GRAPH', '0')
    K.evaluateRec(FL, m, batches, gold, [train], i_map, log, eval_descending=False)
    assert (seen['topk'], seen['walk']) == (1, 0)                         # one call for the whole pass, no batch walk
    rows, lists = seen['rows'], seen['lists'].cpu().numpy()
    present = [u for u in range(NU) if u in gold]
    assert rows.shape == (len(present), 5) and lists.shape == (NU, 10) and (lists >= 0).all()
    # the rows are the metrics of the pass's own lists: exactly what the metric kernel (K18b) gives for a host copy of them, in the
    # order of the users that have gold items ...
    idx = Dr.rank_index(batches, gold, [train])
    again = ops().rec_metrics(torch.from_numpy(lists.copy()).to(DEV), idx.g_off, idx.g_ids).cpu().numpy()
    np.testing.assert_array_equal(rows, again[[u in gold for u in range(NU)]])
    # ... and the host arithmetic's (utils/ranking.py): precision, recall and hit exactly; f1 and ndcg to the bound at which
    # tests/test_hip_eval.py pins K18b to that arithmetic -- measured here: 4 of 400 entries differ, by 1.1e-16 (the last bit of
    # ndcg: the kernel's log2 and its hit-by-hit sum against numpy's), with either distance
    want = np.array([RK.rec_metrics([int(i) for i in lists[u]], gold[u]) for u in present], dtype=np.float64)
    print('largest |driver row - host metrics of the same lists| = %.3g' % float(np.abs(rows - want).max()))
    np.testing.assert_array_equal(rows[:, 1:4], want[:, 1:4])
    np.testing.assert_allclose(rows, want, rtol=1e-12, atol=0)
    for u in present:
        assert not (set(lists[u].tolist()) & train[u])                    # filtered in item (j) space
    monkeypatch.setenv('KTUP_EVAL_PASS', '0')
    K.evaluateRec(FL, m, batches, gold, [train], i_map, log, eval_descending=False)
    assert seen['topk'] == 1 and seen['walk'] == len(batches)
    walk = seen['rows']
    assert walk.shape == rows.shape
    nq = len(present)
    print('metric means: pass %s, walk %s' % (rows.mean(0), walk.mean(0)))
    assert (np.abs(rows.mean(0) - walk.mean(0)) <= 2.0 / nq).all()        # one near-tie swap moves a mean by at most 1 / nq


def test_periodic_passes_are_captured_and_follow_the_tables(monkeypatch):
    """evaluateRec three times on unchanged tables (eager, capture + replay, replay): the same rows; after an in-place change of a
    table the replay returns that table's rows -- the candidate ids the captured launch reads are the tensor kept on the model."""
    from jTransUP.models import _driver as Dr
    from jTransUP.models import knowledgable_recommendation as K
    m, i_map, gold, train, batches = _world(True, seed=17)
    seen = _spy(monkeypatch, m)
    FL = types.SimpleNamespace(topn=10, share_embeddings=True)
    log = logging.getLogger('cfkg-pass')
    monkeypatch.delenv('KTUP_EVAL_GRAPH', raising=False)
    monkeypatch.delenv('KTUP_EVAL_PASS', raising=False)
    rows = []
    for k in range(3):
        K.evaluateRec(FL, m, batches, gold, [train], i_map, log, eval_descending=False)
        rows.append(seen['rows'].copy())
        torch.empty(1 << 20, device=DEV).fill_(7.0)                       # allocator traffic between the passes
    assert seen['walk'] == 0 and seen['topk'] == 2                        # eager once, once under capture, then replays only
    cand = m._pass_cand[1]
    assert cand.tolist() == [i_map[i] for i in range(NI)]
    graphs = [v for v in Dr._EVAL_GRAPHS.values() if v[2] is batches]
    assert len(graphs) == 1 and graphs[0][0] is not None
    np.testing.assert_array_equal(rows[1], rows[0])
    np.testing.assert_array_equal(rows[2], rows[0])
    with torch.no_grad():
        m.user_embeddings.weight.add_(torch.randn_like(m.user_embeddings.weight) * 0.5)
    K.evaluateRec(FL, m, batches, gold, [train], i_map, log, eval_descending=False)
    assert seen['topk'] == 2 and m._pass_cand[1] is cand                  # a replay, on the same id tensor
    changed = seen['rows'].copy()
    assert not np.array_equal(changed, rows[0])
    monkeypatch.setenv('KTUP_EVAL_GRAPH', '0')
    K.evaluateRec(FL, m, batches, gold, [train], i_map, log, eval_descending=False)
    np.testing.assert_array_equal(changed, seen['rows'])                  # ... the rows of an eager pass on the changed table
