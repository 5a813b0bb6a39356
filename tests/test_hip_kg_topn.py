"""The link-prediction list pass (ktup_eval_kg_topk: the filtered top-n entities of every key in one sweep, TransE and TransH, both
distances, both directions) on the GPU, judged by the referee of tests/_kg_topn_case.py on fp64 scores computed from the fp32 tables
with the formulas of evaluateHead / evaluateTail.

The referee's tolerance tol(s) = 1e-4 |s| + 1e-5 is about 60 times the arithmetic's error, so in every case at least 90 % of the keys
must also return EXACTLY the fp64 list as an id sequence.  (A numpy fp32 model of the pass's arithmetic on inputs of this kind --
tables randn x 0.5, 70 keys, 300 entities, topn 64, d in {20, 36, 50, 100, 256} -- differs from the fp64 list for at most 2 of 70
keys, with a score error of at most 0.016 tol.)

Exact properties (torch.equal): lists and scores are identical for every nsplit; the topn-10 list is the prefix of the topn-16, -32
and -64 lists of the same inputs, ids and score bits alike; with_scores=False gives the same ids."""
import numpy as np
import pytest
import torch

from tests import _kg_topn_case as KC

pytestmark = pytest.mark.gpu
DEV = 'cuda'
# (d, n_rel, n_cand, nq, topn): one and two key blocks with a ragged last wave, candidate counts that are no multiple of the
# 16-candidate tile or of a stage, fewer candidates than topn, d = 50 on the element-wise loads, every list width (16 / 32 / 64 keys)
# at its edges, every row width of the launch ladder up to d = 256
SHAPES = [(20, 4, 53, 9, 10), (36, 4, 177, 65, 16), (50, 3, 60, 20, 17), (64, 5, 300, 70, 33), (100, 5, 300, 70, 64),
          (100, 2, 9, 63, 10), (128, 4, 70, 17, 1), (192, 3, 70, 17, 32), (256, 4, 211, 37, 10)]
SEPARATE = 256          # this width ranks the rows of a candidate table of its own
PITCHED = 20            # this width reads column slices: pitches > d, rows off a 16-byte boundary
EXACT_SHARE = 0.9
_CASES = {}


def ops():
    from jTransUP.hip import ops as o
    return o


def case(shape, wnorm=1.0):
    """Tables, keys and filter lists of a shape, made once and left unchanged; the fp64 scores per (model, distance, direction)."""
    key = (shape, wnorm)
    if key in _CASES:
        return _CASES[key]
    d, n_rel, nc, nq, topn = shape
    gen = torch.Generator().manual_seed(d * 7 + nc + nq)
    rng = np.random.RandomState(nc + nq)
    ne = 40 if d == SEPARATE else nc
    E, R = torch.randn(ne, d, generator=gen) * 0.5, torch.randn(n_rel, d, generator=gen) * 0.5
    N = torch.nn.functional.normalize(torch.randn(n_rel, d, generator=gen), dim=1) * wnorm
    C = torch.randn(nc, d, generator=gen) * 0.5 if d == SEPARATE else E
    if nc >= 8:
        C[5] = C[2]                                                        # the same row twice: exactly equal scores
    q, r = torch.randint(0, ne, (nq,), generator=gen), torch.randint(0, n_rel, (nq,), generator=gen)
    if nq > 4:
        q[4], r[4] = q[0], r[0]                                            # a repeated key
    off, flat, banned = KC.filters(rng, nq, nc)

    def dev(t):
        if d != PITCHED:
            return t.to(DEV)
        wide = torch.zeros(t.shape[0], d + 7, device=DEV)
        wide[:, 3:3 + d] = t
        return wide[:, 3:3 + d]
    c = {'E': dev(E), 'R': dev(R), 'N': dev(N), 'q': q.to(DEV), 'r': r.to(DEV), 'host': (E.numpy(), R.numpy(), N.numpy(), C.numpy()),
         'qr': (q.numpy(), r.numpy()), 'off': torch.from_numpy(off).to(DEV), 'flat': torch.from_numpy(flat).to(DEV), 'banned': banned,
         'ref': {}}
    c['C'] = dev(C) if d == SEPARATE else None
    _CASES[key] = c
    return c


def ref64(c, transh, l1, head):
    k = (transh, l1, head)
    if k not in c['ref']:
        E, R, N, C = c['host']
        c['ref'][k] = KC.scores64(E, R, N if transh else None, C, c['qr'][0], c['qr'][1], l1, head)
    return c['ref'][k]


def run(c, transh, l1, head, topn, filt, with_scores=True, nsplit=0):
    return ops().eval_kg_topk(c['E'], c['R'], c['N'] if transh else None, c['q'], c['r'], l1, head, topn, filt_off=c['off'] if filt else None,
                              filt_ids=c['flat'] if filt else None, candidates=c['C'], with_scores=with_scores, nsplit=nsplit)


def judge(c, transh, l1, head, topn, what):
    """Every nsplit, with and without filters: the referee, the exact-list condition, equality across nsplit and without scores."""
    ref = ref64(c, transh, l1, head)
    nq, nc = ref.shape
    for filt in (True, False):
        banned = c['banned'] if filt else None
        first = None
        for nsplit in (0, 1, 3):
            tag = '%s nsplit=%d filter=%s' % (what, nsplit, filt)
            got = run(c, transh, l1, head, topn, filt, nsplit=nsplit)
            assert got is not None, tag + ': the entry point declined'
            if first is None:
                first = got
                ids, sc = got[0].cpu().numpy(), got[1].cpu().numpy()
                exact = KC.exact_fraction(ids, ref, banned, topn)
                print('%s: %.1f %% of the keys return exactly the fp64 list' % (tag, 100 * exact))
                KC.referee(ids, sc, ref, banned, topn, tag)
                assert exact >= EXACT_SHARE, (tag, exact)
                if filt and nq > 2:
                    assert (ids[1] == -1).all() and (sc[1] == 0.0).all(), tag    # key 1: everything filtered
                    assert (ids[2, :min(topn, nc)] >= 0).all(), tag             # key 2: a row of -1 filters nothing
                if nc < topn:
                    assert (ids[:, nc:] == -1).all(), tag
            else:
                assert torch.equal(got[0], first[0]) and torch.equal(got[1], first[1]), tag + ': differs from nsplit 0'
        only = run(c, transh, l1, head, topn, filt, with_scores=False)
        assert only.dtype == torch.int32 and torch.equal(only, first[0]), what + ': ids without scores'


@pytest.mark.parametrize('head', [False, True])
@pytest.mark.parametrize('l1', [True, False])
@pytest.mark.parametrize('transh', [False, True])
@pytest.mark.parametrize('shape', SHAPES)
def test_lists_are_right_for_the_fp64_scores(shape, transh, l1, head):
    what = '%s %s %s %s' % (shape, 'TransH' if transh else 'TransE', 'L1' if l1 else 'L2', 'head' if head else 'tail')
    judge(case(shape), transh, l1, head, shape[4], what)


@pytest.mark.parametrize('head', [False, True])
@pytest.mark.parametrize('l1', [True, False])
def test_transh_does_not_assume_unit_normals(l1, head):
    shape = SHAPES[3]
    judge(case(shape, wnorm=0.7), True, l1, head, shape[4], '%s |w| = 0.7 %s %s' % (shape, 'L1' if l1 else 'L2', 'head' if head else 'tail'))


@pytest.mark.parametrize('l1', [True, False])
@pytest.mark.parametrize('transh', [False, True])
@pytest.mark.parametrize('shape', [SHAPES[2], SHAPES[4], SHAPES[8]])
def test_a_shorter_list_is_the_prefix_of_a_longer_one(shape, transh, l1):
    """The same inputs at every list width (one, two and four 16-key segments; at d = 256 with L1 a smaller stage under the wide
    lists): ids and score bits of the topn-10 list open the topn-16, -32 and -64 lists."""
    c = case(shape)
    ids10, sc10 = run(c, transh, l1, False, 10, True)
    for topn in (16, 32, 64):
        ids, sc = run(c, transh, l1, False, topn, True, nsplit=topn // 16)
        assert torch.equal(ids[:, :10], ids10) and torch.equal(sc[:, :10], sc10), (shape, transh, l1, topn)


def test_an_empty_filter_id_list_means_no_filter():
    c = case(SHAPES[0])
    off = torch.zeros(SHAPES[0][3] + 1, dtype=torch.int64, device=DEV)
    got = ops().eval_kg_topk(c['E'], c['R'], c['N'], c['q'], c['r'], True, False, 10, filt_off=off,
                             filt_ids=torch.zeros(0, dtype=torch.int32, device=DEV))
    KC.referee(got.cpu().numpy(), None, ref64(c, True, True, False), None, 10, 'empty filter')


def test_declined_shapes_return_none():
    c = case(SHAPES[0])
    assert ops().eval_kg_topk(c['E'], c['R'], None, c['q'], c['r'], True, False, 65) is None
    assert ops().eval_kg_topk(c['E'], c['R'], None, c['q'][:0], c['r'][:0], True, False, 10) is None
    wide = torch.zeros(8, 260, device=DEV)
    assert ops().eval_kg_topk(wide, wide, wide, c['q'][:3] % 8, c['r'][:3], False, True, 10) is None


# ------------------------------------------------------------------------------------------ the models
NE, NR, D = 230, 6, 36


def _model(kind, l1):
    torch.manual_seed(11)
    if kind == 'transe':
        from jTransUP.models.transE import TransEModel
        m = TransEModel(l1, D, NE, NR)
    elif kind == 'transh':
        from jTransUP.models.transH import TransHModel
        m = TransHModel(l1, D, NE, NR)
    else:
        from jTransUP.models.jTransUP import jTransUPModel
        ni = 20
        m = jTransUPModel(l1, D, 9, ni, NE - 1, NR, {i: i for i in range(ni)}, {i: (i, i) for i in range(ni)}, False, False)
    with torch.no_grad():
        for prm in m.parameters():
            prm.add_(torch.randn_like(prm) * 0.3)
    return m.eval()


@pytest.mark.parametrize('l1', [True, False])
@pytest.mark.parametrize('kind', ['transe', 'transh', 'jtransup'])
def test_predict_entities_of_the_models(kind, l1):
    m = _model(kind, l1)
    E, R = m.ent_embeddings.weight.detach(), m.rel_embeddings.weight.detach()
    N = None if kind == 'transe' else m.norm_embeddings.weight.detach()
    assert E.shape[0] == NE
    gen = torch.Generator().manual_seed(5)
    nq = 70
    q, r = torch.randint(0, NE, (nq,), generator=gen), torch.randint(0, NR, (nq,), generator=gen)
    off, flat, banned = KC.filters(np.random.RandomState(8), nq, NE)
    qd, rd, offd, flatd = q.to(DEV), r.to(DEV), torch.from_numpy(off).to(DEV), torch.from_numpy(flat).to(DEV)
    host = [t.cpu().numpy() for t in (E, R)] + [None if N is None else N.cpu().numpy()]
    for head in (False, True):
        ref = KC.scores64(host[0], host[1], host[2], host[0], q.numpy(), r.numpy(), l1, head)
        ids, sc = m.predict_entities(qd, rd, head, 20, offd, flatd, with_scores=True)
        assert ops().KG_TOPK_ROUTE[0].startswith('no score matrix')
        want = ops().eval_kg_topk(E, R, N, qd, rd, l1, head, 20, offd, flatd, with_scores=True)
        assert torch.equal(ids, want[0]) and torch.equal(sc, want[1])
        KC.referee(ids.cpu().numpy(), sc.cpu().numpy(), ref, banned, 20, '%s predict_entities' % kind)
        assert KC.exact_fraction(ids.cpu().numpy(), ref, banned, 20) >= EXACT_SHARE
        assert torch.equal(m.predict_entities(qd, rd, head, 20, offd, flatd), ids)
        # beyond the pass's list length: the score matrix in chunks + topk_filtered, as before
        ids, sc = m.predict_entities(qd, rd, head, 70, offd, flatd, with_scores=True)
        assert ops().KG_TOPK_ROUTE[0].startswith('chunked score matrix')
        KC.referee(ids.cpu().numpy(), sc.cpu().numpy(), ref, banned, 70, '%s predict_entities, topn 70' % kind)
        KC.referee(m.predict_entities(qd, rd, head, 70).cpu().numpy(), None, ref, None, 70, '%s topn 70, no filter' % kind)
