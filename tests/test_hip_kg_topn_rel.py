"""The relation-bucketed link-prediction list pass (ktup_eval_kg_topk_rel: the filtered top-n entities of every key in one sweep for
TransR / CKE and TransD, both distances, both directions) on the GPU, judged by the referee of tests/_kg_topn_case.py on fp64 scores
computed from the fp32 tables with the formulas of evaluateHead / evaluateTail (tests/_kg_topn_rel_case.py).

The referee's tolerance is tol(s) = 1e-4 |s| + 1e-5, and in every case at least 90 % of the keys must also return EXACTLY the fp64
list as an id sequence.  (A numpy fp32 model of the pass's arithmetic on inputs of this kind -- tables randn x 0.5, M randn x 0.5 /
sqrt(d), 70 keys, 300 entities, topn 64, d in {20, 36, 50, 100, 128, 256}, three seeds, both directions -- misses the exact list for
at most 1 of 70 keys; its worst score errors are 0.004 tol for TransR, 0.036 tol for TransD with L1 and 0.25 tol for TransD's
squared-L2 expansion at d = 256.)

Exact properties (torch.equal): lists and score bits are identical for every nsplit; the topn-10 list is the prefix of the topn-16,
-32 and -64 lists; with_scores=False gives the same ids; shuffling the keys permutes the output rows and changes nothing else (the
test of the buckets, the filter bits by position and the move back to key order)."""
import numpy as np
import pytest
import torch

from tests import _kg_topn_rel_case as KC

pytestmark = pytest.mark.gpu
DEV = 'cuda'
# (d, n_rel, n_ent, nq, topn): the nine shapes of tests/test_hip_kg_topn.py; then the bucket edges (relation ids set by hand: 64 keys
# on relation 0, 65 on relation 1, one on relation 2, none on relation 3, the rest over 4 - 6), more relations than keys, and every
# key on the one relation there is
EDGES, MANY_RELS, ONE_REL = (36, 7, 120, 200, 10), (64, 300, 90, 40, 10), (20, 1, 53, 130, 10)
SHAPES = [(20, 4, 53, 9, 10), (36, 4, 177, 65, 16), (50, 3, 60, 20, 17), (64, 5, 300, 70, 33), (100, 5, 300, 70, 64),
          (100, 2, 9, 63, 10), (128, 4, 70, 17, 1), (192, 3, 70, 17, 32), (256, 4, 211, 37, 10), EDGES, MANY_RELS, ONE_REL]
PITCHED = 20            # this width reads column slices: pitches > d, rows off a 16-byte boundary
EXACT_SHARE = 0.9
_CASES = {}


def ops():
    from jTransUP.hip import ops as o
    return o


def case(shape):
    """Tables, keys and filter lists of a shape, made once and left unchanged; the fp64 scores per (model, distance, direction)."""
    if shape in _CASES:
        return _CASES[shape]
    d, n_rel, ne, nq, topn = shape
    gen = torch.Generator().manual_seed(d * 7 + ne + nq)
    rng = np.random.RandomState(ne + nq)
    E, R, Ep, Rp = (torch.randn(n, d, generator=gen) * 0.5 for n in (ne, n_rel, ne, n_rel))
    M = torch.randn(n_rel, d * d, generator=gen) * (0.5 / d ** 0.5)
    E[5] = E[2]                                                            # the same row twice: exactly equal scores
    q, r = torch.randint(0, ne, (nq,), generator=gen), torch.randint(0, n_rel, (nq,), generator=gen)
    if shape == EDGES:
        z = torch.zeros(64, dtype=torch.int64)
        r = torch.cat([z, z[:1] + 1, z + 1, z[:1] + 2, 4 + torch.arange(nq - 130) % 3])[torch.randperm(nq, generator=gen)]
        assert [int((r == k).sum()) for k in range(7)] == [64, 65, 1, 0, 24, 23, 23]
        twice = (r == 0).nonzero().flatten()[:2]
        q[twice[1]] = q[twice[0]]                                          # a repeated key (the counts stay)
    elif nq > 4:
        q[4], r[4] = q[0], r[0]                                            # a repeated key
    off, flat, banned = KC.filters(rng, nq, ne)

    def dev(t):
        if d != PITCHED:
            return t.to(DEV)
        wide = torch.zeros(t.shape[0], t.shape[1] + 7, device=DEV)
        wide[:, 3:3 + t.shape[1]] = t
        return wide[:, 3:3 + t.shape[1]]
    c = {'E': dev(E), 'R': dev(R), 'M': dev(M), 'Ep': dev(Ep), 'Rp': dev(Rp), 'q': q.to(DEV), 'r': r.to(DEV),
         'host': {'E': E.numpy(), 'R': R.numpy(), 'M': M.numpy(), 'Ep': Ep.numpy(), 'Rp': Rp.numpy()}, 'qr': (q.numpy(), r.numpy()),
         'csr': (off, flat), 'off': torch.from_numpy(off).to(DEV), 'flat': torch.from_numpy(flat).to(DEV), 'banned': banned, 'ref': {}}
    _CASES[shape] = c
    return c


def ref64(c, transd, l1, head):
    k = (transd, l1, head)
    if k not in c['ref']:
        h, (q, r) = c['host'], c['qr']
        c['ref'][k] = KC.scores64_transd(h['E'], h['R'], h['Ep'], h['Rp'], q, r, l1, head) if transd else \
            KC.scores64_transr(h['E'], h['R'], h['M'], q, r, l1, head)
    return c['ref'][k]


def run(c, transd, l1, head, topn, filt, with_scores=True, nsplit=0, q=None, r=None, off=None, flat=None):
    q, r = c['q'] if q is None else q, c['r'] if r is None else r
    kw = dict(filt_off=(c['off'] if off is None else off) if filt else None, filt_ids=(c['flat'] if flat is None else flat) if filt else None,
              with_scores=with_scores, nsplit=nsplit)
    if transd:
        return ops().eval_kg_topk_transd(c['E'], c['R'], c['Ep'], c['Rp'], q, r, l1, head, topn, **kw)
    return ops().eval_kg_topk_transr(c['E'], c['R'], c['M'], q, r, l1, head, topn, **kw)


def judge(c, transd, l1, head, topn, what):
    """Every nsplit, with and without filters: the referee, the exact-list condition, equality across nsplit and without scores."""
    ref = ref64(c, transd, l1, head)
    nq, ne = ref.shape
    for filt in (True, False):
        banned = c['banned'] if filt else None
        first = None
        for nsplit in (0, 1, 3):
            tag = '%s nsplit=%d filter=%s' % (what, nsplit, filt)
            got = run(c, transd, l1, head, topn, filt, nsplit=nsplit)
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
                    assert (ids[2, :min(topn, ne)] >= 0).all(), tag             # key 2: a row of -1 filters nothing
                if ne < topn:
                    assert (ids[:, ne:] == -1).all(), tag
            else:
                assert torch.equal(got[0], first[0]) and torch.equal(got[1], first[1]), tag + ': differs from nsplit 0'
        only = run(c, transd, l1, head, topn, filt, with_scores=False)
        assert only.dtype == torch.int32 and torch.equal(only, first[0]), what + ': ids without scores'


def _what(shape, transd, l1, head=None):
    return '%s %s %s %s' % (shape, 'TransD' if transd else 'TransR', 'L1' if l1 else 'L2', {None: '', False: 'tail', True: 'head'}[head])


@pytest.mark.parametrize('head', [False, True])
@pytest.mark.parametrize('l1', [True, False])
@pytest.mark.parametrize('transd', [False, True])
@pytest.mark.parametrize('shape', SHAPES)
def test_lists_are_right_for_the_fp64_scores(shape, transd, l1, head):
    judge(case(shape), transd, l1, head, shape[4], _what(shape, transd, l1, head))


@pytest.mark.parametrize('l1', [True, False])
@pytest.mark.parametrize('transd', [False, True])
@pytest.mark.parametrize('shape', [SHAPES[2], SHAPES[4], SHAPES[8]])
def test_a_shorter_list_is_the_prefix_of_a_longer_one(shape, transd, l1):
    """The same inputs at every list width (one, two and four 16-key segments; at d = 256 with L1 a smaller stage under the wide
    lists): ids and score bits of the topn-10 list open the topn-16, -32 and -64 lists."""
    c = case(shape)
    ids10, sc10 = run(c, transd, l1, False, 10, True)
    for topn in (16, 32, 64):
        ids, sc = run(c, transd, l1, False, topn, True, nsplit=topn // 16)
        assert torch.equal(ids[:, :10], ids10) and torch.equal(sc[:, :10], sc10), (_what(shape, transd, l1), topn)


@pytest.mark.parametrize('l1', [True, False])
@pytest.mark.parametrize('transd', [False, True])
@pytest.mark.parametrize('shape', [SHAPES[0], SHAPES[3], EDGES, MANY_RELS, ONE_REL])
def test_shuffling_the_keys_permutes_the_rows_and_nothing_else(shape, transd, l1):
    c = case(shape)
    nq, topn = shape[3], shape[4]
    off, flat = c['csr']
    perm = np.random.RandomState(nq).permutation(nq)
    sizes = (off[1:] - off[:-1])[perm]
    poff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    pflat = np.concatenate([flat[off[b]:off[b + 1]] for b in perm] + [np.zeros(0, dtype=np.int32)]).astype(np.int32)
    pd = torch.from_numpy(perm).to(DEV)
    for head in (False, True):
        for filt in (True, False):
            ids, sc = run(c, transd, l1, head, topn, filt)
            pids, psc = run(c, transd, l1, head, topn, filt, q=c['q'][pd].contiguous(), r=c['r'][pd].contiguous(),
                            off=torch.from_numpy(poff).to(DEV), flat=torch.from_numpy(pflat).to(DEV))
            assert torch.equal(pids, ids[pd]) and torch.equal(psc, sc[pd]), (_what(shape, transd, l1, head), filt)


def test_an_empty_filter_id_list_means_no_filter():
    c = case(SHAPES[0])
    off = torch.zeros(SHAPES[0][3] + 1, dtype=torch.int64, device=DEV)
    for transd in (False, True):
        got = run(c, transd, True, False, 10, True, with_scores=False, off=off, flat=torch.zeros(0, dtype=torch.int32, device=DEV))
        KC.referee(got.cpu().numpy(), None, ref64(c, transd, True, False), None, 10, 'empty filter')


def test_declined_shapes_return_none():
    c = case(SHAPES[0])
    o = ops()
    assert o.eval_kg_topk_transr(c['E'], c['R'], c['M'], c['q'], c['r'], True, False, 65) is None
    assert o.eval_kg_topk_transd(c['E'], c['R'], c['Ep'], c['Rp'], c['q'], c['r'], True, False, 65) is None
    assert o.eval_kg_topk_transr(c['E'], c['R'], c['M'], c['q'][:0], c['r'][:0], True, False, 10) is None
    assert o.eval_kg_topk_transd(c['E'], c['R'], c['Ep'], c['Rp'], c['q'][:0], c['r'][:0], False, True, 10) is None
    wide, mats = torch.zeros(8, 260, device=DEV), torch.zeros(8, 260 * 260, device=DEV)
    assert o.eval_kg_topk_transr(wide, wide, mats, c['q'][:3] % 8, c['r'][:3], False, True, 10) is None
    assert o.eval_kg_topk_transd(wide, wide, wide, wide, c['q'][:3] % 8, c['r'][:3], False, True, 10) is None


# ------------------------------------------------------------------------------------------ the models
NE, NR, D = 230, 6, 36
NI = 20


def _model(kind, l1):
    torch.manual_seed(11)
    if kind == 'transr':
        from jTransUP.models.transR import TransRModel
        m = TransRModel(l1, D, NE, NR)
    elif kind == 'transd':
        from jTransUP.models.transD import TransDModel
        m = TransDModel(l1, D, NE, NR)
    elif kind == 'cke':
        from jTransUP.models.CKE import CKE
        m = CKE(l1, D, 9, NI, NE - 1, NR, {i: i for i in range(NI)}, {i: (i, i) for i in range(NI)})
    elif kind == 'cfkg':
        from jTransUP.models.CFKG import CFKG
        m = CFKG(l1, D, 9, NI, NE, NR)
    else:
        from jTransUP.models.cofm import coFM
        m = coFM(l1, D, 9, NI, NE, NR, False)
    with torch.no_grad():
        for prm in m.parameters():
            prm.add_(torch.randn_like(prm) * 0.3)
    return m.eval()


@pytest.mark.parametrize('l1', [True, False])
@pytest.mark.parametrize('kind', ['transr', 'cke', 'transd', 'cfkg', 'cofm'])
def test_predict_entities_of_the_models(kind, l1):
    from tests import _kg_topn_case as TE
    m = _model(kind, l1)
    o = ops()
    E, R = m.ent_embeddings.weight.detach(), m.rel_embeddings.weight.detach()
    ne, nr = E.shape[0], R.shape[0]
    if kind == 'cke':
        assert ne == NE                                                    # the pad row is a candidate
    gen = torch.Generator().manual_seed(5)
    nq = 70
    q, r = torch.randint(0, ne, (nq,), generator=gen), torch.randint(0, min(nr, NR), (nq,), generator=gen)
    off, flat, banned = KC.filters(np.random.RandomState(8), nq, ne)
    qd, rd, offd, flatd = q.to(DEV), r.to(DEV), torch.from_numpy(off).to(DEV), torch.from_numpy(flat).to(DEV)
    Eh, Rh = E.cpu().numpy(), R.cpu().numpy()
    if kind in ('transr', 'cke'):
        M = m.proj_embeddings.weight.detach()
        score = lambda head: KC.scores64_transr(Eh, Rh, M.cpu().numpy(), q.numpy(), r.numpy(), l1, head)
        direct = lambda head, topn: o.eval_kg_topk_transr(E, R, M, qd, rd, l1, head, topn, offd, flatd, with_scores=True)
    elif kind == 'transd':
        Ep, Rp = m.ent_proj_embeddings.weight.detach(), m.rel_proj_embeddings.weight.detach()
        score = lambda head: KC.scores64_transd(Eh, Rh, Ep.cpu().numpy(), Rp.cpu().numpy(), q.numpy(), r.numpy(), l1, head)
        direct = lambda head, topn: o.eval_kg_topk_transd(E, R, Ep, Rp, qd, rd, l1, head, topn, offd, flatd, with_scores=True)
    else:
        score = lambda head: TE.scores64(Eh, Rh, None, Eh, q.numpy(), r.numpy(), l1, head)
        direct = lambda head, topn: o.eval_kg_topk(E, R, None, qd, rd, l1, head, topn, offd, flatd, with_scores=True)
    for head in (False, True):
        ref = score(head)
        ids, sc = m.predict_entities(qd, rd, head, 20, offd, flatd, with_scores=True)
        assert o.KG_TOPK_ROUTE[0].startswith('no score matrix')
        want = direct(head, 20)
        assert torch.equal(ids, want[0]) and torch.equal(sc, want[1])
        KC.referee(ids.cpu().numpy(), sc.cpu().numpy(), ref, banned, 20, '%s predict_entities' % kind)
        assert KC.exact_fraction(ids.cpu().numpy(), ref, banned, 20) >= EXACT_SHARE
        assert torch.equal(m.predict_entities(qd, rd, head, 20, offd, flatd), ids)
        # beyond the pass's list length: the score matrix in chunks + topk_filtered
        ids, sc = m.predict_entities(qd, rd, head, 70, offd, flatd, with_scores=True)
        assert o.KG_TOPK_ROUTE[0].startswith('chunked score matrix')
        KC.referee(ids.cpu().numpy(), sc.cpu().numpy(), ref, banned, 70, '%s predict_entities, topn 70' % kind)
        KC.referee(m.predict_entities(qd, rd, head, 70).cpu().numpy(), None, ref, None, 70, '%s topn 70, no filter' % kind)
    if kind == 'cke':
        # the pad row (the last one) is a candidate like every other: with all other rows filtered it is the list
        allbut = torch.arange(ne - 1, dtype=torch.int32, device=DEV).repeat(3)
        only = m.predict_entities(qd[:3], rd[:3], False, 20, torch.arange(4, device=DEV) * (ne - 1), allbut, all_e_ids=torch.arange(5, device=DEV))
        assert (only[:, 0] == ne - 1).all() and (only[:, 1:] == -1).all()
