"""TransR's and CKE's link-prediction pass without the score matrix (ktup_eval_kg_ranks_transr_fused,
ops.eval_kg_ranks_transr(fused=True)).

Everything here compares INTEGERS, with no tolerance and no exempted share.  The reference is the chunked route (fused=False:
ktup_eval_kg_ranks_transr, which tests/test_hip_eval.py pins to the per-batch route); the pass forms the same fp32 scores with the
same device code -- csrc/ktup_kg_mc_tile.h (kg_tile_dot1 / kg_l2_score) on the matrix cores, pair_group_scores on the pair route --
so a candidate's 64-bit ranking key has the same bits on both routes and the filtered ranks are equal, also where scores tie
exactly (ids decide) or are NaN (the keys decide).

Shapes the pass declines (KTUP_ERR_UNSUPPORTED before any HIP call; the wrapper then takes the chunked route): rows wider than 256
floats, more than 65535 x 64 keys in one call, 2^31 or more entities, more than 16384 relations, and on the matrix-core route a
norm table or entity-table band beyond the 32-bit buffer range."""
import json
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from tests.synth import make_dataset
from tests.test_hip_transd import _rank_case, eval_mc
from tests.test_hip_transd_pass import csr, seeded_keys, seeded_lists

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'joint-kg-recommender_amd')
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
NAMES = ('ent_embeddings.weight', 'rel_embeddings.weight', 'proj_embeddings.weight')


def ops():
    from jTransUP.hip import ops as o
    return o


def lib():
    from jTransUP.hip import lib as L
    return L


def seeded_tables(ne, nr, d, seed, e_pitch=None, m_pitch=None):
    """fp32 tables on the device -> (E, R, M): entity / relation rows of norm 0.5 .. 1.5, projection matrices N(0, 1/d);
    e_pitch / m_pitch > the row length: rows of a wider buffer (non-contiguous rows)."""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for rows in (ne, nr):
        w = torch.randn(rows, d, generator=gen)
        out.append(w / w.norm(dim=1, keepdim=True) * (0.5 + torch.rand(rows, 1, generator=gen)))
    out.append(torch.randn(nr, d * d, generator=gen) / d ** 0.5)
    E, R, M = (w.to(DEV) for w in out)
    if e_pitch:
        buf = torch.zeros(ne, e_pitch, device=DEV)
        buf[:, :d] = E
        E = buf[:, :d]
    if m_pitch:
        buf = torch.zeros(nr, m_pitch, device=DEV)
        buf[:, :d * d] = M
        M = buf[:, :d * d]
    return E, R, M


def both_routes(W, q, r, l1, head, desc, golds, filts, what='', prepared=True):
    """The pass and the chunked route on the same input, against an entity side prepared under the current eval_mc setting -> the
    (equal) ranks as a list."""
    E, R, M = W
    g_off, g_ids = csr(golds)
    f_off, f_ids = (None, None) if filts is None else csr(filts)
    n = int(g_off[-1])
    ents = ops().eval_transr_entities(E, M, R.shape[0], l1) if prepared else None
    want = ops().eval_kg_ranks_transr(E, R, M, q, r, l1, head, desc, g_off, g_ids, f_off, f_ids, ents=ents, fused=False)
    assert ops().TRANSR_PASS_ROUTE[0].startswith('chunked')
    got = ops().eval_kg_ranks_transr(E, R, M, q, r, l1, head, desc, g_off, g_ids, f_off, f_ids, ents=ents, fused=True)
    assert ops().TRANSR_PASS_ROUTE[0].startswith('no score matrix'), ops().TRANSR_PASS_ROUTE[0]
    got, want = got.cpu().numpy()[:n], want.cpu().numpy()[:n]
    print('%-70s %d of %d ranks differ' % (what, int((got != want).sum()), n))
    assert got.tolist() == want.tolist(), what
    return got.tolist()


# ------------------------------------------------------------------------------------------------ 1. the reference's integers
@pytest.mark.parametrize('mc', [1, 0])
@pytest.mark.parametrize('route', ['chunked', 'pass'])
@pytest.mark.parametrize('d', [64, 100])
def test_routes_reproduce_the_reference_integers(d, route, mc):
    """tests/golden/transr_pass.*: the reference's TransRModel.evaluateHead / evaluateTail + its own rank walk, near-ties removed
    from the input (margin and dropped counts in the json).  230 entities are 4 stages over 8 bands: half the sweep's bands are
    empty.  The chunked leg shows the fixture is sound on code the pass does not touch."""
    g = np.load(os.path.join(GOLDEN, 'transr_pass.npz'))
    meta = json.load(open(os.path.join(GOLDEN, 'transr_pass.json')))
    E, R, M = (torch.from_numpy(g['d%d.%s' % (d, n)]).to(DEV) for n in NAMES)
    for l1 in (True, False):
        for side in ('head', 'tail'):
            case = meta['cases']['d%d.%s.%s' % (d, 'L1' if l1 else 'L2', side)]
            q, r, g_off, g_ids, f_off, f_ids, expect, mean = _rank_case(case)
            with eval_mc(mc):
                ents = ops().eval_transr_entities(E, M, R.shape[0], l1)
                ranks = ops().eval_kg_ranks_transr(E, R, M, q, r, l1, side == 'head', False, g_off, g_ids, f_off, f_ids, ents=ents,
                                                   fused=route == 'pass')
            assert ops().TRANSR_PASS_ROUTE[0].startswith('no score matrix' if route == 'pass' else 'chunked')
            got = ranks.cpu().numpy()[:len(expect)].astype(np.int64)
            print('d=%d %s %s %s eval_mc=%d: %d of %d ranks differ' % (d, 'L1' if l1 else 'L2', side, route, mc,
                                                                      int((got != np.asarray(expect)).sum()), len(expect)))
            assert got.tolist() == expect
            np.testing.assert_allclose([float((got < 10).mean()), float(got.mean())], mean, rtol=1e-12)


# ------------------------------------------------------------------------------------------------ 2. seeded shapes
# (d, l1, n_ent, nq, n_rel).  Squared L2 at d in {64, 100, 128} takes the matrix-core sweep (d = 100: the b32-operand tail MFMA);
# squared L2 at d in {20, 36, 50, 256} and L1 take the pair kernel's COUNT form over the projected table (TransR has no matrix route
# there).  Every n_ent and nq appears at d = 100 squared L2 and on the pair form.
SHAPES = [(100, False, 1, 1, 7), (100, False, 63, 63, 7), (100, False, 64, 65, 7), (100, False, 65, 130, 7), (100, False, 512, 63, 7),
          (100, False, 513, 65, 7), (100, False, 1100, 130, 7), (100, False, 1100, 1, 7),
          (64, False, 65, 130, 7), (64, False, 1100, 65, 7), (128, False, 513, 130, 7), (128, False, 1100, 63, 7), (128, False, 64, 1, 7),
          (100, True, 1, 1, 7), (100, True, 63, 63, 7), (100, True, 64, 65, 7), (100, True, 65, 130, 7), (100, True, 512, 63, 7),
          (100, True, 513, 1, 7), (100, True, 1100, 130, 7), (36, True, 1100, 65, 7), (36, True, 64, 130, 7),
          (20, False, 513, 65, 7), (36, False, 1100, 63, 7), (50, False, 513, 65, 7), (50, False, 63, 130, 7),
          (256, False, 513, 63, 2)]


@pytest.mark.parametrize('d,l1,n_ent,nq,n_rel', SHAPES)
def test_seeded_shapes_equal_the_chunked_route(d, l1, n_ent, nq, n_rel):
    W = seeded_tables(n_ent, n_rel, d, seed=11 * d + n_ent)
    q, r = seeded_keys(n_ent, n_rel, nq, seed=nq + d)
    golds, filts = seeded_lists(nq, n_ent, 3, seed=n_ent + nq)
    for desc in (False, True):
        for head in (True, False):
            both_routes(W, q, r, l1, head, desc, golds, filts, what='d=%d l1=%d n_ent=%d nq=%d desc=%d head=%d' % (d, l1, n_ent, nq, desc, head))


# ------------------------------------------------------------------------------------------------ 3. relation edges
def _rel_case(kind, ne, nq):
    """-> (n_rel, the keys' relation ids)."""
    if kind == 'one_relation_table':
        return 1, [0] * nq
    if kind == 'unused_and_single_key':                       # relation 2 is used by no key, relation 4 by key 0 alone
        return 6, [4] + [(0, 1, 3, 5)[i % 4] for i in range(1, nq)]
    if kind == 'all_keys_one_relation':
        return 5, [3] * nq
    if kind == 'descending_relations':
        return 7, sorted([i % 7 for i in range(nq)], reverse=True)
    assert kind == 'bucket_sizes'                             # buckets of 1, 4, 5, 64 and 65 keys
    rel = [0] * 1 + [1] * 4 + [2] * 5 + [3] * 64 + [4] * 65
    rng = np.random.RandomState(3)
    rng.shuffle(rel)
    return 5, rel


@pytest.mark.parametrize('d,l1', [(100, False), (100, True), (64, False), (36, False)])
@pytest.mark.parametrize('kind', ['one_relation_table', 'unused_and_single_key', 'all_keys_one_relation', 'descending_relations', 'bucket_sizes'])
def test_relation_edges(kind, d, l1):
    ne = 300
    nq = 139 if kind == 'bucket_sizes' else 70
    n_rel, rel = _rel_case(kind, ne, nq)
    W = seeded_tables(ne, n_rel, d, seed=61)
    q, _ = seeded_keys(ne, n_rel, nq, seed=62)
    r = torch.tensor(rel, dtype=torch.int64, device=DEV)
    golds, filts = seeded_lists(nq, ne, 3, seed=63)
    for head in (True, False):
        both_routes(W, q, r, l1, head, False, golds, filts, what='%s d=%d l1=%d head=%d' % (kind, d, l1, head))


@pytest.mark.parametrize('d,l1', [(100, False), (100, True), (50, False)])
def test_projection_table_with_a_pitch(d, l1):
    ne, nr, nq = 300, 7, 70
    W = seeded_tables(ne, nr, d, seed=65, m_pitch=d * d + 4)
    assert W[2].stride(0) == d * d + 4
    q, r = seeded_keys(ne, nr, nq, seed=66)
    golds, filts = seeded_lists(nq, ne, 3, seed=67)
    got = both_routes(W, q, r, l1, True, False, golds, filts, what='M pitch d*d + 4')
    Wc = (W[0], W[1], W[2].contiguous())
    assert got == both_routes(Wc, q, r, l1, True, False, golds, filts, what='M contiguous')


# ------------------------------------------------------------------------------------------------ 4. gold and filter list edges
@pytest.mark.parametrize('max_golds', [1, 3, 4, 5, 9])
@pytest.mark.parametrize('l1', [True, False])
def test_gold_and_filter_list_edges(l1, max_golds):
    d, ne, nq = 100, 300, 70
    W = seeded_tables(ne, 7, d, seed=5)
    q, r = seeded_keys(ne, 7, nq, seed=6)
    golds, filts = seeded_lists(nq, ne, max_golds, seed=max_golds)
    golds[1] = []                                            # a key with no gold
    golds[2], filts[2] = [17], [3, 17, 40]                   # a gold that is itself filtered
    if max_golds >= 3:
        golds[3], filts[3] = [8, 21], [5, 21, 90]            # ... beside a gold of the same key that is not
        golds[4], filts[4] = [10, 20, 30], [20, 250]         # another gold of the key is also in the filter list
    filts[5] = [44, 7, 199, 7, 3]                            # unsorted, with a duplicate
    golds[6] = [ne - 1]
    assert max(len(x) for x in golds) == max_golds
    got = both_routes(W, q, r, l1, True, False, golds, filts, what='list edges')
    off = np.cumsum([0] + [len(x) for x in golds])
    assert got[off[2]] == -1
    if max_golds >= 3:
        assert got[off[3] + 1] == -1 and got[off[3]] >= 0
        assert got[off[4] + 1] == -1 and got[off[4]] >= 0 and got[off[4] + 2] >= 0
    both_routes(W, q, r, l1, False, True, golds, filts, what='list edges, descending tail')
    # no filter at all, and filter lists that are all empty
    a = both_routes(W, q, r, l1, True, False, golds, None, what='no filter')
    b = both_routes(W, q, r, l1, True, False, golds, [[] for _ in range(nq)], what='empty filter lists')
    assert a == b and all(x >= 0 for x in a)


@pytest.mark.parametrize('max_golds', [4, 5])
@pytest.mark.parametrize('d', [64, 128])
def test_four_gold_sweep_loop_at_the_other_widths(d, max_golds):
    """kg_count_mc_kernel<FGeom<16, 3>, 4> (the one new instantiation that spills) and <FGeom<32, 3>, 4>: the sweep launch that also
    holds the four-gold loop runs only for a pass whose longest gold list exceeds three; max_golds = 5 adds a second sweep launch."""
    ne, nq = 300, 70
    W = seeded_tables(ne, 7, d, seed=15 + d)
    q, r = seeded_keys(ne, 7, nq, seed=16)
    golds, filts = seeded_lists(nq, ne, max_golds, seed=17 + max_golds)
    golds[2], filts[2] = [17, 40, 41, 250], [3, 17, 40]      # two of four golds are themselves filtered
    assert max(len(x) for x in golds) == max_golds
    for head, desc in ((True, False), (False, True)):
        got = both_routes(W, q, r, False, head, desc, golds, filts, what='four-gold loop d=%d max_golds=%d head=%d desc=%d' % (d, max_golds, head, desc))
    off = np.cumsum([0] + [len(x) for x in golds])
    assert got[off[2]] == -1 and got[off[2] + 1] == -1 and got[off[2] + 2] >= 0 and got[off[2] + 3] >= 0


# ------------------------------------------------------------------------------------------------ 5. ties and unordered scores
@pytest.mark.parametrize('d,l1', [(100, False), (64, False), (128, False), (100, True), (50, False)])
@pytest.mark.parametrize('kind', ['rows_x3', 'eighths', 'nan_row', 'nan_matrix'])
def test_ties_and_unordered_scores_follow_the_keys(kind, d, l1):
    """Every key's gold meets itself in the sweep: ranks off by one across the board would mean that the list and sweep scores do not
    have the same bits.  Exact ties are broken by id; a NaN score is ordered by its key -- one entity's under every relation, or every
    candidate's under one relation."""
    ne, nr, nq = 300, 7, 70
    E, R, M = seeded_tables(ne, nr, d, seed=3)
    if kind == 'rows_x3':
        E = E[:ne // 3].repeat_interleave(3, dim=0).contiguous()            # every row three times
    elif kind == 'eighths':
        gen = torch.Generator().manual_seed(9)
        E, R, M = ((torch.randint(-8, 9, w.shape, generator=gen).float() / 8).to(DEV) for w in (E, R, M))
    elif kind == 'nan_row':
        E = E.clone()
        E[37, d // 2] = float('nan')
    else:
        M = M.clone()
        M[2, (d // 3) * d + d // 2] = float('nan')
    q, r = seeded_keys(ne, nr, nq, seed=4)
    golds, filts = seeded_lists(nq, ne, 3, seed=8)
    for desc in (False, True):
        both_routes((E, R, M), q, r, l1, True, desc, golds, filts, what='%s d=%d l1=%d desc=%d' % (kind, d, l1, desc))


# ------------------------------------------------------------------------------------------------ 6. layout
@pytest.mark.parametrize('l1', [True, False])
def test_entity_table_with_a_pitch(l1):
    d, ne, nq = 100, 400, 70
    W = seeded_tables(ne, 7, d, seed=21, e_pitch=d + 4)
    assert W[0].stride(0) == d + 4
    q, r = seeded_keys(ne, 7, nq, seed=22)
    golds, filts = seeded_lists(nq, ne, 3, seed=23)
    both_routes(W, q, r, l1, True, False, golds, filts, what='pitch d + 4')
    both_routes(W, q, r, l1, False, True, golds, filts, what='pitch d + 4, descending tail')


@pytest.mark.parametrize('l1', [True, False])
@pytest.mark.parametrize('layout', ['unaligned_base', 'odd_pitch'])
def test_unaligned_entity_tables_take_the_pair_form_and_agree(layout, l1):
    d, ne, nq = 100, 300, 70
    E, R, M = seeded_tables(ne, 7, d, seed=31)
    if layout == 'unaligned_base':
        flat = torch.zeros(ne * d + 1, device=DEV)
        C = flat[1:].view(ne, d)
        assert C.data_ptr() % 16 == 4
    else:
        C = torch.zeros(ne, d + 1, device=DEV)[:, :d]
        assert C.stride(0) % 4 == 1
    C.copy_(E)
    q, r = seeded_keys(ne, 7, nq, seed=32)
    golds, filts = seeded_lists(nq, ne, 3, seed=33)
    got = both_routes((C, R, M), q, r, l1, True, False, golds, filts, what=layout)
    # (the aligned table's squared-L2 ranks come from the matrix-core scores, the unaligned one's from the pair form's)
    assert got == both_routes((E, R, M), q, r, l1, True, False, golds, filts, what=layout + ': the aligned table')


# ------------------------------------------------------------------------------------------------ 7. routing
def _transr_model(l1, d, ne, nr, W):
    from jTransUP.models import transR
    m = transR.TransRModel(l1, d, ne, nr)
    m.load_state_dict({n: w.contiguous() for n, w in zip(NAMES, W)})
    return m


def _cke_model(l1, d, ne, nr, W):
    """A CKE whose TransR side holds W: ne - 1 entities + the pad row (the last row of the entity table)."""
    from jTransUP.models import CKE
    ni = 11
    m = CKE.CKE(l1, d, 5, ni, ne - 1, nr, {i: i for i in range(ni)}, {i: ((i * 3) % (ne - 1) if i % 4 else -1, i) for i in range(ni)})
    sd = m.state_dict()
    E = W[0].clone()
    E[ne - 1] = 0.                                            # the pad row
    sd.update({NAMES[0]: E, NAMES[1]: W[1].contiguous(), NAMES[2]: W[2].contiguous()})
    m.load_state_dict(sd)
    return m, (E, W[1], W[2])


@pytest.mark.parametrize('l1', [True, False])
@pytest.mark.parametrize('model', ['transr', 'cke'])
def test_model_and_option_routing(model, l1):
    d, ne, nr, nq = 100, 300, 7, 70
    W = seeded_tables(ne, nr, d, seed=41)
    if model == 'transr':
        m = _transr_model(l1, d, ne, nr, W)
    else:
        m, W = _cke_model(l1, d, ne, nr, W)
    q, r = seeded_keys(ne, nr, nq, seed=42)
    golds, filts = seeded_lists(nq, ne, 3, seed=43)
    golds[3] = [ne - 1]                                       # (CKE: the pad row is a candidate like any other)
    want = both_routes(W, q, r, l1, True, False, golds, filts, what='routing reference')
    assert want == both_routes(W, q, r, l1, True, False, golds, filts, what='fused=True prepares the entity side itself', prepared=False)
    g_off, g_ids = csr(golds)
    f_off, f_ids = csr(filts)
    default = ops().TRANSR_FUSED_DEFAULT[bool(l1)]
    for ents in (None, m.prepare_entities()):
        got = m.rank_entities(q, r, True, False, g_off, g_ids, f_off, f_ids, ents=ents)
        assert ops().TRANSR_PASS_ROUTE[0].startswith('no score matrix' if default else 'chunked')
        assert got.cpu().numpy()[:len(want)].tolist() == want
    old = lib().set_option('transr_fused', 0)
    try:
        got = m.rank_entities(q, r, True, False, g_off, g_ids, f_off, f_ids)
        assert ops().TRANSR_PASS_ROUTE[0].startswith('chunked')
    finally:
        lib().set_option('transr_fused', old)
    assert got.cpu().numpy()[:len(want)].tolist() == want


def test_declined_shapes_take_the_chunked_route():
    L = lib().load()
    for d in (1, 20, 50, 64, 100, 128, 256):
        assert L.ktup_eval_kg_ranks_transr_fused_supported(d, 0, 3) == 1 and L.ktup_eval_kg_ranks_transr_fused_supported(d, 1, 99) == 1
    assert L.ktup_eval_kg_ranks_transr_fused_supported(260, 0, 3) == 0 and L.ktup_eval_kg_ranks_transr_fused_supported(0, 0, 3) == 0
    # more keys than one sweep takes: the call declines before any launch, the wrapper quietly ranks them chunk by chunk
    nq, ne, nr, d = 65535 * 64 + 1, 3, 2, 4
    E, R, M = seeded_tables(ne, nr, d, seed=51)
    q, r = seeded_keys(ne, nr, nq, seed=52)
    g_off = torch.arange(nq + 1, dtype=torch.int64, device=DEV)
    g_ids = (torch.arange(nq, device=DEV) % ne).to(torch.int32)
    ents = ops().eval_transr_entities(E, M, nr, False)
    ws = torch.empty(L.ktup_eval_kg_ranks_transr_fused_workspace_bytes(d, nq, nq, 0, ne, nr), dtype=torch.uint8, device=DEV)
    ranks = torch.empty(nq, dtype=torch.int32, device=DEV)

    def direct(ents_ptr, n):
        lib().call('ktup_eval_kg_ranks_transr_fused', E.data_ptr(), d, R.data_ptr(), d, M.data_ptr(), d * d, d, ne, nr, ents_ptr, q.data_ptr(),
                   r.data_ptr(), n, 0, 1, 0, None, None, 0, g_off.data_ptr(), g_ids.data_ptr(), n, 1, ranks.data_ptr(), ws.data_ptr(), None)

    with pytest.raises(lib().KtupError) as ei:
        direct(ents.ws.data_ptr(), nq)
    assert ei.value.code == lib().ERR_UNSUPPORTED
    with pytest.raises(lib().KtupError) as ei:                 # the entity side is required
        direct(None, 64)
    assert ei.value.code not in (0, lib().ERR_UNSUPPORTED) and 'ents_ws' in str(ei.value)
    got = ops().eval_kg_ranks_transr(E, R, M, q, r, False, True, False, g_off, g_ids, ents=ents, fused=True, chunk=65536)
    assert ops().TRANSR_PASS_ROUTE[0].startswith('chunked')
    want = ops().eval_kg_ranks_transr(E, R, M, q, r, False, True, False, g_off, g_ids, ents=ents, fused=False, chunk=65536)
    assert torch.equal(got, want) and int(got.min()) >= 0 and int(got.max()) <= ne - 1


def test_workspace_does_not_grow_with_keys_times_entities():
    L = lib().load()
    big = L.ktup_eval_kg_ranks_transr_fused_workspace_bytes(100, 20480, 40960, 409600, 1000000, 20)
    small = L.ktup_eval_kg_ranks_transr_fused_workspace_bytes(100, 20480, 40960, 409600, 1000, 20)
    print('workspace bytes: %d at 1,000,000 entities, %d at 1,000' % (big, small))
    assert small > 0 and 0 <= big - small <= 16 * 999000 + 4096


# ------------------------------------------------------------------------------------------------ 8. CKE through the driver
@pytest.mark.parametrize('want_rows', [False, True])
def test_cke_whole_pass_route_equals_the_batch_walk(want_rows, monkeypatch):
    """_driver.kg_eval_pass with CKEModel.rank_entities returns what the batch walk over evaluateHead / evaluateTail returns, the pad
    row being a candidate (and once a gold), with a key without golds and a filtered gold; KTUP_EVAL_PASS=0 steps aside."""
    from jTransUP.models import _driver as D
    rng = np.random.RandomState(8)
    d, ne, nr, nq = 64, 301, 6, 300
    m, _ = _cke_model(False, d, ne, nr, seeded_tables(ne, nr, d, seed=71))
    m.eval(); m.disable_grad()
    FL = types.SimpleNamespace(topn=10)
    keys = list(dict.fromkeys((int(rng.randint(ne - 1)), int(rng.randint(nr))) for _ in range(nq)))
    gold = {k: set(rng.choice(ne, size=rng.randint(1, 4), replace=False).tolist()) for k in keys if k[0] % 11}
    gold[keys[1]] = {ne - 1}                                   # the pad row as a gold
    filt = {k: set(rng.choice(ne, size=20, replace=False).tolist()) | (set(list(gold[k])[:1]) if k in gold and k[0] % 3 == 0 else set()) for k in keys}
    assert any(k not in gold for k in keys) and any(k in gold and gold[k] & filt[k] for k in keys)
    batches = [keys[s:s + 64] for s in range(0, len(keys), 64)]
    ents = m.prepare_entities()
    for head in (True, False):
        score_fn = (lambda q, r: m.evaluateHead(q, r, ents=ents)) if head else (lambda q, r: m.evaluateTail(q, r, ents=ents))
        rank_fn = lambda q, r, desc, go, gi, fo, fi: m.rank_entities(q, r, head, desc, go, gi, fo, fi, all_e_ids=None, ents=ents)
        for desc in (False, True):
            walk = D.kg_eval_pass(FL, score_fn, batches, gold, [filt], desc, want_rows=want_rows)
            fused = D.kg_eval_pass(FL, score_fn, batches, gold, [filt], desc, want_rows=want_rows, rank_fn=rank_fn)
            if want_rows:
                assert fused == walk and len(walk) > 0
            else:
                assert fused.shape == walk.shape and walk.shape[0] > 0
                np.testing.assert_array_equal(fused, walk)
    calls = []
    monkeypatch.setenv('KTUP_EVAL_PASS', '0')
    D.kg_eval_pass(FL, score_fn, batches, gold, [filt], False, want_rows=want_rows, rank_fn=lambda *a: calls.append(1))
    assert not calls


# ------------------------------------------------------------------------------------------------ 9. the command line
@pytest.fixture(scope='module')
def dataset(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('ds')
    make_dataset(str(tmp))
    return tmp


def run_cli(tmp, script, name, model, extra, env=None):
    data = str(tmp)
    logs = os.path.join(data, 'log')
    os.makedirs(logs, exist_ok=True)
    cmd = [sys.executable, os.path.join(PKG, script), '-data_path', data, '-log_path', logs, '-dataset', 'ml1m',
           '-experiment_name', name, '-nohas_visualization', '-batch_size', '32', '-embedding_size', '20', '-seed', '3',
           '-eval_interval_steps', '10', '-training_steps', '25', '-early_stopping_steps_to_wait', '0', '-learning_rate', '0.05',
           '-topn', '10', '-model_type', model] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return open(os.path.join(logs, name + '.log')).read()


METRIC_LINE = r'avg hit:\d\.\d+, avg mean rank:\d+\.\d+, topn:10'
PASS_ROUTE = 'no score matrix (ktup_eval_kg_ranks_transr_fused)'
CHUNKED_ROUTE = 'chunked score matrix (ktup_eval_kg_ranks_transr)'


def test_cli_transr_reports_the_same_metrics_on_both_routes(dataset):
    extra = ['-kg_test_files', 'valid.dat:test.dat']
    fused = run_cli(dataset, 'run_knowledge_representation.py', 'kg-transr-pass', 'transr', extra, {'KTUP_TRANSR_FUSED': '1'})
    chunked = run_cli(dataset, 'run_knowledge_representation.py', 'kg-transr-chunked', 'transr', extra, {'KTUP_TRANSR_FUSED': '0'})
    rows, rows0 = re.findall(METRIC_LINE, fused), re.findall(METRIC_LINE, chunked)
    assert len(rows) >= 6 and rows == rows0
    assert 'TransR link-prediction pass: ' + CHUNKED_ROUTE in chunked
    assert 'TransR link-prediction pass: ' + (PASS_ROUTE if ops().TRANSR_FUSED_DEFAULT[False] else CHUNKED_ROUTE) in fused


def test_cli_cke_reports_the_same_metrics_with_and_without_the_pass(dataset):
    extra = ['-rec_test_files', 'valid.dat', '-kg_test_files', 'valid.dat', '-joint_ratio', '0.5']
    fused = run_cli(dataset, 'run_knowledgable_recommendation.py', 'cke-pass', 'cke', extra, {'KTUP_TRANSR_FUSED': '1'})
    walk = run_cli(dataset, 'run_knowledgable_recommendation.py', 'cke-walk', 'cke', extra, {'KTUP_EVAL_PASS': '0'})
    rows, rows0 = re.findall(METRIC_LINE, fused), re.findall(METRIC_LINE, walk)
    assert len(rows) >= 3 and rows == rows0
    assert 'CKE link-prediction pass: ' + (PASS_ROUTE if ops().TRANSR_FUSED_DEFAULT[False] else CHUNKED_ROUTE) in fused
    assert 'CKE link-prediction pass' not in walk
