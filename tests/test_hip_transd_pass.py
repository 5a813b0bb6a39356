"""TransD's link-prediction pass without the score matrix (ktup_eval_kg_ranks_transd_fused, ops.eval_kg_ranks_transd(fused=True)).

Everything here compares INTEGERS, with no tolerance and no exempted share.  The reference is the chunked route (fused=False:
ktup_eval_kg_ranks_transd), which tests/test_hip_transd.py pins to the reference implementation's recorded ranks and to fp64; the
pass forms the same fp32 scores with the same device code (csrc/ktup_transd_eval.hip: tile_dots3 / row_norm8 / mc_score on the matrix
cores, transd_pair_scores on the pair route), so a candidate's 64-bit ranking key has the same bits on both routes and the filtered
ranks are equal -- also where scores tie exactly (ids decide) or are NaN (the keys decide).

Shapes the pass declines (KTUP_ERR_UNSUPPORTED before any HIP call; the wrapper then takes the chunked route): rows wider than 640
floats (the pair kernels' LDS stage; the chunked route declines those as well), more than 65535 x 64 keys in one call, 2^31 or more
candidates."""
import json
import os
import re

import numpy as np
import pytest
import torch

from tests.synth import make_dataset
from tests.test_hip_transd import NAMES, _rank_case, eval_mc, run_cli, seeded_tables

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')


def ops():
    from jTransUP.hip import ops as o
    return o


def lib():
    from jTransUP.hip import lib as L
    return L


def dv(a, dt):
    return torch.tensor(a, dtype=dt, device=DEV)


def csr(lists):
    off, ids = [0], []
    for l in lists:
        ids += list(l)
        off.append(len(ids))
    return dv(off, torch.int64), dv(ids, torch.int32)


def seeded_lists(nq, n_cand, max_golds, seed, max_filt=20):
    """Per key 1 .. max_golds sorted distinct golds (key 0 gets exactly max_golds) and 0 .. max_filt sorted distinct filtered ids; the
    two may overlap (a gold that is filtered ranks -1, another gold of the key that is filtered is subtracted once)."""
    rng = np.random.RandomState(seed)
    golds, filts = [], []
    for i in range(nq):
        ng = min(n_cand, max_golds if i == 0 else int(rng.randint(1, max_golds + 1)))
        golds.append(sorted(rng.choice(n_cand, ng, replace=False).tolist()))
        nf = min(n_cand, int(rng.randint(0, max_filt + 1)))
        filts.append(sorted(rng.choice(n_cand, nf, replace=False).tolist()))
    return golds, filts


def both_routes(W, q, r, l1, head, desc, golds, filts, candidates=None, what=''):
    """The pass and the chunked route on the same input -> the (equal) ranks as a list."""
    E, R, Ep, Rp = W
    g_off, g_ids = csr(golds)
    f_off, f_ids = (None, None) if filts is None else csr(filts)
    n = int(g_off[-1])
    want = ops().eval_kg_ranks_transd(E, R, Ep, Rp, q, r, l1, head, desc, g_off, g_ids, f_off, f_ids, candidates=candidates, fused=False)
    got = ops().eval_kg_ranks_transd(E, R, Ep, Rp, q, r, l1, head, desc, g_off, g_ids, f_off, f_ids, candidates=candidates, fused=True)
    assert ops().TRANSD_PASS_ROUTE[0].startswith('no score matrix'), ops().TRANSD_PASS_ROUTE[0]
    got, want = got.cpu().numpy()[:n], want.cpu().numpy()[:n]
    wrong = int((got != want).sum())
    print('%-70s %d of %d ranks differ' % (what, wrong, n))
    assert got.tolist() == want.tolist(), what
    return got.tolist()


def seeded_keys(ne, nr, nq, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randint(0, ne, (nq,), generator=gen).to(DEV), torch.randint(0, nr, (nq,), generator=gen).to(DEV)


# ------------------------------------------------------------------------------------------------ 1. the reference's integers
@pytest.mark.parametrize('mc', [1, 0])
@pytest.mark.parametrize('l1', [True, False])
@pytest.mark.parametrize('side', ['head', 'tail'])
def test_pass_reproduces_the_reference_integers(l1, side, mc):
    """230 candidates are 4 stages over 8 bands: half the sweep's bands are empty."""
    g = np.load(os.path.join(GOLDEN, 'transd.npz'))
    case = json.load(open(os.path.join(GOLDEN, 'transd.json')))['rank']['cases']['%s.%s' % ('L1' if l1 else 'L2', side)]
    E, R, Ep, Rp = (torch.from_numpy(g['rank.' + n]).to(DEV) for n in NAMES)
    q, r, g_off, g_ids, f_off, f_ids, expect, mean = _rank_case(case)
    with eval_mc(mc):
        ranks = ops().eval_kg_ranks_transd(E, R, Ep, Rp, q, r, l1, side == 'head', False, g_off, g_ids, f_off, f_ids, fused=True)
    assert ops().TRANSD_PASS_ROUTE[0].startswith('no score matrix')
    got = ranks.cpu().numpy()[:len(expect)].astype(np.int64)
    print('%s %s eval_mc=%d: %d of %d ranks differ' % ('L1' if l1 else 'L2', side, mc, int((got != np.asarray(expect)).sum()), len(expect)))
    assert got.tolist() == expect
    np.testing.assert_allclose([float((got < 10).mean()), float(got.mean())], mean, rtol=1e-12)


# ------------------------------------------------------------------------------------------------ 2. seeded shapes
# (d, l1, n_cand, nq).  Squared L2 at d in {20, 36, 64, 100, 128} takes the matrix-core sweep (d % 16 == 4: the b32-operand tail MFMA;
# d % 16 == 0: none); d in {50, 256, 300} and L1 take the pair kernel's COUNT form.  Every n_cand and nq below appears at d = 100
# squared L2 and on the pair form.
SHAPES = [(100, False, 1, 1), (100, False, 63, 63), (100, False, 64, 65), (100, False, 65, 130), (100, False, 512, 63),
          (100, False, 513, 65), (100, False, 1100, 130), (100, False, 1100, 1),
          (20, False, 513, 65), (36, False, 1100, 63), (64, False, 65, 130), (64, False, 1100, 65), (128, False, 513, 130),
          (128, False, 1100, 63), (128, False, 64, 1),
          (100, True, 1, 1), (100, True, 63, 63), (100, True, 64, 65), (100, True, 65, 130), (100, True, 512, 63), (100, True, 513, 1),
          (100, True, 1100, 130), (36, True, 1100, 65), (36, True, 64, 130),
          (50, False, 513, 65), (50, False, 63, 130), (256, False, 1100, 63), (256, False, 65, 1), (300, False, 512, 130),
          (300, False, 1, 63)]


@pytest.mark.parametrize('d,l1,n_cand,nq', SHAPES)
def test_seeded_shapes_equal_the_chunked_route(d, l1, n_cand, nq):
    W = seeded_tables(n_cand, 7, d, seed=11 * d + n_cand)
    q, r = seeded_keys(n_cand, 7, nq, seed=nq + d)
    golds, filts = seeded_lists(nq, n_cand, 3, seed=n_cand + nq)
    for desc in (False, True):
        for head in (True, False):
            both_routes(W, q, r, l1, head, desc, golds, filts, what='d=%d l1=%d n_cand=%d nq=%d desc=%d head=%d' % (d, l1, n_cand, nq, desc, head))


# ------------------------------------------------------------------------------------------------ 3. gold and filter list edges
@pytest.mark.parametrize('max_golds', [1, 3, 4, 5, 9])
@pytest.mark.parametrize('l1', [True, False])
def test_gold_and_filter_list_edges(l1, max_golds):
    d, n_cand, nq = 100, 300, 70
    W = seeded_tables(n_cand, 7, d, seed=5)
    q, r = seeded_keys(n_cand, 7, nq, seed=6)
    golds, filts = seeded_lists(nq, n_cand, max_golds, seed=max_golds)
    golds[1] = []                                            # a key with no gold
    golds[2], filts[2] = [17], [3, 17, 40]                   # a gold that is itself filtered
    if max_golds >= 3:
        golds[3], filts[3] = [8, 21], [5, 21, 90]            # ... beside a gold of the same key that is not
        golds[4], filts[4] = [10, 20, 30], [20, 250]         # another gold of the key is also in the filter list
    filts[5] = [44, 7, 199, 7, 3]                            # unsorted, with a duplicate
    golds[6] = [n_cand - 1]
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


# ------------------------------------------------------------------------------------------------ 4. ties and self-comparison
@pytest.mark.parametrize('d,l1', [(100, False), (36, False), (128, False), (100, True), (50, False)])
@pytest.mark.parametrize('kind', ['rows_x3', 'eighths', 'nan_row'])
def test_ties_and_unordered_scores_follow_the_keys(kind, d, l1):
    """Every key's gold meets itself in the sweep: ranks off by one across the board would mean that the list and sweep scores do not
    have the same bits.  Exact ties are broken by id; a NaN score is ordered by its key."""
    n_cand, nq = 300, 70
    E, R, Ep, Rp = seeded_tables(n_cand, 7, d, seed=3)
    if kind == 'rows_x3':
        E = E[:n_cand // 3].repeat_interleave(3, dim=0).contiguous()         # every row three times
    elif kind == 'eighths':
        gen = torch.Generator().manual_seed(9)
        E, R, Ep, Rp = ((torch.randint(-8, 9, w.shape, generator=gen).float() / 8).to(DEV) for w in (E, R, Ep, Rp))
    else:
        E = E.clone()
        E[37, d // 2] = float('nan')
    q, r = seeded_keys(n_cand, 7, nq, seed=4)
    golds, filts = seeded_lists(nq, n_cand, 3, seed=8)
    for desc in (False, True):
        both_routes((E, R, Ep, Rp), q, r, l1, True, desc, golds, filts, what='%s d=%d l1=%d desc=%d' % (kind, d, l1, desc))


# ------------------------------------------------------------------------------------------------ 5. layout
@pytest.mark.parametrize('l1', [True, False])
def test_strided_tables_and_a_candidate_slice(l1):
    d, ne, nq = 100, 400, 70
    W = seeded_tables(ne, 7, d, seed=21, pitch=(d + 4,))
    assert W[0].stride(0) == d + 4
    q, r = seeded_keys(ne, 7, nq, seed=22)
    golds, filts = seeded_lists(nq, ne, 3, seed=23)
    both_routes(W, q, r, l1, True, False, golds, filts, what='pitch d + 4')
    lo, hi = 130, 333                                         # ids local to the slice
    golds, filts = seeded_lists(nq, hi - lo, 3, seed=24)
    both_routes(W, q, r, l1, False, False, golds, filts, candidates=W[0][lo:hi], what='candidate slice, pitch d + 4')
    Wc = seeded_tables(ne, 7, d, seed=21)
    both_routes(Wc, q, r, l1, False, False, golds, filts, candidates=Wc[0][lo:hi], what='candidate slice, contiguous')


@pytest.mark.parametrize('l1', [True, False])
@pytest.mark.parametrize('layout', ['unaligned_base', 'odd_pitch'])
def test_unaligned_candidate_tables_take_the_pair_form_and_agree(layout, l1):
    d, ne, nq = 100, 300, 70
    W = seeded_tables(ne, 7, d, seed=31)
    if layout == 'unaligned_base':
        flat = torch.zeros(ne * d + 1, device=DEV)
        C = flat[1:].view(ne, d)
        assert C.data_ptr() % 16 == 4
    else:
        C = torch.zeros(ne, d + 1, device=DEV)[:, :d]
        assert C.stride(0) % 4 == 1
    C.copy_(W[0])
    q, r = seeded_keys(ne, 7, nq, seed=32)
    golds, filts = seeded_lists(nq, ne, 3, seed=33)
    got = both_routes(W, q, r, l1, True, False, golds, filts, candidates=C, what=layout)
    assert got == both_routes(W, q, r, l1, True, False, golds, filts, what=layout + ': the aligned table')


# ------------------------------------------------------------------------------------------------ 6. routing
@pytest.mark.parametrize('l1', [True, False])
def test_model_and_option_routing(l1):
    from jTransUP.models import transD
    d, ne, nq = 100, 300, 70
    E, R, Ep, Rp = seeded_tables(ne, 7, d, seed=41)
    q, r = seeded_keys(ne, 7, nq, seed=42)
    golds, filts = seeded_lists(nq, ne, 3, seed=43)
    want = both_routes((E, R, Ep, Rp), q, r, l1, True, False, golds, filts, what='routing reference')
    m = transD.TransDModel(l1, d, ne, 7)
    m.load_state_dict({n: w for n, w in zip(NAMES, (E, R, Ep, Rp))})
    g_off, g_ids = csr(golds)
    f_off, f_ids = csr(filts)
    default = ops().TRANSD_FUSED_DEFAULT[bool(l1)]
    got = m.rank_entities(q, r, True, False, g_off, g_ids, f_off, f_ids)
    assert ops().TRANSD_PASS_ROUTE[0].startswith('no score matrix' if default else 'chunked')
    assert got.cpu().numpy()[:len(want)].tolist() == want
    old = lib().set_option('transd_fused', 0)
    try:
        got = m.rank_entities(q, r, True, False, g_off, g_ids, f_off, f_ids)
        assert ops().TRANSD_PASS_ROUTE[0].startswith('chunked')
    finally:
        lib().set_option('transd_fused', old)
    assert got.cpu().numpy()[:len(want)].tolist() == want


def test_declined_shapes_take_the_chunked_route():
    L = lib().load()
    for d in (1, 20, 50, 100, 128, 300, 640):
        assert L.ktup_eval_kg_ranks_transd_fused_supported(d, 0, 3) == 1 and L.ktup_eval_kg_ranks_transd_fused_supported(d, 1, 99) == 1
    assert L.ktup_eval_kg_ranks_transd_fused_supported(644, 0, 3) == 0 and L.ktup_eval_kg_ranks_transd_fused_supported(0, 0, 3) == 0
    # more keys than one sweep takes: the call declines, the wrapper quietly ranks them chunk by chunk
    nq, ne = 65535 * 64 + 1, 3
    E, R, Ep, Rp = seeded_tables(ne, 2, 4, seed=51)
    q, r = seeded_keys(ne, 2, nq, seed=52)
    g_off = torch.arange(nq + 1, dtype=torch.int64, device=DEV)
    g_ids = (torch.arange(nq, device=DEV) % ne).to(torch.int32)
    with pytest.raises(lib().KtupError) as ei:
        ws = torch.empty(L.ktup_eval_kg_ranks_transd_fused_workspace_bytes(4, nq, nq, 0, ne), dtype=torch.uint8, device=DEV)
        ranks = torch.empty(nq, dtype=torch.int32, device=DEV)
        lib().call('ktup_eval_kg_ranks_transd_fused', E.data_ptr(), 4, Ep.data_ptr(), 4, R.data_ptr(), 4, Rp.data_ptr(), 4, 4, E.data_ptr(), 4, ne,
                   q.data_ptr(), r.data_ptr(), nq, 0, 1, 0, None, None, 0, g_off.data_ptr(), g_ids.data_ptr(), nq, 1, ranks.data_ptr(),
                   ws.data_ptr(), None)
    assert ei.value.code == lib().ERR_UNSUPPORTED
    got = ops().eval_kg_ranks_transd(E, R, Ep, Rp, q, r, False, True, False, g_off, g_ids, fused=True, chunk=65536)
    assert ops().TRANSD_PASS_ROUTE[0].startswith('chunked')
    want = ops().eval_kg_ranks_transd(E, R, Ep, Rp, q, r, False, True, False, g_off, g_ids, fused=False, chunk=65536)
    assert torch.equal(got, want) and int(got.min()) >= 0 and int(got.max()) <= ne - 1


def test_workspace_does_not_grow_with_keys_times_candidates():
    L = lib().load()
    big = L.ktup_eval_kg_ranks_transd_fused_workspace_bytes(100, 20480, 40960, 409600, 1000000)
    small = L.ktup_eval_kg_ranks_transd_fused_workspace_bytes(100, 20480, 40960, 409600, 1000)
    print('workspace bytes: %d at 1,000,000 candidates, %d at 1,000' % (big, small))
    assert 0 < big - small <= 16 * 999000 + 4096


# ------------------------------------------------------------------------------------------------ 7. the command line
@pytest.fixture(scope='module')
def dataset(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('ds')
    make_dataset(str(tmp))
    return tmp


METRIC_LINE = r'avg hit:\d\.\d+, avg mean rank:\d+\.\d+, topn:10'


def test_cli_reports_the_same_metrics_on_both_routes(dataset):
    extra = ['-kg_test_files', 'valid.dat:test.dat']
    fused, _ = run_cli(dataset, 'kg-transd-pass', extra, {'KTUP_TRANSD_FUSED': '1'})
    chunked, _ = run_cli(dataset, 'kg-transd-chunked', extra, {'KTUP_TRANSD_FUSED': '0'})
    rows, rows0 = re.findall(METRIC_LINE, fused), re.findall(METRIC_LINE, chunked)
    assert len(rows) >= 6 and rows == rows0
    assert 'TransD link-prediction pass: chunked score matrix (ktup_eval_kg_ranks_transd)' in chunked
    route = 'no score matrix (ktup_eval_kg_ranks_transd_fused)' if ops().TRANSD_FUSED_DEFAULT[False] else 'chunked score matrix'
    assert 'TransD link-prediction pass: ' + route in fused
