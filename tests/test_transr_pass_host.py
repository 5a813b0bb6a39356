"""Host-side surface of TransR's / CKE's link-prediction pass without the score matrix: the C header, the ctypes table, the Python
defaults and the recorded fixture.  No GPU."""
import inspect
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('ktup_eval_kg_ranks_transr_fused_supported', 'ktup_eval_kg_ranks_transr_fused_workspace_bytes', 'ktup_eval_kg_ranks_transr_fused')


def _declared_args(header, name):
    m = re.search(r'\b(?:int|size_t)\s+' + name + r'\s*\(([^;]*?)\)\s*;', header, re.S)
    assert m, name + ' is not declared in include/ktup_hip.h'
    return [a for a in m.group(1).split(',') if a.strip()]


def test_header_declares_the_entry_points_and_lib_binds_them():
    import ctypes
    from jTransUP.hip import lib as L
    header = open(os.path.join(ROOT, 'include', 'ktup_hip.h')).read()
    for name in SYMBOLS:
        args = _declared_args(header, name)
        assert name in L.SIGNATURES, name + ' has no binding row in jTransUP/hip/lib.py'
        assert len(L.SIGNATURES[name]) == len(args), '%s: %d arguments declared, %d bound' % (name, len(args), len(L.SIGNATURES[name]))
    assert L._RESTYPE['ktup_eval_kg_ranks_transr_fused_workspace_bytes'] is ctypes.c_size_t
    assert re.search(r'size_t\s+ktup_eval_kg_ranks_transr_fused_workspace_bytes', header)
    runtime = open(os.path.join(ROOT, 'joint-kg-recommender_amd', 'csrc', 'ktup_runtime.hip')).read()
    assert '{"transr_fused", "KTUP_TRANSR_FUSED"' in runtime


def test_python_defaults_and_model_surface():
    from jTransUP.hip import ops
    from jTransUP.models import CKE, transR
    assert set(ops.TRANSR_FUSED_DEFAULT) == {False, True} and all(isinstance(v, bool) for v in ops.TRANSR_FUSED_DEFAULT.values())
    assert ops.TRANSR_PASS_ROUTE == [None] or isinstance(ops.TRANSR_PASS_ROUTE[0], str)
    assert 'fused' in inspect.signature(ops.eval_kg_ranks_transr).parameters
    cke = inspect.signature(CKE.CKE.rank_entities).parameters
    assert list(cke)[:8] == ['self', 'q', 'r', 'head', 'descending', 'gold_off', 'gold_ids', 'filt_off'] and 'ents' in cke and 'all_e_ids' in cke
    assert list(inspect.signature(transR.TransRModel.rank_entities).parameters) == \
        ['self', 'q', 'r', 'head', 'descending', 'gold_off', 'gold_ids', 'filt_off', 'filt_ids', 'ents']


def test_fixture_records_its_margin_and_dropped_share():
    meta = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'transr_pass.json')))
    assert 0 < meta['tie_margin'] < 1e-3
    assert meta['n_ent'] == 230 and meta['n_rel'] == 5 and meta['dims'] == [64, 100]
    assert len(meta['cases']) == 8
    for name, case in meta['cases'].items():
        assert case['dropped_near_ties'] <= 0.05 * case['candidate_keys'], name
        assert len(case['keys']) == case['candidate_keys'] - case['dropped_near_ties']
        assert max(len(v) for _, _, v in case['eval']) <= 3
    for f in ('transr_pass.npz', 'transr_pass.json'):
        assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', f)) < 1000000
