"""TransD without a GPU: the model factory and class surface, the workspace sizes, host-side argument validation of the entry
points, and the fixtures against their generator."""
import filecmp
import inspect
import json
import logging
import os
import subprocess
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')
# a checkout of the reference (TaoMiner/joint-kg-recommender): where the build container keeps it, or wherever the variable says
REFERENCE = os.environ.get('KTUP_REFERENCE_CHECKOUT', '/root/reference')


@pytest.fixture(scope='module')
def lib():
    from jTransUP.hip import lib as L
    if not os.path.exists(L.LIB_PATH):
        import importlib.util
        spec = importlib.util.spec_from_file_location('build_hip', os.path.join(ROOT, 'joint-kg-recommender_amd', 'build_hip.py'))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mod.build(verbose=False)
    return L


def _flags(**kw):
    return types.SimpleNamespace(**dict(dict(model_type='transd', L1_flag=False, embedding_size=20), **kw))


def test_init_model_builds_transd_with_the_reference_layout():
    from jTransUP.models.base import ACCELERATED, REFERENCE_ONLY, init_model
    assert 'transd' in ACCELERATED and 'transd' not in REFERENCE_ONLY
    torch.manual_seed(5)
    m = init_model(_flags(), 0, 0, 31, 6, logging.getLogger('transd-test'))
    sd = m.state_dict()
    assert sorted(sd) == ['ent_embeddings.weight', 'ent_proj_embeddings.weight', 'rel_embeddings.weight', 'rel_proj_embeddings.weight']
    assert tuple(sd['ent_embeddings.weight'].shape) == (31, 20) and tuple(sd['ent_proj_embeddings.weight'].shape) == (31, 20)
    assert tuple(sd['rel_embeddings.weight'].shape) == (6, 20) and tuple(sd['rel_proj_embeddings.weight'].shape) == (6, 20)
    for k in ('ent_embeddings.weight', 'rel_embeddings.weight'):
        assert torch.allclose(sd[k].float().cpu().norm(dim=1), torch.ones(sd[k].shape[0]), atol=1e-5), k
    for k in ('ent_proj_embeddings.weight', 'rel_proj_embeddings.weight'):
        assert float(sd[k].abs().max()) == 0.0, k
    assert (m.L1_flag, m.embedding_size, m.ent_total, m.rel_total, m.is_pretrained) == (False, 20, 31, 6, False)
    # none of the existing dispatches may take a TransD model for another one
    assert type(m).__name__ == 'TransDModel'
    assert not hasattr(m, 'norm_embeddings') and not hasattr(m, 'proj_embeddings') and not hasattr(m, 'prepare_entities')
    m.disable_grad()
    assert not any(p.requires_grad for p in m.parameters())
    m.enable_grad()
    assert all(p.requires_grad for p in m.parameters())


def test_class_surface_covers_the_reference():
    from jTransUP.models import transD
    rec = json.load(open(os.path.join(GOLD, 'transd.json')))
    assert rec['reference_evaluateTail_raises_NameError'] is True
    surface = rec['surface']
    assert 'build_model' in surface['functions'] and 'TransHModel' in surface['classes']
    for name, args in surface['functions'].items():
        ours = list(inspect.signature(getattr(transD, name)).parameters)
        assert ours[:len(args)] == args, (name, ours, args)
    for cname, methods in surface['classes'].items():
        cls = getattr(transD, cname)
        assert cls is transD.TransDModel
        for mname, args in methods.items():
            ours = list(inspect.signature(getattr(cls, mname)).parameters)
            assert ours[:len(args)] == args, (cname, mname, ours, args)
    for extra in ('rank_entities', 'evaluateHead', 'evaluateTail', 'forward', 'disable_grad', 'enable_grad'):
        assert callable(getattr(transD.TransDModel, extra))


def test_workspace_sizes(lib):
    loaded = lib.load()
    assert loaded.ktup_eval_transd_workspace_bytes(100, 512) == (512 * 3 * 100 + 512 * 4) * 4
    assert loaded.ktup_eval_transd_workspace_bytes(50, 8) == (8 * 3 * 52 + 8 * 4) * 4      # rows padded to whole 16-byte chunks
    assert loaded.ktup_eval_transd_workspace_bytes(0, 8) == 0
    assert loaded.ktup_eval_kg_ranks_transd_workspace_bytes(100, 230, 16) >= 2 * 16 * 230 * 4 + loaded.ktup_eval_transd_workspace_bytes(100, 16)


def test_host_side_validation_of_the_transd_entry_points(lib):
    """Every rejection happens before any launch (no GPU needed).  `p`: a non-null dummy, validated, never dereferenced on the host."""
    p = 16
    with pytest.raises(lib.KtupError) as e:                # d <= 0
        lib.call('ktup_score_transd_fwd', p, 100, p, 100, p, 100, p, 100, 0, p, p, p, 5, 0, p, None)
    assert 'embedding_size' in str(e.value) and e.value.code == -1
    with pytest.raises(lib.KtupError) as e:                # null relation-projection table
        lib.call('ktup_score_transd_fwd', p, 100, p, 100, p, 100, None, 100, 100, p, p, p, 5, 0, p, None)
    assert 'Rp' in str(e.value)
    with pytest.raises(lib.KtupError) as e:
        lib.call('ktup_score_transd_bwd', p, 100, p, 100, p, 100, p, 100, -4, p, p, p, 5, 0, p, p, p, p, p, None)
    assert 'embedding_size' in str(e.value)
    with pytest.raises(lib.KtupError) as e:                # null gradient buffer of the entity projections
        lib.call('ktup_score_transd_bwd', p, 100, p, 100, p, 100, p, 100, 100, p, p, p, 5, 0, p, p, p, None, p, None)
    assert 'gEp' in str(e.value)
    with pytest.raises(lib.KtupError):                     # d <= 0
        lib.call('ktup_eval_transd_scores', p, 100, p, 100, p, 100, p, 100, 0, p, 100, 50, p, p, 4, 0, 1, p, 50, p, None)
    with pytest.raises(lib.KtupError) as e:                # null entity-projection table
        lib.call('ktup_eval_transd_scores', p, 100, None, 100, p, 100, p, 100, 100, p, 100, 50, p, p, 4, 0, 1, p, 50, p, None)
    assert 'null pointer' in str(e.value)
    with pytest.raises(lib.KtupError) as e:                # output pitch below the number of candidates
        lib.call('ktup_eval_transd_scores', p, 100, p, 100, p, 100, p, 100, 100, p, 100, 50, p, p, 4, 0, 1, p, 49, p, None)
    assert 'pitch' in str(e.value)
    with pytest.raises(lib.KtupError):                     # d <= 0
        lib.call('ktup_eval_kg_ranks_transd', p, 100, p, 100, p, 100, p, 100, 0, p, 100, 50, p, p, 4, 0, 1, 0, None, None, p, p, p, 512, p, None)
    with pytest.raises(lib.KtupError) as e:                # null table
        lib.call('ktup_eval_kg_ranks_transd', p, 100, p, 100, None, 100, p, 100, 100, p, 100, 50, p, p, 4, 0, 1, 0, None, None, p, p, p, 512, p, None)
    assert 'null pointer' in str(e.value)
    with pytest.raises(lib.KtupError) as e:                # filter offsets without ids
        lib.call('ktup_eval_kg_ranks_transd', p, 100, p, 100, p, 100, p, 100, 100, p, 100, 50, p, p, 4, 0, 1, 0, p, None, p, p, p, 512, p, None)
    assert 'filter' in str(e.value)
    # the wrapper's own check: CSR offsets are nq + 1 long
    from jTransUP.hip import ops
    E, R = torch.zeros(9, 8), torch.zeros(3, 8)
    q = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(lib.KtupError) as e:
        ops.eval_kg_ranks_transd(E, R, E, R, q, q, False, True, False, torch.zeros(4, dtype=torch.int64), torch.zeros(4, dtype=torch.int32))
    assert 'len(q) + 1' in str(e.value)
    with pytest.raises(lib.KtupError) as e:
        ops.eval_kg_ranks_transd(E, R, E, R, q, q, False, True, False, torch.zeros(5, dtype=torch.int64), torch.zeros(4, dtype=torch.int32),
                                 torch.zeros(7, dtype=torch.int64), torch.zeros(4, dtype=torch.int32))
    assert 'len(q) + 1' in str(e.value)


def test_cpu_tensors_fail_loudly(lib):
    from jTransUP.models import transD
    if torch.cuda.is_available():
        pytest.skip('GPU present: covered by the gpu tests')
    m = transD.TransDModel(False, 8, 5, 3)
    with pytest.raises(lib.KtupError):
        m(torch.tensor([0]), torch.tensor([1]), torch.tensor([2]))
    with pytest.raises(lib.KtupError):
        m.evaluateTail(torch.tensor([0]), torch.tensor([1]))


def test_fixtures_are_what_the_generator_writes(tmp_path):
    """Regenerating from the reference reproduces the committed files byte for byte (the reference is not on every machine)."""
    if not os.path.isdir(os.path.join(REFERENCE, 'jTransUP')):
        pytest.skip('the reference checkout is not on this machine')
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE='1')
    subprocess.run([sys.executable, os.path.join(GOLD, 'make_transd_goldens.py'), '--ref', REFERENCE, '--out', str(tmp_path)],
                   check=True, env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
    for name in ('transd.npz', 'transd.json'):
        assert filecmp.cmp(os.path.join(GOLD, name), str(tmp_path / name), shallow=False), name
    rec = json.load(open(os.path.join(GOLD, 'transd.json')))
    for case in rec['rank']['cases'].values():
        assert case['dropped_near_ties'] <= 0.05 * case['candidate_keys']
    assert os.path.getsize(os.path.join(GOLD, 'transd.npz')) + os.path.getsize(os.path.join(GOLD, 'transd.json')) < 1024 * 1024
