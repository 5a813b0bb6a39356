"""CFKG's one-launch rec step and one-sweep rec evaluation pass without a GPU: the width query, the workspace size, the model's, the
stepper's and the wrapper's surface, and host-side argument validation of both entry points (no launch is made)."""
import ctypes
import inspect
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID, ERR_UNSUPPORTED = -1, -3


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


def test_supported_widths(lib):
    loaded = lib.load()
    assert [loaded.ktup_train_cfkg_rec_step_supported(d) for d in (1, 50, 256)] == [1, 1, 1]
    assert [loaded.ktup_train_cfkg_rec_step_supported(d) for d in (0, 257)] == [0, 0]


def test_the_option_deterministic_declines_without_a_launch(lib):
    loaded = lib.load()
    old = lib.set_option('deterministic', 1)
    try:
        assert loaded.ktup_train_cfkg_rec_step_supported(50) == 0
        with pytest.raises(lib.KtupError) as e:
            lib.call('ktup_train_cfkg_rec_step', 64, 64, 64, 64, 64, 64, 3, 64, 64, 64, 5, 1, -1.0, 1.0, 64, 64, 64, 64, None)
        assert e.value.code == ERR_UNSUPPORTED
    finally:
        lib.set_option('deterministic', old)
    assert loaded.ktup_train_cfkg_rec_step_supported(50) == 1


def test_host_side_validation_of_the_step_entry_point(lib):
    """Every rejection happens before any launch (no GPU needed).  `p`: a non-null, 16-byte aligned dummy, validated, never
    dereferenced on the host."""
    p = 64

    def status(U=p, ldu=64, E=p, lde=64, R=p, ldr=64, rel=3, d=64, u=p, i=p, B=5, loss=p, gU=p, gE=p, gR=p):
        with pytest.raises(lib.KtupError) as e:
            lib.call('ktup_train_cfkg_rec_step', U, ldu, E, lde, R, ldr, rel, d, u, i, B, 0, -1.0, 1.0, loss, gU, gE, gR, None)
        assert 'ktup_train_cfkg_rec_step' in str(e.value)
        return e.value.code

    for name in ('U', 'E', 'R', 'u', 'i', 'loss', 'gU', 'gE', 'gR'):
        assert status(**{name: None}) == ERR_INVALID, name
    assert status(B=0) == ERR_INVALID
    assert status(d=0) == ERR_INVALID
    for name in ('ldu', 'lde', 'ldr'):
        assert status(**{name: 63}) == ERR_INVALID, name        # a pitch below the width
    assert status(rel=-1) == ERR_INVALID
    assert status(d=257, ldu=257, lde=257, ldr=257) == ERR_UNSUPPORTED
    assert lib.ERR_UNSUPPORTED == ERR_UNSUPPORTED


def test_workspace_sizes(lib):
    fn = lib.load().ktup_eval_cfkg_topk_workspace_bytes
    assert fn.restype is ctypes.c_size_t
    # the partial lists of the splits (8 bytes a key), one filter bit per (user, candidate), one float per candidate
    one = fn(64, 100, 3240, 10, 1)
    assert one >= 100 * 10 * 8 + 100 * ((3240 + 31) // 32) * 4 + 3240 * 4
    sizes = [fn(64, 100, 3240, 10, ns) for ns in (1, 2, 3, 4, 8)]
    assert sizes == sorted(sizes) and sizes[3] >= one + 100 * 10 * 8 * 3        # monotone in nsplit
    assert fn(64, 100, 3240, 10, 0) >= one
    assert fn(64, 0, 3240, 10, 0) == 0
    assert fn(64, 100, 3240, 17, 0) == 0


def test_host_side_validation_of_the_pass_entry_point(lib):
    p = 64

    def status(U=p, ldu=64, R=p, ldr=64, rel=3, E=p, lde=64, ne=100, cand=None, nc=100, d=64, u=p, nq=5, topn=10, nsplit=0, top=p, ws=p,
               fo=None, fi=None):
        with pytest.raises(lib.KtupError) as e:
            lib.call('ktup_eval_cfkg_topk', U, ldu, R, ldr, rel, E, lde, ne, cand, nc, d, u, nq, 1, fo, fi, topn, nsplit, top, None, ws, None)
        assert 'ktup_eval_cfkg_topk' in str(e.value)
        return e.value.code

    for name in ('U', 'R', 'E', 'u', 'top', 'ws'):
        assert status(**{name: None}) == ERR_INVALID, name
    assert status(nq=-1) == ERR_INVALID
    assert status(topn=0) == ERR_INVALID
    assert status(d=0) == ERR_INVALID
    assert status(nc=0, cand=p) == ERR_INVALID
    assert status(nc=99) == ERR_INVALID                         # no cand_ids: the candidates are the entity rows, all of them
    for name in ('ldu', 'ldr', 'lde'):
        assert status(**{name: 63}) == ERR_INVALID, name        # a pitch below the width
    assert status(rel=-1) == ERR_INVALID
    assert status(fo=p) == ERR_INVALID                          # filter offsets without ids
    assert status(nsplit=-1) == ERR_INVALID
    assert status(d=257, ldu=257, ldr=257, lde=257) == ERR_UNSUPPORTED
    assert status(topn=17) == ERR_UNSUPPORTED
    assert status(nc=2 ** 31, cand=p) == ERR_UNSUPPORTED
    assert status(nc=2 ** 31, ne=2 ** 31) == ERR_UNSUPPORTED
    # an empty pass is fine and launches nothing
    assert lib.load().ktup_eval_cfkg_topk(p, 64, p, 64, 3, p, 64, 100, None, 100, 64, p, 0, 1, None, None, 10, 0, p, None, p, None) == 0


def test_model_wrapper_and_stepper_surface():
    from jTransUP.hip import ops
    from jTransUP.models import CFKG
    from jTransUP.utils import fast_train_dot
    cls = CFKG.CFKG
    assert list(inspect.signature(cls.evaluate_topk).parameters) == ['self', 'u_ids', 'items', 'topn', 'filt_off', 'filt_ids']
    assert cls.topk_descending is False
    assert not hasattr(cls, 'prepare_items')                    # the drivers key the TUP item-side cache and `items=` on it
    par = inspect.signature(ops.eval_cfkg_topk).parameters
    assert list(par) == ['U', 'R', 'rel', 'E', 'u', 'topn', 'l1', 'cand_ids', 'filt_off', 'filt_ids', 'with_scores', 'nsplit']
    assert par['nsplit'].default == 0 and par['with_scores'].default is False and par['cand_ids'].default is None
    # BaselineJointStepper takes a CFKG model: its third case binds the one-launch rec step to tables (U, E, R)
    assert callable(fast_train_dot.cfkg_step_supported)
    src = inspect.getsource(fast_train_dot.BaselineJointStepper)
    assert 'self.cfkg' in src and "'ktup_train_cfkg_rec_step'" in src and 'self.tabs = (U, E, R)' in src
    assert "touch = {'rec': (U, E, R), 'kg': (E, R)}" in src


def test_the_joint_driver_routes_cfkg_to_the_stepper_and_the_pass():
    from jTransUP.models import knowledgable_recommendation as K
    src = inspect.getsource(K.train_loop)
    assert "('cofm', 'cke', 'cfkg')" in src and "cofm, cke, cfkg'" in src
    src = inspect.getsource(K.evaluateRec)
    assert 'topk_takes_candidates' in src and 'cand.data_ptr()' in src       # the candidate ids are part of the capture's key


def test_wrapper_rejects_cpu_tensors(lib):
    import torch
    from jTransUP.hip import ops
    U, R, E = torch.zeros(9, 8), torch.zeros(3, 8), torch.zeros(7, 8)
    with pytest.raises(lib.KtupError):
        ops.eval_cfkg_topk(U, R, 2, E, torch.zeros(4, dtype=torch.int64), 10, True)
