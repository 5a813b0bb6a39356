"""The training step of the inner-product recommenders without a GPU: the width query, and host-side argument validation of the
two entry points (no launch is made)."""
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
    assert [loaded.ktup_train_dot_step_supported(d) for d in (1, 50, 256)] == [1, 1, 1]
    assert [loaded.ktup_train_dot_step_supported(d) for d in (0, 257)] == [0, 0]


def test_the_option_deterministic_declines(lib):
    loaded = lib.load()
    old = lib.set_option('deterministic', 1)
    try:
        assert loaded.ktup_train_dot_step_supported(50) == 0
        with pytest.raises(lib.KtupError) as e:
            lib.call('ktup_train_dot_step', 64, 64, 64, 64, None, 0, None, -1, None, None, None, 64, 64, 64, 5, 1.0, 1.0, 64, 64, 64,
                     None, None, None)
        assert e.value.code == ERR_UNSUPPORTED
    finally:
        lib.set_option('deterministic', old)
    assert loaded.ktup_train_dot_step_supported(50) == 1


def test_host_side_validation_of_the_step_entry_point(lib):
    """Every rejection happens before any launch (no GPU needed).  `p`: a non-null, 16-byte aligned dummy, validated, never
    dereferenced on the host."""
    p = 64

    def status(U=p, ldu=64, I=p, ldi=64, X=None, ldx=0, xmap=None, d=64, u=p, i=p, B=5, loss=p, gU=p, gI=p, gX=None):
        with pytest.raises(lib.KtupError) as e:
            lib.call('ktup_train_dot_step', U, ldu, I, ldi, X, ldx, xmap, -1, None, None, None, d, u, i, B, 1.0, 1.0, loss, gU, gI, gX,
                     None, None)
        assert 'ktup_train_dot_step' in str(e.value)
        return e.value.code

    assert status(B=0) == ERR_INVALID
    assert status(U=None) == ERR_INVALID
    assert status(X=p, ldx=64, gX=p) == ERR_INVALID             # a second item-side table without its map
    assert status(xmap=p) == ERR_INVALID                        # and the other way round
    assert status(X=p, ldx=64, xmap=p) == ERR_INVALID           # ... without its gradient
    assert status(d=0) == ERR_INVALID
    assert status(ldi=63) == ERR_INVALID                        # a pitch below the width
    assert status(loss=None) == ERR_INVALID
    assert status(gI=None) == ERR_INVALID
    assert status(d=257, ldu=257, ldi=257) == ERR_UNSUPPORTED
    assert lib.ERR_UNSUPPORTED == ERR_UNSUPPORTED


def test_host_side_validation_of_the_alignment_entry_point(lib):
    p = 64

    def rc(A=p, lda=36, B=p, ldb=36, d=36, a=p, b=p, n_dev=p, n_host=-1, cap=16, loss=p, gA=p, gB=p):
        return lib.load().ktup_reg_align_pairs(A, lda, B, ldb, d, a, b, n_dev, n_host, cap, 1, 1.0, loss, gA, gB, None)

    assert rc(n_host=17) == ERR_INVALID                         # more pairs than the fixed buffers hold, where the host knows
    assert rc(d=0) == ERR_INVALID
    assert rc(A=None) == ERR_INVALID
    assert rc(n_dev=None) == ERR_INVALID
    assert rc(lda=35) == ERR_INVALID
    assert rc(cap=-1) == ERR_INVALID
    assert rc(n_host=0) == 0                                    # nothing to add: no launch
    assert rc(cap=0, n_host=-1) == 0
