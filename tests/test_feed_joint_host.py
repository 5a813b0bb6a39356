"""ktup_feed_remap_ids / ktup_feed_align_lists (csrc/ktup_feed_joint.hip) without a GPU: the three new symbols are declared, exported and
bound, and everything that cannot work is refused on the host before any launch.  (`BaselineJointStepper.can_feed` needs a device:
tests/test_fast_train_dot_fed.py.)"""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'ktup_hip.h')
NEW = ['ktup_feed_align_lists', 'ktup_feed_align_lists_supported', 'ktup_feed_align_lists_workspace_bytes', 'ktup_feed_remap_ids']
P = 16                      # a non-null dummy pointer: validated, never dereferenced on the host


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


def test_the_new_symbols_are_declared_exported_and_bound(lib):
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    handle = ctypes.CDLL(lib.LIB_PATH)
    for name in NEW:
        assert re.search(r'\b%s\s*\(' % name, text), name + ' is not declared in include/ktup_hip.h'
        assert hasattr(handle, name), name + ' is not exported'
        assert name in lib.SIGNATURES, name + ' is not bound'
    assert lib._RESTYPE['ktup_feed_align_lists_workspace_bytes'] is ctypes.c_size_t
    assert len(lib.SIGNATURES['ktup_feed_remap_ids']) == 8 and len(lib.SIGNATURES['ktup_feed_align_lists']) == 13


def test_supported_id_counts(lib):
    so = lib.load()
    top = 4 * 4096
    assert so.ktup_feed_align_lists_supported(1) == 1 and so.ktup_feed_align_lists_supported(1600) == 1
    assert so.ktup_feed_align_lists_supported(top) == 1
    assert so.ktup_feed_align_lists_supported(0) == 0 and so.ktup_feed_align_lists_supported(-5) == 0
    # the table must stay at most half full: whatever the largest accepted count is, the next one is refused
    hi = top
    while so.ktup_feed_align_lists_supported(2 * hi):
        hi *= 2
        assert hi < 1 << 40
    assert so.ktup_feed_align_lists_supported(2 * hi) == 0


def _align(lib, a=P, na=8, b=None, nb=0, partner=P, n_partner=100, ent=0, cap=8, n_out=P, e_ids=P, i_ids=P, ws=None):
    lib.call('ktup_feed_align_lists', a, na, b, nb, partner, n_partner, ent, cap, n_out, e_ids, i_ids, ws, None)


def test_align_lists_refuses_before_any_launch(lib):
    so = lib.load()
    with pytest.raises(lib.KtupError) as e:
        _align(lib, na=8, b=P, nb=8, cap=15)
    assert 'cap' in str(e.value) and e.value.code == -1            # KTUP_ERR_INVALID_ARG
    for bad in ({'n_out': None}, {'e_ids': None}, {'i_ids': None}, {'partner': None}):
        with pytest.raises(lib.KtupError) as e:
            _align(lib, **bad)
        assert 'null' in str(e.value) and e.value.code == -1
    with pytest.raises(lib.KtupError) as e:
        _align(lib, na=0, nb=0, cap=8)
    assert 'no ids' in str(e.value)
    with pytest.raises(lib.KtupError):                             # ids promised, no array
        _align(lib, a=None, na=8)
    with pytest.raises(lib.KtupError):
        _align(lib, b=None, nb=3, cap=11)
    with pytest.raises(lib.KtupError):
        _align(lib, n_partner=0)
    with pytest.raises(lib.KtupError):
        _align(lib, n_partner=1 << 31)
    n = 1
    while so.ktup_feed_align_lists_supported(n):
        n *= 2
    with pytest.raises(lib.KtupError) as e:                        # an id count beyond _supported
        _align(lib, na=n, cap=n)
    assert e.value.code == lib.ERR_UNSUPPORTED
    for n in (1, 1600, 4 * 4096):                                  # a missing workspace wherever one is asked for
        if so.ktup_feed_align_lists_workspace_bytes(n) > 0:
            with pytest.raises(lib.KtupError):
                _align(lib, na=n, cap=n, ws=None)


def test_remap_refuses_before_any_launch(lib):
    with pytest.raises(lib.KtupError) as e:
        lib.call('ktup_feed_remap_ids', None, 10, P, 4, None, 0, None, None)
    assert 'null' in str(e.value)
    with pytest.raises(lib.KtupError):
        lib.call('ktup_feed_remap_ids', P, 10, None, 4, None, 0, None, None)
    with pytest.raises(lib.KtupError):
        lib.call('ktup_feed_remap_ids', P, 10, P, 4, None, 3, None, None)
    with pytest.raises(lib.KtupError):
        lib.call('ktup_feed_remap_ids', P, 0, P, 4, None, 0, None, None)
    with pytest.raises(lib.KtupError):
        lib.call('ktup_feed_remap_ids', P, 10, P, -1, None, 0, None, None)
    lib.call('ktup_feed_remap_ids', P, 10, None, 0, None, 0, None, None)      # nothing to do is not an error, and launches nothing
