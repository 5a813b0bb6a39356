"""The wide-list evaluation passes (ktup_eval_dot_topk_wide, ktup_eval_cfkg_topk_wide: cut-offs up to 64) without a GPU: the symbols,
the workspace sizes and the split rule, host-side argument validation of both entry points (no launch is made), the narrow entry
points' unchanged cap, and the Python surface."""
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


def test_the_four_symbols_and_their_return_types(lib):
    loaded = lib.load()
    for name in ('ktup_eval_dot_topk_wide', 'ktup_eval_cfkg_topk_wide'):
        assert name in lib.SIGNATURES and name + '_workspace_bytes' in lib.SIGNATURES
        assert getattr(loaded, name).restype is ctypes.c_int
        assert getattr(loaded, name + '_workspace_bytes').restype is ctypes.c_size_t
        assert lib.SIGNATURES[name] == lib.SIGNATURES[name.replace('_wide', '')]          # the narrow entry point's argument list
        assert lib.SIGNATURES[name + '_workspace_bytes'] == lib.SIGNATURES[name.replace('_wide', '') + '_workspace_bytes']


@pytest.mark.parametrize('entry,cand_floats', [('ktup_eval_dot_topk_wide', 0), ('ktup_eval_cfkg_topk_wide', 1)])
def test_workspace_sizes_and_the_split_rule(lib, entry, cand_floats):
    fn = getattr(lib.load(), entry + '_workspace_bytes')
    nq, n = 100, 4000                                                           # (1 to 8 and 25 splits of whole 16-candidate tiles)
    bits = nq * ((n + 31) // 32) * 4 + cand_floats * n * 4
    one = fn(64, nq, n, 64, 1)
    assert one >= nq * 64 * 8 + bits
    sizes = [fn(64, nq, n, 64, ns) for ns in range(1, 9)]
    assert sizes == sorted(sizes) and len(set(sizes)) == 8                      # grows with every split up to 8 ...
    assert sizes[7] >= one + nq * 64 * 8 * 7
    assert [fn(64, nq, n, 64, ns) for ns in (9, 17, 32)] == [sizes[7]] * 3      # ... and no further: 512 / 64 splits is what the merge holds
    assert fn(64, nq, n, 20, 32) >= nq * 20 * 8 * 25 + bits                     # 512 / 20 = 25 splits at topn 20
    assert fn(64, nq, n, 20, 32) == fn(64, nq, n, 20, 25) > fn(64, nq, n, 20, 20)
    assert fn(64, nq, n, 64, 0) >= one
    assert fn(64, nq, n, 10, 1) >= nq * 10 * 8 + bits                           # values at or below 16 are accepted
    assert fn(64, nq, n, 65, 0) == 0
    assert fn(64, nq, n, 0, 0) == 0
    assert fn(64, 0, n, 64, 0) == 0


def test_host_side_validation_of_the_wide_dot_entry_point(lib):
    """Every rejection happens before any launch (no GPU needed).  `p`: a non-null, 16-byte aligned dummy, validated, never
    dereferenced on the host."""
    p = 64

    def status(U=p, ldu=64, I=p, ldi=64, d=64, u=p, nq=5, ni=100, topn=50, nsplit=0, top=p, ws=p, fo=None, fi=None):
        with pytest.raises(lib.KtupError) as e:
            lib.call('ktup_eval_dot_topk_wide', U, ldu, I, ldi, d, u, nq, ni, None, None, fo, fi, topn, nsplit, top, None, ws, None)
        assert 'ktup_eval_dot_topk_wide' in str(e.value)
        return e.value.code

    for name in ('U', 'I', 'u', 'top', 'ws'):
        assert status(**{name: None}) == ERR_INVALID, name
    assert status(topn=0) == ERR_INVALID
    assert status(ldu=63) == ERR_INVALID                    # a pitch below the width
    assert status(ldi=63) == ERR_INVALID
    assert status(nsplit=-2) == ERR_INVALID
    assert status(fo=p) == ERR_INVALID                      # filter offsets without ids
    assert status(ws=72) == ERR_INVALID                     # a workspace off the 16-byte boundary
    assert status(topn=65) == ERR_UNSUPPORTED
    assert status(d=257, ldu=257, ldi=257) == ERR_UNSUPPORTED
    assert status(ni=2 ** 31) == ERR_UNSUPPORTED
    # an empty pass is fine and launches nothing, at every list width
    for topn in (1, 16, 17, 32, 33, 64):
        assert lib.load().ktup_eval_dot_topk_wide(p, 64, p, 64, 64, p, 0, 100, None, None, None, None, topn, 0, p, None, p, None) == 0


def test_host_side_validation_of_the_wide_cfkg_entry_point(lib):
    p = 64

    def status(U=p, ldu=64, R=p, ldr=64, rel=3, E=p, lde=64, ne=100, cand=None, nc=100, d=64, u=p, nq=5, topn=50, nsplit=0, top=p, ws=p,
               fo=None, fi=None):
        with pytest.raises(lib.KtupError) as e:
            lib.call('ktup_eval_cfkg_topk_wide', U, ldu, R, ldr, rel, E, lde, ne, cand, nc, d, u, nq, 1, fo, fi, topn, nsplit, top, None, ws,
                     None)
        assert 'ktup_eval_cfkg_topk_wide' in str(e.value)
        return e.value.code

    for name in ('U', 'R', 'E', 'u', 'top', 'ws'):
        assert status(**{name: None}) == ERR_INVALID, name
    assert status(topn=0) == ERR_INVALID
    for name in ('ldu', 'ldr', 'lde'):
        assert status(**{name: 63}) == ERR_INVALID, name        # a pitch below the width
    assert status(nsplit=-2) == ERR_INVALID
    assert status(fo=p) == ERR_INVALID                          # filter offsets without ids
    assert status(nc=99) == ERR_INVALID                         # no cand_ids: the candidates are the entity rows, all of them
    assert status(topn=65) == ERR_UNSUPPORTED
    assert status(d=257, ldu=257, ldr=257, lde=257) == ERR_UNSUPPORTED
    assert status(nc=2 ** 31, cand=p) == ERR_UNSUPPORTED
    assert status(nc=2 ** 31, ne=2 ** 31) == ERR_UNSUPPORTED
    for topn in (1, 16, 17, 32, 33, 64):
        assert lib.load().ktup_eval_cfkg_topk_wide(p, 64, p, 64, 3, p, 64, 100, None, 100, 64, p, 0, 1, None, None, topn, 0, p, None, p,
                                                   None) == 0


def test_the_narrow_entry_points_keep_their_cap(lib):
    p = 64
    with pytest.raises(lib.KtupError) as e:
        lib.call('ktup_eval_dot_topk', p, 64, p, 64, 64, p, 5, 100, None, None, None, None, 17, 0, p, None, p, None)
    assert e.value.code == ERR_UNSUPPORTED and 'topn 17 > 16' in str(e.value)
    with pytest.raises(lib.KtupError) as e:
        lib.call('ktup_eval_cfkg_topk', p, 64, p, 64, 3, p, 64, 100, None, 100, 64, p, 5, 1, None, None, 17, 0, p, None, p, None)
    assert e.value.code == ERR_UNSUPPORTED and 'topn 17 > 16' in str(e.value)
    assert lib.load().ktup_eval_dot_topk_workspace_bytes(64, 100, 3240, 17, 0) == 0
    assert lib.load().ktup_eval_cfkg_topk_workspace_bytes(64, 100, 3240, 17, 0) == 0
    assert lib.load().ktup_eval_dot_topk_workspace_bytes(64, 100, 3240, 16, 32) >= 100 * 16 * 8 * 32      # 32 splits up to topn 16


def test_python_surface(lib):
    import torch
    from jTransUP.hip import ops
    for narrow, wide in ((ops.eval_dot_topk, ops.eval_dot_topk_wide), (ops.eval_cfkg_topk, ops.eval_cfkg_topk_wide)):
        assert inspect.signature(wide) == inspect.signature(narrow)
    assert (ops.TOPN_MAX, ops.TOPN_WIDE_MAX) == (16, 64)
    with pytest.raises(lib.KtupError):
        ops.eval_dot_topk_wide(torch.zeros(9, 8), torch.zeros(7, 8), torch.zeros(4, dtype=torch.int64), 20)
    with pytest.raises(lib.KtupError):
        ops.eval_cfkg_topk_wide(torch.zeros(9, 8), torch.zeros(3, 8), 2, torch.zeros(7, 8), torch.zeros(4, dtype=torch.int64), 20, True)


def test_the_option_and_the_route_choice(lib):
    """eval_wide_topn: -1 = the measured default of the model (ops.WIDE_TOPN_DEFAULT), 0 = the batch walk above 16, 1 = the wide
    sweep; up to 16 the narrow wrapper whatever the option says, above 64 nothing."""
    from jTransUP.hip import ops
    assert set(ops.WIDE_TOPN_DEFAULT) == {'dot', 'cfkg_l1', 'cfkg_l2'}
    old = lib.get_option('eval_wide_topn')
    try:
        for value in (-1, 0, 1):
            lib.set_option('eval_wide_topn', value)
            for model, default in ops.WIDE_TOPN_DEFAULT.items():
                wide = 'wide' if value == 1 or (value == -1 and default) else None
                got = [ops.topk_sweep_for(topn, 'narrow', 'wide', model) for topn in (1, 16, 17, 20, 64, 65)]
                assert got == ['narrow', 'narrow', wide, wide, wide, None], (value, model)
    finally:
        lib.set_option('eval_wide_topn', old)
