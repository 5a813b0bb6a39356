"""The wide-list evaluation passes of TUP / KTUP (ktup_eval_pref_topk_wide, ktup_eval_pref_topk_hard_wide: cut-offs up to 64) without
a GPU: the symbols, host-side argument validation of both entry points (no launch is made), the workspace sizes, the narrow entry
points' unchanged cap, and the route choice of the Python surface."""
import ctypes
import inspect
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID, ERR_UNSUPPORTED = -1, -3
WIDE = ('ktup_eval_pref_topk_wide', 'ktup_eval_pref_topk_hard_wide')


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


def _header_arity(name):
    """Parameters of `name`'s prototype in include/ktup_hip.h."""
    import re
    text = open(os.path.join(ROOT, 'include', 'ktup_hip.h')).read()
    m = re.search(r'\b' + name + r'\(([^;]*?)\);', text)
    assert m, name
    return len(m.group(1).split(','))


def test_the_four_symbols_and_their_arities(lib):
    loaded = lib.load()
    for name in WIDE:
        narrow = name.replace('_wide', '')
        assert name in lib.SIGNATURES and name + '_workspace_bytes' in lib.SIGNATURES
        assert getattr(loaded, name).restype is ctypes.c_int
        assert getattr(loaded, name + '_workspace_bytes').restype is ctypes.c_size_t
        assert lib.SIGNATURES[name] == lib.SIGNATURES[narrow]                     # the narrow entry point's argument list
        assert lib.SIGNATURES[name + '_workspace_bytes'] == lib.SIGNATURES[narrow + '_workspace_bytes']
        assert len(lib.SIGNATURES[name]) == _header_arity(name) == _header_arity(narrow)
        assert len(lib.SIGNATURES[name + '_workspace_bytes']) == _header_arity(name + '_workspace_bytes') == 5


def test_host_side_validation_of_the_wide_preference_space_entry(lib):
    """Every rejection happens before any launch.  `p`: a non-null, 16-byte aligned dummy, validated, never dereferenced on the host."""
    p = 64
    entry = 'ktup_eval_pref_topk_wide'

    def call(U=p, I=p, pws=p, u=p, nq=5, ni=100, l1=0, topn=50, top=p, ws=p, fo=None, fi=None, d=64, E=None, i2e=None, raw=False):
        args = (U, d, I, d, E, d, i2e, pws, 20, d, u, nq, ni, l1, fo, fi, topn, top, None, ws, None)
        return getattr(lib.load(), entry)(*args) if raw else lib.call(entry, *args)

    def status(**kw):
        with pytest.raises(lib.KtupError) as e:
            call(**kw)
        assert entry in str(e.value)                          # the error names the entry point
        return e.value.code

    for name in ('U', 'I', 'pws', 'u', 'top', 'ws'):
        assert status(**{name: None}) == ERR_INVALID, name
    assert status(topn=0) == ERR_INVALID
    assert status(fo=p) == ERR_INVALID                        # filter offsets without ids
    assert status(E=p) == ERR_INVALID                         # E without item2ent
    assert status(ws=72) == ERR_INVALID                       # a workspace off the 16-byte boundary
    assert status(topn=65) == ERR_UNSUPPORTED
    assert status(topn=65, nq=0) == ERR_UNSUPPORTED
    assert status(l1=1) == ERR_UNSUPPORTED                    # as the narrow entry point: squared L2 only
    for topn in (1, 16, 17, 32, 33, 64):                      # an empty pass is fine and launches nothing, at every list width
        assert call(nq=0, topn=topn, raw=True) == 0


def test_host_side_validation_of_the_wide_sweep_entry(lib):
    p = 64
    entry = 'ktup_eval_pref_topk_hard_wide'

    def call(U=p, I=p, pws=p, u=p, nq=5, ni=100, l1=0, mode=0, uni=None, topn=50, top=p, ws=p, fo=None, fi=None, d=64, P=20, raw=False):
        args = (U, d, I, d, None, d, None, pws, P, d, u, nq, ni, l1, mode, uni, 1, 0, fo, fi, topn, top, None, ws, None)
        return getattr(lib.load(), entry)(*args) if raw else lib.call(entry, *args)

    def status(**kw):
        with pytest.raises(lib.KtupError) as e:
            call(**kw)
        assert entry in str(e.value)
        return e.value.code

    for name in ('U', 'I', 'pws', 'u', 'top', 'ws'):
        assert status(**{name: None}) == ERR_INVALID, name
    assert status(topn=0) == ERR_INVALID
    assert status(topn=0, nq=0) == ERR_INVALID
    assert status(fo=p) == ERR_INVALID
    assert status(ws=72) == ERR_INVALID
    assert status(mode=1) == ERR_INVALID                      # KTUP_GUMBEL_INPUT without the uniform tensor
    assert status(mode=4) == ERR_INVALID
    assert status(P=33) == ERR_INVALID                        # as the narrow entry point
    assert status(topn=65) == ERR_UNSUPPORTED
    assert status(topn=65, nq=0) == ERR_UNSUPPORTED
    assert status(d=260) == ERR_UNSUPPORTED
    for topn in (1, 16, 17, 32, 33, 64):
        assert call(nq=0, topn=topn, raw=True) == 0


def test_workspace_sizes(lib):
    loaded = lib.load()
    d, P, nq, ni = 100, 20, 6040, 3240
    for name in WIDE:
        fn = getattr(loaded, name + '_workspace_bytes')
        narrow = getattr(loaded, name.replace('_wide', '') + '_workspace_bytes')
        assert fn(d, P, nq, ni, 64) >= narrow(d, P, nq, ni, 16)
        sizes = [fn(d, P, nq, ni, t) for t in (1, 16, 17, 20, 32, 33, 50, 64)]
        assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes)          # the partial lists are sized by topn
        assert sizes[-1] - sizes[0] >= nq * 8 * 63 * 8                            # 8 splits x topn keys per user
        assert fn(d, P, nq, ni, 65) == 0
        assert fn(d, P, nq, ni, 0) == 0
    assert loaded.ktup_eval_pref_topk_wide_workspace_bytes(d, P, 0, ni, 20) == 0


def test_the_narrow_entry_points_answer_as_before(lib):
    p = 64
    with pytest.raises(lib.KtupError) as e:
        lib.call('ktup_eval_pref_topk', p, 64, p, 64, None, 64, None, p, 20, 64, p, 5, 100, 0, None, None, 17, p, None, p, None)
    assert e.value.code == ERR_UNSUPPORTED and 'no fused pass kernel for d=64, n_pref=20, topn=17' in str(e.value)
    with pytest.raises(lib.KtupError) as e:
        lib.call('ktup_eval_pref_topk_hard', p, 64, p, 64, None, 64, None, p, 20, 64, p, 5, 100, 0, 0, None, 1, 0, None, None, 17, p, None, p,
                 None)
    assert e.value.code == ERR_INVALID and 'ktup_eval_pref_topk_hard: needs items, 32-bit item ids, topn <= 16' in str(e.value)
    loaded = lib.load()
    # the narrow workspaces do not depend on what the wide ones need: 8 x 16 keys per user / 8 x topn keys per user, as they were
    a, b = (loaded.ktup_eval_pref_topk_workspace_bytes(100, 20, 6040, 3240, t) for t in (1, 16))
    assert a == b
    a, b = (loaded.ktup_eval_pref_topk_hard_workspace_bytes(100, 20, 6040, 3240, t) for t in (10, 11))
    assert b - a == 6040 * 8 * 8


def test_python_surface(lib):
    from jTransUP.hip import ops
    for narrow, wide in ((ops.eval_pref_topk, ops.eval_pref_topk_wide), (ops.eval_pref_topk_hard, ops.eval_pref_topk_hard_wide)):
        assert inspect.signature(wide) == inspect.signature(narrow)
    assert (ops.TOPN_MAX, ops.TOPN_WIDE_MAX) == (16, 64)


def test_the_route_choice(lib):
    """eval_wide_topn: -1 = the measured default of the route (ops.PREF_WIDE_TOPN_DEFAULT), 0 = the batch walk above 16, 1 = the wide
    sweep; up to 16 the narrow wrapper whatever the option says, above 64 nothing.  The three keys of WIDE_TOPN_DEFAULT answer as
    they did."""
    from jTransUP.hip import ops
    assert set(ops.PREF_WIDE_TOPN_DEFAULT) == {'pref_q', 'pref_soft', 'pref_hard'}
    assert all(isinstance(v, bool) for v in ops.PREF_WIDE_TOPN_DEFAULT.values())
    assert set(ops.WIDE_TOPN_DEFAULT) == {'dot', 'cfkg_l1', 'cfkg_l2'}
    old = lib.get_option('eval_wide_topn')
    try:
        for value in (-1, 0, 1):
            lib.set_option('eval_wide_topn', value)
            for table in (ops.PREF_WIDE_TOPN_DEFAULT, ops.WIDE_TOPN_DEFAULT):
                for model, default in table.items():
                    wide = 'wide' if value == 1 or (value == -1 and default) else None
                    got = [ops.topk_sweep_for(topn, 'narrow', 'wide', model) for topn in (1, 16, 17, 20, 64, 65)]
                    assert got == ['narrow', 'narrow', wide, wide, wide, None], (value, model)
        with pytest.raises(KeyError):
            ops.topk_sweep_for(20, 'narrow', 'wide', 'no such model')
    finally:
        lib.set_option('eval_wide_topn', old)
