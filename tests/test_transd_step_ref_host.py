"""CPU checks around ktup_train_transd_step: tests/_transd_step_ref.py, its fp64 reference, reproduces the reference's goldens
(tests/golden/transd.npz) and its case generator meets its conditions within its caps for every case tests/test_hip_transd_step.py
names; the two entry points are exported and bound, and every rejection happens on the host before any HIP call (no GPU needed)."""
import os

import numpy as np
import pytest
import torch

from tests import _transd_step_ref as T
from tests._train_step_ref import MAX_DRAWS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT, AT, GAT = 1e-4, 1e-5, 3e-5                     # the project's bars (tests/test_hip_transd.py)
OK, INVALID, UNSUPPORTED = 0, -1, -3


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


# ------------------------------------------------------------------------------------------------ the reference against the goldens
@pytest.mark.parametrize('l1', [True, False])
@pytest.mark.parametrize('d', [36, 50, 64, 100])
def test_reference_reproduces_the_goldens(d, l1):
    c, want = T.golden_case(d, l1)
    assert c['B'] == 48 and bool((c['nr'] == c['r']).all())
    Tb = T.tables(c)
    h2, t2, r2 = T.ids(c)
    s = T.score(Tb, h2, t2, r2, c['l1'])
    hinge = float((s[:48] - s[48:] + 1.0).abs().min())
    edge = float(((Tb['E'] ** 2).sum(1) - 1).abs().min()), float(((Tb['R'] ** 2).sum(1) - 1).abs().min())
    print('d=%d %s: smallest |hinge argument| %.3g, smallest ||x|^2 - 1| %.3g (E) %.3g (R)' % ((d, 'L1' if l1 else 'L2', hinge) + edge))
    assert hinge >= 2e-3 and min(edge) >= 1e-3                          # the fixture is clear of knife edges
    np.testing.assert_allclose(s[:48].numpy(), want['pos'], rtol=RT, atol=AT, err_msg='pos')
    np.testing.assert_allclose(s[48:].numpy(), want['neg'], rtol=RT, atol=AT, err_msg='neg')
    slots, grads = T.reference(c, 1.0, 1.0, 6)
    assert slots[1] == 0.0
    np.testing.assert_allclose(slots[0] + slots[2] + slots[3], want['loss'], rtol=RT, atol=AT, err_msg='loss')
    for k in T.TABLES:
        np.testing.assert_allclose(grads[k].numpy(), want['grad'][k], rtol=RT, atol=GAT, err_msg='grad ' + k)
    touched = T.touched_rows(c, 1.0, 6)
    for k in T.TABLES:                                                  # what the reference leaves at zero is what touched_rows names idle
        idle = ~touched[k]
        assert float(np.abs(want['grad'][k][idle.numpy()]).max() if bool(idle.any()) else 0.0) == 0.0, k


def test_reference_gradients_are_the_closed_forms():
    """The header's adds, example by example, in numpy fp64, against autograd -- with strays, both distances, every regs."""
    for l1 in (0, 1):
        c = T.stray_case(36, l1)
        d, B = c['d'], c['B']
        tab = {k: v.numpy() for k, v in T.tables(c).items()}
        h2, t2, r2 = (x.numpy() for x in T.ids(c))
        for regs, gscale in ((6, 0.5), (0, 1.0), (2, 1.0), (4, 0.5)):
            slots, grads = T.reference(c, 1.0, gscale, regs)
            want = {k: np.zeros_like(v) for k, v in tab.items()}
            al = (tab['E'][h2] * tab['Ep'][h2]).sum(1)
            be = (tab['E'][t2] * tab['Ep'][t2]).sum(1)
            v = (tab['E'][h2] - tab['E'][t2]) + tab['R'][r2] + (al - be)[:, None] * tab['Rp'][r2]
            s = np.abs(v).sum(1) if l1 else (v * v).sum(1)
            arg = s[:B] - s[B:] + 1.0
            assert abs(np.maximum(arg, 0).sum() - slots[0]) <= 1e-12 * max(1.0, abs(slots[0]))
            for k in range(2 * B):
                if arg[k % B] <= 0:
                    continue
                g = (gscale if k < B else -gscale) * (np.sign(v[k]) if l1 else 2 * v[k])
                gam = float(g @ tab['Rp'][r2[k]])
                want['E'][h2[k]] += g + gam * tab['Ep'][h2[k]]
                want['Ep'][h2[k]] += gam * tab['E'][h2[k]]
                want['E'][t2[k]] -= g + gam * tab['Ep'][t2[k]]
                want['Ep'][t2[k]] -= gam * tab['E'][t2[k]]
                want['R'][r2[k]] += g
                want['Rp'][r2[k]] += (al[k] - be[k]) * g
            for name, rows, bit in (('E', np.concatenate([h2, t2]), 2), ('R', r2, 4)):
                if regs & bit:
                    for x in rows:
                        if (tab[name][x] ** 2).sum() > 1:
                            want[name][x] += 2 * gscale * tab[name][x]
            for k in T.TABLES:
                np.testing.assert_allclose(grads[k].numpy(), want[k], rtol=1e-12, atol=1e-13, err_msg='%s regs %d' % (k, regs))


def test_every_named_case_meets_the_conditions_within_the_caps():
    specs = T.grid_specs()
    assert len({T.spec_id(s) for s in specs}) == len(specs)
    grid = [s for s in specs if s['B'] <= 67]
    for key in ('regs', 'gscale', 'pitch'):                             # every value of a rotated parameter meets every width and distance
        values = {tuple(s[key]) if key == 'pitch' else s[key] for s in grid}
        for d in T.WIDTHS:
            for l1 in (0, 1):
                seen = {tuple(s[key]) if key == 'pitch' else s[key] for s in grid if s['d'] == d and s['l1'] == l1}
                assert seen == values, (key, d, l1, seen)
    assert {s['regs'] for s in grid} == {0, 2, 4, 6} and {s['gscale'] for s in grid} == {1.0, 0.5}
    assert all(min(s['pitch']) > 0 for s in specs)                      # pitches above d for all four tables
    for d in T.WIDTHS:
        G = T.per_workgroup(d)
        assert G == {4: 16, 60: 16, 64: 16, 68: 8, 100: 8, 128: 8, 132: 4, 252: 4, 256: 4}[d]
        assert {s['B'] for s in grid if s['d'] == d} == {1, G - 1, G, G + 1, 67}
    beyond = [s for s in specs if s['B'] > 67]
    assert {(s['d'], s['l1']) for s in beyond} == {(132, 0), (132, 1), (256, 0), (256, 1)}
    assert all(s['B'] > T.GRID_CAP * T.per_workgroup(s['d']) for s in beyond)
    for s in specs:
        c = T.spec_case(s)
        assert T.conditions(c, (1.0,)) is None
        assert c['ne'] == 40 and c['n_rel'] == 3
        if s['B'] >= 67:                                                # the collisions the cases are there for
            h2, t2, _ = T.ids(c)
            assert bool((c['h'] == c['t']).any()), 'no triple with h == t'
            pos_rows, neg_rows = set(torch.cat([c['h'], c['t']]).tolist()), set(torch.cat([c['nh'], c['nt']]).tolist())
            assert pos_rows & neg_rows, 'no entity that is both a positive and a negative row'
            assert torch.bincount(torch.cat([h2, t2]), minlength=40).max() >= 4
    for d in (36, 100):
        for l1 in (0, 1):
            c = T.stray_case(d, l1)
            assert T.conditions(c, (1.0,)) is None and int((c['nr'] != c['r']).sum()) == 6
            c = T.inactive_case(d, l1)
            _, active, inactive = T._state(c, (T.INACTIVE_MARGIN,))
            assert bool(inactive.all()) and not bool(active.any())
            c = T.active_case(d, l1)
            _, active, inactive = T._state(c, (T.ACTIVE_MARGIN,))
            assert bool(active.all()) and not bool(inactive.any())
            c = T.zero_proj_case(d, l1)
            assert T.conditions(c, (1.0,)) is None and float(c['Ep'][:, :d].abs().max()) == 0.0 and float(c['Rp'][:, :d].abs().max()) == 0.0
    print('seeds per case (largest) %s, inner rounds (largest) %s' % (T.DRAWS, T.ROUNDS))
    for fam in ('transd', 'transd_stray', 'transd_inactive', 'transd_active', 'transd_zero'):
        assert T.DRAWS[fam] <= MAX_DRAWS and T.ROUNDS[fam] <= MAX_DRAWS
        assert T.DRAWS[fam] <= 3, 'a construction that needs many seeds is a wrong construction'


# ------------------------------------------------------------------------------------------------ the ABI on the host
def test_symbols_are_exported_and_bound(lib):
    assert 'ktup_train_transd_step' in lib.SIGNATURES and 'ktup_train_transd_step_supported' in lib.SIGNATURES
    assert len(lib.SIGNATURES['ktup_train_transd_step']) == 24
    loaded = lib.load()
    assert callable(loaded.ktup_train_transd_step) and callable(loaded.ktup_train_transd_step_supported)
    header = open(os.path.join(ROOT, 'include', 'ktup_hip.h')).read()
    assert 'int ktup_train_transd_step_supported(int d);' in header and 'int ktup_train_transd_step(const float* E' in header


def test_supported_widths(lib):
    loaded = lib.load()
    assert [loaded.ktup_train_transd_step_supported(d) for d in (4, 36, 64, 100, 128, 256)] == [1] * 6
    assert [loaded.ktup_train_transd_step_supported(d) for d in (0, 50, 258, 260, -4)] == [0] * 5


def _call(lib, d=100, regs=6, B=5, ld=None, gEp=16, E=16, gnorm=None):
    """`p`: a non-null, 16-byte aligned dummy; validated, never dereferenced on the host."""
    p = 16
    ld = d if ld is None else ld
    return lib.load().ktup_train_transd_step(E, ld, p, ld, p, ld, p, ld, d, p, p, p, B, 0, 1.0, 1.0, regs, p, p, p, gEp, p, gnorm, None)


def test_host_side_validation_happens_before_any_hip_call(lib):
    loaded = lib.load()
    err = lambda: loaded.ktup_last_error().decode() if isinstance(loaded.ktup_last_error(), bytes) else str(loaded.ktup_last_error())
    assert _call(lib, regs=1) == INVALID and 'regs' in err()
    assert _call(lib, regs=8) == INVALID and 'regs' in err()
    assert _call(lib, regs=7) == INVALID
    assert _call(lib, gEp=None) == INVALID and 'gEp' in err()
    assert _call(lib, E=None) == INVALID and "'E'" in err()
    assert _call(lib, d=0) == INVALID and 'embedding_size' in err()
    assert _call(lib, d=-4) == INVALID
    assert _call(lib, B=-1) == INVALID
    assert _call(lib, d=50, ld=52) == UNSUPPORTED and 'ktup_train_transd_step_supported' in err()
    assert _call(lib, d=260) == UNSUPPORTED
    assert _call(lib, d=100, ld=102) == UNSUPPORTED                     # a pitch that is no multiple of 4 floats
    assert _call(lib, E=20) == UNSUPPORTED                              # a table 4 bytes off a 16-byte boundary
    assert _call(lib, B=0) == OK                                        # nothing to do, nothing launched
    assert _call(lib, B=0, gnorm=64) == INVALID                         # (as ktup_train_kg_step: an empty batch tracks no norm)
