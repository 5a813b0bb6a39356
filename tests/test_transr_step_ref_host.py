"""CPU checks of tests/_transr_step_ref.py, the fp64 reference of ktup_train_transr_step: its case generator meets its conditions
within its caps for every case tests/test_hip_transr_step.py names, and its autograd gradients equal the closed forms documented in
include/ktup_hip.h, computed explicitly in numpy fp64."""
import numpy as np
import pytest
import torch

from tests import _transr_step_ref as T
from tests._train_step_ref import MAX_DRAWS


def _all_specs():
    return T.grid_specs() + T.edge_specs()


def test_every_named_case_meets_the_conditions_within_the_caps():
    specs = _all_specs()
    assert len({T.spec_id(s) for s in specs}) == len(specs)
    for key in ('nsplit', 'regs', 'gscale', 'pitch'):                   # every value of a rotated parameter meets every width and distance
        values = {tuple(s[key]) if key == 'pitch' else s[key] for s in specs}
        for d in (64, 100, 128):
            for l1 in (0, 1):
                seen = {tuple(s[key]) if key == 'pitch' else s[key] for s in T.grid_specs() if s['d'] == d and s['l1'] == l1}
                assert seen == values, (key, d, l1, seen)
    assert {s['B'] for s in T.grid_specs()} == {1, 15, 16, 17, 67, 300} and {s['n_rel'] for s in T.grid_specs()} == {1, 4, 7}
    kinds = set()
    for s in specs:
        c = T.spec_case(s)
        assert T.conditions(c, (1.0,)) is None
        counts = torch.bincount(c['r'], minlength=c['n_rel']).tolist()
        if s['kind'] == 'skip':
            assert counts[0] == 0
        if s['kind'] == 'edge':
            assert 16 in counts and 17 in counts
        if s['kind'] == 'major':
            assert max(counts) > c['B'] // 2
        kinds.add(s['kind'])
        n2 = (c['E'][:, :c['d']].double() ** 2).sum(1)
        assert bool((n2 > 1).any()) and bool((n2 < 1).any())             # both sides of normLoss's threshold
        M = c['M'][:, :c['d'] ** 2].view(-1, c['d'], c['d'])
        assert float((M[0] - torch.eye(c['d'])).abs().max()) > 0.1     # not the identity
    assert kinds == {'random', 'skip', 'major', 'edge'}
    for d in (64, 100, 128):
        for l1 in (0, 1):
            c = T.stray_case(d, l1)
            assert T.conditions(c, (1.0,)) is None and int((c['nr'] != c['r']).sum()) == 3
            c = T.inactive_case(d, l1)
            _, active, inactive = T._state(c, (T.INACTIVE_MARGIN,))
            assert bool(inactive.all()) and not bool(active.any())
    print('seeds per case (largest) %s, inner rounds (largest) %s' % (T.DRAWS, T.ROUNDS))
    for fam in ('transr', 'transr_stray', 'transr_inactive'):
        assert T.DRAWS[fam] <= MAX_DRAWS and T.ROUNDS[fam] <= MAX_DRAWS
        assert T.DRAWS[fam] <= 3, 'a construction that needs many seeds is a wrong construction'


def _closed_form(c, margin, gscale, regs):
    """The header's formulas, example by example, in numpy fp64."""
    d, B = c['d'], c['B']
    E, R = c['E'][:, :d].double().numpy(), c['R'][:, :d].double().numpy()
    M = c['M'][:, :d * d].double().numpy().reshape(-1, d, d)
    h2, t2, r2 = (x.numpy() for x in T.ids(c))
    gE, gR, gM = np.zeros_like(E), np.zeros_like(R), np.zeros_like(M)
    loss = [0.0, 0.0, 0.0, 0.0]

    def y_of(k):
        q = E[h2[k]] - E[t2[k]]
        return M[r2[k]] @ q + R[r2[k]], q

    def score(y):
        return np.abs(y).sum() if c['l1'] else (y * y).sum()

    for k in range(B):
        (yp, qp), (yn, qn) = y_of(k), y_of(k + B)
        arg = score(yp) - score(yn) + margin
        if arg > 0:
            loss[0] += arg
            for kk, y, q, g in ((k, yp, qp, gscale), (k + B, yn, qn, -gscale)):
                gy = g * (np.sign(y) if c['l1'] else 2.0 * y)
                gR[r2[kk]] += gy
                gM[r2[kk]] += np.outer(gy, q)
                gq = M[r2[kk]].T @ gy
                gE[h2[kk]] += gq
                gE[t2[kk]] -= gq
    if regs & 2:
        for e in np.concatenate([c['h'].numpy(), c['t'].numpy(), c['nh'].numpy(), c['nt'].numpy()]):
            n2 = (E[e] ** 2).sum()
            if n2 > 1:
                loss[2] += n2 - 1
                gE[e] += 2.0 * gscale * E[e]
    if regs & 4:
        for r in r2:
            n2 = (R[r] ** 2).sum()
            if n2 > 1:
                loss[3] += n2 - 1
                gR[r] += 2.0 * gscale * R[r]
    return loss, {'E': gE, 'R': gR, 'M': gM.reshape(-1, d * d)}


@pytest.mark.parametrize('l1', [0, 1])
@pytest.mark.parametrize('regs,gscale', [(6, 1.0), (0, 0.37), (2, 0.37), (4, 1.0)])
def test_the_reference_equals_the_closed_forms_of_the_header(l1, regs, gscale):
    for c in (T.case(64, 37, 4, l1, 11, r=T.rel_ids(37, 4, 'skip', 11), pitch=(4, 0, 4)), T.stray_case(64, l1)):
        want_loss, want = _closed_form(c, 1.0, gscale, regs)
        got_loss, got = T.reference(c, 1.0, gscale, regs)
        np.testing.assert_allclose(got_loss, want_loss, rtol=1e-12, atol=1e-12)
        for k in want:
            np.testing.assert_allclose(got[k].numpy(), want[k], rtol=1e-11, atol=1e-12, err_msg=k)
        unused = np.setdiff1d(np.arange(c['n_rel']), torch.cat([c['r'], c['nr']]).numpy())
        assert float(np.abs(got['M'].numpy()[unused]).max() if unused.size else 0.0) == 0.0


def test_a_relation_without_an_active_example_gets_no_projection_gradient():
    c = T.inactive_case(64, 0)
    loss, g = T.reference(c, T.INACTIVE_MARGIN, 1.0, 0)
    assert loss == [0.0, 0.0, 0.0, 0.0] and all(float(v.abs().max()) == 0.0 for v in g.values())


def test_untouched_rows_are_zero_in_the_reference_and_identical_twins_count_as_touched():
    """touched_rows is what the GPU test holds the launch to bit for bit: the reference must be zero wherever it says nothing lands,
    and an example whose twin is the same triple (active at exactly `margin`, gradients cancelling) must count as touching its rows."""
    twins = 0
    for s in T.grid_specs() + T.edge_specs():
        c = T.spec_case(s)
        t = T.touched_rows(c, 1.0, s['regs'])
        _, g = T.reference(c, 1.0, s['gscale'], s['regs'])
        for k in g:
            assert float(g[k][~t[k]].abs().max() if bool((~t[k]).any()) else 0.0) == 0.0, (T.spec_id(s), k)
        same = (c['h'] == c['nh']) & (c['t'] == c['nt']) & (c['r'] == c['nr'])
        twins += int(same.sum())
        assert bool(t['E'][c['h'][same]].all()) and bool(t['M'][c['r'][same]].all())
    assert twins > 0
