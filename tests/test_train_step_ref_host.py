"""tests/_train_step_ref.py -- the fp64 reference tests/test_hip_train_step.py holds the fused step kernels to -- pinned to the
oracle's step bodies on the CPU, so that the reference cannot drift: its table gradients are autograd of
oracle.cpu_ref.ktup_rec_step_loss / tup_rec_step_loss / kg_step_loss in fp64, its stored rows scattered by id reproduce the table
gradients, and its sumsq is the stated sum.  No GPU."""
import pytest
import torch

from oracle import cpu_ref as O
from tests import _train_step_ref as R

TIGHT = dict(rtol=1e-11, atol=1e-13)        # fp64 against fp64: two orders of summation of the same terms


def _autograd(loss_fn, tables):
    T = {k: v.clone().requires_grad_(True) for k, v in tables.items()}
    loss = loss_fn(T)
    loss.backward()
    return float(loss.detach()), {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in T.items()}


def _uni(c):
    B = c['B']
    return (None, None) if c['uni'] is None else (c['uni'][:B].double(), c['uni'][B:].double())


@pytest.mark.parametrize('hard', [False, True])
@pytest.mark.parametrize('l1', [False, True])
@pytest.mark.parametrize('d,n_pref,B', [(64, 5, 13), (100, 17, 9)])
def test_ktup_rec_reference_is_the_oracle_step(d, n_pref, B, l1, hard):
    c = R.rec_case(d, n_pref, B, True, hard, l1, seed=d + n_pref + 2 * l1 + hard)
    up, un = _uni(c)
    for target in (-1.0, 1.0):
        want_loss, want = _autograd(lambda T: O.ktup_rec_step_loss(T['U'], T['I'], T['E'], T['P'], T['Pn'], T['R'], T['Rn'], c['i2e'], c['u'],
                                                                   c['pi'], c['ni'], l1, target, up, un), R.rec_tables(c))
        want['E'][c['ne']] = 0.0                                    # nn.Embedding(padding_idx): autograd on a plain tensor fills it
        loss, got = R.rec_reference(c, target, 1.0, 1)
        assert abs(loss[0] + loss[1] - want_loss) <= 1e-12 * abs(want_loss)
        for k in want:
            torch.testing.assert_close(got[k], want[k], **TIGHT)
        assert float(got['E'][c['ne']].abs().max()) == 0.0
        assert float(got['E'][2].abs().max()) > 0.0                 # item 0's entity is a real row
        # gscale scales the gradients and not the values; without orth the second slot stays empty
        loss_h, got_h = R.rec_reference(c, target, 0.25, 0)
        _, want_h = _autograd(lambda T: 0.25 * R.rec_loss_terms(c, T, target, 0)[0], R.rec_tables(c))
        want_h['E'][c['ne']] = 0.0
        assert loss_h == [loss[0], 0.0]
        for k in want_h:
            torch.testing.assert_close(got_h[k], want_h[k], **TIGHT)
        # the mixed-table gradient goes to both summands
        torch.testing.assert_close(got_h['R'], got_h['P'], **TIGHT)
        torch.testing.assert_close(got_h['Rn'], got_h['Pn'], **TIGHT)


@pytest.mark.parametrize('hard', [False, True])
@pytest.mark.parametrize('l1', [False, True])
def test_tup_rec_reference_plus_reg_rows_is_the_oracle_step(l1, hard):
    """item_recommendation.py's step = the fused step (bpr + orth) + the row regularisers of ktup_train_rec_reg_rows."""
    c = R.rec_case(100, 20, 13, False, hard, l1, seed=31 + 2 * l1 + hard)
    up, un = _uni(c)
    want_loss, want = _autograd(lambda T: O.tup_rec_step_loss(T['U'], T['I'], T['P'], T['Pn'], c['u'], c['pi'], c['ni'], l1, -1.0, up, un),
                                R.rec_tables(c))
    loss, got = R.rec_reference(c, -1.0, 1.0, 1)
    loss_r, rows, sumsq = R.rec_rows_reference(c, -1.0, 1.0, 1)
    assert loss_r == pytest.approx(loss, rel=1e-12)
    reg_loss, GU, GV, gP = R.reg_rows_reference(c, rows['GU'], rows['GV'], rows['P'], 1.0, 1.0)
    assert abs(sum(loss) + sum(reg_loss) - want_loss) <= 1e-12 * abs(want_loss)
    scattered = R.scatter_rec_rows(c, {'GU': GU, 'GV': GV})
    torch.testing.assert_close(scattered['U'], want['U'], **TIGHT)
    torch.testing.assert_close(scattered['I'], want['I'], **TIGHT)
    torch.testing.assert_close(gP, want['P'], **TIGHT)
    torch.testing.assert_close(rows['Pn'], want['Pn'], **TIGHT)
    torch.testing.assert_close(got['Pn'], want['Pn'], **TIGHT)
    assert float((sumsq - ((rows['GU'] ** 2).sum() + (rows['GV'] ** 2).sum())).abs()) <= 1e-12 * sumsq


@pytest.mark.parametrize('ktup', [False, True])
@pytest.mark.parametrize('hard', [False, True])
@pytest.mark.parametrize('l1', [False, True])
def test_rec_rows_scatter_to_the_table_gradients(l1, hard, ktup):
    c = R.rec_case(64, 4, 13, ktup, hard, l1, seed=53 + 4 * ktup + 2 * l1 + hard)
    for gscale, orth in ((1.0, 1), (0.25, 0)):
        loss, want = R.rec_reference(c, -1.0, gscale, orth)
        loss_r, rows, sumsq = R.rec_rows_reference(c, -1.0, gscale, orth)
        assert loss_r == pytest.approx(loss, rel=1e-12)
        got = R.scatter_rec_rows(c, rows)
        for k in got:
            torch.testing.assert_close(got[k], want[k], **TIGHT)
        for k in ('P', 'Pn') + (('R', 'Rn') if ktup else ()):
            torch.testing.assert_close(rows[k], want[k], **TIGHT)
        i2 = torch.cat([c['pi'], c['ni']])
        twice = (c['i2e'][i2] != c['ne']) if ktup else torch.zeros(26, dtype=torch.bool)
        stated = (rows['GU'] ** 2).sum() + (rows['GV'] ** 2).sum() + (rows['GV'][twice] ** 2).sum()
        assert abs(sumsq - float(stated)) <= 1e-12 * sumsq
        if ktup:
            assert bool(twice.any()) and not bool(twice.all())


@pytest.mark.parametrize('transh', [False, True])
@pytest.mark.parametrize('l1', [False, True])
@pytest.mark.parametrize('d,B', [(20, 5), (100, 17)])
def test_kg_reference_is_the_oracle_step(d, B, l1, transh):
    c = R.kg_case(d, B, transh, l1, seed=d + B + 2 * l1 + transh, margins=(1.0, 0.3))
    for margin in (1.0, 0.3):
        want_loss, want = _autograd(lambda T: O.kg_step_loss(T['E'], T['R'], T.get('N'), c['h'], c['t'], c['r'], c['nh'], c['nt'], c['r'],
                                                             l1, margin, 0.5), R.kg_tables(c))
        loss, got = R.kg_reference(c, margin, 0.5, 7)
        assert abs(0.5 * sum(loss) - want_loss) <= 1e-12 * abs(want_loss)     # the slots are not scaled, the oracle's loss is
        assert (loss[1] != 0.0) == transh
        for k in want:
            torch.testing.assert_close(got[k], want[k], **TIGHT)
        # the regs bits switch exactly their slots
        for regs in (0, 1, 2, 4):
            part, _ = R.kg_reference(c, margin, 0.5, regs)
            assert part[0] == loss[0]
            for s, bit in ((1, 1), (2, 2), (3, 4)):
                assert part[s] == (loss[s] if regs & bit else 0.0)
        # stored rows: scattered by id they are the entity-table gradient; the twins' kept ends stay unwritten
        loss_r, GE, written, small, sumsq = R.kg_rows_reference(c, margin, 0.5, 7)
        assert loss_r == pytest.approx(loss, rel=1e-12)
        torch.testing.assert_close(R.scatter_kg_rows(c, GE), want['E'], **TIGHT)
        for k in small:
            torch.testing.assert_close(small[k], want[k], **TIGHT)
        assert int((~written).sum()) == B and abs(sumsq - float((GE[written] ** 2).sum())) <= 1e-12 * sumsq
        ids = R.kg_rows_ids(c, -1)
        assert bool(((ids < 0) == ~written).all())


@pytest.mark.parametrize('transh', [False, True])
def test_exact_zero_case_has_no_margin_gradient_on_its_entity(transh):
    c = R.kg_exact_zero_case(36, transh, True, seed=3 + transh)
    _, g = R.kg_reference(c, 1.0, 0.5, 0)
    assert float(g['E'][c['zero_entity']].abs().max()) == 0.0
    assert float(g['E'][c['zero_entity'] + 1].abs().max()) > 0.0    # its twin is active


def test_redraw_counts_are_small():
    for d, P in ((64, 1), (100, 17), (256, 20)):
        for hard in (False, True):
            R.rec_case(d, P, 13, True, hard, True, seed=d + P, family='host')
    R.kg_case(36, 67, True, True, seed=1, margins=(1.0, 0.3), family='host')
    print('seeds needed:', R.DRAWS, 'inner rounds:', R.ROUNDS)
    assert R.DRAWS['host'] <= 5 and R.ROUNDS['host'] <= 5
