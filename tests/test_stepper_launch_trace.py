"""Which entry points each training route of the GPU-resident steppers (utils/fast_train.py, utils/fast_train_dot.py) launches, in
order, step by step: the guard that a new step form cannot silently change another route's launches.  The launches are issued one
by one (use_graphs=False) on the toy models of the stepper tests at B = 16, SGD, one process; `lib.bind` is wrapped so that a bound
launcher records its entry point when it is CALLED, `lib.call` (the optimizer launch) so that it records the name it is given."""
import pytest
import torch

from tests.test_fast_train import DEV, _trainer_for

pytestmark = pytest.mark.gpu
B, D = 16, 64
NU, NI, NE, NR = 50, 40, 70, 6

OPTIM = ('optim_clip_step',)
NORM2 = ('reg_norm_fused',) * 2
KG_ONE = ('train_kg_step',) + OPTIM


def _kg_seq(model):
    orth = ('reg_orth_fused',) if model == 'transh' else ()
    return ('score_%s_fwd' % model, 'loss_margin_fused', 'score_%s_bwd' % model) + orth + NORM2 + OPTIM


DOT = ('train_dot_step',) + OPTIM
# (stepper, model, d, KTUP_FUSED_STEP) -> (launches of a rec step, launches of a kg step), without the ktup_ prefix
CASES = {
    ('joint', 'jtransup', 64, '1'): (('train_rec_step',) + OPTIM, KG_ONE),
    ('joint', 'jtransup', 36, '1'): (('pref_prepare', 'score_ktup_fwd', 'loss_bpr_fused', 'score_ktup_bwd', 'reg_orth_fused') + OPTIM,
                                     _kg_seq('transh')),
    ('rec', 'bprmf', 64, '1'): (('score_bprmf_fwd', 'loss_bpr_fused', 'score_bprmf_bwd') + OPTIM, None),
    ('rec', 'transup', 64, '1'): (('train_rec_step',) + ('reg_norm_fused',) * 3 + OPTIM, None),
    ('rec', 'transup', 36, '1'): (('pref_prepare', 'score_tup_fwd', 'loss_bpr_fused', 'score_tup_bwd', 'reg_orth_fused')
                                  + ('reg_norm_fused',) * 3 + OPTIM, None),
    ('kg', 'transe', 64, '1'): (None, KG_ONE),
    ('kg', 'transh', 64, '1'): (None, KG_ONE),
    ('kg', 'transr', 64, '1'): (None, ('train_transr_step',) + OPTIM),
    ('kg', 'transd', 64, '1'): (None, ('train_transd_step',) + OPTIM),
    ('kg', 'transe', 64, '0'): (None, _kg_seq('transe')),
    ('kg', 'transh', 64, '0'): (None, _kg_seq('transh')),
    ('kg', 'transr', 64, '0'): (None, _kg_seq('transr')),
    ('kg', 'transd', 64, '0'): (None, _kg_seq('transd')),
    ('dot', 'fm', 64, '1'): (DOT, None),
    ('baseline', 'cofm-shared', 64, '1'): (DOT, KG_ONE),
    ('baseline', 'cofm', 64, '1'): (('train_dot_step', 'reg_align_pairs') + OPTIM, ('train_kg_step', 'reg_align_pairs') + OPTIM),
    ('baseline', 'cke', 64, '1'): (DOT, ('train_transr_step',) + OPTIM),
    ('baseline', 'cke', 64, '0'): (DOT, _kg_seq('transr')),
    ('baseline', 'cfkg', 64, '1'): (('train_cfkg_rec_step',) + OPTIM, KG_ONE),
    ('baseline', 'cofm-shared', 64, '0'): (DOT, _kg_seq('transe')),
}


def _make(tmp_path, stepper, model, d):
    """(stepper object, draw(is_rec) -> (positional ids, keyword arguments)) from the helpers of the stepper tests."""
    from jTransUP.utils.fast_train import JointStepper, KGStepper, RecStepper
    gen = torch.Generator().manual_seed(9)
    rnd = lambda hi: torch.randint(0, hi, (B,), generator=gen).to(DEV)

    def kg_ids():
        ph, pt, pr, nh, nt = rnd(NE), rnd(NE), rnd(NR), rnd(NE), rnd(NE)
        return (ph, pt, pr, nh, nt, pr)

    plain = lambda is_rec: ((rnd(NU), rnd(NI), rnd(NI)) if is_rec else kg_ids(), {})
    if stepper == 'joint':
        from tests.test_fast_train import build
        FLAGS, m, tr, _ = build(tmp_path, 'SGD', False, d)
        return JointStepper(m, tr, FLAGS, B, use_graphs=False), plain
    if stepper == 'rec':
        from jTransUP.models import bprmf, transUP
        torch.manual_seed(4)
        m = transUP.TransUPModel(False, d, NU, NI, 5, False) if model == 'transup' else bprmf.BPRMF(d, NU, NI)
        FLAGS, tr = _trainer_for(tmp_path, model, m, 'SGD')
        return RecStepper(m, tr, FLAGS, B, use_graphs=False), plain
    if stepper == 'kg':
        from jTransUP.models import transE, transH, transR
        from tests.test_fast_train_transd import _model
        torch.manual_seed(4)
        m = {'transe': lambda: transE.TransEModel(False, d, NE, NR), 'transh': lambda: transH.TransHModel(True, d, NE, NR),
             'transr': lambda: transR.TransRModel(False, d, NE, NR), 'transd': lambda: _model(False, d)}[model]()
        FLAGS, tr = _trainer_for(tmp_path, model, m, 'SGD')
        return KGStepper(m, tr, FLAGS, B, use_graphs=False), plain
    if model == 'cfkg':
        from tests import test_fast_train_cfkg as TC
        from jTransUP.utils.fast_train_dot import BaselineJointStepper
        FLAGS, m, tr = TC.build(tmp_path, 'SGD', d, False)
        return BaselineJointStepper(m, tr, FLAGS, B, use_graphs=False), lambda is_rec: (TC.draw(gen, B, is_rec), {})
    from jTransUP.utils.fast_train_dot import BaselineJointStepper, DotRecStepper
    from tests import test_fast_train_dot as TD
    FLAGS, m, tr = TD.build(tmp_path, model, 'SGD', d)
    fast = (DotRecStepper if model == 'fm' else BaselineJointStepper)(m, tr, FLAGS, B, use_graphs=False)

    def draw(is_rec):
        ids, align = TD.draw(model, gen, B, is_rec)
        return ids, ({} if model == 'fm' else {'align': align})
    return fast, draw


@pytest.mark.parametrize('case', sorted(CASES), ids=lambda c: '-'.join(str(x) for x in c))
def test_every_route_issues_its_launches_in_order(tmp_path, monkeypatch, case):
    from jTransUP.hip import lib as L
    stepper, model, d, fused = case
    monkeypatch.setenv('KTUP_FUSED_STEP', fused)
    trace = []
    real_bind, real_call = L.bind, L.call

    def bind(name, *a):
        run = real_bind(name, *a)
        return lambda: (trace.append(name), run())[1]

    def call(name, *a):
        trace.append(name)
        return real_call(name, *a)

    monkeypatch.setattr(L, 'bind', bind)
    monkeypatch.setattr(L, 'call', call)
    fast, draw = _make(tmp_path, stepper, model, d)
    assert not fast.use_graphs and fast.world == 1
    want = dict(zip((True, False), CASES[case]))
    for step in range(3):
        for is_rec in (True, False):
            if want[is_rec] is None:
                continue
            ids, kw = draw(is_rec)
            del trace[:]
            (fast.rec_step if is_rec else fast.kg_step)(*ids, **kw)
            torch.cuda.synchronize()
            got = list(trace)
            print('step %d %s: %s' % (step, 'rec' if is_rec else 'kg', got))
            assert got == ['ktup_' + n for n in want[is_rec]], (step, is_rec)
    assert not fast._graphs
