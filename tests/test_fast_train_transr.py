"""The one-launch TransR training step (ktup_train_transr_step) inside the steppers: KGStepper on TransR and BaselineJointStepper on
CKE against the autograd route that mirrors the reference's step bodies, with the criterion of tests/test_fast_train.py
(test_kg_stepper_matches_the_autograd_route: loss rtol 1e-5 / atol 1e-6 and its table check) and of tests/test_fast_train_dot.py;
which route is bound, what is captured and replayed, and one command-line run that trains TransR at d = 100 through a replayed graph."""
import copy
import os
import re
import subprocess
import sys

import pytest
import torch

from tests.synth import make_dataset
from tests.test_fast_train import DEV, _assert_tables_close, _trainer_for

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'joint-kg-recommender_amd')
NE, NR, B, STEPS = 70, 6, 64, 12


def _pair(tmp_path, D, l1, optimizer, use_graphs):
    from jTransUP.models import transR
    from jTransUP.utils.fast_train import KGStepper
    torch.manual_seed(4)
    m1, m2 = transR.TransRModel(l1, D, NE, NR), transR.TransRModel(l1, D, NE, NR)
    m2.load_state_dict(copy.deepcopy(m1.state_dict()))
    FLAGS, tr1 = _trainer_for(tmp_path, 'transr', m1, optimizer)
    _, tr2 = _trainer_for(tmp_path, 'transr', m2, optimizer)
    return FLAGS, m1, tr1, m2, tr2, KGStepper(m2, tr2, FLAGS, B, use_graphs=use_graphs)


def _run(FLAGS, m1, tr1, m2, tr2, fast, steps=STEPS):
    from jTransUP.utils import loss
    gen = torch.Generator().manual_seed(9)
    rnd = lambda hi: torch.randint(0, hi, (B,), generator=gen).to(DEV)
    for step in range(steps):
        ph, pt, pr, nh, nt = rnd(NE), rnd(NE), rnd(NR), rnd(NE), rnd(NE)
        tr1.optimizer_zero_grad()
        losses = loss.marginLoss()(m1(ph, pt, pr), m1(nh, nt, pr), FLAGS.margin)
        rel_ids = torch.cat([pr, pr])
        losses = losses + loss.normLoss(m1.ent_embeddings.weight, ids=torch.cat([ph, pt, nh, nt])) \
            + loss.normLoss(m1.rel_embeddings.weight, ids=rel_ids)
        losses.backward()
        tr1.clip_and_step(FLAGS.clipping_max_value)
        fast_loss = fast.kg_step(ph, pt, pr, nh, nt, pr)
        print('step %d: loss %.9g (autograd %.9g)' % (step, float(fast_loss), float(losses)))
        torch.testing.assert_close(fast_loss.reshape(()), losses.detach().reshape(()), rtol=1e-5, atol=1e-6)
        assert tr1.step == tr2.step == step + 1
        _assert_tables_close(m1, m2, step)


@pytest.mark.parametrize('use_graphs', [False, True])
@pytest.mark.parametrize('optimizer', ['SGD', 'Adagrad'])
@pytest.mark.parametrize('l1', [False, True])
@pytest.mark.parametrize('D', [64, 100])
def test_kg_stepper_takes_the_one_launch_transr_step(tmp_path, D, l1, optimizer, use_graphs):
    FLAGS, m1, tr1, m2, tr2, fast = _pair(tmp_path, D, l1, optimizer, use_graphs)
    _run(FLAGS, m1, tr1, m2, tr2, fast)
    assert fast.transr_step is True and fast.fused_step is False and fast.rws is None
    if use_graphs:
        assert 'kg' in fast._graphs and fast.replays['kg'] >= 4
    else:
        assert not fast._graphs and fast.replays['kg'] == 0


def test_the_bucketed_route_is_never_captured(tmp_path, monkeypatch):
    """KTUP_FUSED_STEP=0 at D = 100: the multi-launch route with its memset, issued launch by launch."""
    monkeypatch.setenv('KTUP_FUSED_STEP', '0')
    FLAGS, m1, tr1, m2, tr2, fast = _pair(tmp_path, 100, False, 'SGD', True)
    _run(FLAGS, m1, tr1, m2, tr2, fast, steps=6)
    assert fast.transr_step is False and fast.fused_step is False and fast.rws is not None
    assert fast._graphs == {} and fast.replays['kg'] == 0


def test_a_width_of_the_generic_kernels_stays_as_it_is(tmp_path):
    """D = 36: no one-launch step, no bucketed kernels, no memset -- the multi-launch step is captured and replayed as before."""
    FLAGS, m1, tr1, m2, tr2, fast = _pair(tmp_path, 36, False, 'SGD', True)
    _run(FLAGS, m1, tr1, m2, tr2, fast, steps=6)
    assert fast.transr_step is False and fast.fused_step is False
    assert 'kg' in fast._graphs and fast.replays['kg'] >= 2


@pytest.mark.parametrize('optimizer', ['Adagrad', 'SGD'])
def test_cke_kg_step_is_the_one_launch(tmp_path, optimizer, monkeypatch):
    """The schedule and the criterion of tests/test_fast_train_dot.py at D = 100; the kg step binds ktup_train_transr_step and none of
    the bucketed entry points, stays outside the graphs, and the pad entity row never moves."""
    from jTransUP.hip import lib as L
    from tests import test_fast_train_dot as TD
    bound = []
    real_bind = L.bind
    monkeypatch.setattr(L, 'bind', lambda name, *a: (bound.append(name), real_bind(name, *a))[1])
    FLAGS, m1, tr1 = TD.build(tmp_path, 'cke', optimizer, 100)
    _, m2, tr2 = TD.build(tmp_path, 'cke', optimizer, 100)
    m2.load_state_dict(copy.deepcopy(m1.state_dict()))
    fast = TD.make_stepper('cke', m2, tr2, FLAGS, 64)
    assert fast.transr_step is True and fast.rws is None
    gen = torch.Generator().manual_seed(9)
    schedule = [True, True, False, True, False, False, True] + [True, False] * 4
    for step, is_rec in enumerate(schedule):
        ids, align = TD.draw('cke', gen, 64, is_rec)
        want = TD.autograd_step('cke', FLAGS, m1, tr1, is_rec, ids, align)
        got = TD.fast_step(fast, is_rec, ids, align)
        print('step %d %s: loss %.9g (autograd %.9g)' % (step, 'rec' if is_rec else 'kg', float(got), float(want)))
        torch.testing.assert_close(got.reshape(()), want.reshape(()), rtol=1e-5, atol=1e-6)
        assert tr1.step == tr2.step == step + 1
        for (k, a), (_, b) in zip(m1.state_dict().items(), m2.state_dict().items()):
            err = (b - a).abs()
            bad = err > 2e-6 + 2e-5 * a.abs()
            assert int(bad.sum()) <= max(6, int(2e-3 * bad.numel())) and float(err.max()) <= TD.STRAY_CAP, \
                '%s after step %d: %d elements off, max %.3g' % (k, step, int(bad.sum()), float(err.max()))
    assert 'ktup_train_transr_step' in bound
    assert not [n for n in bound if n.startswith('ktup_score_transr')], bound
    assert set(fast._graphs) == {'rec'}
    assert float(m2.ent_embeddings.weight.detach()[m2.ent_total - 1].abs().sum()) == 0.0


def test_cke_keeps_the_bucketed_route_when_asked(tmp_path, monkeypatch):
    from tests import test_fast_train_dot as TD
    monkeypatch.setenv('KTUP_FUSED_STEP', '0')
    FLAGS, m, tr = TD.build(tmp_path, 'cke', 'SGD', 100)
    fast = TD.make_stepper('cke', m, tr, FLAGS, 64)
    assert fast.transr_step is False and fast.rws is not None


def test_transr_cli_trains_through_a_replayed_graph(tmp_path):
    """run_knowledge_representation.py -model_type transr at d = 100, in the style of tests/test_e2e_cli.py."""
    data = str(tmp_path)
    make_dataset(data)
    logs = os.path.join(data, 'log')
    os.makedirs(logs, exist_ok=True)
    name = 'kg-transr-d100'
    cmd = [sys.executable, os.path.join(PKG, 'run_knowledge_representation.py'), '-data_path', data, '-log_path', logs, '-dataset', 'ml1m',
           '-experiment_name', name, '-nohas_visualization', '-batch_size', '32', '-embedding_size', '100', '-seed', '3',
           '-eval_interval_steps', '10', '-training_steps', '20', '-early_stopping_steps_to_wait', '0', '-learning_rate', '0.05',
           '-topn', '10', '-model_type', 'transr', '-kg_test_files', 'valid.dat']
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    log = open(os.path.join(logs, name + '.log')).read()
    assert len(re.findall(r'avg hit:\d\.\d+, avg mean rank:\d+\.\d+, topn:10', log)) >= 2
    hit = re.search(r'TransR training step: one launch \(ktup_train_transr_step\); (\d+) steps were graph replays', log)
    assert hit and int(hit.group(1)) >= 4, log[-2000:]
    assert os.path.isfile(os.path.join(logs, name + '.ckpt_final'))
