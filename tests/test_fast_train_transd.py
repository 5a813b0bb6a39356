"""The one-launch TransD training step (ktup_train_transd_step) inside KGStepper: against the autograd route that mirrors the
reference's step body, with the criterion of tests/test_fast_train.py (test_kg_stepper_matches_the_autograd_route: loss rtol 1e-5 /
atol 1e-6 and its table check); clipped steps with and without the tracked norm; which route is bound; the device-fed steps against
the host-fed ones on the same batches; and command-line runs at d = 100 with and without -device_sampling."""
import copy
import os
import re
import subprocess
import sys

import pytest
import torch

from tests.synth import make_dataset
from tests.test_fast_train import DEV, STRAY_CAP, _assert_tables_close, _trainer_for

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'joint-kg-recommender_amd')
NE, NR, B, STEPS = 70, 6, 64, 20


def _model(l1, D):
    """The projection tables start non-zero: at the reference's zero initialisation their gradients vanish identically."""
    from jTransUP.models import transD
    m = transD.TransDModel(l1, D, NE, NR)
    with torch.no_grad():
        m.ent_proj_embeddings.weight.copy_(torch.randn(NE, D) * 0.2)
        m.rel_proj_embeddings.weight.copy_(torch.randn(NR, D) * 0.2)
    return m


def _pair(tmp_path, D, l1, optimizer, use_graphs, clip=None):
    from jTransUP.models import transD
    from jTransUP.utils.fast_train import KGStepper
    torch.manual_seed(4)
    m1 = _model(l1, D)
    m2 = transD.TransDModel(l1, D, NE, NR)
    m2.load_state_dict(copy.deepcopy(m1.state_dict()))
    FLAGS, tr1 = _trainer_for(tmp_path, 'transd', m1, optimizer)
    _, tr2 = _trainer_for(tmp_path, 'transd', m2, optimizer)
    if clip is not None:
        FLAGS.clipping_max_value = clip
    return FLAGS, m1, tr1, m2, tr2, KGStepper(m2, tr2, FLAGS, B, use_graphs=use_graphs)


def _run(FLAGS, m1, tr1, m2, tr2, fast, steps=STEPS, clipped=False):
    from jTransUP.utils import loss
    gen = torch.Generator().manual_seed(9)
    rnd = lambda hi: torch.randint(0, hi, (B,), generator=gen).to(DEV)
    start = copy.deepcopy(m1.state_dict())
    for step in range(steps):
        ph, pt, pr, nh, nt = rnd(NE), rnd(NE), rnd(NR), rnd(NE), rnd(NE)
        tr1.optimizer_zero_grad()
        losses = loss.marginLoss()(m1(ph, pt, pr), m1(nh, nt, pr), FLAGS.margin)
        rel_ids = torch.cat([pr, pr])
        losses = losses + loss.normLoss(m1.ent_embeddings.weight, ids=torch.cat([ph, pt, nh, nt])) \
            + loss.normLoss(m1.rel_embeddings.weight, ids=rel_ids)
        losses.backward()
        tr1.clip_and_step(FLAGS.clipping_max_value)
        if clipped:
            assert tr1.fused.total_norm() > FLAGS.clipping_max_value, 'step %d of the reference was not clipped' % step
        fast_loss = fast.kg_step(ph, pt, pr, nh, nt, pr)
        print('step %d: loss %.9g (autograd %.9g)' % (step, float(fast_loss), float(losses.detach())))
        torch.testing.assert_close(fast_loss.reshape(()), losses.detach().reshape(()), rtol=1e-5, atol=1e-6)
        assert tr1.step == tr2.step == step + 1
        _assert_tables_close(m1, m2, step)
    for k, a in m1.state_dict().items():                                # every table trained, the projection tables included
        assert float((a - start[k]).abs().max()) > 1e-4, k


@pytest.mark.parametrize('use_graphs', [False, True])
@pytest.mark.parametrize('optimizer', ['SGD', 'Adagrad'])
@pytest.mark.parametrize('D,l1', [(36, False), (100, True), (256, False)])
def test_kg_stepper_takes_the_one_launch_transd_step(tmp_path, monkeypatch, D, l1, optimizer, use_graphs):
    from jTransUP.hip import lib as L
    bound = []
    real_bind = L.bind
    monkeypatch.setattr(L, 'bind', lambda name, *a: (bound.append(name), real_bind(name, *a))[1])
    FLAGS, m1, tr1, m2, tr2, fast = _pair(tmp_path, D, l1, optimizer, use_graphs)
    assert fast.transd and fast.transd_step is True
    _run(FLAGS, m1, tr1, m2, tr2, fast)
    assert fast.transd_step is True and fast.fused_step is False
    assert 'ktup_train_transd_step' in bound and not [n for n in bound if n.startswith('ktup_score_transd') or n.startswith('ktup_reg_')], bound
    if use_graphs:
        assert 'kg' in fast._graphs and fast.replays['kg'] >= 4
    else:
        assert not fast._graphs and fast.replays['kg'] == 0


@pytest.mark.parametrize('tracked', ['0', '1'])
@pytest.mark.parametrize('use_graphs', [False, True])
@pytest.mark.parametrize('D,l1', [(36, False), (100, True), (256, False)])
def test_clipped_steps_with_and_without_the_tracked_norm(tmp_path, monkeypatch, D, l1, use_graphs, tracked):
    monkeypatch.setenv('KTUP_TRACKED_NORM', tracked)
    FLAGS, m1, tr1, m2, tr2, fast = _pair(tmp_path, D, l1, 'Adagrad', use_graphs, clip=0.05)
    assert fast.max_norm == 0.05 and fast.transd_step is True
    assert (fast._gn is not None) == (tracked == '1' and D <= 128)      # (the base class tracks no norm above d = 128)
    _run(FLAGS, m1, tr1, m2, tr2, fast, clipped=True)
    if fast._gn is not None:
        assert int(fast._gn[:1].view(torch.int64).item()) == STEPS      # the workspace counted every step


def test_fused_step_switch_keeps_the_multi_launch_route(tmp_path, monkeypatch):
    from jTransUP.hip import lib as L
    monkeypatch.setenv('KTUP_FUSED_STEP', '0')
    bound = []
    real_bind = L.bind
    monkeypatch.setattr(L, 'bind', lambda name, *a: (bound.append(name), real_bind(name, *a))[1])
    FLAGS, m1, tr1, m2, tr2, fast = _pair(tmp_path, 100, False, 'SGD', True)
    _run(FLAGS, m1, tr1, m2, tr2, fast, steps=6)
    assert fast.transd_step is False and fast.fused_step is False
    assert 'ktup_score_transd_fwd' in bound and 'ktup_score_transd_bwd' in bound and 'ktup_train_transd_step' not in bound
    assert fast.can_feed('kg') is False


def test_deterministic_mode_takes_the_one_launch_and_refuses_the_other_route(tmp_path, monkeypatch):
    from jTransUP.hip import lib as L
    old = L.set_option('deterministic', 1)
    try:
        FLAGS, m1, tr1, m2, tr2, fast = _pair(tmp_path, 36, False, 'SGD', False)
        _run(FLAGS, m1, tr1, m2, tr2, fast, steps=3)
        assert fast.transd_step is True
        monkeypatch.setenv('KTUP_FUSED_STEP', '0')
        FLAGS, m1, tr1, m2, tr2, fast = _pair(tmp_path, 36, False, 'SGD', False)
        assert fast.transd_step is False
        ids = [torch.zeros(B, dtype=torch.int64, device=DEV)] * 6
        with pytest.raises(L.KtupError) as e:
            fast.kg_step(*ids)
        assert 'KTUP_DETERMINISTIC' in str(e.value)
    finally:
        L.set_option('deterministic', old)


@pytest.mark.parametrize('D,l1', [(100, False), (36, True)])
def test_fed_steps_match_the_host_fed_steps(tmp_path, D, l1):
    """Two steppers on copies of one model, feeders and samplers of the same seed: 12 fed_steps and one fed_cycle of ten against
    kg_step on feed.next_cols() and sampler.sample_kg().  Same seeds -> the same batches, bit for bit after every single step."""
    from jTransUP.models import transD
    from jTransUP.utils.device_sampler import DeviceSampler
    from jTransUP.utils.fast_train import DeviceFeeder, KGStepper
    FB = 16
    torch.manual_seed(4)
    init = _model(l1, D).state_dict()
    gen = torch.Generator().manual_seed(21)
    triples = [(int(h), int(t), int(r)) for h, t, r in zip(torch.randint(0, NE, (500,), generator=gen), torch.randint(0, NE, (500,), generator=gen),
                                                           torch.randint(0, NR, (500,), generator=gen))]
    runs = []
    for fed in (True, False):
        m = transD.TransDModel(l1, D, NE, NR)
        m.load_state_dict(copy.deepcopy(init))
        FLAGS, tr = _trainer_for(tmp_path, 'transd', m, 'Adagrad')
        sampler = DeviceSampler(DEV, seed=5)
        sampler.set_triples(NE, NR, [triples])
        feed = DeviceFeeder(triples, FB, DEV, seed=4)
        st = KGStepper(m, tr, FLAGS, FB)
        if fed:
            st.attach_feeds(sampler, kg=feed)
            assert st.can_feed('kg') is True and st.transd_step is True and st.fused_step is False
        runs.append(dict(m=m, tr=tr, sampler=sampler, feed=feed, st=st, total=0.0))
    a, b = runs
    for step in range(12):
        a['st'].fed_step('kg')
        ph, pt, pr = b['feed'].next_cols()
        nh, nt = b['sampler'].sample_kg(ph, pt, pr)
        b['total'] += float(b['st'].kg_step(ph, pt, pr, nh, nt, pr))
        for k in ('h2', 't2', 'r2'):
            assert torch.equal(getattr(a['st'], k), getattr(b['st'], k)), (k, step)
        _assert_tables_close(b['m'], a['m'], step)
    assert a['st'].fed_cycle(('kg',) * 10) == 10                        # 500 triples / 16: the epoch does not end inside it
    for step in range(12, 22):
        ph, pt, pr = b['feed'].next_cols()
        nh, nt = b['sampler'].sample_kg(ph, pt, pr)
        b['total'] += float(b['st'].kg_step(ph, pt, pr, nh, nt, pr))
    for k in ('h2', 't2', 'r2'):                                          # the cycle's last batch is the host-fed run's last batch
        assert torch.equal(getattr(a['st'], k), getattr(b['st'], k)), k
    _assert_tables_close(b['m'], a['m'], 22)
    assert a['tr'].step == b['tr'].step == 22
    a['sampler'].check(); b['sampler'].check()
    assert sorted(a['st']._graphs) == ['cycle:' + ','.join(['kg'] * 10), 'kg+fed']
    sums = a['st'].take_sums()
    print('fed sum %.9g, host-fed sum %.9g' % (sums['kg'], b['total']))
    assert abs(sums['kg'] - b['total']) <= 1e-5 * abs(b['total'])
    assert a['st'].take_sums() == {'kg': 0.0}


# ------------------------------------------------------------------------------------------------ the command line
@pytest.fixture(scope='module')
def dataset(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('ds')
    make_dataset(str(tmp))
    return tmp


def _cli(data, name, extra):
    data = str(data)
    logs = os.path.join(data, 'log')
    os.makedirs(logs, exist_ok=True)
    cmd = [sys.executable, os.path.join(PKG, 'run_knowledge_representation.py'), '-data_path', data, '-log_path', logs, '-dataset', 'ml1m',
           '-experiment_name', name, '-nohas_visualization', '-batch_size', '32', '-embedding_size', '100', '-seed', '3',
           '-eval_interval_steps', '10', '-training_steps', '30', '-early_stopping_steps_to_wait', '0', '-learning_rate', '0.05',
           '-topn', '10', '-model_type', 'transd', '-kg_test_files', 'valid.dat'] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    log = open(os.path.join(logs, name + '.log')).read()
    assert len(re.findall(r'avg hit:\d\.\d+, avg mean rank:\d+\.\d+, topn:10', log)) >= 3
    assert os.path.isfile(os.path.join(logs, name + '.ckpt_final'))
    hit = re.search(r'TransD training step: (.*); (\d+) steps were graph replays; device-fed: (yes|no)', log)
    assert hit, log[-2000:]
    return hit.group(1), int(hit.group(2)), hit.group(3)


def test_transd_cli_trains_device_fed_through_replayed_graphs(dataset):
    route, replays, fed = _cli(dataset, 'kg-transd-d100', [])
    assert route == 'one launch (ktup_train_transd_step)' and fed == 'yes' and replays > 0


def test_transd_cli_host_fed_replays_the_step(dataset):
    route, replays, fed = _cli(dataset, 'kg-transd-d100-host', ['-nodevice_sampling'])
    assert route == 'one launch (ktup_train_transd_step)' and fed == 'no' and replays >= 4
