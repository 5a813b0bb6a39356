"""The GPU-resident training steps of FM, coFM and CKE (utils/fast_train_dot.py) against the autograd step bodies the drivers
would have run (item_recommendation.py:160-195, knowledgable_recommendation.py:330-401): same losses, same tables after a mixed
rec / kg schedule; two data-parallel replicas against one process; the command lines."""
import copy
import logging
import os
import re
import subprocess
import sys

import pytest
import torch

from tests.synth import make_dataset

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'joint-kg-recommender_amd')
STRAY_CAP = 2.1 * 0.05      # tests/test_fast_train.py: a stray element may be a whole first step apart (+-lr, lr = 0.05); the COUNT is the test
NU, NI, NE, NR = 50, 40, 70, 6
MODELS = ['fm', 'cofm', 'cofm-shared', 'cke']


def world_maps():
    """Items 0, 5, 10, ... have no entity; the others map to distinct entities; entities no item maps to have a key of their own."""
    i_map = {i: 'k%d' % i for i in range(NI)}
    ikg = {'k%d' % i: ((i * 3) % NE if i % 5 else -1, i) for i in range(NI)}
    e_map = {e: 'e%d' % e for e in range(NE)}
    for key, (e, i) in list(ikg.items()):
        if e != -1:
            e_map[e] = key
    for e in range(NE):
        if e_map[e] == 'e%d' % e:
            ikg['e%d' % e] = (e, -1)
    return i_map, e_map, ikg


def build(tmp_path, kind, optimizer, D):
    from jTransUP.models import CKE, cofm, fm
    from jTransUP.models.base import get_flags
    from jTransUP.utils.flags import FLAGS
    from jTransUP.utils.trainer import ModelTrainer
    model_type = kind.split('-')[0]
    get_flags(); FLAGS.reset()
    FLAGS(['prog', '-model_type', model_type, '-share_embeddings' if kind == 'cofm-shared' else '-noshare_embeddings', '-log_path',
           str(tmp_path), '-experiment_name', 'ftd', '-optimizer_type', optimizer, '-learning_rate', '0.05', '-kg_lambda', '0.5',
           '-norm_lambda', '0.7', '-L1_flag' if kind in ('cofm', 'cke') else '-noL1_flag'])
    FLAGS.ckpt_path = str(tmp_path)
    i_map, e_map, ikg = world_maps()
    torch.manual_seed(4)
    if kind == 'fm':
        m = fm.FM(D, NU, NI)
    elif kind == 'cofm':
        m = cofm.coFM(True, D, NU, NI, NE, NR, False)
    elif kind == 'cofm-shared':
        m = cofm.coFM(False, D, NU, NE, NE, NR, True)
    else:
        m = CKE.CKE(True, D, NU, NI, NE, NR, i_map, ikg)
    tr = ModelTrainer(m, logging.getLogger('ftd'), 10, FLAGS)
    return FLAGS, m, tr


def make_stepper(kind, m, tr, FLAGS, B):
    from jTransUP.utils.fast_train_dot import BaselineJointStepper, DotRecStepper
    return (DotRecStepper if kind == 'fm' else BaselineJointStepper)(m, tr, FLAGS, B)


def draw(kind, gen, B, is_rec):
    """One global batch as host lists (what the samplers hand the drivers) + the alignment lists of the step."""
    from jTransUP.models.knowledgable_recommendation import getMappedEntities, getMappedItems
    i_map, e_map, ikg = world_maps()
    rnd = lambda hi: torch.randint(0, hi, (B,), generator=gen).tolist()
    n_items = NE if kind == 'cofm-shared' else NI
    if is_rec:
        ids = (rnd(NU), rnd(n_items), rnd(n_items))
        align = getMappedEntities(ids[1] + ids[2], i_map, ikg) if kind == 'cofm' else None
    else:
        ph, pt, pr, nh, nt = rnd(NE), rnd(NE), rnd(NR), rnd(NE), rnd(NE)
        ids = (ph, pt, pr, nh, nt, pr)
        align = getMappedItems(ph + pt + nh + nt, e_map, ikg) if kind == 'cofm' else None
    return tuple(torch.tensor(x, dtype=torch.int64, device=DEV) for x in ids), align


def autograd_step(kind, FLAGS, m, tr, is_rec, ids, align):
    """The step body of the drivers' autograd route."""
    from jTransUP.utils import loss
    tr.optimizer_zero_grad()
    if kind == 'fm':
        u, pi, ni = ids
        losses = loss.bprLoss(m(u, pi), m(u, ni), target=tr.model_target)
    elif is_rec:
        u, pi, ni = ids
        losses = loss.bprLoss(m((u, pi), None, is_rec=True), m((u, ni), None, is_rec=True), target=tr.model_target)
    else:
        ph, pt, pr, nh, nt, nr = ids
        losses = loss.marginLoss()(m(None, (ph, pt, pr), is_rec=False), m(None, (nh, nt, nr), is_rec=False), FLAGS.margin)
        rel_ids = torch.cat([pr, nr])
        losses = losses + loss.normLoss(m.ent_embeddings.weight, ids=torch.cat([ph, pt, nh, nt])) \
            + loss.normLoss(m.rel_embeddings.weight, ids=rel_ids)
        losses = FLAGS.kg_lambda * losses
    if kind == 'cofm':
        e_ids, i_ids = (torch.tensor(x, dtype=torch.int64, device=DEV) for x in align)
        losses = losses + FLAGS.norm_lambda * loss.pNormLoss(m.ent_embeddings(e_ids), m.item_embeddings(i_ids), L1_flag=FLAGS.L1_flag)
    losses.backward()
    if kind != 'cke':
        # what ktup_train_dot_step relies on: the gradients of the user bias and of the global bias are g + (-g)
        for p in (m.user_bias.weight, m.bias):
            if p.grad is not None:
                assert float(p.grad.abs().max()) == 0.0
    tr.clip_and_step(FLAGS.clipping_max_value)
    return losses.detach()


def fast_step(fast, is_rec, ids, align):
    if not is_rec:
        return fast.kg_step(*ids, align=align)
    return fast.rec_step(*ids, align=align) if hasattr(fast, 'set_alignment') else fast.rec_step(*ids)


@pytest.mark.parametrize('D', [36, 100])
@pytest.mark.parametrize('optimizer', ['Adagrad', 'SGD', 'Adam'])
@pytest.mark.parametrize('kind', MODELS)
def test_dot_steppers_match_the_autograd_route(tmp_path, kind, optimizer, D):
    FLAGS, m1, tr1 = build(tmp_path, kind, optimizer, D)
    _, m2, tr2 = build(tmp_path, kind, optimizer, D)
    m2.load_state_dict(copy.deepcopy(m1.state_dict()))
    B = 64
    fast = make_stepper(kind, m2, tr2, FLAGS, B)
    gen = torch.Generator().manual_seed(9)
    # The seven mixed steps (five for FM) end before anything has been replayed twice: the first kg step wakes the relation side,
    # which drops the graphs and restarts the two eager steps every kind takes before its capture.  The schedule therefore goes on
    # until every captured kind has been replayed at least four times, with alignment lists of another length at every step.
    schedule = [True] * 7 if kind == 'fm' else [True, True, False, True, False, False, True] + [True, False] * 4
    replays, lengths = {}, set()
    for step, is_rec in enumerate(schedule):
        ids, align = draw(kind, gen, B, is_rec)
        before = {k: v[0] for k, v in fast._graphs.items()}
        want = autograd_step(kind, FLAGS, m1, tr1, is_rec, ids, align)
        got = fast_step(fast, is_rec, ids, align)
        print('step %d %s: loss %.9g (autograd %.9g)' % (step, 'rec' if is_rec else 'kg', float(got), float(want)))
        torch.testing.assert_close(got.reshape(()), want.reshape(()), rtol=1e-5, atol=1e-6)
        assert tr1.step == tr2.step == step + 1
        name = 'rec' if is_rec else 'kg'
        if name in fast._graphs and (name not in before or before[name] is fast._graphs[name][0]):
            replays[name] = replays.get(name, 0) + 1                       # this step was a replay (the capturing step replays too)
            if align is not None:
                lengths.add(len(align[0]))                                 # list lengths of REPLAYED steps only
        for (k, a), (_, b) in zip(m1.state_dict().items(), m2.state_dict().items()):
            err = (b - a).abs()
            bad = err > 2e-6 + 2e-5 * a.abs()
            print('  %s: %d of %d beyond, max %.3g' % (k, int(bad.sum()), bad.numel(), float(err.max())))
            assert int(bad.sum()) <= max(6, int((2e-2 if optimizer == 'Adam' else 2e-3) * bad.numel())) and float(err.max()) <= STRAY_CAP, \
                '%s after step %d: %d elements off, max %.3g' % (k, step, int(bad.sum()), float(err.max()))
    # CKE's kg step is never captured: its TransR kernels clear their bucket counters with a memset
    captured = ('rec',) if kind in ('fm', 'cke') else ('rec', 'kg')
    print('replays %s, alignment list lengths %s' % (replays, sorted(lengths)))
    assert fast._graphs and set(fast._graphs) == set(captured)
    assert all(replays.get(k, 0) >= 4 for k in captured), replays
    assert kind != 'cofm' or len(lengths) >= 4
    if kind == 'cke':                       # the pad entity row never moves
        assert float(m2.ent_embeddings.weight.detach()[m2.ent_total - 1].abs().sum()) == 0.0


def _run_schedule(kind, fast, B, schedule):
    gen = torch.Generator().manual_seed(9)
    losses = []
    for is_rec in schedule:
        ids, align = draw(kind, gen, B, is_rec)
        losses.append(float(fast_step(fast, is_rec, ids, align)))
    return losses


def _dp_worker(rank, world, port, tmp, out, D):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group('gloo', rank=rank, world_size=world)     # both ranks share the one GPU: RCCL refuses that, gloo does not
    try:
        FLAGS, m, tr = build(os.path.join(tmp, 'r%d' % rank), 'cofm', 'Adagrad', D)
        B = 64
        fast = make_stepper('cofm', m, tr, FLAGS, B)
        assert fast.world == world and fast.B == B // world
        losses = _run_schedule('cofm', fast, B, [True, False, True, False])
        torch.save({'state': {k: v.cpu() for k, v in m.state_dict().items()}, 'losses': losses}, os.path.join(out, 'rank%d.pt' % rank))
    finally:
        dist.destroy_process_group()


def test_data_parallel_steps_match_one_process(tmp_path):
    """Two replicas (gloo, sharing the GPU) on halves of each global batch == one process on the whole batch: coFM with its own
    tables, so the replicated alignment term is in it."""
    import socket
    import torch.multiprocessing as mp
    D = 36
    for r in range(2):
        os.makedirs(os.path.join(str(tmp_path), 'r%d' % r))
    s = socket.socket(); s.bind(('127.0.0.1', 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_dp_worker, args=(2, port, str(tmp_path), str(tmp_path), D), nprocs=2, join=True)
    FLAGS, m, tr = build(tmp_path, 'cofm', 'Adagrad', D)
    losses = _run_schedule('cofm', make_stepper('cofm', m, tr, FLAGS, 64), 64, [True, False, True, False])
    r0 = torch.load(os.path.join(str(tmp_path), 'rank0.pt'))
    r1 = torch.load(os.path.join(str(tmp_path), 'rank1.pt'))
    for k, v in m.state_dict().items():
        assert torch.equal(r0['state'][k], r1['state'][k]), k                 # replicas stay identical
        err = (r0['state'][k] - v.cpu()).abs()
        bad = err > 2e-6 + 2e-5 * v.cpu().abs()
        assert float(bad.float().mean()) <= 2e-3 and float(err.max()) <= STRAY_CAP, (k, int(bad.sum()), float(err.max()))
    torch.testing.assert_close(torch.tensor(r0['losses']), torch.tensor(losses), rtol=1e-5, atol=1e-6)


# ---------------------------------------------------------------------------------------------------- command lines
@pytest.fixture(scope='module')
def dataset(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('ds')
    make_dataset(str(tmp))
    return tmp


COMMON = ['-dataset', 'ml1m', '-nohas_visualization', '-batch_size', '32', '-embedding_size', '20', '-seed', '3', '-eval_interval_steps',
          '10', '-training_steps', '25', '-early_stopping_steps_to_wait', '0', '-learning_rate', '0.05', '-topn', '10']


@pytest.mark.parametrize('fast', [True, False])
@pytest.mark.parametrize('model', ['fm', 'cofm'])
def test_cli_takes_the_new_route(dataset, model, fast, monkeypatch):
    data = str(dataset)
    logs = os.path.join(data, 'log')
    os.makedirs(logs, exist_ok=True)
    name = 'dot-%s-%d' % (model, fast)
    if not fast:
        monkeypatch.setenv('KTUP_FAST_TRAIN', '0')
    if model == 'fm':
        script, extra = 'run_item_recommendation.py', ['-rec_test_files', 'valid.dat']
    else:
        script, extra = 'run_knowledgable_recommendation.py', ['-rec_test_files', 'valid.dat', '-kg_test_files', 'valid.dat', '-joint_ratio', '0.7']
    cmd = [sys.executable, os.path.join(PKG, script), '-data_path', data, '-log_path', logs, '-experiment_name', name, '-model_type', model] \
        + COMMON + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    log = open(os.path.join(logs, name + '.log')).read()
    assert ('GPU-resident training step enabled' in log) == fast
    assert ('device-resident' in log) == (fast and model == 'fm')           # FM's step is device-fed; the joint baselines are host-fed
    assert ('host-fed batches only' in log) == (fast and model == 'cofm')
    losses = [float(x) for x in re.findall(r'train loss:(\d+\.\d+)', log)]
    assert len(losses) >= 2 and all(l == l and l < 1e4 for l in losses)
    assert len(re.findall(r'f1:\d\.\d+', log)) >= 3


@pytest.mark.parametrize('model,port', [('cofm', 29547), ('cke', 29549)])
def test_joint_baseline_cli_data_parallel_torchrun(dataset, model, port):
    """torchrun with two ranks (gloo test hook: they share the GPU): both replicas log the same metrics."""
    data = str(dataset)
    logs = os.path.join(data, 'log')
    env = dict(os.environ, KTUP_DIST_BACKEND='gloo')
    name = model + '-dp'
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
           '--master-port', str(port), os.path.join(PKG, 'run_knowledgable_recommendation.py'), '-data_path', data, '-log_path', logs,
           '-experiment_name', name, '-model_type', model, '-rec_test_files', 'valid.dat', '-kg_test_files', 'valid.dat',
           '-joint_ratio', '0.7'] + COMMON
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    log0 = open(os.path.join(logs, name + '.log')).read()
    log1 = open(os.path.join(logs, name + '.rank1.log')).read()
    assert 'GPU-resident training step enabled' in log0 and 'GPU-resident training step enabled' in log1
    pat = r'f1:\d\.\d+, p:\d\.\d+, r:\d\.\d+, hit:\d\.\d+, ndcg:\d\.\d+'
    m0, m1 = re.findall(pat, log0), re.findall(pat, log1)
    assert len(m0) >= 3 and m0 == m1
    pat = r'rec train loss:\d+\.\d+, kg train loss:\d+\.\d+'
    assert re.findall(pat, log0) == re.findall(pat, log1)
