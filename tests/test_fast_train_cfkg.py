"""The GPU-resident training step of CFKG (utils/fast_train_dot.py BaselineJointStepper, rec step = ktup_train_cfkg_rec_step) against
the autograd step body the joint driver would have run (knowledgable_recommendation.py:330-401): same losses, same tables after a
mixed rec / kg schedule; two data-parallel replicas against one process; the command line.

The harness, the comparison rule and its constants are those of tests/test_fast_train_dot.py."""
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
NU, NE, NR = 50, 70, 6


def build(tmp_path, optimizer, D, l1):
    from jTransUP.models import CFKG
    from jTransUP.models.base import get_flags
    from jTransUP.utils.flags import FLAGS
    from jTransUP.utils.trainer import ModelTrainer
    get_flags(); FLAGS.reset()
    FLAGS(['prog', '-model_type', 'cfkg', '-share_embeddings', '-log_path', str(tmp_path), '-experiment_name', 'ftc', '-optimizer_type',
           optimizer, '-learning_rate', '0.05', '-kg_lambda', '0.5', '-norm_lambda', '0.7', '-L1_flag' if l1 else '-noL1_flag'])
    FLAGS.ckpt_path = str(tmp_path)
    torch.manual_seed(4)
    m = CFKG.CFKG(l1, D, NU, NE, NE, NR)             # items are drawn from the entity range: -share_embeddings is forced for CFKG
    tr = ModelTrainer(m, logging.getLogger('ftc'), 10, FLAGS)
    assert tr.model_target == -1
    return FLAGS, m, tr


def make_stepper(m, tr, FLAGS, B):
    from jTransUP.utils.fast_train_dot import BaselineJointStepper
    return BaselineJointStepper(m, tr, FLAGS, B)


def draw(gen, B, is_rec):
    """One global batch as device id tensors (what the driver hands the stepper: item ids already mapped to entity rows)."""
    rnd = lambda hi: torch.randint(0, hi, (B,), generator=gen).tolist()
    if is_rec:
        ids = (rnd(NU), rnd(NE), rnd(NE))
    else:
        ph, pt, pr, nh, nt = rnd(NE), rnd(NE), rnd(NR), rnd(NE), rnd(NE)
        ids = (ph, pt, pr, nh, nt, pr)
    return tuple(torch.tensor(x, dtype=torch.int64, device=DEV) for x in ids)


def autograd_step(FLAGS, m, tr, is_rec, ids):
    """The step body of the driver's autograd route (no alignment term: the item table is the entity table)."""
    from jTransUP.utils import loss
    tr.optimizer_zero_grad()
    if is_rec:
        u, pi, ni = ids
        losses = loss.bprLoss(m((u, pi), None, is_rec=True), m((u, ni), None, is_rec=True), target=tr.model_target)
    else:
        ph, pt, pr, nh, nt, nr = ids
        losses = loss.marginLoss()(m(None, (ph, pt, pr), is_rec=False), m(None, (nh, nt, nr), is_rec=False), FLAGS.margin)
        rel_ids = torch.cat([pr, nr])
        losses = losses + loss.normLoss(m.ent_embeddings.weight, ids=torch.cat([ph, pt, nh, nt])) \
            + loss.normLoss(m.rel_embeddings.weight, ids=rel_ids)
        losses = FLAGS.kg_lambda * losses
    losses.backward()
    tr.clip_and_step(FLAGS.clipping_max_value)
    return losses.detach()


def fast_step(fast, is_rec, ids):
    return fast.rec_step(*ids) if is_rec else fast.kg_step(*ids)


@pytest.mark.parametrize('l1', [True, False])
@pytest.mark.parametrize('D', [36, 100])
@pytest.mark.parametrize('optimizer', ['Adagrad', 'SGD', 'Adam'])
def test_cfkg_stepper_matches_the_autograd_route(tmp_path, optimizer, D, l1):
    FLAGS, m1, tr1 = build(tmp_path, optimizer, D, l1)
    _, m2, tr2 = build(tmp_path, optimizer, D, l1)
    m2.load_state_dict(copy.deepcopy(m1.state_dict()))
    B = 64
    fast = make_stepper(m2, tr2, FLAGS, B)
    assert fast.cfkg and not fast.align and [tuple(t.shape) for t in fast.tabs] == [(NU, D), (NE, D), (NR + 1, D)]
    gen = torch.Generator().manual_seed(9)
    # the mixed schedule of tests/test_fast_train_dot.py, extended until every captured kind has been replayed at least four times
    schedule = [True, True, False, True, False, False, True] + [True, False] * 4
    replays = {}
    for step, is_rec in enumerate(schedule):
        ids = draw(gen, B, is_rec)
        before = {k: v[0] for k, v in fast._graphs.items()}
        want = autograd_step(FLAGS, m1, tr1, is_rec, ids)
        got = fast_step(fast, is_rec, ids)
        print('step %d %s: loss %.9g (autograd %.9g)' % (step, 'rec' if is_rec else 'kg', float(got), float(want)))
        torch.testing.assert_close(got.reshape(()), want.reshape(()), rtol=1e-5, atol=1e-6)
        assert tr1.step == tr2.step == step + 1
        name = 'rec' if is_rec else 'kg'
        if name in fast._graphs and (name not in before or before[name] is fast._graphs[name][0]):
            replays[name] = replays.get(name, 0) + 1                       # this step was a replay (the capturing step replays too)
        for (k, a), (_, b) in zip(m1.state_dict().items(), m2.state_dict().items()):
            err = (b - a).abs()
            bad = err > 2e-6 + 2e-5 * a.abs()
            print('  %s: %d of %d beyond, max %.3g' % (k, int(bad.sum()), bad.numel(), float(err.max())))
            assert int(bad.sum()) <= max(6, int((2e-2 if optimizer == 'Adam' else 2e-3) * bad.numel())) and float(err.max()) <= STRAY_CAP, \
                '%s after step %d: %d elements off, max %.3g' % (k, step, int(bad.sum()), float(err.max()))
    print('replays %s' % replays)
    assert fast._graphs and set(fast._graphs) == {'rec', 'kg'}
    assert all(replays.get(k, 0) >= 4 for k in ('rec', 'kg')), replays


def _run_schedule(fast, B, schedule):
    gen = torch.Generator().manual_seed(9)
    return [float(fast_step(fast, is_rec, draw(gen, B, is_rec))) for is_rec in schedule]


def _dp_worker(rank, world, port, tmp, out, D):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group('gloo', rank=rank, world_size=world)     # both ranks share the one GPU: RCCL refuses that, gloo does not
    try:
        FLAGS, m, tr = build(os.path.join(tmp, 'r%d' % rank), 'Adagrad', D, True)
        B = 64
        fast = make_stepper(m, tr, FLAGS, B)
        assert fast.world == world and fast.B == B // world
        losses = _run_schedule(fast, B, [True, False, True, False])
        torch.save({'state': {k: v.cpu() for k, v in m.state_dict().items()}, 'losses': losses}, os.path.join(out, 'rank%d.pt' % rank))
    finally:
        dist.destroy_process_group()


def test_data_parallel_steps_match_one_process(tmp_path):
    """Two replicas (gloo, sharing the GPU) on halves of each global batch == one process on the whole batch."""
    import socket
    import torch.multiprocessing as mp
    D = 36
    for r in range(2):
        os.makedirs(os.path.join(str(tmp_path), 'r%d' % r))
    s = socket.socket(); s.bind(('127.0.0.1', 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_dp_worker, args=(2, port, str(tmp_path), str(tmp_path), D), nprocs=2, join=True)
    FLAGS, m, tr = build(tmp_path, 'Adagrad', D, True)
    losses = _run_schedule(make_stepper(m, tr, FLAGS, 64), 64, [True, False, True, False])
    r0 = torch.load(os.path.join(str(tmp_path), 'rank0.pt'))
    r1 = torch.load(os.path.join(str(tmp_path), 'rank1.pt'))
    for k, v in m.state_dict().items():
        assert torch.equal(r0['state'][k], r1['state'][k]), k                 # replicas stay identical
        err = (r0['state'][k] - v.cpu()).abs()
        bad = err > 2e-6 + 2e-5 * v.cpu().abs()
        assert float(bad.float().mean()) <= 2e-3 and float(err.max()) <= STRAY_CAP, (k, int(bad.sum()), float(err.max()))
    torch.testing.assert_close(torch.tensor(r0['losses']), torch.tensor(losses), rtol=1e-5, atol=1e-6)


# ---------------------------------------------------------------------------------------------------- command line
@pytest.fixture(scope='module')
def dataset(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('ds')
    make_dataset(str(tmp))
    return tmp


COMMON = ['-dataset', 'ml1m', '-nohas_visualization', '-batch_size', '32', '-embedding_size', '20', '-seed', '3', '-eval_interval_steps',
          '10', '-training_steps', '25', '-early_stopping_steps_to_wait', '0', '-learning_rate', '0.05', '-topn', '10']


@pytest.mark.parametrize('fast', [True, False])
def test_cli_takes_the_new_route(dataset, fast, monkeypatch):
    data = str(dataset)
    logs = os.path.join(data, 'log')
    os.makedirs(logs, exist_ok=True)
    name = 'cfkg-%d' % fast
    if not fast:
        monkeypatch.setenv('KTUP_FAST_TRAIN', '0')
    cmd = [sys.executable, os.path.join(PKG, 'run_knowledgable_recommendation.py'), '-data_path', data, '-log_path', logs, '-experiment_name',
           name, '-model_type', 'cfkg', '-rec_test_files', 'valid.dat', '-kg_test_files', 'valid.dat', '-joint_ratio', '0.7'] + COMMON
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    log = open(os.path.join(logs, name + '.log')).read()
    assert ('GPU-resident training step enabled' in log) == fast
    losses = [float(x) for x in re.findall(r'train loss:(\d+\.\d+)', log)]
    assert len(losses) >= 2 and all(l == l and l < 1e4 for l in losses)
    assert len(re.findall(r'f1:\d\.\d+', log)) >= 3
    assert os.path.isfile(os.path.join(logs, name + '.ckpt'))
