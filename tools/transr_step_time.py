"""Times the TransR training step through its old and its new route, at ml1m-size tables (14,709 entities, 20 relations), d = 100:

    python tools/transr_step_time.py [--rounds 21] [--steps 10] [-o profiles/transr_step_times.txt]

  kg     KGStepper on TransR, B = 512, Adagrad, squared L2:
         (a) the bucketed multi-launch route as eager launches (KTUP_FUSED_STEP=0: memset, three bucket launches, forward, margin
             loss, backward, two regularisers) -- never replayed from a graph here or anywhere
         (b) the one launch (ktup_train_transr_step) issued eagerly
         (c) the one launch replayed from its captured graph
  cke    BaselineJointStepper on CKE, B = 400, Adagrad, L1, the 10-step cycle of the joint driver (7 rec, 3 kg), graphs on (the rec
         step replays, the kg step is issued eagerly on both routes):
         (a) kg step on the bucketed route (KTUP_FUSED_STEP=0)      (b) kg step as the one launch

Old and new routes alternate inside one process, round by round; a round's figure is the device time per step between two events
around `--steps` steps; reported is the median over the rounds and their spread (max - min).  A new route counts as FASTER if it is
below the old one by more than the larger of the two spreads.  Run it twice, each call under its own time limit; the larger spread of
the two repeats is what the default is decided on."""
import argparse
import logging
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'joint-kg-recommender_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)
import torch

NU, NI, NE, NR, D = 6040, 3240, 14709, 20, 100


def _flags(tmp, model_type, extra):
    from jTransUP.models.base import get_flags
    from jTransUP.utils.flags import FLAGS
    get_flags(); FLAGS.reset()
    FLAGS(['prog', '-model_type', model_type, '-log_path', tmp, '-experiment_name', 'time-' + model_type, '-optimizer_type', 'Adagrad'] + extra)
    FLAGS.ckpt_path = tmp
    return FLAGS


def _trainer(m, FLAGS):
    from jTransUP.utils.trainer import ModelTrainer
    log = logging.getLogger('transr_step_time')
    log.setLevel(logging.WARNING)
    return ModelTrainer(m, log, 1000, FLAGS)


def _with_fused(on, make):
    """Build a stepper with KTUP_FUSED_STEP set for its constructor (the steppers read it once, when they are made)."""
    old = os.environ.get('KTUP_FUSED_STEP')
    os.environ['KTUP_FUSED_STEP'] = '1' if on else '0'
    try:
        return make()
    finally:
        if old is None:
            del os.environ['KTUP_FUSED_STEP']
        else:
            os.environ['KTUP_FUSED_STEP'] = old


def kg_legs(tmp):
    from jTransUP.models import transR
    from jTransUP.utils.fast_train import KGStepper
    B = 512
    dev = torch.device('cuda')
    legs = []
    for label, fused, graphs in (('(a) bucketed route, eager launches', False, False), ('(b) one launch, issued eagerly', True, False),
                                 ('(c) one launch, graph replay', True, True)):
        FLAGS = _flags(tmp, 'transr', ['-batch_size', str(B), '-embedding_size', str(D)])
        torch.manual_seed(2)
        m = transR.TransRModel(False, D, NE, NR)
        tr = _trainer(m, FLAGS)
        st = _with_fused(fused, lambda: KGStepper(m, tr, FLAGS, B, use_graphs=graphs))
        assert st.transr_step == fused
        gen = torch.Generator().manual_seed(3)
        pool = [[torch.randint(0, hi, (B,), generator=gen).to(dev) for hi in (NE, NE, NR, NE, NE)] for _ in range(10)]

        def step(s, st=st, pool=pool):
            i = pool[s % len(pool)]
            return st.kg_step(i[0], i[1], i[2], i[3], i[4], i[2])
        for s in range(10):                                           # eager steps, the capture, first replays
            last = step(s)
        assert float(last) == float(last), 'loss is not finite'
        torch.cuda.synchronize()
        assert bool(st._graphs) == graphs
        legs.append((label, step))
    return legs


def cke_legs(tmp):
    from jTransUP.models import CKE
    from jTransUP.models import _driver as Dr
    from jTransUP.utils.fast_train_dot import BaselineJointStepper
    import random
    B = 400
    i_map = {i: 'k%d' % i for i in range(NI)}
    new_map = {'k%d' % i: ((i * 4) % NE, i) for i in range(NI)}        # distinct entity rows (4 and 14,709 are coprime)
    rng = random.Random(5)
    draw = lambda hi: [rng.randrange(hi) for _ in range(B)]
    pool = []
    for s in range(20):
        if s % 10 < 7:
            pool.append((True, tuple(Dr.ids(x) for x in (draw(NU), draw(NI), draw(NI)))))
        else:
            pr = draw(NR)
            pool.append((False, tuple(Dr.ids(x) for x in (draw(NE), draw(NE), pr, draw(NE), draw(NE), pr))))
    legs = []
    for label, fused in (('(a) kg step on the bucketed route', False), ('(b) kg step as the one launch', True)):
        FLAGS = _flags(tmp, 'cke', ['-noshare_embeddings', '-learning_rate', '0.005', '-batch_size', str(B), '-embedding_size', str(D),
                                    '-joint_ratio', '0.7', '-L1_flag', '-kg_lambda', '1'])
        torch.manual_seed(3)
        m = CKE.CKE(True, D, NU, NI, NE, NR, i_map, new_map)
        tr = _trainer(m, FLAGS)
        st = _with_fused(fused, lambda: BaselineJointStepper(m, tr, FLAGS, B, use_graphs=True))
        assert st.transr_step == fused

        def step(s, st=st):
            is_rec, ids = pool[s % len(pool)]
            return st.rec_step(*ids) if is_rec else st.kg_step(*ids)
        for s in range(20):
            last = step(s)
        assert float(last) == float(last), 'loss is not finite'
        torch.cuda.synchronize()
        assert set(st._graphs) == {'rec'}
        legs.append((label, step))
    return legs


def measure(name, legs, rounds, steps, out):
    per = {label: [] for label, _ in legs}
    for _ in range(rounds):
        for label, step in legs:                                       # the routes alternate, round by round
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for s in range(steps):
                step(s)
            b.record()
            b.synchronize()
            per[label].append(a.elapsed_time(b) / steps * 1e3)
    res = {}
    for label, _ in legs:
        med, spread = statistics.median(per[label]), max(per[label]) - min(per[label])
        res[label] = (med, spread)
        out.append('%-4s %-36s median %8.1f us per step   spread %7.1f us   [min %.1f max %.1f]   (%d rounds x %d steps)'
                   % (name, label, med, spread, min(per[label]), max(per[label]), rounds, steps))
        print(out[-1], flush=True)
    old = legs[0][0]
    for label, _ in legs[1:]:
        gain, bar = res[old][0] - res[label][0], max(res[old][1], res[label][1])
        out.append('%-4s (a) - %s = %.1f us, larger spread %.1f us, ratio %.2f: the new route is %s'
                   % (name, label[:3], gain, bar, res[old][0] / res[label][0], 'FASTER' if gain > bar else 'NOT faster'))
        print(out[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=21)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--only', default='', choices=['', 'kg', 'cke'])
    ap.add_argument('-o', '--out', default='')
    a = ap.parse_args()
    assert a.rounds >= 20, 'median of at least 20 rounds'
    out = ['# python tools/transr_step_time.py --rounds %d --steps %d%s   (%s)'
           % (a.rounds, a.steps, ' --only ' + a.only if a.only else '', torch.cuda.get_device_name(0))]
    with tempfile.TemporaryDirectory() as tmp:
        if a.only in ('', 'kg'):
            measure('kg', kg_legs(tmp), a.rounds, a.steps, out)
        if a.only in ('', 'cke'):
            measure('cke', cke_legs(tmp), a.rounds, a.steps, out)
    if a.out:
        with open(a.out, 'a') as f:
            f.write('\n'.join(out) + '\n')


if __name__ == '__main__':
    main()
