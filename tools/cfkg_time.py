"""Times CFKG's training step and its rec evaluation pass through their old and new routes:

    python tools/cfkg_time.py [--rounds 5] [--steps 200] [--passes 20] [-o profiles/cfkg_times.txt]

at ml1m-size tables (6040 users, 14,709 entities, 3240 items mapped to distinct entity rows, 20 relations + buy), d = 100:

  step   B = 400, Adagrad, L1, joint_ratio 0.7: the 10-step cycle of the joint driver (7 rec, 3 kg), every leg from host id lists
         (a) the autograd route: the step body of the driver (model(...), bprLoss / marginLoss, normLoss, .backward(),
             clip_and_step) -- what KTUP_FAST_TRAIN=0 runs
         (b) BaselineJointStepper (utils/fast_train_dot.py) issuing its launches one by one (KTUP_TRAIN_GRAPHS=0)
         (c) the same stepper replaying its HIP graphs
  pass   6040 users, ~165 filtered items each, topn 10, through knowledgable_recommendation.evaluateRec, for L1 and squared L2
         (a) the batch walk (KTUP_EVAL_PASS=0): evaluateRec per 512 users + the ranking kernel
         (b) the one-sweep pass (CFKG.evaluate_topk -> ktup_eval_cfkg_topk), replayed as a graph from its third call on

Old and new routes alternate in one process; a round's figure is the mean wall time per step / per pass (device idle before and
after); reported is the median over the rounds and their spread (max - min).  A new route counts as FASTER if it is below its
yardstick by more than the larger of the two spreads.  Every GPU leg (step, pass L1, pass L2) is a child process of its own under
its own time limit; a leg that fails ends the run."""
import argparse
import logging
import os
import statistics
import subprocess
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'joint-kg-recommender_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

NU, NI, NE, NR, D, B = 6040, 3240, 14709, 20, 100, 400
LEG_LIMIT_S = 240


def item_map():
    return {i: (i * 4) % NE for i in range(NI)}                          # distinct entity rows (4 and 14,709 are coprime)


# ---------------------------------------------------------------------------------------------------- the training step
def build(tmp):
    import torch
    from jTransUP.models import CFKG
    from jTransUP.models.base import get_flags
    from jTransUP.utils.flags import FLAGS
    from jTransUP.utils.trainer import ModelTrainer
    get_flags(); FLAGS.reset()
    FLAGS(['prog', '-model_type', 'cfkg', '-share_embeddings', '-log_path', tmp, '-experiment_name', 'cfkgt', '-optimizer_type', 'Adagrad',
           '-learning_rate', '0.005', '-batch_size', str(B), '-embedding_size', str(D), '-joint_ratio', '0.7', '-L1_flag', '-kg_lambda', '1'])
    FLAGS.ckpt_path = tmp
    torch.manual_seed(3)
    m = CFKG.CFKG(True, D, NU, NE, NE, NR)
    log = logging.getLogger('cfkgt')
    log.setLevel(logging.WARNING)
    return FLAGS, m, ModelTrainer(m, log, 1000, FLAGS)


def step_batches(n=20, seed=5):
    """Host id lists of n steps of the 10-step cycle, item ids already mapped to entity rows (the driver's `i_map` lookups)."""
    import random
    rng = random.Random(seed)
    i_map = item_map()
    draw = lambda hi: [rng.randrange(hi) for _ in range(B)]
    out = []
    for s in range(n):
        if s % 10 < 7:
            out.append((True, (draw(NU), [i_map[i] for i in draw(NI)], [i_map[i] for i in draw(NI)])))
        else:
            pr = draw(NR)
            out.append((False, (draw(NE), draw(NE), pr, draw(NE), draw(NE), pr)))
    return out


class StepLeg(object):
    def __init__(self, route, tmp):
        from jTransUP.models import _driver as Dr
        self.route, self.Dr = route, Dr
        self.FLAGS, self.m, self.tr = build(tmp)
        self.fast = None
        if route != 'autograd':
            from jTransUP.utils.fast_train_dot import BaselineJointStepper
            self.fast = BaselineJointStepper(self.m, self.tr, self.FLAGS, B, use_graphs=route.endswith('graphs'))

    def step(self, is_rec, lists):
        import torch
        Dr, m, tr, FLAGS = self.Dr, self.m, self.tr, self.FLAGS
        ids = tuple(Dr.ids(x) for x in lists)
        if self.fast is not None:
            return self.fast.rec_step(*ids) if is_rec else self.fast.kg_step(*ids)
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
        Dr.clip_and_step(FLAGS, m, tr)
        return losses


def leg_step(a, tmp):
    import torch
    routes = ['autograd', 'stepper-eager', 'stepper-graphs']
    labels = ['(a) autograd route', '(b) stepper, KTUP_TRAIN_GRAPHS=0', '(c) stepper, graph replay']
    legs = [StepLeg(r, tmp) for r in routes]
    pool = step_batches()
    for leg in legs:                                                      # eager steps, captures, first replays
        for s in range(20):
            last = leg.step(*pool[s % len(pool)])
        last = float(last.detach())
        assert last == last, 'loss is not finite'
    per = {r: [] for r in routes}
    for _ in range(a.rounds):
        for leg in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for s in range(a.steps):
                leg.step(*pool[s % len(pool)])
            torch.cuda.synchronize()
            per[leg.route].append((time.perf_counter() - t0) / a.steps * 1e3)
    out, res = [], {}
    for r, lab in zip(routes, labels):
        med, spread = statistics.median(per[r]), max(per[r]) - min(per[r])
        res[r] = (med, spread)
        out.append('%-12s %-34s median %8.4f ms   spread %7.4f ms   (rounds: %s)' % ('step', lab, med, spread, ' '.join('%.4f' % x for x in per[r])))
    for new in ('stepper-eager', 'stepper-graphs'):
        gain, bar = res['autograd'][0] - res[new][0], max(res['autograd'][1], res[new][1])
        out.append('%-12s (a) - %s = %.4f ms, larger spread %.4f ms, ratio %.2f: the stepper is %s'
                   % ('step', '(b)' if new.endswith('eager') else '(c)', gain, bar, res['autograd'][0] / res[new][0], 'FASTER' if gain > bar else 'NOT faster'))
    return out


# ---------------------------------------------------------------------------------------------------- the evaluation pass
def world(l1, seed=7):
    import numpy as np
    import torch
    from jTransUP.models import CFKG
    torch.manual_seed(seed)
    rng = np.random.RandomState(seed)
    m = CFKG.CFKG(l1, D, NU, NE, NE, NR)
    m.eval(); m.disable_grad()
    users = list(range(NU))
    gold = {u: set(rng.randint(0, NI, size=5).tolist()) for u in users}
    train = {u: set(rng.randint(0, NI, size=165).tolist()) for u in users}
    batches = [users[s:s + 512] for s in range(0, NU, 512)]
    return m, gold, train, batches


def leg_pass(a, l1):
    import numpy as np
    import torch
    from jTransUP.models import _driver as Dr
    from jTransUP.models import knowledgable_recommendation as K
    m, gold, train, batches = world(l1)
    i_map = item_map()
    FL = types.SimpleNamespace(topn=10, share_embeddings=True)
    log = logging.getLogger('cfkgt')
    log.setLevel(logging.WARNING)
    rows = {}
    keep = Dr.rec_eval_pass

    def recording(*args, **kw):
        rows['last'] = keep(*args, **kw)
        return rows['last']
    Dr.rec_eval_pass = recording

    def one_pass(fused):
        os.environ['KTUP_EVAL_PASS'] = '1' if fused else '0'
        K.evaluateRec(FL, m, batches, gold, [train], i_map, log, eval_descending=False)
        return rows['last']
    ref = one_pass(False)
    for _ in range(3):                                                    # eager, capture, first replay
        got = one_pass(True)
    assert ref.shape == got.shape and float(np.abs(ref.mean(0) - got.mean(0)).max()) <= 2.0 / len(ref), 'the two routes disagree'
    per = {False: [], True: []}
    for _ in range(a.rounds):
        for fused in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.passes):
                one_pass(fused)
            torch.cuda.synchronize()
            per[fused].append((time.perf_counter() - t0) / a.passes * 1e3)
    name = 'pass %s' % ('L1' if l1 else 'L2')
    out, res = [], {}
    for fused in (False, True):
        med, spread = statistics.median(per[fused]), max(per[fused]) - min(per[fused])
        res[fused] = (med, spread)
        out.append('%-12s %-34s median %8.3f ms   spread %7.3f ms   (rounds: %s)'
                   % (name, '(b) one-sweep pass' if fused else '(a) batch walk', med, spread, ' '.join('%.3f' % x for x in per[fused])))
    gain, bar = res[False][0] - res[True][0], max(res[False][1], res[True][1])
    out.append('%-12s (a) - (b) = %.3f ms, larger spread %.3f ms, ratio %.2f: the pass is %s'
               % (name, gain, bar, res[False][0] / res[True][0], 'FASTER' if gain > bar else 'NOT faster'))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--passes', type=int, default=20)
    ap.add_argument('--leg', choices=['step', 'pass-l1', 'pass-l2'], help='run one leg in this process and print its lines')
    ap.add_argument('-o', '--output', default=os.path.join(ROOT, 'profiles', 'cfkg_times.txt'))
    a = ap.parse_args()
    if a.leg:
        import tempfile
        import torch
        print('# %s' % torch.cuda.get_device_name(0))
        if a.leg == 'step':
            with tempfile.TemporaryDirectory(prefix='cfkg_time_') as tmp:
                lines = leg_step(a, tmp)
        else:
            lines = leg_pass(a, a.leg == 'pass-l1')
        print('\n'.join(lines))
        return 0
    assert a.rounds >= 5, 'at least five rounds'
    out = ['# tools/cfkg_time.py: CFKG at ml1m-size tables (%d users, %d entities, %d items), d = %d -- old route vs new route, alternating in one process'
           % (NU, NE, NI, D),
           '# step: B = %d, Adagrad, L1, %d rounds x %d steps per leg, wall time per step of the 10-step joint cycle in ms' % (B, a.rounds, a.steps),
           '# pass: %d users x %d items, topn 10, %d rounds x %d passes per route, wall time per pass in ms' % (NU, NI, a.rounds, a.passes)]
    for leg in ('step', 'pass-l1', 'pass-l2'):                            # a GPU process each, under its own time limit; stop at the first failure
        cmd = ['timeout', '-k', '10', str(LEG_LIMIT_S), sys.executable, os.path.abspath(__file__), '--leg', leg, '--rounds', str(a.rounds),
               '--steps', str(a.steps), '--passes', str(a.passes)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-3000:] + r.stderr[-3000:])
            sys.stderr.write('\nleg %s ended with status %d: nothing further is started\n' % (leg, r.returncode))
            return r.returncode
        lines = r.stdout.strip().splitlines()
        if len(out) == 3:
            out.insert(1, lines[0])
        out += [ln for ln in lines[1:] if ln.startswith(('step', 'pass'))]
    text = '\n'.join(out) + '\n'
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.output)), exist_ok=True)
    open(a.output, 'w').write(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
