"""Times the training step of FM, coFM and CKE through its three routes, in ONE process:

    python tools/dot_step_time.py [--rounds 5] [--steps 200] [--repeats 2] [-o profiles/dot_step_times.txt]

  (a) the autograd route: the step body of the drivers (model(...), bprLoss / marginLoss, regularisers, the alignment term,
      .backward(), clip_and_step) -- what KTUP_FAST_TRAIN=0 runs
  (b) the GPU-resident stepper (utils/fast_train_dot.py) issuing its launches one by one (KTUP_TRAIN_GRAPHS=0)
  (c) the same stepper replaying its HIP graphs (CKE: the rec step only -- its TransR kg step records a memset and is never
      captured, DESIGN.md section 8 -- so three steps in ten of CKE's leg (c) are eager launches)
at ml1m-size tables (6040 users, 3240 items, 14,709 entities, 20 relations): FM at B = 1024, d = 100, Adagrad (fm.sh); coFM (own
item table: the alignment term is in every step) and CKE at B = 400, d = 100, L1, Adam, joint_ratio 0.7 (cofm.sh, cke.sh).
Every leg starts from host id lists, as the drivers' host-fed steps do (coFM's alignment set walk included), and runs the
10-step cycle of the joint driver (7 rec, 3 kg).  Rounds alternate between the legs; a round's figure is the mean wall time per
step of its steps (device idle before and after); reported is the median over the rounds and their spread (max - min).  The whole
measurement is repeated from fresh models.  Also recorded, not acted on: BPRMF through ktup_train_dot_step against its present
three-launch step (RecStepper)."""
import argparse
import logging
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'joint-kg-recommender_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

NU, NI, NE, NR = 6040, 3240, 14709, 20
CONFIG = {'fm': (1024, 'Adagrad', '0.1', '1e-5'), 'bprmf': (1024, 'Adagrad', '0.1', '1e-5'), 'cofm': (400, 'Adam', '0.001', '0'),
          'cke': (400, 'Adam', '0.001', '0')}


def maps():
    """Nine items in ten have an entity (distinct ones), as in ml1m."""
    i_map = {i: 'k%d' % i for i in range(NI)}
    ikg = {'k%d' % i: ((i * 4) % NE if i % 10 else -1, i) for i in range(NI)}
    e_map = {e: 'e%d' % e for e in range(NE)}
    for key, (e, i) in list(ikg.items()):
        if e != -1:
            e_map[e] = key
    for e in range(NE):
        if e_map[e] == 'e%d' % e:
            ikg['e%d' % e] = (e, -1)
    return i_map, e_map, ikg


def build(kind, tmp):
    import torch
    from jTransUP.models import CKE, bprmf, cofm, fm
    from jTransUP.models.base import get_flags
    from jTransUP.utils.flags import FLAGS
    from jTransUP.utils.trainer import ModelTrainer
    B, opt, lr, l2 = CONFIG[kind]
    get_flags(); FLAGS.reset()
    FLAGS(['prog', '-model_type', kind, '-noshare_embeddings', '-log_path', tmp, '-experiment_name', 'dst', '-optimizer_type', opt,
           '-learning_rate', lr, '-l2_lambda', l2, '-batch_size', str(B), '-embedding_size', '100', '-joint_ratio', '0.7', '-L1_flag',
           '-norm_lambda', '1', '-kg_lambda', '1'])
    FLAGS.ckpt_path = tmp
    i_map, e_map, ikg = maps()
    torch.manual_seed(3)
    if kind == 'fm':
        m = fm.FM(100, NU, NI)
    elif kind == 'bprmf':
        m = bprmf.BPRMF(100, NU, NI)
    elif kind == 'cofm':
        m = cofm.coFM(True, 100, NU, NI, NE, NR, False)
    else:
        m = CKE.CKE(True, 100, NU, NI, NE, NR, i_map, ikg)
    log = logging.getLogger('dst')
    log.setLevel(logging.WARNING)
    return FLAGS, m, ModelTrainer(m, log, 1000, FLAGS)


def batches(kind, n=20, seed=5):
    """Host id lists of n steps of the 10-step cycle + coFM's alignment lists' inputs."""
    import random
    rng = random.Random(seed)
    B = CONFIG[kind][0]
    out = []
    for s in range(n):
        is_rec = kind in ('fm', 'bprmf') or s % 10 < 7
        if is_rec:
            out.append((True, ([rng.randrange(NU) for _ in range(B)], [rng.randrange(NI) for _ in range(B)], [rng.randrange(NI) for _ in range(B)])))
        else:
            pr = [rng.randrange(NR) for _ in range(B)]
            out.append((False, ([rng.randrange(NE) for _ in range(B)], [rng.randrange(NE) for _ in range(B)], pr,
                                [rng.randrange(NE) for _ in range(B)], [rng.randrange(NE) for _ in range(B)], pr)))
    return out


class Leg(object):
    def __init__(self, kind, route, tmp):
        from jTransUP.models import _driver as D
        from jTransUP.models.knowledgable_recommendation import getMappedEntities, getMappedItems
        self.kind, self.route, self.D = kind, route, D
        self.FLAGS, self.m, self.tr = build(kind, tmp)
        self.i_map, self.e_map, self.ikg = maps()
        self.gme, self.gmi = getMappedEntities, getMappedItems
        self.fast = None
        if route != 'autograd':
            from jTransUP.utils.fast_train import RecStepper
            from jTransUP.utils.fast_train_dot import BaselineJointStepper, DotRecStepper
            cls = RecStepper if route.startswith('rec3') else DotRecStepper if kind in ('fm', 'bprmf') else BaselineJointStepper
            self.fast = cls(self.m, self.tr, self.FLAGS, CONFIG[kind][0], use_graphs=route.endswith('graphs'))

    def step(self, is_rec, lists):
        D, m, tr, FLAGS, kind = self.D, self.m, self.tr, self.FLAGS, self.kind
        align = None
        if kind == 'cofm':
            align = self.gme(lists[1] + lists[2], self.i_map, self.ikg) if is_rec else \
                self.gmi(lists[0] + lists[1] + lists[3] + lists[4], self.e_map, self.ikg)
        ids = tuple(D.ids(x) for x in lists)
        if self.fast is not None:
            if kind in ('fm', 'bprmf'):
                return self.fast.rec_step(*ids)
            return self.fast.rec_step(*ids, align=align) if is_rec else self.fast.kg_step(*ids, align=align)
        from jTransUP.utils import loss
        tr.optimizer_zero_grad()
        if kind in ('fm', 'bprmf'):
            u, pi, ni = ids
            losses = loss.bprLoss(m(u, pi), m(u, ni), target=tr.model_target)
        elif is_rec:
            u, pi, ni = ids
            losses = loss.bprLoss(m((u, pi), None, is_rec=True), m((u, ni), None, is_rec=True), target=tr.model_target)
        else:
            import torch
            ph, pt, pr, nh, nt, nr = ids
            losses = loss.marginLoss()(m(None, (ph, pt, pr), is_rec=False), m(None, (nh, nt, nr), is_rec=False), FLAGS.margin)
            rel_ids = torch.cat([pr, nr])
            losses = losses + loss.normLoss(m.ent_embeddings.weight, ids=torch.cat([ph, pt, nh, nt])) \
                + loss.normLoss(m.rel_embeddings.weight, ids=rel_ids)
            losses = FLAGS.kg_lambda * losses
        if kind == 'cofm':
            losses = losses + FLAGS.norm_lambda * loss.pNormLoss(m.ent_embeddings(D.ids(align[0])), m.item_embeddings(D.ids(align[1])),
                                                                 L1_flag=FLAGS.L1_flag)
        losses.backward()
        D.clip_and_step(FLAGS, m, tr)
        return losses


def measure(kind, routes, labels, rounds, steps, tmp, out):
    import torch
    legs = [Leg(kind, r, tmp) for r in routes]
    pool = batches(kind)
    for leg in legs:                                                      # eager steps, captures, first replays
        for s in range(20):
            last = leg.step(*pool[s % len(pool)])
        last = float(last.detach())
        assert last == last, 'loss is not finite'
    per = {r: [] for r in routes}
    for _ in range(rounds):
        for leg in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for s in range(steps):
                leg.step(*pool[s % len(pool)])
            torch.cuda.synchronize()
            per[leg.route].append((time.perf_counter() - t0) / steps * 1e3)
    res = {}
    for r, lab in zip(routes, labels):
        med, spread = statistics.median(per[r]), max(per[r]) - min(per[r])
        res[r] = (med, spread)
        out.append('%-22s %-34s median %8.4f ms   spread %7.4f ms   (rounds: %s)' % (kind, lab, med, spread, ' '.join('%.4f' % x for x in per[r])))
    return res


def run(a, tmp):
    import torch
    out = ['# tools/dot_step_time.py: training step of FM / coFM / CKE -- autograd route vs GPU-resident stepper, from host id lists',
           '# %s, %d rounds x %d steps per leg, alternating; wall time per step in ms; %d repeats from fresh models'
           % (torch.cuda.get_device_name(0), a.rounds, a.steps, a.repeats)]
    routes = ['autograd', 'stepper-eager', 'stepper-graphs']
    labels = ['(a) autograd route', '(b) stepper, KTUP_TRAIN_GRAPHS=0', '(c) stepper, graph replay']
    verdict = {}
    for rep in range(a.repeats):
        out.append('# repeat %d' % (rep + 1))
        for kind in ('fm', 'cofm', 'cke'):
            res = measure(kind, routes, labels, a.rounds, a.steps, tmp, out)
            gain, bar = res['autograd'][0] - res['stepper-graphs'][0], max(v[1] for v in res.values())
            ok = gain > bar
            verdict[kind] = verdict.get(kind, True) and ok
            out.append('%-22s (a) - (c) = %.4f ms, largest spread %.4f ms, (a) / (c) = %.2f: the stepper is %s'
                       % (kind, gain, bar, res['autograd'][0] / res['stepper-graphs'][0], 'FASTER' if ok else 'NOT faster'))
        measure('bprmf', ['rec3-graphs', 'dot-graphs'], ['three-launch step, graph replay', 'ktup_train_dot_step, graph replay'],
                a.rounds, a.steps, tmp, out)
    for kind in ('fm', 'cofm', 'cke'):
        out.append('# %s: (c) below (a) by more than the spread in every repeat: %s' % (kind, 'yes' if verdict[kind] else 'NO'))
    return '\n'.join(out) + '\n'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--repeats', type=int, default=2)
    ap.add_argument('-o', '--output', default=os.path.join(ROOT, 'profiles', 'dot_step_times.txt'))
    a = ap.parse_args()
    import tempfile
    with tempfile.TemporaryDirectory(prefix='dot_step_time_') as tmp:
        text = run(a, tmp)
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.output)), exist_ok=True)
    open(a.output, 'w').write(text)


if __name__ == '__main__':
    main()
