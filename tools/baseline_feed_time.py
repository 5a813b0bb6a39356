"""Device-fed steps of the joint baselines (coFM, CKE, CFKG; utils/fast_train_dot.py) against their host-fed steps, in ONE process:

    python tools/baseline_feed_time.py [--rounds 5] [--steps 200] [--repeats 2] [-o profiles/baseline_feed_times.txt]

  (a) the host-fed stepper replaying its graphs from ready HOST id lists -- what the command line runs without KTUP_BASELINE_FEED=1,
      minus the Python samplers: the lists exist already; what is timed is their copy to the device, coFM's alignment set walk
      (getMappedEntities / getMappedItems), CFKG's `[i_map[i] for i in ...]` and one graph launch per step (CKE's kg step: eager launches)
  (b) `fed_cycle` of the ten-step 7 : 3 cycle: batch, negatives, joint-table rows and alignment lists drawn on the device, ten steps
      per graph replay
at ml1m-size tables (6040 users, 3240 items, 14,709 entities, 20 relations), d = 100, B = 400, Adam: coFM with its own item table and
L1 (the README's configuration), CKE with L1, CFKG.  Rounds alternate between the legs; a round's figure is the mean wall time per step
(device idle before and after); reported are the median over the rounds and their spread (max - min), the whole measurement repeated
from fresh models.  A gain counts if it exceeds the larger spread.

Then, each in processes of their own: the device time of the two new launches (`feed_remap_ids_kernel`, `feed_align_lists_kernel`)
from one `rocprofv3 --kernel-trace --stats` run of the fed cycles (`--workload`), and the command line's steps per second for the
three models with and without the switch (the pattern of tools/cli_throughput.py).  `--skip-trace` / `--skip-cli` leave those out."""
import argparse
import csv
import datetime
import glob
import logging
import os
import random
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'joint-kg-recommender_amd')
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

NU, NI, NE, NR, D, B = 6040, 3240, 14709, 20, 100, 400
KINDS = ('cofm', 'cke', 'cfkg')
CYCLE = ('rec',) * 7 + ('kg',) * 3


def maps():
    """Nine items in ten have an entity (distinct ones), as in ml1m; the vocabulary load_kg_rating_data.load_data would build."""
    from jTransUP.data.load_kg_rating_data import rebuildEntityItemVocab
    ents = {'e%d' % e: e for e in range(NE)}
    items = {'i%d' % i: i for i in range(NI)}
    links = {'e%d' % ((i * 4) % NE): 'i%d' % i for i in range(NI) if i % 10}
    ikg, e_map, i_map, _ = rebuildEntityItemVocab(ents, items, links)
    return i_map, e_map, ikg


def build(kind, tmp):
    import torch
    from jTransUP.models import CFKG, CKE, cofm
    from jTransUP.models.base import get_flags
    from jTransUP.utils.flags import FLAGS
    from jTransUP.utils.trainer import ModelTrainer
    get_flags(); FLAGS.reset()
    FLAGS(['prog', '-model_type', kind, '-share_embeddings' if kind == 'cfkg' else '-noshare_embeddings', '-log_path', tmp,
           '-experiment_name', 'bft', '-optimizer_type', 'Adam', '-learning_rate', '0.001', '-l2_lambda', '0', '-batch_size', str(B),
           '-embedding_size', str(D), '-joint_ratio', '0.7', '-noL1_flag' if kind == 'cfkg' else '-L1_flag', '-norm_lambda', '1',
           '-kg_lambda', '1'])
    FLAGS.ckpt_path = tmp
    i_map, e_map, ikg = maps()
    torch.manual_seed(3)
    if kind == 'cofm':
        m = cofm.coFM(True, D, NU, NI, NE, NR, False)
    elif kind == 'cke':
        m = CKE.CKE(True, D, NU, NI, NE, NR, i_map, ikg)
    else:
        m = CFKG.CFKG(False, D, NU, len(ikg), len(ikg), NR)
    log = logging.getLogger('bft')
    log.setLevel(logging.WARNING)
    return FLAGS, m, ModelTrainer(m, log, 1000, FLAGS)


def host_batches(n=20, seed=5):
    rng = random.Random(seed)
    out = []
    for s in range(n):
        if s % 10 < 7:
            out.append((True, ([rng.randrange(NU) for _ in range(B)], [rng.randrange(NI) for _ in range(B)], [rng.randrange(NI) for _ in range(B)])))
        else:
            pr = [rng.randrange(NR) for _ in range(B)]
            out.append((False, ([rng.randrange(NE) for _ in range(B)], [rng.randrange(NE) for _ in range(B)], pr,
                                [rng.randrange(NE) for _ in range(B)], [rng.randrange(NE) for _ in range(B)], pr)))
    return out


class Leg(object):
    def __init__(self, kind, route, tmp):
        from jTransUP.models import _driver as Dr
        from jTransUP.models.knowledgable_recommendation import getMappedEntities, getMappedItems
        from jTransUP.utils.fast_train_dot import BaselineJointStepper
        self.kind, self.route, self.Dr = kind, route, Dr
        self.FLAGS, self.m, self.tr = build(kind, tmp)
        self.i_map, self.e_map, self.ikg = maps()
        self.gme, self.gmi = getMappedEntities, getMappedItems
        self.st = BaselineJointStepper(self.m, self.tr, self.FLAGS, B)
        self.pool = host_batches()
        self.at = 0
        if route == 'fed':
            from jTransUP.utils.device_sampler import DeviceSampler
            from jTransUP.utils.fast_train import DeviceFeeder
            rng = random.Random(11)
            ratings = [(rng.randrange(NU), rng.randrange(NI)) for _ in range(120000)]
            triples = [(rng.randrange(NE), rng.randrange(NE), rng.randrange(NR)) for _ in range(60000)]
            rated = {}
            for u, i in ratings:
                rated.setdefault(u, set()).add(i)
            self.sampler = DeviceSampler(Dr.DEV, seed=3)
            self.sampler.set_rating_dicts(NU, NI, [rated])
            self.sampler.set_triples(NE, NR, [triples])
            self.st.set_id_maps(self.i_map, self.e_map, self.ikg, NI, NE)
            self.st.attach_feeds(self.sampler, rec=DeviceFeeder(ratings, B, Dr.DEV, seed=3), kg=DeviceFeeder(triples, B, Dr.DEV, seed=4))
            if not (self.st.can_feed('rec') and self.st.can_feed('kg')):
                raise SystemExit('%s cannot be fed at this shape' % kind)

    def ten(self):
        """Ten steps of the 7 : 3 cycle."""
        st = self.st
        if self.route == 'fed':
            if not st.fed_cycle(CYCLE):                                   # warm-up, or the epoch ends inside the cycle
                for k in CYCLE:
                    st.fed_step(k)
            return
        Dr = self.Dr
        for _ in range(10):
            is_rec, lists = self.pool[self.at % len(self.pool)]
            self.at += 1
            align = None
            if is_rec:
                u, pi, ni = lists
                if st.align:
                    align = self.gme(pi + ni, self.i_map, self.ikg)
                if st.remaps:
                    pi = [self.i_map[i] for i in pi]; ni = [self.i_map[i] for i in ni]
                st.rec_step(Dr.ids(u), Dr.ids(pi), Dr.ids(ni), align=align)
            else:
                ph, pt, pr, nh, nt, nr = lists
                if st.align:
                    align = self.gmi(ph + pt + nh + nt, self.e_map, self.ikg)
                if st.remaps:
                    ph, pt, nh, nt = ([self.e_map[e] for e in x] for x in (ph, pt, nh, nt))
                st.kg_step(*(Dr.ids(x) for x in (ph, pt, pr, nh, nt, nr)), align=align)

    def finite(self):
        import torch
        torch.cuda.synchronize()
        if self.route == 'fed':
            self.sampler.check()
            sums = self.st.take_sums()
            assert all(v == v for v in sums.values()), sums
        assert all(bool(torch.isfinite(t).all()) for t in self.st.tabs), 'a table is not finite'


def measure(kind, rounds, steps, tmp, out):
    import torch
    routes = ['host-fed', 'fed']
    labels = ['(a) host-fed, graph replay', '(b) fed_cycle, ten steps a replay']
    legs = [Leg(kind, r, tmp) for r in routes]
    for leg in legs:                                                      # eager steps, captures, first replays
        for _ in range(6):
            leg.ten()
        leg.finite()
    per = {r: [] for r in routes}
    for _ in range(rounds):
        for leg in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps // 10):
                leg.ten()
            torch.cuda.synchronize()
            per[leg.route].append((time.perf_counter() - t0) / (steps // 10 * 10) * 1e3)
    for leg in legs:
        leg.finite()
    st = legs[1].st
    out.append('%-5s fed graphs %s, fed replays %s' % (kind, sorted(st._graphs), st.fed_replays))
    res = {}
    for r, lab in zip(routes, labels):
        med, spread = statistics.median(per[r]), max(per[r]) - min(per[r])
        res[r] = (med, spread)
        out.append('%-5s %-36s median %8.4f ms   spread %7.4f ms   (rounds: %s)' % (kind, lab, med, spread, ' '.join('%.4f' % x for x in per[r])))
    return res


def timing(a, tmp):
    import torch
    out = ['# tools/baseline_feed_time.py: training step of coFM / CKE / CFKG -- host-fed stepper from ready host id lists vs device-fed ten-step graphs',
           '# %s, d = %d, B = %d, Adam, %d rounds x %d steps per leg, alternating; wall time per step in ms; %d repeats from fresh models'
           % (torch.cuda.get_device_name(0), D, B, a.rounds, a.steps, a.repeats)]
    verdict = {}
    for rep in range(a.repeats):
        out.append('# repeat %d' % (rep + 1))
        for kind in KINDS:
            res = measure(kind, a.rounds, a.steps, tmp, out)
            gain, bar = res['host-fed'][0] - res['fed'][0], max(v[1] for v in res.values())
            ok = gain > bar
            verdict[kind] = verdict.get(kind, True) and ok
            out.append('%-5s (a) - (b) = %.4f ms, larger spread %.4f ms, (a) / (b) = %.2f: the fed steps are %s'
                       % (kind, gain, bar, res['host-fed'][0] / res['fed'][0], 'FASTER' if ok else 'NOT faster'))
    for kind in KINDS:
        out.append('# %s: (b) below (a) by more than the larger spread in every repeat: %s' % (kind, 'yes' if verdict[kind] else 'NO'))
    return out


def workload(tmp):
    """What the kernel trace runs: fed cycles of coFM (ktup_feed_align_lists) and CFKG (ktup_feed_remap_ids)."""
    for kind in ('cofm', 'cfkg'):
        leg = Leg(kind, 'fed', tmp)
        for _ in range(30):
            leg.ten()
        leg.finite()


def trace(out):
    d = tempfile.mkdtemp(prefix='bft_trace_', dir='/tmp')
    cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '--', sys.executable, os.path.abspath(__file__),
           '--workload']
    r = subprocess.run(cmd, cwd='/tmp', env=dict(os.environ, TMPDIR='/tmp'), capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit('rocprofv3 failed: ' + r.stdout[-2000:] + r.stderr[-2000:])
    hits = glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True)
    if not hits:
        raise SystemExit('no kernel_stats.csv under ' + d)
    out.append('# device time of the new launches: rocprofv3 --kernel-trace --stats over 300 fed steps each of coFM and CFKG (B = 400: 800 ids per rec '
               'step, 1,600 per kg step)')
    for row in csv.DictReader(open(hits[0])):
        if 'feed_' in row['Name']:
            out.append('%-72s calls %5s   avg %6.2f us   min %6.2f us   max %6.2f us'
                       % (row['Name'].replace('(anonymous namespace)::', '').replace('void ', '')[:72], row['Calls'], float(row['AverageNs']) / 1e3,
                          float(row['MinNs']) / 1e3, float(row['MaxNs']) / 1e3))
    shutil.rmtree(d, ignore_errors=True)


def cli_run(data, model, fed, steps, intervals=4):
    logs = os.path.join(data, 'log')
    os.makedirs(logs, exist_ok=True)
    name = '%s-%d' % (model, fed)
    cmd = [sys.executable, os.path.join(PKG, 'run_knowledgable_recommendation.py'), '-data_path', data, '-log_path', logs,
           '-dataset', 'ml1m', '-experiment_name', name, '-nohas_visualization', '-batch_size', str(B), '-embedding_size', str(D),
           '-seed', '3', '-eval_interval_steps', str(steps), '-training_steps', str((intervals + 1) * steps + 1),
           '-early_stopping_steps_to_wait', '0', '-learning_rate', '0.001', '-topn', '10', '-model_type', model, '-rec_test_files', 'valid.dat',
           '-kg_test_files', 'valid.dat', '-joint_ratio', '0.7', '-optimizer_type', 'Adam', '-log_level', 'info', '-device_sampling']
    env = dict(os.environ, KTUP_BASELINE_FEED='1' if fed else '0')
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1700, env=env)
    if r.returncode != 0:
        raise SystemExit(r.stdout[-2000:] + r.stderr[-3000:])
    text = open(os.path.join(logs, name + '.log')).read()
    assert ('device-resident' in text) == bool(fed), 'the switch did not select the route'
    stamps = [datetime.datetime.strptime(line[:23], '%Y-%m-%d %H:%M:%S,%f') for line in text.splitlines() if 'rec train loss' in line]
    assert len(stamps) >= intervals + 1, 'expected evaluations at steps 0, N, 2N, ...'
    spans = [(stamps[k + 1] - stamps[k]).total_seconds() for k in range(1, intervals)]
    return steps / spans[0], steps / min(spans), spans


def cli(out):
    from tests.synth import make_dataset
    out.append('# the command line, steps per second between two evaluations (one evaluation pass of the small validation files included), '
               '-device_sampling, B = %d, d = %d, Adam' % (B, D))
    with tempfile.TemporaryDirectory() as tmp:
        make_dataset(tmp, n_users=6040, n_items=3240, n_ent=14708, n_rel=20, n_ratings=120000, n_triples=60000, aligned=2934)
        for model in KINDS:
            for fed in (0, 1):
                steps = 3000 if fed else 300
                first, best, spans = cli_run(tmp, model, fed, steps)
                out.append('%-5s KTUP_BASELINE_FEED=%d: %8.0f steps/s (first interval), fastest of %d intervals %8.0f steps/s; %d steps per interval in %s s'
                           % (model, fed, first, len(spans), best, steps, ' '.join('%.3f' % s for s in spans)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--repeats', type=int, default=2)
    ap.add_argument('--workload', action='store_true', help='run the fed cycles the kernel trace wraps, nothing else')
    ap.add_argument('--skip-trace', action='store_true')
    ap.add_argument('--skip-cli', action='store_true')
    ap.add_argument('-o', '--output', default=os.path.join(ROOT, 'profiles', 'baseline_feed_times.txt'))
    a = ap.parse_args()
    with tempfile.TemporaryDirectory(prefix='baseline_feed_time_') as tmp:
        if a.workload:
            return workload(tmp)
        out = timing(a, tmp)
    if not a.skip_trace:
        trace(out)
    if not a.skip_cli:
        cli(out)
    text = '\n'.join(out) + '\n'
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.output)), exist_ok=True)
    open(a.output, 'w').write(text)


if __name__ == '__main__':
    main()
