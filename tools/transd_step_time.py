"""Times the TransD training step of the KG driver through its routes, at ml1m-size tables (14,709 entities, 20 relations), d = 100,
B = 512, Adagrad, squared L2:

    python tools/transd_step_time.py [--rounds 21] [--steps 10] [--legs all|old] [-o profiles/transd_step_times.txt]

  (a)   the multi-launch route issued eagerly (KTUP_FUSED_STEP=0: a clearing of the loss, forward, margin loss, backward, two
        regularisers, clip + optimizer with its own norm pass)
  (a')  the multi-launch route replayed from its captured graph
  (b)   the one launch (ktup_train_transd_step) + the optimizer launch, issued eagerly
  (c)   the one launch replayed from its captured graph
  (d)   device-fed: ten steps (feed launch, step launch, optimizer launch each) as ONE replay of a ten-step cycle (fed_cycle)
  (e)   host-fed on -device_sampling's path as it was before the one launch: DeviceFeeder.next_cols, DeviceSampler.sample_kg, the id
        packing and a replay of the multi-launch step's graph per step -- WALL time per step (the host work is what it measures)

`--legs old` runs (a), (a') and (e) only: they need nothing of the one-launch step, so the same file times a build of the parent
commit (copy it there); alternate such runs with this tree's.  The routes alternate inside one process, round by round; a round's
figure is the time per step between two events (leg (e): two host clock readings around a synchronised stretch) around `--steps`
steps; reported is the median over the rounds and their spread (max - min).  A route counts as FASTER than the parent's figure if
it is below it by more than the larger of the two spreads.  Run it twice, each call under its own time limit."""
import argparse
import logging
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'joint-kg-recommender_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)
import torch

NE, NR, D, B, N_TRIPLES = 14709, 20, 100, 512, 400000


def _flags(tmp):
    from jTransUP.models.base import get_flags
    from jTransUP.utils.flags import FLAGS
    get_flags(); FLAGS.reset()
    FLAGS(['prog', '-model_type', 'transd', '-log_path', tmp, '-experiment_name', 'time-transd', '-optimizer_type', 'Adagrad',
           '-batch_size', str(B), '-embedding_size', str(D)])
    FLAGS.ckpt_path = tmp
    return FLAGS


def _stepper(tmp, fused, graphs):
    """A KGStepper on a fresh TransD model whose projection tables are non-zero (KTUP_FUSED_STEP is read when it is made)."""
    from jTransUP.models import transD
    from jTransUP.utils.fast_train import KGStepper
    from jTransUP.utils.trainer import ModelTrainer
    FLAGS = _flags(tmp)
    torch.manual_seed(2)
    m = transD.TransDModel(False, D, NE, NR)
    with torch.no_grad():
        m.ent_proj_embeddings.weight.copy_(torch.randn(NE, D) * 0.1)
        m.rel_proj_embeddings.weight.copy_(torch.randn(NR, D) * 0.1)
    log = logging.getLogger('transd_step_time')
    log.setLevel(logging.WARNING)
    tr = ModelTrainer(m, log, 1000, FLAGS)
    old = os.environ.get('KTUP_FUSED_STEP')
    os.environ['KTUP_FUSED_STEP'] = '1' if fused else '0'
    try:
        st = KGStepper(m, tr, FLAGS, B, use_graphs=graphs)
    finally:
        if old is None:
            del os.environ['KTUP_FUSED_STEP']
        else:
            os.environ['KTUP_FUSED_STEP'] = old
    assert bool(getattr(st, 'transd_step', False)) == fused
    return st


def _feeds(seed):
    from jTransUP.utils.device_sampler import DeviceSampler
    from jTransUP.utils.fast_train import DeviceFeeder
    dev = torch.device('cuda')
    gen = torch.Generator().manual_seed(seed)
    rows = torch.stack([torch.randint(0, NE, (N_TRIPLES,), generator=gen), torch.randint(0, NE, (N_TRIPLES,), generator=gen),
                        torch.randint(0, NR, (N_TRIPLES,), generator=gen)], dim=1)
    sampler = DeviceSampler(dev, seed=5)
    sampler.set_triples(NE, NR, None)
    return sampler, DeviceFeeder(rows, B, dev, seed=4)


def legs_of(tmp, which):
    """[(label, run(steps), wall)]: `run` issues `steps` steps (a multiple of ten for the cycle)."""
    dev = torch.device('cuda')
    legs = []
    plain = [("(a)  multi-launch route, eager", False, False), ("(a') multi-launch route, graph replay", False, True)]
    if which == 'all':
        plain += [('(b)  one launch, issued eagerly', True, False), ('(c)  one launch, graph replay', True, True)]
    for label, fused, graphs in plain:
        st = _stepper(tmp, fused, graphs)
        gen = torch.Generator().manual_seed(3)
        pool = [[torch.randint(0, hi, (B,), generator=gen).to(dev) for hi in (NE, NE, NR, NE, NE)] for _ in range(10)]

        def run(steps, st=st, pool=pool):
            for s in range(steps):
                i = pool[s % len(pool)]
                last = st.kg_step(i[0], i[1], i[2], i[3], i[4], i[2])
            return last
        last = run(10)                                                  # eager steps, the capture, first replays
        assert float(last) == float(last), 'loss is not finite'
        torch.cuda.synchronize()
        assert bool(st._graphs) == graphs
        legs.append((label, run, False))
    if which == 'all':
        st = _stepper(tmp, True, True)
        sampler, feed = _feeds(7)
        st.attach_feeds(sampler, kg=feed)
        assert st.can_feed('kg')

        def run_fed(steps, st=st):
            done = 0
            while done < steps:
                n = st.fed_cycle(('kg',) * 10) if steps - done >= 10 else 0
                if not n:                                               # warm-up, or an epoch that ends inside the cycle
                    st.fed_step('kg')
                    n = 1
                done += n
        run_fed(30)
        torch.cuda.synchronize()
        sampler.check()
        assert any(k.startswith('cycle:') for k in st._graphs)
        legs.append(('(d)  device-fed, ten-step cycle', run_fed, False))
    st = _stepper(tmp, False, True)
    sampler, feed = _feeds(7)

    def run_host(steps, st=st, sampler=sampler, feed=feed):
        for _ in range(steps):
            ph, pt, pr = feed.next_cols()
            nh, nt = sampler.sample_kg(ph, pt, pr)
            st.kg_step(ph, pt, pr, nh, nt, pr)
    run_host(10)
    torch.cuda.synchronize()
    sampler.check()
    assert 'kg' in st._graphs
    legs.append(('(e)  host-fed multi-launch replay, WALL', run_host, True))
    return legs


def measure(legs, rounds, steps, out):
    per = {label: [] for label, _, _ in legs}
    for _ in range(rounds):
        for label, run, wall in legs:                                   # the routes alternate, round by round
            torch.cuda.synchronize()
            if wall:
                t0 = time.perf_counter()
                run(steps)
                torch.cuda.synchronize()
                per[label].append((time.perf_counter() - t0) / steps * 1e6)
            else:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                run(steps)
                b.record()
                b.synchronize()
                per[label].append(a.elapsed_time(b) / steps * 1e3)
    for label, _, _ in legs:
        med, spread = statistics.median(per[label]), max(per[label]) - min(per[label])
        out.append('kg   %-40s median %8.1f us per step   spread %7.1f us   [min %.1f max %.1f]   (%d rounds x %d steps)'
                   % (label, med, spread, min(per[label]), max(per[label]), rounds, steps))
        print(out[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=21)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--legs', default='all', choices=['all', 'old'])
    ap.add_argument('--tag', default='', help='a word for the header line, e.g. "parent" or "this tree"')
    ap.add_argument('-o', '--out', default='')
    a = ap.parse_args()
    assert a.rounds >= 20, 'median of at least 20 rounds'
    assert a.steps % 10 == 0, 'whole ten-step cycles'
    out = ['# python tools/transd_step_time.py --rounds %d --steps %d --legs %s%s   (%s)'
           % (a.rounds, a.steps, a.legs, '   [%s]' % a.tag if a.tag else '', torch.cuda.get_device_name(0))]
    with tempfile.TemporaryDirectory() as tmp:
        measure(legs_of(tmp, a.legs), a.rounds, a.steps, out)
    if a.out:
        with open(a.out, 'a') as f:
            f.write('\n'.join(out) + '\n')


if __name__ == '__main__':
    main()
