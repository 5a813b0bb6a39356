"""TransD timings on one MI355X, one process:

  * the whole link-prediction pass at the shape of tools/kg_eval_pass.py (20,480 keys x 14,709 entities, 20 relations, d = 100,
    1-3 gold entities and 20 filtered entities per key), squared L2 and L1: ops.eval_kg_ranks_transd(fused=False) against TransH through the same
    kind of route, ops.eval_kg_ranks(..., fused=False) (score matrix per 512-key chunk + the rank kernel), on tables of the same shape;
  * the B = 512 KGStepper step for TransD against TransR's multi-launch step (same launch-count class), d = 100: both as eager
    launches, TransD also replayed from its captured graph (see step_figures for why TransR is not).

Event timing, warm-up first, median of REPEATS runs.  One line per figure; `--out FILE` also writes them there.

    python tools/transd_time.py [--repeats 21] [--out profiles/transd_times.txt]
"""
import argparse
import logging
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'joint-kg-recommender_amd'))
import torch


def median_ms(fn, repeats, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times), max(times)


def pass_figures(repeats, lines):
    from jTransUP.hip import ops
    dev = torch.device('cuda')
    rng = np.random.RandomState(1)
    gen = torch.Generator().manual_seed(1)
    ne, nr, d, nq = 14709, 20, 100, 20480

    def table(rows):
        w = torch.randn(rows, d, generator=gen)
        return (w / w.norm(dim=1, keepdim=True)).to(dev)
    E, R, Ep, Rp = table(ne), table(nr), table(ne), table(nr)       # Rp doubles as TransH's norm table: same shape
    q = torch.from_numpy(rng.randint(0, ne, nq)).to(dev)
    r = torch.from_numpy(rng.randint(0, nr, nq)).to(dev)
    ng = rng.randint(1, 4, nq)
    g_off = torch.from_numpy(np.concatenate([[0], np.cumsum(ng)])).to(dev)
    g_ids = torch.from_numpy(rng.randint(0, ne, int(ng.sum())).astype(np.int32)).to(dev)
    f_off = torch.arange(0, 20 * nq + 1, 20, dtype=torch.int64, device=dev)
    f_ids = torch.from_numpy(rng.randint(0, ne, 20 * nq).astype(np.int32)).to(dev)
    for l1 in (False, True):
        th = median_ms(lambda: ops.eval_kg_ranks(E, R, Rp, q, r, l1, False, False, g_off, g_ids, f_off, f_ids, chunk=512, fused=False), repeats)
        td = median_ms(lambda: ops.eval_kg_ranks_transd(E, R, Ep, Rp, q, r, l1, False, False, g_off, g_ids, f_off, f_ids, chunk=512, fused=False), repeats)
        kind = 'L1' if l1 else 'L2'
        lines.append('pass %s  %d keys x %d entities d=%d chunk 512: TransH (eval_kg_ranks fused=False) %.3f ms [min %.3f max %.3f]   '
                     'TransD (eval_kg_ranks_transd) %.3f ms [min %.3f max %.3f]   ratio TransD / TransH %.3f   (median of %d)'
                     % (kind, nq, ne, d, th[0], th[1], th[2], td[0], td[1], td[2], td[0] / th[0], repeats))
        print(lines[-1], flush=True)


def step_figures(repeats, lines, tmp):
    """TransR's step is timed as eager launches only: its relation-bucketed forward clears its counters with hipMemsetAsync, and a
    memset node captured into a graph is replayed wrongly by the HIP runtime torch bundles, so that step must
    not be replayed from a graph at this shape.  TransD's step records no memset: eager and graph replay."""
    from jTransUP.models import transD, transR
    from jTransUP.models.base import get_flags
    from jTransUP.utils.fast_train import KGStepper
    from jTransUP.utils.flags import FLAGS
    from jTransUP.utils.trainer import ModelTrainer
    dev = torch.device('cuda')
    ne, nr, d, B = 14709, 20, 100, 512
    out = {}
    for name, cls, graphs in (('transr', transR.TransRModel, False), ('transd', transD.TransDModel, False), ('transd', transD.TransDModel, True)):
        get_flags(); FLAGS.reset()
        FLAGS(['prog', '-model_type', name, '-log_path', tmp, '-experiment_name', 'time-' + name, '-optimizer_type', 'Adagrad'])
        FLAGS.ckpt_path = tmp
        torch.manual_seed(2)
        m = cls(False, d, ne, nr)
        if name == 'transd':
            with torch.no_grad():
                m.ent_proj_embeddings.weight.normal_(0, 0.1); m.rel_proj_embeddings.weight.normal_(0, 0.1)
        tr = ModelTrainer(m, logging.getLogger('time'), 100, FLAGS)
        st = KGStepper(m, tr, FLAGS, B, use_graphs=graphs)
        gen = torch.Generator().manual_seed(3)
        ids = [torch.randint(0, hi, (B,), generator=gen).to(dev) for hi in (ne, ne, nr, ne, ne)]
        step = lambda: st.kg_step(ids[0], ids[1], ids[2], ids[3], ids[4], ids[2])
        for _ in range(5):                                      # past the eager steps: with graphs the rest replay the captured one
            step()
        torch.cuda.synchronize()
        assert bool(st._graphs) == graphs

        def ten():
            for _ in range(10):
                step()
        t = median_ms(ten, repeats)
        out[(name, graphs)] = t[0] / 10
        lines.append('step B=%d d=%d %s KGStepper (multi-launch, %s): %.1f us per step [min %.1f max %.1f]   (median of %d x 10 steps)'
                     % (B, d, name, 'graph replay' if graphs else 'eager launches', 1e3 * t[0] / 10, 1e3 * t[1] / 10, 1e3 * t[2] / 10, repeats))
        print(lines[-1], flush=True)
    lines.append('step ratio TransD / TransR, eager launches %.3f' % (out[('transd', False)] / out[('transr', False)]))
    print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=21)
    ap.add_argument('--out', default='')
    ap.add_argument('--only', default='', choices=['', 'pass', 'step'])
    args = ap.parse_args()
    assert args.repeats >= 20, 'median of at least 20 repeats'
    import tempfile
    lines = ['# python tools/transd_time.py --repeats %d%s   (%s)' % (args.repeats, ' --only ' + args.only if args.only else '',
                                                                  torch.cuda.get_device_name(0))]
    if args.only in ('', 'pass'):
        pass_figures(args.repeats, lines)
    if args.only in ('', 'step'):
        with tempfile.TemporaryDirectory() as tmp:
            step_figures(args.repeats, lines, tmp)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
