"""Link prediction as lists on one MI355X: the filtered top-n entities of every key through the score matrix -- ops.eval_transe /
ops.eval_transh on 512 keys at a time + ops.topk_filtered, the only route before ktup_eval_kg_topk and still the route beyond its list
length -- against the one sweep without the matrix (ops.eval_kg_topk), at the size the drivers evaluate: 20,480 keys x 14,709
entities, 20 relations, d in {100, 128}, TransE and TransH, both distances, topn in {10, 50}, filter lists of ml1m's density (20
entities per key, as tools/transd_pass_time.py).

The two routes ALTERNATE round by round in one process (Python's garbage collector held off inside the timed rounds); device-event
timing; median and spread (max - min) of the rounds per route; the whole measurement RUNS times.  No default depends on these
numbers: ops.eval_kg_topk is a new call, and the matrix route is unchanged.  The rule of DESIGN.md 6o is applied for the reader: a
gain counts only where it exceeds the larger of the two spreads in both runs.

    python tools/kg_topn_time.py [--rounds 11] [--runs 2] [-o profiles/kg_topn_times.txt]
"""
import argparse
import gc
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'joint-kg-recommender_amd'))
import torch


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=11)
    ap.add_argument('--runs', type=int, default=2)
    ap.add_argument('-o', '--out', default='')
    args = ap.parse_args()
    from jTransUP.hip import ops
    dev = torch.device('cuda')
    ne, nr, nq, chunk = 14709, 20, 20480, 512
    lines = ['# python tools/kg_topn_time.py --rounds %d --runs %d   (%s)' % (args.rounds, args.runs, torch.cuda.get_device_name(0)),
             '# %d keys x %d entities, %d relations, 20 filtered entities per key; matrix = eval_trans{e,h} on %d keys at a time + topk_filtered; '
             'sweep = eval_kg_topk; ms per pass, median [spread = max - min] of %d alternating rounds' % (nq, ne, nr, chunk, args.rounds)]
    print('\n'.join(lines), flush=True)
    for run in range(args.runs):
        for d in (100, 128):
            rng = np.random.RandomState(1)
            gen = torch.Generator().manual_seed(1)
            E, R = (torch.randn(ne, d, generator=gen) * 0.5).to(dev), (torch.randn(nr, d, generator=gen) * 0.5).to(dev)
            W = torch.nn.functional.normalize(torch.randn(nr, d, generator=gen), dim=1).to(dev)
            q = torch.from_numpy(rng.randint(0, ne, nq)).to(dev)
            r = torch.from_numpy(rng.randint(0, nr, nq)).to(dev)
            f_off = torch.arange(0, 20 * nq + 1, 20, dtype=torch.int64, device=dev)
            f_ids = torch.from_numpy(rng.randint(0, ne, 20 * nq).astype(np.int32)).to(dev)
            for model, N in (('TransE', None), ('TransH', W)):
                for l1 in (False, True):
                    for topn in (10, 50):
                        def matrix():
                            out = []
                            for lo in range(0, nq, chunk):
                                hi = min(nq, lo + chunk)
                                m = ops.eval_transe(E, R, q[lo:hi], r[lo:hi], l1, False) if N is None else \
                                    ops.eval_transh(E, R, N, q[lo:hi], r[lo:hi], l1, False)
                                out.append(ops.topk_filtered(m, False, topn, f_off[lo:hi + 1], f_ids))
                            return torch.cat(out)

                        def sweep():
                            return ops.eval_kg_topk(E, R, N, q, r, l1, False, topn, f_off, f_ids)
                        a, b = matrix(), sweep()
                        assert b is not None, 'the entry point declined'
                        same = float((a == b).all(1).float().mean().item())       # (two fp32 evaluations: near ties may swap)
                        for _ in range(2):
                            matrix(); sweep()
                        torch.cuda.synchronize()
                        t = {'matrix': [], 'sweep': []}
                        gc.collect(); gc.disable()
                        try:
                            for _ in range(args.rounds):                          # the routes alternate round by round
                                t['matrix'].append(timed(matrix))
                                t['sweep'].append(timed(sweep))
                        finally:
                            gc.enable()
                        med = {k: statistics.median(v) for k, v in t.items()}
                        spread = {k: max(v) - min(v) for k, v in t.items()}
                        gain, bar = med['matrix'] - med['sweep'], max(spread.values())
                        lines.append('run %d  %s %s d=%d topn=%d: matrix %.3f ms [spread %.3f]   sweep %.3f ms [spread %.3f]   gain %.3f ms (x%.2f) %s '
                                     'the larger spread %.3f   keys with identical lists: %.2f %%'
                                     % (run + 1, model, 'L1' if l1 else 'L2', d, topn, med['matrix'], spread['matrix'], med['sweep'], spread['sweep'],
                                        gain, med['matrix'] / med['sweep'], 'exceeds' if gain > bar else 'DOES NOT exceed', bar, 100 * same))
                        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
