"""Link prediction as lists for TransR / CKE and TransD on one MI355X: the filtered top-n entities of every key through the score
matrix -- ops.eval_transr (entity side prepared once, outside the timed region) or ops.eval_transd on 512 keys at a time +
ops.topk_filtered, the only route before ktup_eval_kg_topk_rel and still the route beyond its list length -- against the one sweep
without the matrix (ops.eval_kg_topk_transr / ops.eval_kg_topk_transd; its timed region includes the buckets, the projection of the
entity table and the b.e table: they are part of every call), at the size the drivers evaluate: 20,480 keys x 14,709 entities, 20
relations, d in {100, 128}, both distances, topn in {10, 50}, filter lists of ml1m's density (20 entities per key, as
tools/kg_topn_time.py).

The two routes ALTERNATE round by round in one process (Python's garbage collector held off inside the timed rounds); device-event
timing; median and spread (max - min) of the rounds per route.  One invocation is one run (--run numbers it; the collection makes
two, each under its own time limit, and appends).  No default depends on these numbers: the sweeps are new calls, and the matrix
route is unchanged.  The rule of DESIGN.md 6o is applied for the reader: a gain counts only where it exceeds the larger of the two
spreads in both runs.

    python tools/kg_topn_rel_time.py [--rounds 11] [--run 1] [-o profiles/kg_topn_rel_times.txt]      (-o appends)
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
    ap.add_argument('--run', type=int, default=1)
    ap.add_argument('-o', '--out', default='')
    args = ap.parse_args()
    from jTransUP.hip import ops
    dev = torch.device('cuda')
    ne, nr, nq, chunk = 14709, 20, 20480, 512
    lines = []
    if args.run == 1:
        lines = ['# python tools/kg_topn_rel_time.py --rounds %d --run N   (%s)' % (args.rounds, torch.cuda.get_device_name(0)),
                 '# %d keys x %d entities, %d relations, 20 filtered entities per key; matrix = eval_transr (prepared entity side) / eval_transd on '
                 '%d keys at a time + topk_filtered; sweep = eval_kg_topk_transr / eval_kg_topk_transd, projection and tables included; ms per '
                 'pass, median [spread = max - min] of %d alternating rounds' % (nq, ne, nr, chunk, args.rounds)]
        print('\n'.join(lines), flush=True)
    for d in (100, 128):
        rng = np.random.RandomState(1)
        gen = torch.Generator().manual_seed(1)
        E, R, Ep, Rp = ((torch.randn(n, d, generator=gen) * 0.5).to(dev) for n in (ne, nr, ne, nr))
        M = (torch.randn(nr, d * d, generator=gen) * (0.5 / d ** 0.5)).to(dev)
        q = torch.from_numpy(rng.randint(0, ne, nq)).to(dev)
        r = torch.from_numpy(rng.randint(0, nr, nq)).to(dev)
        f_off = torch.arange(0, 20 * nq + 1, 20, dtype=torch.int64, device=dev)
        f_ids = torch.from_numpy(rng.randint(0, ne, 20 * nq).astype(np.int32)).to(dev)
        for model in ('TransR', 'TransD'):
            for l1 in (False, True):
                ents = ops.eval_transr_entities(E, M, nr, l1) if model == 'TransR' else None
                for topn in (10, 50):
                    def matrix():
                        out = []
                        for lo in range(0, nq, chunk):
                            hi = min(nq, lo + chunk)
                            m = ops.eval_transr(E, R, M, q[lo:hi], r[lo:hi], l1, False, ents=ents) if model == 'TransR' else \
                                ops.eval_transd(E, R, Ep, Rp, q[lo:hi], r[lo:hi], l1, False)
                            out.append(ops.topk_filtered(m, False, topn, f_off[lo:hi + 1], f_ids))
                        return torch.cat(out)

                    def sweep():
                        if model == 'TransR':
                            return ops.eval_kg_topk_transr(E, R, M, q, r, l1, False, topn, f_off, f_ids)
                        return ops.eval_kg_topk_transd(E, R, Ep, Rp, q, r, l1, False, topn, f_off, f_ids)
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
                                 % (args.run, model, 'L1' if l1 else 'L2', d, topn, med['matrix'], spread['matrix'], med['sweep'], spread['sweep'],
                                    gain, med['matrix'] / med['sweep'], 'exceeds' if gain > bar else 'DOES NOT exceed', bar, 100 * same))
                    print(lines[-1], flush=True)
    if args.out:
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
