"""The rank of every gold item of a TUP / KTUP evaluation pass (soft gate, squared L2) on one MI355X: the matrix walk -- 12 batches of
512 users, the score matrix of a batch (ops.eval_tup / ops.eval_ktup on a shared item side) + ops.gold_ranks -- against the one sweep
without the matrix (ops.eval_pref_ranks: the operand tables, the filter bits, the gold-key launch and the count sweep are all inside
the timed region), at ml1m size: 6040 users x 3240 items, d = 100, 20 preferences, about 17 golds and 165 filtered ids per user.  As
a yardstick the list pass for the same users (ops.eval_pref_topk, topn 10) is timed beside them.

Two worlds: `random` tables, where about half of a user's scores lie below its worst gold -- the adverse case for the sweep's fast
exit --, and `planted`, where a user's row is the mean of its gold item rows plus noise, so the golds rank nearer the top as after
training.

The routes ALTERNATE round by round in one process (Python's garbage collector held off inside the timed rounds), all warmed up;
device-event timing; median and spread (max - min) of the rounds per route.  One invocation is one run (--run numbers it; a collection
makes two and appends).  No default depends on these numbers: the pass is opt-in (KTUP_REC_RANKS=1).

    python tools/pref_ranks_time.py [--rounds 11] [--run 1] [-o profiles/pref_ranks_times.txt]      (-o appends)
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

from tools.rec_ranks_time import csr, timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=11)
    ap.add_argument('--run', type=int, default=1)
    ap.add_argument('-o', '--out', default='')
    args = ap.parse_args()
    from jTransUP.hip import ops
    dev = torch.device('cuda')
    nu, ni, ne, chunk, d, P = 6040, 3240, 3000, 512, 100, 20
    lines = []
    if args.run == 1:
        lines = ['# python tools/pref_ranks_time.py --rounds %d --run N   (%s)' % (args.rounds, torch.cuda.get_device_name(0)),
                 '# %d users x %d items, d = %d, %d preferences, ~17 golds and ~165 filtered ids per user; walk = the score matrix of %d users at a '
                 'time + gold_ranks (12 batches, the item side prepared once outside the timed region); sweep = eval_pref_ranks, operand tables, '
                 'filter bits and gold keys included; list = the top-10 list pass of the same users (a yardstick, not a route to the ranks); ms '
                 'per pass, median [spread = max - min] of %d alternating rounds' % (nu, ni, d, P, chunk, args.rounds)]
        print('\n'.join(lines), flush=True)
    rng = np.random.RandomState(1)
    g_off_h, g_ids_h, golds = csr(rng, nu, ni, 17)
    f_off_h, f_ids_h, _ = csr(rng, nu, ni, 165, avoid=golds)
    g_off, g_ids, f_off, f_ids = (torch.from_numpy(x).to(dev) for x in (g_off_h, g_ids_h, f_off_h, f_ids_h))
    u = torch.arange(nu, device=dev)
    for model in ('TUP', 'KTUP'):
        ktup = model == 'KTUP'
        for world in ('random', 'planted'):
            gen = torch.Generator().manual_seed(d + ktup)
            mk = lambda rows, scale: torch.randn(rows, d, generator=gen) * scale
            I, Pm, Pn, R, Rn = mk(ni, 0.5), mk(P, 0.3), mk(P, 0.3), mk(P, 0.3), mk(P, 0.3)
            E = torch.cat([mk(ne, 0.3), torch.zeros(1, d)])
            i2e = torch.randint(0, ne + 1, (ni,), generator=gen).to(torch.int32)
            if world == 'random':
                U = mk(nu, 0.5)
            else:
                rows = I + E[i2e.long()] if ktup else I
                U = torch.stack([rows[torch.from_numpy(g.astype(np.int64))].mean(0) for g in golds]) + mk(nu, 0.05)
            U, I, E, Pm, Pn, R, Rn, i2e = (t.to(dev) for t in (U, I, E, Pm, Pn, R, Rn, i2e))
            items = ops.eval_pref_items(I, E if ktup else None, Pm, Pn, R if ktup else None, Rn if ktup else None, i2e if ktup else None)
            _ = items.items_ws                                                # (the walk's per-item projections: once per pass, not timed)

            def walk():
                out = []
                for lo in range(0, nu, chunk):
                    hi = min(nu, lo + chunk)
                    if ktup:
                        m = ops.eval_ktup(U, I, E, Pm, Pn, R, Rn, i2e, u[lo:hi], False, ops.GUMBEL_OFF, None, 0, 0, items=items)
                    else:
                        m = ops.eval_tup(U, I, Pm, Pn, u[lo:hi], False, ops.GUMBEL_OFF, None, 0, 0, items=items)
                    g0, f0 = int(g_off_h[lo]), int(f_off_h[lo])
                    out.append(ops.gold_ranks(m, False, g_off[lo:hi + 1] - g0, g_ids[g0:], f_off[lo:hi + 1] - f0, f_ids[f0:])[:int(g_off_h[hi]) - g0])
                return torch.cat(out)

            def sweep():
                return ops.eval_pref_ranks(U, u, items, False, g_off, g_ids, f_off, f_ids)

            def lists():
                return ops.eval_pref_topk(U, u, items, False, 10, f_off, f_ids)
            a, b = walk(), sweep()
            assert b is not None, 'the entry point declined'
            same = float((a == b).float().mean().item())                      # (two fp32 evaluations: near ties may differ by one)
            off_by = int((a - b).abs().max().item())
            mean_rank = float(b[b >= 0].float().mean().item())
            for _ in range(2):
                walk(); sweep(); lists()
            torch.cuda.synchronize()
            t = {'walk': [], 'sweep': [], 'list': []}
            gc.collect(); gc.disable()
            try:
                for _ in range(args.rounds):                                  # the routes alternate round by round
                    t['walk'].append(timed(walk))
                    t['sweep'].append(timed(sweep))
                    t['list'].append(timed(lists))
            finally:
                gc.enable()
            med = {k: statistics.median(v) for k, v in t.items()}
            spread = {k: max(v) - min(v) for k, v in t.items()}
            gain, bar = med['walk'] - med['sweep'], max(spread['walk'], spread['sweep'])
            lines.append('run %d  %s d=%d P=%d %s (mean rank %.1f): walk %.3f ms [spread %.3f]   sweep %.3f ms [spread %.3f]   gain %.3f ms (x%.2f) %s '
                         'the larger spread %.3f   list pass %.3f ms [spread %.3f]   equal ranks: %.2f %% (largest difference %d)'
                         % (args.run, model, d, P, world, mean_rank, med['walk'], spread['walk'], med['sweep'], spread['sweep'], gain,
                            med['walk'] / med['sweep'], 'exceeds' if gain > bar else 'DOES NOT exceed', bar, med['list'], spread['list'], 100 * same,
                            off_by))
            print(lines[-1], flush=True)
    if args.out:
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
