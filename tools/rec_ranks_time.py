"""The rank of every gold item of a rec evaluation pass on one MI355X: the matrix walk -- 12 batches of 512 users, the score matrix
of a batch (ops.eval_bprmf, or ops.eval_transe on the buy relation for CFKG) + ops.gold_ranks -- against the one sweep without the
matrix (ops.eval_dot_ranks / ops.eval_cfkg_ranks: filter bits, gold-key launch and count sweep are all inside the timed region), at
ml1m size: 6040 users x 3240 items, about 17 golds and 165 filtered ids per user; BPRMF at d = 64, CFKG at d = 100 with L1 and with
squared L2.  As a yardstick the list pass for the same users (eval_dot_topk / eval_cfkg_topk, topn 10) is timed beside them.

Two worlds: `random` tables, where about half of a user's scores beat its worst gold -- the adverse case for the sweep's fast exit --
and `planted`, where a user's row is the mean of its gold item rows plus noise (CFKG: minus the relation row), so the golds rank near
the top as after training.

The routes ALTERNATE round by round in one process (Python's garbage collector held off inside the timed rounds), both warmed up;
device-event timing; median and spread (max - min) of the rounds per route.  One invocation is one run (--run numbers it; a collection
makes two and appends).  No default depends on these numbers: the pass is opt-in (KTUP_REC_RANKS=1).

    python tools/rec_ranks_time.py [--rounds 11] [--run 1] [-o profiles/rec_ranks_times.txt]      (-o appends)
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


def csr(rng, nq, n, mean, avoid=None):
    """Lists of about `mean` distinct ids per user (sorted), not in `avoid`'s list of the same user."""
    lists = []
    for b in range(nq):
        k = int(rng.randint(max(1, mean // 2), mean + mean // 2 + 1))
        ids = rng.choice(n, size=k, replace=False)
        if avoid is not None:
            ids = np.setdiff1d(ids, avoid[b])
        lists.append(np.sort(ids).astype(np.int32))
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    return off, np.concatenate(lists), lists


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=11)
    ap.add_argument('--run', type=int, default=1)
    ap.add_argument('-o', '--out', default='')
    args = ap.parse_args()
    from jTransUP.hip import ops
    dev = torch.device('cuda')
    nu, ni, chunk = 6040, 3240, 512
    lines = []
    if args.run == 1:
        lines = ['# python tools/rec_ranks_time.py --rounds %d --run N   (%s)' % (args.rounds, torch.cuda.get_device_name(0)),
                 '# %d users x %d items, ~17 golds and ~165 filtered ids per user; walk = the score matrix of %d users at a time + gold_ranks (12 '
                 'batches); sweep = eval_dot_ranks / eval_cfkg_ranks, filter bits and gold keys included; list = the top-10 list pass of the '
                 'same users (a yardstick, not a route to the ranks); ms per pass, median [spread = max - min] of %d alternating rounds'
                 % (nu, ni, chunk, args.rounds)]
        print('\n'.join(lines), flush=True)
    rng = np.random.RandomState(1)
    g_off_h, g_ids_h, golds = csr(rng, nu, ni, 17)
    f_off_h, f_ids_h, _ = csr(rng, nu, ni, 165, avoid=golds)
    g_off, g_ids, f_off, f_ids = (torch.from_numpy(x).to(dev) for x in (g_off_h, g_ids_h, f_off_h, f_ids_h))
    u = torch.arange(nu, device=dev)
    for model, d, l1 in (('BPRMF', 64, False), ('CFKG', 100, True), ('CFKG', 100, False)):
        for world in ('random', 'planted'):
            gen = torch.Generator().manual_seed(d + l1)
            I = torch.randn(ni, d, generator=gen) * 0.5
            R = torch.randn(4, d, generator=gen) * 0.5
            if world == 'random':
                U = torch.randn(nu, d, generator=gen) * 0.5
            else:
                U = torch.stack([I[torch.from_numpy(g.astype(np.int64))].mean(0) for g in golds]) + torch.randn(nu, d, generator=gen) * 0.05
                if model == 'CFKG':
                    U = U - R[3]
            U, I, R = U.to(dev), I.to(dev), R.to(dev)
            buy = torch.full((chunk,), 3, dtype=torch.int64, device=dev)

            def walk():
                out = []
                for lo in range(0, nu, chunk):
                    hi = min(nu, lo + chunk)
                    m = ops.eval_bprmf(U, I, u[lo:hi]) if model == 'BPRMF' else ops.eval_transe(U, R, u[lo:hi], buy[:hi - lo], l1, False, candidates=I)
                    g0, f0 = int(g_off_h[lo]), int(f_off_h[lo])
                    out.append(ops.gold_ranks(m, model == 'BPRMF', g_off[lo:hi + 1] - g0, g_ids[g0:], f_off[lo:hi + 1] - f0, f_ids[f0:])[:int(g_off_h[hi]) - g0])
                return torch.cat(out)

            def sweep():
                if model == 'BPRMF':
                    return ops.eval_dot_ranks(U, I, u, g_off, g_ids, f_off, f_ids)
                return ops.eval_cfkg_ranks(U, R, 3, I, u, l1, g_off, g_ids, filt_off=f_off, filt_ids=f_ids)

            def lists():
                if model == 'BPRMF':
                    return ops.eval_dot_topk(U, I, u, 10, f_off, f_ids)
                return ops.eval_cfkg_topk(U, R, 3, I, u, 10, l1, filt_off=f_off, filt_ids=f_ids)
            a, b = walk(), sweep()
            assert b is not None, 'the entry point declined'
            same = float((a == b).float().mean().item())                      # (CFKG: two fp32 evaluations, near ties may differ by one)
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
            lines.append('run %d  %s %s d=%d %s (mean rank %.1f): walk %.3f ms [spread %.3f]   sweep %.3f ms [spread %.3f]   gain %.3f ms (x%.2f) %s '
                         'the larger spread %.3f   list pass %.3f ms [spread %.3f]   equal ranks: %.2f %%'
                         % (args.run, model, 'L1' if l1 else ('L2' if model == 'CFKG' else 'dot'), d, world, mean_rank, med['walk'], spread['walk'],
                            med['sweep'], spread['sweep'], gain, med['walk'] / med['sweep'], 'exceeds' if gain > bar else 'DOES NOT exceed', bar,
                            med['list'], spread['list'], 100 * same))
            print(lines[-1], flush=True)
    if args.out:
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
