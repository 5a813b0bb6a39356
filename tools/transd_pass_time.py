"""TransD's link-prediction pass on one MI355X: the chunked score-matrix route (ops.eval_kg_ranks_transd(fused=False), chunk 512) against
the pass without the score matrix (fused=True), at tools/transd_time.py's shape -- 20,480 keys x 14,709 entities, 20 relations, d = 100,
1-3 gold entities and 20 filtered entities per key -- squared L2 and L1 (`--d 128` for the width whose sweep keeps one stage buffer).

The two routes ALTERNATE round by round in one process; device-event timing; median and spread (max - min) of REPEATS rounds per route.
TransH's pass without the score matrix (ops.eval_kg_ranks, fused) on tables of the same shape is timed in the same rounds for
orientation only.  The decision rule of the defaults (ops.TRANSD_FUSED_DEFAULT): the pass is a distance's default only if its median
gain over the chunked route exceeds the larger of the two spreads, in BOTH runs of this tool.

    python tools/transd_pass_time.py [--repeats 21] [--d 100] [--out profiles/transd_pass_times.txt]     (--out appends)
"""
import argparse
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
    ap.add_argument('--repeats', type=int, default=21)
    ap.add_argument('--d', type=int, default=100)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    assert args.repeats >= 21, 'median of at least 21 rounds'
    from jTransUP.hip import ops
    dev = torch.device('cuda')
    rng = np.random.RandomState(1)
    gen = torch.Generator().manual_seed(1)
    ne, nr, d, nq = 14709, 20, args.d, 20480

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
    lines = ['# python tools/transd_pass_time.py --repeats %d --d %d   (%s)' % (args.repeats, d, torch.cuda.get_device_name(0))]
    for l1 in (False, True):
        routes = [('chunked', lambda: ops.eval_kg_ranks_transd(E, R, Ep, Rp, q, r, l1, False, False, g_off, g_ids, f_off, f_ids, chunk=512, fused=False)),
                  ('fused', lambda: ops.eval_kg_ranks_transd(E, R, Ep, Rp, q, r, l1, False, False, g_off, g_ids, f_off, f_ids, fused=True)),
                  ('transh_fused', lambda: ops.eval_kg_ranks(E, R, Rp, q, r, l1, False, False, g_off, g_ids, f_off, f_ids))]
        same = torch.equal(routes[0][1](), routes[1][1]())
        assert same and ops.TRANSD_PASS_ROUTE[0].startswith('no score matrix')
        for _ in range(3):
            for _, fn in routes:
                fn()
        torch.cuda.synchronize()
        t = {name: [] for name, _ in routes}
        for _ in range(args.repeats):                                # the routes alternate round by round
            for name, fn in routes:
                t[name].append(timed(fn))
        med = {k: statistics.median(v) for k, v in t.items()}
        spread = {k: max(v) - min(v) for k, v in t.items()}
        gain, bar = med['chunked'] - med['fused'], max(spread['chunked'], spread['fused'])
        lines.append('pass %s  %d keys x %d entities d=%d: chunked (chunk 512) %.3f ms [spread %.3f]   fused %.3f ms [spread %.3f]   gain %.3f ms '
                     '(x%.2f) %s the larger spread %.3f   ranks equal: %s   | TransH fused, same shape: %.3f ms [spread %.3f]   (median of %d rounds)'
                     % ('L1' if l1 else 'L2', nq, ne, d, med['chunked'], spread['chunked'], med['fused'], spread['fused'], gain,
                        med['chunked'] / med['fused'], 'exceeds' if gain > bar else 'DOES NOT exceed', bar, same, med['transh_fused'],
                        spread['transh_fused'], args.repeats))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
