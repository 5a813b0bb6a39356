"""TransR's link-prediction pass on one MI355X: the chunked score-matrix route (ops.eval_kg_ranks_transr(fused=False), chunk 512) against
the pass without the score matrix (fused=True), at tools/transd_pass_time.py's shape -- 20,480 keys x 14,709 entities, 20 relations,
d = 100 (`--d 128` for the other width), 1-3 gold entities and 20 filtered entities per key -- squared L2 and L1.  The entity side
(ops.eval_transr_entities) is prepared ONCE per distance, outside the timed region, and handed to both routes.

The two routes ALTERNATE round by round in one process; device-event timing; median and spread (max - min) of REPEATS rounds per route.
The decision rule of the defaults (ops.TRANSR_FUSED_DEFAULT): the pass is a distance's default only if its median gain over the chunked
route exceeds the larger of the two spreads, in BOTH runs of this tool.

`--cke` adds CKE's KG evaluation through the driver (_driver.kg_eval_pass, one direction, the same size, want_rows=False): the batch
walk over evaluateTail (40 batches of 512 keys, what CKE's evaluation was before it had rank_entities) against the whole pass through
CKE.rank_entities; wall clock with a device synchronisation, median of 5 alternating rounds, entity side prepared outside.

    python tools/transr_pass_time.py [--repeats 21] [--d 100] [--cke] [--out profiles/transr_pass_times.txt]     (--out appends)
"""
import argparse
import os
import statistics
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'joint-kg-recommender_amd'))
import torch


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record()
    b.synchronize()
    return a.elapsed_time(b)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def cke_lines(ne, nr, d, nq, rng):
    """CKE's KG evaluation of one direction: the batch walk against the whole pass, through the driver."""
    from jTransUP.models import CKE
    from jTransUP.models import _driver as D
    lines = []
    for l1 in (False, True):
        m = CKE.CKE(l1, d, 8, 8, ne - 1, nr, {i: i for i in range(8)}, {i: (i, i) for i in range(8)})
        m.eval(); m.disable_grad()
        keys = list(dict.fromkeys((int(e), int(r)) for e, r in zip(rng.randint(0, ne, 2 * nq), rng.randint(0, nr, 2 * nq))))[:nq]
        gold = {k: set(rng.randint(0, ne, rng.randint(1, 4)).tolist()) for k in keys}
        filt = {k: set(rng.randint(0, ne, 20).tolist()) for k in keys}
        batches = [keys[s:s + 512] for s in range(0, len(keys), 512)]
        FL = types.SimpleNamespace(topn=10)
        ents = m.prepare_entities()
        score_fn = lambda q, r: m.evaluateTail(q, r, ents=ents)
        rank_fn = lambda q, r, desc, go, gi, fo, fi: m.rank_entities(q, r, False, desc, go, gi, fo, fi, ents=ents)
        walk = lambda: D.kg_eval_pass(FL, score_fn, batches, gold, [filt], False, want_rows=False)
        whole = lambda: D.kg_eval_pass(FL, score_fn, batches, gold, [filt], False, want_rows=False, rank_fn=rank_fn)
        same = bool(np.array_equal(walk(), whole()))
        t = {'walk': [], 'pass': []}
        for _ in range(5):
            t['walk'].append(wall(walk)); t['pass'].append(wall(whole))
        med = {k: statistics.median(v) for k, v in t.items()}
        spread = {k: max(v) - min(v) for k, v in t.items()}
        from jTransUP.hip import ops
        lines.append('CKE kg_eval_pass %s  %d keys x %d entities d=%d, one direction, wall clock: batch walk %.2f ms [spread %.2f]   whole pass '
                     '(%s) %.2f ms [spread %.2f]   gain %.2f ms (x%.1f)   metric rows equal: %s   (median of 5 rounds)'
                     % ('L1' if l1 else 'L2', len(keys), ne, d, med['walk'], spread['walk'], ops.TRANSR_PASS_ROUTE[0], med['pass'], spread['pass'],
                        med['walk'] - med['pass'], med['walk'] / med['pass'], same))
        print(lines[-1], flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=21)
    ap.add_argument('--d', type=int, default=100)
    ap.add_argument('--cke', action='store_true')
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
    E, R = table(ne), table(nr)
    M = (torch.randn(nr, d * d, generator=gen) / d ** 0.5).to(dev)
    q = torch.from_numpy(rng.randint(0, ne, nq)).to(dev)
    r = torch.from_numpy(rng.randint(0, nr, nq)).to(dev)
    ng = rng.randint(1, 4, nq)
    g_off = torch.from_numpy(np.concatenate([[0], np.cumsum(ng)])).to(dev)
    g_ids = torch.from_numpy(rng.randint(0, ne, int(ng.sum())).astype(np.int32)).to(dev)
    f_off = torch.arange(0, 20 * nq + 1, 20, dtype=torch.int64, device=dev)
    f_ids = torch.from_numpy(rng.randint(0, ne, 20 * nq).astype(np.int32)).to(dev)
    lines = ['# python tools/transr_pass_time.py --repeats %d --d %d%s   (%s)' % (args.repeats, d, ' --cke' if args.cke else '', torch.cuda.get_device_name(0))]
    for l1 in (False, True):
        ents = ops.eval_transr_entities(E, M, nr, l1)                # outside the timed region, for both routes
        routes = [('chunked', lambda: ops.eval_kg_ranks_transr(E, R, M, q, r, l1, False, False, g_off, g_ids, f_off, f_ids, ents=ents, chunk=512, fused=False)),
                  ('fused', lambda: ops.eval_kg_ranks_transr(E, R, M, q, r, l1, False, False, g_off, g_ids, f_off, f_ids, ents=ents, fused=True))]
        same = torch.equal(routes[0][1](), routes[1][1]())
        assert same and ops.TRANSR_PASS_ROUTE[0].startswith('no score matrix')
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
                     '(x%.2f) %s the larger spread %.3f   ranks equal: %s   (median of %d rounds)'
                     % ('L1' if l1 else 'L2', nq, ne, d, med['chunked'], spread['chunked'], med['fused'], spread['fused'], gain,
                        med['chunked'] / med['fused'], 'exceeds' if gain > bar else 'DOES NOT exceed', bar, same, args.repeats))
        print(lines[-1], flush=True)
    if args.cke:
        lines += cke_lines(ne, nr, d, nq, rng)
    if args.out:
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
