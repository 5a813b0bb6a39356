"""Times the TUP / KTUP rec evaluation pass at embedding size 256 (soft gate, squared L2) on its two routes, in ONE process per model:

    python tools/pref_q256_time.py [--rounds 5] [--passes 20] [--runs 2] [-o profiles/pref_q256_times.txt]

the pair kernel's sweep with the hybrid stage (sweep_soft_kernel; library option eval_q256 = 0 -- all there was at this width) and
the preference-space pass (eval_pass_q_kernel<QGeom<64, .>>; eval_q256 = 1), both through _driver.rec_eval_pass with the model's
evaluate_topk as pass_fn, each replayed as the graph the drivers replay (the graph key holds the option, so each route has its own).
Rounds alternate between the routes; a round's figure is the mean wall time of its passes (device idle before and after); reported
per run is the median over the rounds and their spread (max - min); Python's cyclic garbage collector runs between the rounds and
is held off inside them, for both routes alike (see measure).  Every case is measured in --runs separate runs, and the pass
counts as faster where its gain exceeds the larger spread in every run, at every cut-off and for both models: the rule by which
ops.PREF_Q256_DEFAULT is set (that of ops.PREF_WIDE_TOPN_DEFAULT).  topn 10, 20 and 50, 6040 users x 3240 items (ml1m size), about
165 filtered ids per user, P = 20.  One further leg: 512 users x 100,000 items through the wrappers, or 'declined' where the entry
point declines it.  Last, per shape of tests/test_hip_pref_q256.py, the largest |pass - matrix route| over the scores of the 64-key
lists in units of 2e-5 |s| + 2e-5 (the bound the pass is held to at d <= 128; the referee of that test allows 2).

Every leg is a child process under its own time limit; the first leg that fails or runs out of time ends the run."""
import argparse
import gc
import os
import statistics
import subprocess
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'joint-kg-recommender_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

TOPNS = (10, 20, 50)
NU, NI, NE, NP, D = 6040, 3240, 14709, 20, 256
LEGS = (('tup', 420), ('ktup', 420), ('big', 300), ('error', 300))       # (leg, its time limit in seconds)


def pref_world(ktup, seed=7):
    """-> one_pass(topn): the metric rows of a whole pass through _driver.rec_eval_pass, on the route the options select."""
    import numpy as np
    import torch
    from jTransUP.models import _driver as Dr
    torch.manual_seed(seed)
    rng = np.random.RandomState(seed)
    if ktup:
        from jTransUP.models import jTransUP as jt
        i_map = {i: i for i in range(NI)}
        new_map = {i: ((i * 4) % NE if i % 5 else -1, i) for i in range(NI)}
        m = jt.jTransUPModel(False, D, NU, NI, NE, NP, i_map, new_map, False, False)
        score = lambda u: m.evaluateRec(u)
    else:
        from jTransUP.models import transUP as tu
        m = tu.TransUPModel(False, D, NU, NI, NP, False)
        score = lambda u: m.evaluate(u)
    m.eval(); m.disable_grad()
    users = list(range(NU))
    gold = {u: set(rng.randint(0, NI, size=5).tolist()) for u in users}
    train = {u: set(rng.randint(0, NI, size=165).tolist()) for u in users}
    batches = [users[s:s + 512] for s in range(0, NU, 512)]
    pass_fn = lambda u, fo, fi, n: m.evaluate_topk(u, m.prepare_items(), n, fo, fi)

    def one_pass(topn):
        FL = types.SimpleNamespace(topn=topn)
        return Dr.rec_eval_pass(FL, score, batches, gold, [train], False, want_rows=False, pass_fn=pass_fn,
                                graph_key=Dr.model_graph_key(m), pass_descending=False)
    return one_pass


def measure(label, one_pass, topn, rounds, passes, runs, out):
    """-> whether the pass beats the sweep by more than the larger spread, in every run."""
    import numpy as np
    import torch
    from jTransUP.hip import lib as L

    def run(q):
        L.set_option('eval_q256', 1 if q else 0)
        return one_pass(topn)
    for _ in range(3):                                                    # eager, capture, first replay -- of either route
        ref = np.array(run(False), copy=True)
        got = np.array(run(True), copy=True)
    assert ref.shape == got.shape
    # scores up to fp32 rounding: one near-tie swap moves a mean by 1 / n
    assert float(np.abs(ref.mean(0) - got.mean(0)).max()) <= 2.0 / len(ref), 'the two routes disagree'
    faster = True
    for k in range(runs):
        per = {False: [], True: []}
        for _ in range(rounds):
            for q in (False, True):
                # Python's cyclic collector is held off inside a timed round (and run between rounds): a full collection walks the
                # ml1m-size gold / filter dicts for ~30 ms (jTransUP/hip/lib.py capture()), and because the allocation sequence of this
                # script is the same in every process it fell into the SAME round of two separate collections (KTUP, topn 20, run 2,
                # third round of the pass: 1.786 and 1.909 ms against 0.436 in the other four) -- a pause of the host, charged to
                # whichever route happened to be running
                gc.collect()
                gc.disable()
                try:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(passes):
                        run(q)
                    torch.cuda.synchronize()
                    per[q].append((time.perf_counter() - t0) / passes * 1e3)
                finally:
                    gc.enable()
        res = {}
        for q in (False, True):
            res[q] = (statistics.median(per[q]), max(per[q]) - min(per[q]))
            out.append('%-22s topn %2d run %d %-22s median %8.3f ms   spread %7.3f ms   (rounds: %s)'
                       % (label, topn, k + 1, 'preference-space pass' if q else 'soft sweep', res[q][0], res[q][1],
                          ' '.join('%.3f' % x for x in per[q])))
        gain, bar = res[False][0] - res[True][0], max(res[False][1], res[True][1])
        out.append('%-22s topn %2d run %d sweep - pass = %.3f ms, larger spread %.3f ms, ratio %.2f: the pass is %s'
                   % (label, topn, k + 1, gain, bar, res[False][0] / res[True][0], 'FASTER' if gain > bar else 'NOT faster'))
        faster &= gain > bar
    return faster


def leg_model(ktup, a, out):
    from jTransUP.hip import lib as L
    L.set_option('eval_wide_topn', 1)
    one_pass = pref_world(ktup)
    ok = True
    for topn in TOPNS:
        ok &= measure(('KTUP' if ktup else 'TUP ') + ' soft L2 d 256', one_pass, topn, a.rounds, a.passes, a.runs, out)
    out.append('VERDICT %s %s' % ('ktup' if ktup else 'tup', 'yes' if ok else 'NO'))


def leg_big(a, out):
    """512 users x 100,000 items, TUP, topn 10: the wrappers under either option, if the entry point takes the shape."""
    import torch
    from jTransUP.hip import lib as L
    from jTransUP.hip import ops as G
    T = __import__('tests.test_hip_pref_q256', fromlist=['World'])
    w = T.World(D, 512, 100000, 512, NP)
    label = 'TUP  512 x 100,000'
    try:
        T.c_entry(w, False, 10, False)
    except L.KtupError as e:
        if e.code != L.ERR_UNSUPPORTED:
            raise
        out.append('%-22s topn 10 declined by ktup_eval_pref_topk (the filter bits of a 12,512-item split do not fit the LDS beside two '
                   'tiles): the soft sweep stays.  %s' % (label, str(e)))
        return
    call = lambda: G.eval_pref_topk(w.U, w.u, w.items(False), False, 10, w.f_off, w.f_ids)
    for k in range(a.runs):
        per = {0: [], 1: []}
        for _ in range(a.rounds):
            for q in (0, 1):
                L.set_option('eval_q256', q)
                call()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.passes):
                    call()
                torch.cuda.synchronize()
                per[q].append((time.perf_counter() - t0) / a.passes * 1e3)
        for q in (0, 1):
            out.append('%-22s topn 10 run %d %-22s median %8.3f ms   spread %7.3f ms (eager wrapper calls)'
                       % (label, k + 1, 'preference-space pass' if q else 'soft sweep', statistics.median(per[q]), max(per[q]) - min(per[q])))


def leg_error(out):
    T = __import__('tests.test_hip_pref_q256', fromlist=['Q256_SHAPES'])
    for shape in T.Q256_SHAPES + [T.ORDER_SHAPE]:
        out.append('largest |pass - matrix route| / (2e-5 |s| + 2e-5), TUP and KTUP, 64-key lists, (d, users, items, nq, P) = %-24s %.4f'
                   % (shape, T.largest_error_ratio(shape)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--passes', type=int, default=20)
    ap.add_argument('--runs', type=int, default=2)
    ap.add_argument('--leg', default=None, choices=[n for n, _ in LEGS])
    ap.add_argument('-o', '--output', default=os.path.join(ROOT, 'profiles', 'pref_q256_times.txt'))
    a = ap.parse_args()
    assert a.rounds >= 5 and a.passes >= 20 and a.runs >= 2, 'at least two runs of five rounds of 20 passes'
    os.environ.setdefault('TQDM_DISABLE', '1')
    if a.leg:                                                             # a child: one leg, its lines on stdout
        out = []
        if a.leg in ('tup', 'ktup'):
            leg_model(a.leg == 'ktup', a, out)
        elif a.leg == 'big':
            leg_big(a, out)
        else:
            leg_error(out)
        import torch
        print('DEVICE ' + torch.cuda.get_device_name(0))
        sys.stdout.write('\n'.join(out) + '\n')
        return
    lines, verdict, device = [], {}, '?'
    for leg, limit in LEGS:
        cmd = [sys.executable, os.path.abspath(__file__), '--leg', leg, '--rounds', str(a.rounds), '--passes', str(a.passes), '--runs', str(a.runs)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            sys.exit('leg %s ran past its %d s: nothing further is started' % (leg, limit))
        if r.returncode != 0:
            sys.exit('leg %s failed (%d): nothing further is started\n%s' % (leg, r.returncode, (r.stdout + r.stderr)[-3000:]))
        for line in r.stdout.splitlines():
            if line.startswith('VERDICT '):
                verdict[line.split()[1]] = line.split()[2] == 'yes'
            elif line.startswith('DEVICE '):
                device = line[7:]
            elif line.strip():
                lines.append(line)
    head = ['# tools/pref_q256_time.py: soft sweep (eval_q256 = 0) vs preference-space pass (eval_q256 = 1) of TUP / KTUP at d = 256, P = 20, through',
            '# _driver.rec_eval_pass, graph replays; %s, %d runs x %d rounds x %d passes per route, alternating; wall time per pass in ms'
            % (device, a.runs, a.rounds, a.passes)]
    every = bool(verdict) and all(verdict.values())
    tail = ['# the pass is faster than the sweep by more than the larger spread for both models, at every cut-off and in every run: %s'
            % ('yes' if every else 'NO')]
    tail += ['# the rule fails on: ' + ' '.join(l.split()) for l in lines if 'NOT faster' in l]
    tail += ['# -> ops.PREF_Q256_DEFAULT = %s' % every]
    text = '\n'.join(head + lines + tail) + '\n'
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.output)), exist_ok=True)
    open(a.output, 'w').write(text)


if __name__ == '__main__':
    main()
