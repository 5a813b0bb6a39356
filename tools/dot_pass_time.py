"""Times the two evaluation routes of the inner-product recommenders against each other, in ONE process:

    python tools/dot_pass_time.py [--rounds 5] [--passes 20] [--no-profile] [-o profiles/dot_pass_times.txt]

the batch walk (K11 + bias adds + ranking kernel + metrics per 512 users; KTUP_EVAL_PASS=0) and the one-sweep pass
(ktup_eval_dot_topk; replayed as a graph, as the drivers run it) through _driver.rec_eval_pass, which reads KTUP_EVAL_PASS per
call.  Rounds alternate between the routes; a round's figure is the mean wall time of its passes (device idle before and after),
reported is the median over the rounds and their spread (max - min).
  (a) BPRMF and FM, 6040 users x 3240 items, d = 64, about 165 filtered ids per user (ml1m size)
  (b) BPRMF, 512 users x 100,000 items, d = 64 (one batch; the matrix route writes and re-reads a 205 MB score matrix)
Unless --no-profile, a child process then runs a few passes of (a) under `rocprofv3 --kernel-trace --stats` and the sweep
kernel's own time and register counts are added to the report."""
import argparse
import csv
import glob
import os
import statistics
import subprocess
import sys
import tempfile
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'joint-kg-recommender_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)


def world(kind, nu, ni, d, n_filt, seed=7):
    import numpy as np
    import torch
    from jTransUP.models import bprmf, fm
    torch.manual_seed(seed)
    rng = np.random.RandomState(seed)
    m = (bprmf.BPRMF if kind == 'bprmf' else fm.FM)(d, nu, ni)
    with torch.no_grad():
        for p in m.parameters():
            p.add_(torch.randn_like(p) * 0.1)
    m.eval(); m.disable_grad()
    users = list(range(nu))
    gold = {u: set(rng.randint(0, ni, size=5).tolist()) for u in users}
    train = {u: set(rng.randint(0, ni, size=n_filt).tolist()) for u in users}
    batches = [users[s:s + 512] for s in range(0, nu, 512)]
    return m, gold, train, batches


def one_pass(m, gold, train, batches, fused):
    from jTransUP.models import _driver as D
    FL = types.SimpleNamespace(topn=10)
    os.environ['KTUP_EVAL_PASS'] = '1' if fused else '0'
    pass_fn = lambda u, fo, fi, n: m.evaluate_topk(u, None, n, fo, fi)
    return D.rec_eval_pass(FL, m.evaluate, batches, gold, [train], True, want_rows=False, pass_fn=pass_fn,
                           graph_key=D.model_graph_key(m), pass_descending=True)


def measure(label, m, gold, train, batches, rounds, passes, out):
    import numpy as np
    import torch
    ref = one_pass(m, gold, train, batches, False)
    for _ in range(3):                                                    # eager, capture, first replay
        got = one_pass(m, gold, train, batches, True)
    assert np.array_equal(ref, got), 'the two routes disagree'
    per = {False: [], True: []}
    for _ in range(rounds):
        for fused in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(passes):
                one_pass(m, gold, train, batches, fused)
            torch.cuda.synchronize()
            per[fused].append((time.perf_counter() - t0) / passes * 1e3)
    res = {}
    for fused in (False, True):
        med, spread = statistics.median(per[fused]), max(per[fused]) - min(per[fused])
        res[fused] = (med, spread)
        out.append('%-34s %-22s median %8.3f ms   spread %7.3f ms   (rounds: %s)'
                   % (label, 'one-sweep pass' if fused else 'batch walk', med, spread, ' '.join('%.3f' % x for x in per[fused])))
    gain, bar = res[False][0] - res[True][0], max(res[False][1], res[True][1])
    out.append('%-34s walk - pass = %.3f ms, larger spread %.3f ms: the pass is %s' % (label, gain, bar, 'FASTER' if gain > bar else 'NOT faster'))
    return gain > bar


def child():
    m, gold, train, batches = world('fm', 6040, 3240, 64, 165)
    os.environ['KTUP_EVAL_GRAPH'] = '0'
    for _ in range(5):
        one_pass(m, gold, train, batches, True)


def profile(out):
    tmp = tempfile.mkdtemp(prefix='dot_pass_prof_')
    cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', tmp, '--', sys.executable, os.path.abspath(__file__), '--child']
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        out.append('rocprofv3 run failed (%d): %s' % (r.returncode, (r.stderr or r.stdout)[-300:].replace('\n', ' | ')))
        return
    rows = []
    for path in glob.glob(os.path.join(tmp, '**', '*kernel_trace.csv'), recursive=True):
        rows += list(csv.DictReader(open(path)))
    for name in ('dot_pass_kernel', 'topk_merge_kernel', 'filter_bits_kernel', 'filter_zero_kernel'):
        mine = [r for r in rows if name in r.get('Kernel_Name', '')]
        if not mine:
            out.append('%s: not in the trace' % name)
            continue
        us = sorted((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3 for r in mine)
        regs = ', '.join('%s %s' % (k, mine[0][k]) for k in ('VGPR_Count', 'Accum_VGPR_Count', 'SGPR_Count', 'LDS_Block_Size', 'Scratch_Size',
                                                             'Group_Segment_Size', 'Private_Segment_Size', 'Grid_Size_X', 'Grid_Size')
                         if mine[0].get(k) not in (None, ''))
        out.append('%-24s %d dispatches, median %.1f us (min %.1f, max %.1f); %s   [FM, 6040 x 3240, d = 64, eager passes]'
                   % (name, len(us), statistics.median(us), us[0], us[-1], regs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--passes', type=int, default=20)
    ap.add_argument('--no-profile', action='store_true')
    ap.add_argument('--child', action='store_true')
    ap.add_argument('-o', '--output', default=os.path.join(ROOT, 'profiles', 'dot_pass_times.txt'))
    a = ap.parse_args()
    if a.child:
        return child()
    assert a.rounds >= 5 and a.passes >= 20, 'at least five rounds of 20 passes'
    os.environ.setdefault('TQDM_DISABLE', '1')                            # the walk's progress bar: off, so that it costs the walk nothing
    import torch
    out = ['# tools/dot_pass_time.py: batch walk vs one-sweep pass of the inner-product recommenders, through _driver.rec_eval_pass',
           '# %s, %d rounds x %d passes per route, alternating; wall time per pass in ms' % (torch.cuda.get_device_name(0), a.rounds, a.passes)]
    ok = True
    for kind in ('bprmf', 'fm'):
        ok &= measure('(a) %s 6040 x 3240, d 64' % kind.upper(), *world(kind, 6040, 3240, 64, 165), a.rounds, a.passes, out)
    ok &= measure('(b) BPRMF 512 x 100000, d 64', *world('bprmf', 512, 100000, 64, 165), a.rounds, a.passes, out)
    out.append('# speed bar (faster than the walk by more than the larger spread, at (a) and (b)): %s' % ('met' if ok else 'NOT met'))
    if not a.no_profile:
        profile(out)
    text = '\n'.join(out) + '\n'
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.output)), exist_ok=True)
    open(a.output, 'w').write(text)


if __name__ == '__main__':
    main()
