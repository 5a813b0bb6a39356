#!/usr/bin/env python3
"""bench.py -- scored (u,i)+(h,r,t) triples/sec of the KTUP scoring path at d=100 on ml1m-shape synthetic data.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full [--no-extras]]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

One step = one pass of the hot path over one batch resident in HBM: 716,800 (u,i) pairs through the KTUP
preference-gated scorer (jTransUP.py:122-143) and 307,200 (h,t,r) triples through its TransH branch
(jTransUP.py:144-157) -- 2,000 reference batches of 512 at joint_ratio 0.7 (7 rec : 3 kg), i.e. one ml1m epoch
worth of scored rows.  Tables are xavier-uniform + row-normalised like the ctors, fp32, soft gate, squared-L2.
N > 1: one process per GPU, tables replicated (9.7 MB), every rank scores its own shard of rows; the scoring path
has no exchange step, so there is no data-path collective (weak scaling; value = all ranks' rows / max time).

A plain run sets up, warms up, times the K steps and prints the headline line (metric, value, unit, ms_per_step, ...).
--dump-outputs DIR: after the timed steps, the scores of the last step (what a caller of the scoring path receives)
are written as DIR/scores_rec.npy and DIR/scores_kg.npy (float32; seeded inputs, the same from run to run).
--full: the line also carries roofline (dominant kernel = KTUP rec forward, algorithmic bytes / HIP-event time),
cpu_baseline (the oracle port timed on this box's host cores, rank 0, N=1 only), and -- timed separately, outside
the K-step region -- the B=512 training step, the all-item Hit@10 evaluation latency and the N-GPU legs
(--full --no-extras: the roofline only).
"""
import argparse
import json
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, 'joint-kg-recommender_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch
import torch.distributed as dist
import torch.nn.functional as F

# ml1m shape: users, items, entities, relations, aligned items
NU, NI, NE, NR, ALIGNED, D = 6040, 3240, 14708, 20, 2934, 100
LEG_TIMEOUT_S = 240          # the N-GPU legs (dp_train_step, config5_step) may take this long before rank 0 reports without them
REC_ROWS, KG_ROWS = 716800, 307200
HBM_PEAK_GBS = 8000.0                      # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
FP32_PEAK_TFLOPS = 157.3                   # dense fp32 MFMA = VALU fp32 peak (same pipe on gfx950, MI355X_MICROARCH.md)
BYTES_REC = 12 * D + 16 + 4 + 4            # 3 gathered fp32 rows + two int64 ids + int32 map entry + fp32 score
BYTES_KG = 8 * D + 24 + 4                  # h, t rows (rel/norm rows: 20-row tables, counted once) + 3 ids + score
FLOP_REC = 6 * D * NR + 10 * D             # three (d x P) contractions + the elementwise tail, soft gate
FLOP_KG = 12 * D
K6_SOURCES = ('ktup_score_pref_mc.hip', 'ktup_pref_geom.h', 'ktup_lane_swap.h', 'ktup_common.h')   # define the dominant kernel


def kernel_src_sha16(files=K6_SOURCES):
    """Hash of the sources that define the dominant kernel: PMC traffic measured on another version of them is stale."""
    import hashlib
    h = hashlib.sha256()
    for f in files:
        with open(os.path.join(ROOT, 'joint-kg-recommender_amd', 'csrc', f), 'rb') as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def make_table(rows, d, gen):
    bound = (6.0 / (rows + d)) ** 0.5
    w = (torch.rand(rows, d, generator=gen) * 2 - 1) * bound
    return F.normalize(w, p=2, dim=1)


def build_world(seed, device):
    gen = torch.Generator().manual_seed(seed)
    W = dict(U=make_table(NU, D, gen), I=make_table(NI, D, gen),
             E=torch.cat([make_table(NE, D, gen), torch.zeros(1, D)]),
             P=make_table(NR, D, gen), Pn=make_table(NR, D, gen), R=make_table(NR, D, gen), Rn=make_table(NR, D, gen))
    i2e = torch.full((NI,), NE, dtype=torch.int64)
    aligned = torch.randperm(NI, generator=gen)[:ALIGNED]
    i2e[aligned] = torch.randperm(NE, generator=gen)[:ALIGNED]
    idx = dict(u=torch.randint(0, NU, (REC_ROWS,), generator=gen), i=torch.randint(0, NI, (REC_ROWS,), generator=gen),
               h=torch.randint(0, NE, (KG_ROWS,), generator=gen), t=torch.randint(0, NE, (KG_ROWS,), generator=gen),
               r=torch.randint(0, NR, (KG_ROWS,), generator=gen))
    return W, i2e, idx


def host_topology():
    """(logical CPUs, physical cores of NUMA node 0, how that was found) -- SURVEY 8(d) asks for "all physical cores" of the node
    the process runs on; hyper-thread siblings are counted once."""
    ncpu = os.cpu_count() or 1
    try:
        cpus = set()
        for part in open('/sys/devices/system/node/node0/cpulist').read().strip().split(','):
            lo, _, hi = part.partition('-')
            cpus.update(range(int(lo), int(hi or lo) + 1))
        cores = set()
        for c in cpus:
            sib = open('/sys/devices/system/cpu/cpu%d/topology/thread_siblings_list' % c).read().strip()
            cores.add(sib)
        return ncpu, max(1, len(cores)), 'NUMA node 0: %d logical CPUs, %d physical cores (sysfs)' % (len(cpus), len(cores))
    except Exception:      # noqa: BLE001
        return ncpu, max(1, ncpu // 2), 'sysfs topology unreadable: logical CPUs / 2'


def _median_ms(fn, iters, warmup=3, budget_s=4.0):
    """Median wall time of fn() over `iters` timed calls after `warmup` (3 warm-up + >= 20 timed, median); stops early --
    and says so through the returned count -- if the budget runs out (an oversubscribed thread count can take seconds per call)."""
    import statistics
    for _ in range(warmup):
        fn()
    ts, t_all = [], time.perf_counter()
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
        if time.perf_counter() - t_all > budget_s and len(ts) >= 5:
            break
    return 1e3 * statistics.median(ts), len(ts)


def cpu_baseline(W, i2e, idx, budget_s=20.0):
    """SURVEY 8(d)'s CPU column: the oracle (a torch-CPU port of the reference's forward; it replaces the reference's per-item
    python dict walk by a tensor lookup, so it is FASTER than the reference itself) on this box's host cores, B = 512, the
    7 rec : 3 kg mix of one ten-step cycle per timed call, 3 warm-up + 20 timed calls, MEDIAN -- at all physical cores of NUMA
    node 0 (what 8(d) prescribes: `at_numa_node_cores`) and at a ladder of smaller thread counts, because B = 512 ops do not
    parallelise: `value` / `cores` is the FASTEST of them (= `best_of_ladder`), so that no ratio is quoted against a slowed-down CPU."""
    from oracle import cpu_ref as O
    ncpu, phys, how = host_topology()
    B = 512
    cands = sorted(set([t for t in (1, 2, 4, 8, 16, 32) if t <= phys] + [phys]))
    by_threads = {}
    threads_before = torch.get_num_threads()

    def cycle():
        for it in range(10):
            lo = (it * B) % (KG_ROWS - B)
            if it < 7:
                O.score_ktup_rec(W['U'], W['I'], W['E'], W['P'], W['Pn'], W['R'], W['Rn'], i2e, idx['u'][lo:lo + B], idx['i'][lo:lo + B], False)
            else:
                O.score_ktup_kg(W['E'], W['R'], W['Rn'], idx['h'][lo:lo + B], idx['t'][lo:lo + B], idx['r'][lo:lo + B], False)
    with torch.no_grad():
        for threads in cands:
            torch.set_num_threads(threads)
            ms, n = _median_ms(cycle, 20, budget_s=budget_s / len(cands))
            by_threads[str(threads)] = {'rows_per_s': 10 * B / (ms * 1e-3), 'median_ms_per_10_batches': ms, 'timed_calls': n}
    torch.set_num_threads(threads_before)
    best = max(by_threads, key=lambda k: by_threads[k]['rows_per_s'])
    # `value` / `cores` = the FASTEST CPU configuration measured (B = 512 ops do not parallelise: at all 64 cores of the node the same
    # port runs ~3x slower than on one thread, and a baseline published at the slow end would inflate every GPU / CPU ratio derived
    # from it); SURVEY 8(d)'s "all physical cores of the node" figure is kept beside it as `at_numa_node_cores`
    return {'value': by_threads[best]['rows_per_s'], 'unit': 'scored rows/s', 'cores': int(best), 'kind': 'port', 'host_cores': ncpu,
            'numa_node_physical_cores': phys, 'topology': how, 'at_numa_node_cores': dict(by_threads[str(phys)], threads=int(phys)),
            'best_of_ladder': {'threads': int(best), 'rows_per_s': by_threads[best]['rows_per_s']},
            'by_threads': by_threads,
            'sample': 'ten batches of 512 (7 rec : 3 kg) per timed call, 3 warm-up + up to 20 timed calls per thread count, median; '
                      'thread counts %s; oracle/cpu_ref.py, torch %s CPU' % (cands, torch.__version__)}


def cpu_train_step_baseline(threads, budget_s=8.0):
    """The reference's whole B = 512 joint step on the host ("full train step" next to the forward-only figure):
    oracle losses (knowledgable_recommendation.py:335-383), backward, clip_grad_norm_ over all tables, dense Adagrad with weight
    decay -- oracle.train_step, the restatement pinned by tests/golden/train_steps.npz -- ten steps (7 rec : 3 kg) per timed call."""
    from oracle import cpu_ref as O
    gen = torch.Generator().manual_seed(3)
    mk = lambda n: torch.nn.Parameter(make_table(n, D, gen))
    Wt = [mk(NU), mk(NI), torch.nn.Parameter(torch.cat([make_table(NE, D, gen), torch.zeros(1, D)])), mk(NR), mk(NR), mk(NR), mk(NR)]
    i2e = torch.where(torch.arange(NI) < ALIGNED, (torch.arange(NI) * 4) % NE, torch.full((NI,), NE))
    opt = O.make_optimizer(Wt, 'Adagrad', 0.005, 1e-5)
    B = 512
    r = lambda hi: torch.randint(0, hi, (B,), generator=gen)
    batches = [(r(NU), r(NI), r(NI), r(NE), r(NE), r(NR), r(NE), r(NE)) for _ in range(10)]

    def cycle():
        for it, (u, pi, ni, ph, pt, pr, nh, nt) in enumerate(batches):
            if it < 7:
                O.train_step(Wt, opt, lambda: O.ktup_rec_step_loss(*Wt, i2e, u, pi, ni), 5.0, pad_row_of=Wt[2])
            else:
                O.train_step(Wt, opt, lambda: O.kg_step_loss(Wt[2], Wt[5], Wt[6], ph, pt, pr, nh, nt, pr), 5.0, pad_row_of=Wt[2])
    before = torch.get_num_threads()
    torch.set_num_threads(threads)
    ms, n = _median_ms(cycle, 20, warmup=2, budget_s=budget_s)
    torch.set_num_threads(before)
    return {'kind': 'port', 'cores': threads, 'ms_per_step': ms / 10, 'scored_rows_per_s': 2 * B / (ms / 10 * 1e-3), 'timed_calls': n,
            'sample': 'ten B=512 steps (7 rec : 3 kg) per timed call, median of the timed calls; oracle.train_step '
                      '(losses + backward + clip_grad_norm_ + dense Adagrad, weight decay 1e-5)'}


def ramp_clocks(fn, device, seconds=0.25, world=1, calls=20):
    """A device that sat idle while the host built a model needs ~50 ms of load to reach its clocks; a 10 ms timed loop started
    cold measures the ramp, not the step (seen as a 7x outlier on one of the B=512 legs per run).  Untimed, like warm-up steps.
    With several ranks and collectives inside `fn` the loop runs a FIXED number of calls: a wall-clock bound lets one rank leave
    the loop a call earlier than its peer, which then waits in an all-to-all forever (round 5: the config-5 leg of the two-rank
    bench test hit the 240 s watchdog once in three runs)."""
    if world > 1:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize(device)
        return
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        fn()
        torch.cuda.synchronize(device)


def train_step_bench(device, steps=200, warmup=20):
    """Secondary figure: the reference's B=512 joint training step (forward pos+neg, loss, backward, global-norm clip,
    dense Adagrad step with weight decay) through the drop-in module, 7 rec : 3 kg; clip + step either by torch
    (clip_grad_norm_ + torch.optim) or by the two K20 launches (utils/fused_optim.py)."""
    from jTransUP.models import jTransUP as jt
    from jTransUP.utils.fused_optim import FusedOptimizer
    B = 512
    gen = torch.Generator().manual_seed(5)
    mk = lambda hi: torch.randint(0, hi, (steps + warmup, B), generator=gen).to(device)
    u, pi, ni_, h, t, nh, nt, r = mk(NU), mk(NI), mk(NI), mk(NE), mk(NE), mk(NE), mk(NE), mk(NR)
    out = {'batch': B, 'steps': steps}
    for mode in ('torch', 'fused'):
        torch.manual_seed(3)
        i_map = {i: i for i in range(NI)}
        new_map = {i: ((i * 4) % NE if i < ALIGNED else -1, i) for i in range(NI)}
        m = jt.jTransUPModel(False, D, NU, NI, NE, NR, i_map, new_map, False, False)
        opt = torch.optim.Adagrad(m.parameters(), lr=0.005, weight_decay=1e-5)
        fused = FusedOptimizer(opt) if mode == 'fused' else None
        params = list(m.parameters())

        def step(s):
            if fused is None:
                opt.zero_grad(set_to_none=False)                     # (the K20 launch leaves the gradients zero-filled itself)
            if s % 10 < 7:
                pos = m((u[s], pi[s]), None, is_rec=True); neg = m((u[s], ni_[s]), None, is_rec=True)
                loss = (-F.logsigmoid(-(pos - neg))).mean()
            else:
                pos = m(None, (h[s], t[s], r[s]), is_rec=False); neg = m(None, (nh[s], nt[s], r[s]), is_rec=False)
                loss = torch.sum(torch.clamp(pos - neg + 1.0, min=0.0))
            loss.backward()                                          # (the score Functions add into the tables' .grad: ops._grad_targets)
            if fused is not None:
                fused.clip_and_step(5.0, zero_grads=True)
            else:
                torch.nn.utils.clip_grad_norm_(params, 5.0)
                opt.step()

        for s in range(warmup):
            step(s)
        ramp_clocks(lambda: step(0), device)
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        for s in range(warmup, warmup + steps):
            step(s)
        torch.cuda.synchronize(device)
        dt = time.perf_counter() - t0
        out['ms_per_step_' + mode] = 1e3 * dt / steps
    # GPU-resident step (utils/fast_train.py JointStepper): what the joint driver runs by default -- two launches per step
    # (fused rec / kg kernel, norm + loss, optimizer) replayed from a HIP graph; KTUP_FUSED_STEP=0 = round 1's ~12 launches
    import types
    from jTransUP.utils.fast_train import JointStepper
    # (gpu_resident_norm_pass: the fused step with round 2's norm pass + grid barrier in the optimizer launch, KTUP_TRACKED_NORM=0)
    outer_tracked = os.environ.get('KTUP_TRACKED_NORM')          # (an A/B run of tools/step_time.py sets it for the legs below)
    for tag, env in (('gpu_resident_multilaunch', '0'), ('gpu_resident_norm_pass', '1'), ('gpu_resident', '1')):
        os.environ['KTUP_FUSED_STEP'] = env
        os.environ['KTUP_TRACKED_NORM'] = '0' if tag == 'gpu_resident_norm_pass' else '1'
        torch.manual_seed(3)
        m = jt.jTransUPModel(False, D, NU, NI, NE, NR, i_map, new_map, False, False)
        opt = torch.optim.Adagrad(m.parameters(), lr=0.005, weight_decay=1e-5)
        tr = types.SimpleNamespace(fused=FusedOptimizer(opt), parameters=list(m.parameters()), model_target=-1, step=0)
        fl = types.SimpleNamespace(margin=1.0, kg_lambda=1.0, clipping_max_value=5.0)
        js = JointStepper(m, tr, fl, B)

        def fstep(s):
            if s % 10 < 7:
                js.rec_step(u[s], pi[s], ni_[s])
            else:
                js.kg_step(h[s], t[s], r[s], nh[s], nt[s], r[s])

        for s in range(warmup):
            fstep(s)
        ramp_clocks(lambda: [fstep(k) for k in range(10)], device)
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        for s in range(warmup, warmup + steps):
            fstep(s)
        torch.cuda.synchronize(device)
        out['ms_per_step_' + tag] = 1e3 * (time.perf_counter() - t0) / steps
        if tag == 'gpu_resident':
            out['fused_step'] = bool(js.fused_step)
            out['tracked_norm'] = js._gn is not None
            # device time of the replayed graphs alone (HIP events around back-to-back replays of each step kind)
            for kind in ('rec', 'kg'):
                g = js._graphs.get(kind)
                if g is None:
                    continue
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize(device)
                a.record()
                for _ in range(50):
                    g[0].replay()
                b.record(); torch.cuda.synchronize(device)
                out['device_ms_per_%s_step' % kind] = a.elapsed_time(b) / 50
    os.environ.pop('KTUP_FUSED_STEP', None)
    os.environ.pop('KTUP_TRACKED_NORM', None)
    if outer_tracked is not None:
        os.environ['KTUP_TRACKED_NORM'] = outer_tracked
    # device-fed steps (what -device_sampling runs): batch slice + negatives drawn by ktup_feed_* at the head of the step's graph;
    # one graph per step, and ten steps (7 rec + 3 kg) per graph -- what the joint driver replays between evaluations
    from jTransUP.utils.device_sampler import DeviceSampler
    from jTransUP.utils.fast_train import DeviceFeeder
    gen2 = torch.Generator().manual_seed(6)
    ratings = torch.stack([torch.randint(0, NU, (96000,), generator=gen2), torch.randint(0, NI, (96000,), generator=gen2)], 1)
    triples = torch.stack([torch.randint(0, NE, (48000,), generator=gen2), torch.randint(0, NE, (48000,), generator=gen2),
                           torch.randint(0, NR, (48000,), generator=gen2)], 1)
    cyc = ('rec',) * 7 + ('kg',) * 3
    torch.manual_seed(3)
    m = jt.jTransUPModel(False, D, NU, NI, NE, NR, i_map, new_map, False, False)
    opt = torch.optim.Adagrad(m.parameters(), lr=0.005, weight_decay=1e-5)
    tr = types.SimpleNamespace(fused=FusedOptimizer(opt), parameters=list(m.parameters()), model_target=-1, step=0)
    js = JointStepper(m, tr, fl, B)
    sm = DeviceSampler(device, seed=1)
    sm.set_rating_dicts(NU, NI, []); sm.set_triples(NE, NR, [triples.tolist()])
    js.attach_feeds(sm, rec=DeviceFeeder(ratings, B, device, seed=1), kg=DeviceFeeder(triples, B, device, seed=2))
    for s_ in range(20):
        js.fed_step(cyc[s_ % 10])
    ramp_clocks(lambda: [js.fed_step(cyc[k]) for k in range(10)], device)
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    for s_ in range(steps):
        js.fed_step(cyc[s_ % 10])
    torch.cuda.synchronize(device)
    out['ms_per_step_device_fed'] = 1e3 * (time.perf_counter() - t0) / steps
    n10 = 0
    js.fed_cycle(cyc)                                            # capture
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    for _ in range(max(steps // 10, 1)):
        n10 += js.fed_cycle(cyc) or sum(1 for k in cyc if js.fed_step(k) is not None)
    torch.cuda.synchronize(device)
    out['ms_per_step_device_fed_x10'] = 1e3 * (time.perf_counter() - t0) / max(n10, 1)
    sm.check()
    out['ms_per_step'] = out['ms_per_step_gpu_resident']
    out['scored_rows_per_s'] = 2 * B / (out['ms_per_step'] * 1e-3)
    out['note'] = ('fwd pos+neg, loss (+ regularisers on the gpu_resident route), bwd, global-norm clip, dense Adagrad with weight '
                   'decay. torch = autograd + clip_grad_norm_ + torch.optim; fused = autograd + K20; gpu_resident = JointStepper, the '
                   'joint driver\'s default: 2 launches per step (ktup_train_rec_step / ktup_train_kg_step, whose gradient atomics track the squared '
                   'gradient norm, then ktup_optim_clip_step: clip + optimizer, no norm pass and no grid barrier since round 4) replayed from a HIP graph; gpu_resident_multilaunch = the same arithmetic as ~12 launches (round 1); '
                   'device_fed = the same step with its batch and negatives drawn by a third launch at the head of the graph (ktup_feed_*, -device_sampling), '
                   'device_fed_x10 = ten such steps per graph replay')
    return out


def forward_b512_bench(device, D_, i2e_d, X, reps=50):
    """BASELINE.md section 3's shape for the forward alone: the reference's batch of 512, the 7 rec : 3 kg mix of one ten-step cycle
    (what cpu_baseline times on the host) -- ktup_pref_prepare + K6 per rec batch, K3 per kg batch, pre-bound launches, (a) issued one
    by one and (b) the ten batches replayed as one HIP graph.  At this size a launch is latency: 512 pairs are 32 wave tiles on a
    1,024-SIMD chip; the headline's one-launch form amortises exactly that."""
    from jTransUP.hip import lib as L
    from jTransUP.hip import ops
    B = 512
    st = torch.cuda.current_stream(device).cuda_stream
    P_ = D_['P']
    ws = ops.pref_workspace(D_['P'], D_['Pn'], D_['R'], D_['Rn'])
    s_out = torch.empty(B, dtype=torch.float32, device=device)

    def bound(stream):
        prep = L.bind('ktup_pref_prepare', P_.data_ptr(), D_['Pn'].data_ptr(), D_['R'].data_ptr(), D_['Rn'].data_ptr(), P_.stride(0),
                      P_.shape[0], P_.shape[1], ws.data_ptr(), stream)
        launches = []
        for it in range(10):
            lo = it * B
            if it < 7:
                rec = L.bind('ktup_score_ktup_fwd', D_['U'].data_ptr(), D_['U'].stride(0), D_['I'].data_ptr(), D_['I'].stride(0),
                             D_['E'].data_ptr(), D_['E'].stride(0), i2e_d.data_ptr(), ws.data_ptr(), P_.shape[0], D,
                             X['u'].data_ptr() + 8 * lo, X['i'].data_ptr() + 8 * lo, B, 0, ops.GUMBEL_OFF, None, 0, 0, s_out.data_ptr(), stream)
                launches += [prep, rec]
            else:
                launches.append(L.bind('ktup_score_transh_fwd', D_['E'].data_ptr(), D_['E'].stride(0), D_['R'].data_ptr(), D_['R'].stride(0),
                                       D_['Rn'].data_ptr(), D_['Rn'].stride(0), D_['R'].shape[0], D, X['h'].data_ptr() + 8 * lo,
                                       X['t'].data_ptr() + 8 * lo, X['r'].data_ptr() + 8 * lo, B, 0, s_out.data_ptr(), stream))
        return launches
    eager = bound(st)

    def cycle():
        for f in eager:
            f()
    for _ in range(5):
        cycle()
    ramp_clocks(cycle, device)
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    for _ in range(reps):
        cycle()
    torch.cuda.synchronize(device)
    ms_eager = 1e3 * (time.perf_counter() - t0) / reps
    graph = torch.cuda.CUDAGraph()
    from jTransUP.hip.lib import capture as _capture
    with _capture(graph):
        for f in bound(torch.cuda.current_stream(device).cuda_stream):
            f()
    graph.replay()
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    for _ in range(reps):
        graph.replay()
    torch.cuda.synchronize(device)
    ms_graph = 1e3 * (time.perf_counter() - t0) / reps
    return {'batch': B, 'batches_per_cycle': 10, 'mix': '7 rec (prepare + K6) : 3 kg (K3)',
            'scored_rows_per_s': 10 * B / (ms_graph * 1e-3), 'ms_per_batch': ms_graph / 10,
            'launch_by_launch': {'scored_rows_per_s': 10 * B / (ms_eager * 1e-3), 'ms_per_batch': ms_eager / 10},
            'note': 'forward only, ids resident; scored_rows_per_s: the ten batches as one HIP graph replay; launch_by_launch: 17 pre-bound launches issued from Python'}


def eval_bench(device, batch=512, seed=11, keep=None):
    """Second half of the metric: all-item Hit@10 evaluation latency at ml1m shape -- every one of the 6040 users scored
    against all 3240 items by KTUP's evaluateRec (K16), filtered top-10 on the device (K17: ~165 filtered items per user,
    1-30 gold items), metric arithmetic on the host -- i.e. one complete pass of knowledgable_recommendation.evaluateRec."""
    import numpy as np
    from jTransUP.models import jTransUP as jt
    from jTransUP.utils import ranking as RK
    torch.manual_seed(3)
    rng = np.random.RandomState(seed)
    i_map = {i: i for i in range(NI)}
    new_map = {i: ((i * 4) % NE if i < ALIGNED else -1, i) for i in range(NI)}
    m = jt.jTransUPModel(False, D, NU, NI, NE, NR, i_map, new_map, False, False)
    m.eval(); m.disable_grad()
    users = list(range(NU))
    train = {u: set(rng.randint(0, NI, size=165).tolist()) for u in users}
    gold = {u: set(rng.randint(0, NI, size=rng.randint(1, 31)).tolist()) - train[u] or {int(rng.randint(NI))} for u in users}
    t0 = time.perf_counter()
    index = RK.RankIndex(users, gold, [train], device)
    t_index = time.perf_counter() - t0
    batches = [users[s:s + batch] for s in range(0, NU, batch)]
    ub = [torch.tensor(b, dtype=torch.long, device=device) for b in batches]

    def one_pass(with_metrics):
        out = []
        items = m.prepare_items()                     # item side of the gate once per pass, like the drivers (weights are frozen)
        for b, u in zip(batches, ub):
            scores = m.evaluateRec(u, items=items)
            if with_metrics:                          # what _driver.rec_eval_pass does: metric columns stay on the device
                out.append(RK.evalRecProcess((b, scores), gold, [train], descending=False, topn=10, index=index, as_array='device'))
            else:
                s, e = index.rows_of(b)
                f_off, f_ids = index.filter_slice(s, e)
                out.append(RK.ops.topk_filtered(scores, False, 10, f_off, f_ids))
        if with_metrics:
            return torch.cat(out).cpu().numpy()       # ONE copy back for the whole pass (syncs)
        torch.cuda.synchronize(device)
        return out
    one_pass(False); one_pass(True)
    reps = 5
    t0 = time.perf_counter()
    for _ in range(reps):
        one_pass(False)
    dev_ms = 1e3 * (time.perf_counter() - t0) / reps
    t0 = time.perf_counter()
    for _ in range(reps):
        rows = one_pass(True)
    full_ms = 1e3 * (time.perf_counter() - t0) / reps
    hit = float(rows[:, 3].mean())
    # the whole pass in one sweep (what the drivers run): item side, users' projections + fused scores / filtered top-10 (no
    # score matrix), merge, per-user metrics, one copy back
    all_u = torch.arange(NU, dtype=torch.long, device=device)

    import types
    from jTransUP.models import _driver
    FL = types.SimpleNamespace(topn=10)
    pass_fn = lambda u, fo, fi, n: m.evaluate_topk(u, m.prepare_items(), n, fo, fi)      # what the drivers hand to rec_eval_pass
    gkey = _driver.model_graph_key(m)

    def fused_pass():                                 # the drivers' own whole-pass route: eager once, captured once, then replayed
        return _driver._rec_eval_fused(FL, pass_fn, batches, index, gkey)
    fused = None
    if m.evaluate_topk(all_u[:64], m.prepare_items(), 10) is not None:
        for _ in range(3):                            # the first pass runs eagerly, the second captures the graph: not timed
            rows_f = fused_pass()
        t0 = time.perf_counter()
        for _ in range(reps * 4):
            rows_f = fused_pass()
        fused_ms = 1e3 * (time.perf_counter() - t0) / (reps * 4)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        items = m.prepare_items()
        a.record()
        for _ in range(20):
            m.evaluate_topk(all_u, items, 10, index.f_off, index.f_ids)
        b.record(); torch.cuda.synchronize(device)
        sweep_ms = a.elapsed_time(b) / 20
        # matrix work of the sweep: every user x item cross term in preference space, K = (d + 2P) + 2P + 2P + P = 240 multiply-adds
        # per pair at d = 100, P = 20 -- 60 MFMAs per 16 x 16 tile; until round 6 the sweep multiplied the zero padding of the last
        # 16-blocks too (272, 68 MFMAs), and the round-5 fractions were quoted on those 544 flop (the six d-long products of the
        # batched route: 600 multiply-adds)
        p4 = 4 if NR <= 4 else 20 if NR <= 20 else 32           # preferences = relations in KTUP
        kpad = sum((D + 2 * p4, 2 * p4, 2 * p4, p4))
        flop = 2.0 * NU * NI * kpad
        fused = {'full_pass_ms_incl_metrics': fused_ms, 'device_ms_scores_and_topk': sweep_ms,
                 'mfma_flop_per_pair': 2 * kpad, 'gemm_tflops_over_sweep': flop / (sweep_ms * 1e-3) / 1e12,
                 'gemm_frac_of_fp32_peak': flop / (sweep_ms * 1e-3) / 1e12 / FP32_PEAK_TFLOPS,
                 'metric_rows_max_abs_diff_vs_batched_route': float(np.abs(rows_f - rows).max()),
                 'rows_equal_batched_route': bool(np.array_equal(rows_f, rows))}
        rows = rows_f
    if keep is not None:                              # for the CPU side-by-side, run after every GPU timing (main)
        keep.update(m=m, users=users, gold=gold, train=train, rows=rows)
    return {'users': NU, 'items': NI, 'batch': batch, 'batches': len(batches), 'topn': 10,
            'full_pass_ms': fused['full_pass_ms_incl_metrics'] if fused else full_ms, 'fused_pass': fused,
            'batched_route': {'device_ms_full_pass': dev_ms, 'device_ms_per_batch': dev_ms / len(batches), 'full_pass_ms_incl_metrics': full_ms},
            'filter_index_build_ms': 1e3 * t_index, 'hit_at_10_random_init': hit,
            'note': 'fused_pass: the drivers\' whole-pass route (_driver._rec_eval_fused) -- item side (1 launch), users projections + '
                    'scores + filtered top-10 in one sweep without the score matrix (ktup_eval_pref_topk), per-user f1/p/r/hit/ndcg on '
                    'the device (K18b), one (users x 5) float64 copy back; run eagerly once, captured once, then ONE graph replay per '
                    'pass (the tables are read in place); batched_route: round 1 shape -- 12 batches of 512 users x (K16 matrix + K17 + K18b). The filter index is built once per run'}


def cpu_eval_baseline(m, users, gold, train, gpu_rows, budget_s=8.0, cb=32):
    """CPU side-by-side for the evaluation half of the metric: the oracle's reference-shaped evaluateRec
    (jTransUP.py:163-191: B x N x d materialisations, so B is reduced to 32 users to fit RAM like SURVEY prescribes) plus the
    evalRecProcess-equivalent ranking walk (utils/misc.py:186-248), on this box's host cores, on a bounded sample of the same
    users; the per-user rate is extrapolated to the 6040-user pass.  Also a parity spot check: the sample's metric rows must
    equal the device pass's rows."""
    import numpy as np
    from oracle import cpu_ref as O
    W = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    i2e = m._eval_item2ent.cpu().long()
    threads_before = torch.get_num_threads()
    ncpu = os.cpu_count() or 1
    torch.set_num_threads(min(ncpu, 32))
    done, t_score, t_rank, worst = 0, 0.0, 0.0, 0.0
    t_start = time.perf_counter()
    with torch.no_grad():
        while time.perf_counter() - t_start < budget_s and done + cb <= len(users):
            ub = users[done:done + cb]
            t0 = time.perf_counter()
            sc = O.eval_ktup_rec(W['user_embeddings.weight'], W['item_embeddings.weight'], W['ent_embeddings.weight'],
                                 W['pref_embeddings.weight'], W['pref_norm_embeddings.weight'], W['rel_embeddings.weight'],
                                 W['norm_embeddings.weight'], i2e, torch.tensor(ub), False).numpy()
            t1 = time.perf_counter()
            out = O.eval_rec_rows(list(zip(ub, sc)), gold, [train], descending=False, topn=10)
            t2 = time.perf_counter()
            t_score += t1 - t0; t_rank += t2 - t1
            want = np.array([r[:5] for r in out], dtype=np.float64)
            worst = max(worst, float(np.abs(want - gpu_rows[done:done + cb]).max()))
            done += cb
    torch.set_num_threads(threads_before)
    per_user_ms = 1e3 * (t_score + t_rank) / max(done, 1)
    return {'kind': 'port', 'cores': min(ncpu, 32), 'host_cores': ncpu, 'users_sampled': done, 'batch': cb,
            'ms_per_user': per_user_ms, 'ms_per_user_scoring': 1e3 * t_score / max(done, 1), 'ms_per_user_ranking': 1e3 * t_rank / max(done, 1),
            'full_pass_ms_extrapolated': per_user_ms * len(users), 'max_abs_metric_diff_vs_device': worst,
            'sample': 'first %d users in batches of %d: oracle eval_ktup_rec (reference-shaped, B x N x d) + eval_rec_rows '
                      '(serial evalRecProcess equivalent), %.1f s of CPU work' % (done, cb, t_score + t_rank)}


def eval_kg_bench(device, nq=20480, batch=512, seed=13):
    """BASELINE config 2's evaluation: TransE (d = 100, squared L2) link prediction at ml1m-kg shape -- `nq` (h, r) keys, every
    one against all 14,708 entities (transE.py:86-105), filtered gold ranks (utils/misc.py:125-146: 1-3 gold tails, ~20 filtered
    entities per key), Hit@10 / mean rank / MRR -- through _driver.kg_eval_pass as the KG driver's periodic evaluation runs it
    (whole pass behind one call, one copy back), with the CPU column: the oracle's reference-shaped evaluateTail (B x N x d
    materialised, so B = 64) + the serial evalKGProcess walk on a bounded sample of the same keys, extrapolated to the pass."""
    import types
    import numpy as np
    from jTransUP.models import _driver as Dr
    from jTransUP.models import transE
    from oracle import cpu_ref as O
    rng = np.random.RandomState(seed)
    torch.manual_seed(seed)
    m = transE.TransEModel(False, D, NE, NR).to(device)
    m.eval(); m.disable_grad()
    FL = types.SimpleNamespace(topn=10)
    keys = list(dict.fromkeys((int(rng.randint(NE)), int(rng.randint(NR))) for _ in range(nq + 4000)))[:nq]
    gold = {k: set(rng.randint(0, NE, size=rng.randint(1, 4)).tolist()) for k in keys}
    filt = {k: set(rng.randint(0, NE, size=20).tolist()) for k in keys}
    batches = [keys[s_:s_ + batch] for s_ in range(0, len(keys), batch)]
    score_fn = lambda q, r: m.evaluateTail(q, r)
    rank_fn = lambda q, r, desc, go, gi, fo, fi: m.rank_entities(q, r, False, desc, go, gi, fo, fi)
    import contextlib
    with contextlib.redirect_stderr(open(os.devnull, 'w')):          # tqdm bars of the walk
        rows = Dr.kg_eval_pass(FL, score_fn, batches, gold, [filt], False, want_rows=False, rank_fn=rank_fn)      # builds the index, warms up
        torch.cuda.synchronize(device)
        times = []
        for _ in range(15):                                        # median of 15 passes (a pass is ~1.5 ms: host jitter is visible in a mean of 5)
            t0 = time.perf_counter()
            rows = Dr.kg_eval_pass(FL, score_fn, batches, gold, [filt], False, want_rows=False, rank_fn=rank_fn)
            times.append(1e3 * (time.perf_counter() - t0))
        pass_ms = sorted(times)[len(times) // 2]
    # CPU column on a bounded sample
    W = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    _, phys, _ = host_topology()
    before = torch.get_num_threads()
    torch.set_num_threads(min(32, phys))
    cb, done, t_score, t_rank, t_start = 64, 0, 0.0, 0.0, time.perf_counter()
    cpu_rows, ref_rows = [], []
    W64 = {k: v.double() for k, v in W.items()}
    with torch.no_grad():
        while time.perf_counter() - t_start < 6.0 and done + cb <= len(keys):
            kb = keys[done:done + cb]
            t0 = time.perf_counter()
            sc = O.eval_transe(W['ent_embeddings.weight'], W['rel_embeddings.weight'], torch.tensor([k[0] for k in kb]),
                               torch.tensor([k[1] for k in kb]), False, False).numpy()
            t1 = time.perf_counter()
            cpu_rows.extend(O.eval_kg_rows(list(zip(kb, sc)), gold, [filt], descending=False, topn=10))
            t2 = time.perf_counter()
            t_score += t1 - t0; t_rank += t2 - t1
            # the referee (untimed): the same formula in fp64 -- the order of the exact scores of the fp32 tables
            sc64 = O.eval_transe(W64['ent_embeddings.weight'], W64['rel_embeddings.weight'], torch.tensor([k[0] for k in kb]),
                                 torch.tensor([k[1] for k in kb]), False, False).numpy()
            ref_rows.extend(O.eval_kg_rows(list(zip(kb, sc64)), gold, [filt], descending=False, topn=10))
            done += cb
    torch.set_num_threads(before)
    n_cpu = len(cpu_rows)
    # the oracle sums (c - e)^2 directly, the device expands |c|^2 - 2 c.e + |e|^2 on the matrix cores: near-ties may swap neighbours
    cr, dr = np.array(sorted(r[1] for r in cpu_rows), dtype=np.int64), np.sort(rows[:n_cpu, 1]).astype(np.int64)
    rr = np.array(sorted(r[1] for r in ref_rows), dtype=np.int64)
    agree = {'ranks_compared': int(n_cpu), 'frac_equal_fp64_referee': float((rr == dr).mean()) if n_cpu else None,
             'max_abs_rank_diff_fp64_referee': int(np.abs(rr - dr).max()) if n_cpu else None,
             'frac_equal_fp32_oracle': float((cr == dr).mean()) if n_cpu else None,
             'fp32_oracle_vs_fp64_referee_frac_equal': float((cr == rr).mean()) if n_cpu else None,
             'note': 'the device decides comparisons near a gold in fp64 (option kg_exact): it must equal the fp64 referee; the fp32 oracle '
                     'sums (c - e)^2 in fp32 and loses a few near ties to its own rounding'}
    per_q = 1e3 * (t_score + t_rank) / max(done, 1)
    return {'model': 'TransE d=%d squared-L2 (BASELINE configs[1])' % D, 'keys': len(keys), 'entities': NE, 'batch': batch,
            'full_pass_ms': pass_ms, 'ms_per_512_keys': pass_ms / len(batches), 'gold_entries': int(rows.shape[0]),
            'hit_at_10_random_init': float(rows[:, 0].mean()), 'mean_rank_random_init': float(rows[:, 1].mean()),
            'mrr_random_init': float((1.0 / (rows[:, 1] + 1.0)).mean()),
            'cpu_baseline': {'kind': 'port', 'cores': min(32, phys), 'keys_sampled': done, 'batch': cb, 'ms_per_key': per_q,
                             'ms_per_key_scoring': 1e3 * t_score / max(done, 1), 'ms_per_key_ranking': 1e3 * t_rank / max(done, 1),
                             'full_pass_ms_extrapolated': per_q * len(keys), 'ranks_vs_device_on_sample': agree,
                             'sample': 'first %d keys in batches of %d: oracle eval_transe (reference-shaped) + eval_kg_rows, %.1f s of CPU work'
                                       % (done, cb, t_score + t_rank)},
            'note': 'one direction (tails) of a link-prediction pass: K12 scores + K18 filtered gold ranks under ONE call per pass '
                    '(ktup_eval_kg_ranks), one copy back of the ranks'}


def eval_ktup_l1_bench(device, batch=512, seed=19):
    """The reference's own run scripts evaluate KTUP / TUP with -L1_flag (ktup.sh, transup.sh): the whole 6040-user pass with the L1
    distance, soft gate -- in one sweep (the pair kernel's arithmetic, top-10 in its epilogue) and batch by batch."""
    import types
    import numpy as np
    from jTransUP.models import _driver as Dr
    from jTransUP.models import jTransUP as jt
    rng = np.random.RandomState(seed)
    torch.manual_seed(seed)
    i_map = {i: i for i in range(NI)}
    new_map = {i: ((i * 4) % NE if i < ALIGNED else -1, i) for i in range(NI)}
    m = jt.jTransUPModel(True, D, NU, NI, NE, NR, i_map, new_map, False, False).to(device)
    m.eval(); m.disable_grad()
    FL = types.SimpleNamespace(topn=10, shard_eval_candidates=False)
    users = list(range(NU))
    train = {u: set(rng.randint(0, NI, size=165).tolist()) for u in users}
    gold = {u: set(rng.randint(0, NI, size=rng.randint(1, 31)).tolist()) - train[u] or {int(rng.randint(NI))} for u in users}
    batches = [users[s_:s_ + batch] for s_ in range(0, NU, batch)]
    items = m.prepare_items()
    score_fn = lambda u: m.evaluateRec(u, items=items)
    pass_fn = lambda u, fo, fi, n: m.evaluate_topk(u, m.prepare_items(), n, fo, fi)
    import contextlib
    with contextlib.redirect_stderr(open(os.devnull, 'w')):
        def timed(**kw):
            rows = Dr.rec_eval_pass(FL, score_fn, batches, gold, [train], False, want_rows=False, **kw)
            torch.cuda.synchronize(device)
            reps = 5
            t0 = time.perf_counter()
            for _ in range(reps):
                rows = Dr.rec_eval_pass(FL, score_fn, batches, gold, [train], False, want_rows=False, **kw)
            return 1e3 * (time.perf_counter() - t0) / reps, rows
        batched_ms, rows_b = timed()
        pass_ms, rows = timed(pass_fn=pass_fn)
    return {'model': 'KTUP d=%d, L1 distance, soft gate (the reference run scripts\' -L1_flag)' % D, 'users': NU, 'items': NI,
            'full_pass_ms': pass_ms, 'batched_route': {'full_pass_ms': batched_ms},
            'metric_rows_max_abs_diff_vs_batched_route': float(np.abs(rows - rows_b).max()) if rows.shape == rows_b.shape else None,
            'note': 'full_pass_ms: one sweep (ktup_eval_pref_topk_hard with KTUP_GUMBEL_OFF: the pair kernel\'s arithmetic, filtered '
                    'top-10 where the scores are made) + metrics; batched_route: K16 (VALU pair kernel) + K17 + K18b per 512 users'}


def eval_tup_hard_bench(device, batch=512, seed=17):
    """BASELINE config 3's evaluation: TUP (transup) at d = 100, 20 preferences, -use_st_gumbel -- every one of the 6040 users
    against all 3240 items with the ST-Gumbel gate drawn per (user, item) pair (transUP.py:84-102,143-170: stochastic in the
    reference too; here Philox on the device), filtered top-10 and the per-user metrics on the device, through
    _driver.rec_eval_pass.  CPU column: the oracle's reference-shaped evaluate with recorded uniforms + the serial evalRecProcess
    walk on a bounded sample."""
    import types
    import numpy as np
    from jTransUP.models import _driver as Dr
    from jTransUP.models import transUP as tu
    from oracle import cpu_ref as O
    rng = np.random.RandomState(seed)
    torch.manual_seed(seed)
    m = tu.TransUPModel(False, D, NU, NI, NR, True).to(device)
    m.eval(); m.disable_grad()
    FL = types.SimpleNamespace(topn=10, shard_eval_candidates=False)
    users = list(range(NU))
    train = {u: set(rng.randint(0, NI, size=165).tolist()) for u in users}
    gold = {u: set(rng.randint(0, NI, size=rng.randint(1, 31)).tolist()) - train[u] or {int(rng.randint(NI))} for u in users}
    batches = [users[s_:s_ + batch] for s_ in range(0, NU, batch)]
    items = m.prepare_items()
    score_fn = lambda u: m.evaluate(u, items=items)
    import contextlib
    pass_fn = lambda u, fo, fi, n: m.evaluate_topk(u, m.prepare_items(), n, fo, fi)      # the drivers' route: the pass in one sweep
    with contextlib.redirect_stderr(open(os.devnull, 'w')):
        def timed(**kw):
            rows = Dr.rec_eval_pass(FL, score_fn, batches, gold, [train], False, want_rows=False, **kw)
            torch.cuda.synchronize(device)
            reps = 5
            t0 = time.perf_counter()
            for _ in range(reps):
                rows = Dr.rec_eval_pass(FL, score_fn, batches, gold, [train], False, want_rows=False, **kw)
            return 1e3 * (time.perf_counter() - t0) / reps, rows
        batched_ms, rows_b = timed()
        pass_ms, rows = timed(pass_fn=pass_fn)
    W = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    _, phys, _ = host_topology()
    before = torch.get_num_threads()
    torch.set_num_threads(min(32, phys))
    cb, done, t_score, t_rank, t_start = 16, 0, 0.0, 0.0, time.perf_counter()
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        while time.perf_counter() - t_start < 6.0 and done + cb <= len(users):
            ub = users[done:done + cb]
            t0 = time.perf_counter()
            uni = torch.rand(cb, NI, NR, generator=g)
            sc = O.eval_tup(W['user_embeddings.weight'], W['item_embeddings.weight'], W['pref_embeddings.weight'],
                            W['pref_norm_embeddings.weight'], torch.tensor(ub), False, uni).numpy()
            t1 = time.perf_counter()
            O.eval_rec_rows(list(zip(ub, sc)), gold, [train], descending=False, topn=10)
            t2 = time.perf_counter()
            t_score += t1 - t0; t_rank += t2 - t1
            done += cb
    torch.set_num_threads(before)
    per_u = 1e3 * (t_score + t_rank) / max(done, 1)
    return {'model': 'TUP d=%d, %d preferences, ST-Gumbel gate (BASELINE configs[2])' % (D, NR), 'users': NU, 'items': NI, 'batch': batch,
            'full_pass_ms': pass_ms, 'ms_per_512_users': pass_ms / len(batches), 'hit_at_10_random_init': float(rows[:, 3].mean()),
            'batched_route': {'full_pass_ms': batched_ms, 'hit_at_10_random_init': float(rows_b[:, 3].mean())},
            'cpu_baseline': {'kind': 'port', 'cores': min(32, phys), 'users_sampled': done, 'batch': cb, 'ms_per_user': per_u,
                             'ms_per_user_scoring': 1e3 * t_score / max(done, 1), 'ms_per_user_ranking': 1e3 * t_rank / max(done, 1),
                             'full_pass_ms_extrapolated': per_u * len(users),
                             'sample': 'first %d users in batches of %d: oracle eval_tup with drawn uniforms (reference-shaped, B x N x P '
                                       'noise + B x N x d tensors) + eval_rec_rows, %.1f s of CPU work' % (done, cb, t_score + t_rank)},
            'note': 'the gate draws fresh noise per (user, item) pair, so this pass has no preference-space shortcut.  full_pass_ms: the '
                    'whole pass in one sweep (ktup_eval_pref_topk_hard: pair arithmetic + filtered top-10 where the scores are made, '
                    'no score matrix) + metrics (K18b), one copy back; batched_route: per 512 users the hard-gate pair kernel, K17, K18b '
                    '(fresh noise per pass in both, so the two hit rates differ by sampling)'}


def gather_stress_bench(device, scale=1000, reps=20, only_rec=False):
    """SURVEY.md 8(d) gather-stress variant = the HBM-bound companion of the headline: the same KTUP forward with every big
    table scaled x1000 in rows (9.7 GB, far beyond L2 and Infinity Cache) and uniform ids, so every row really comes from
    HBM.  A 400-byte row at its natural pitch costs four 128-byte lines (traffic ~ 512/400 x algorithmic), which caps useful
    row bytes at ~72 % of the HBM peak; tools/gather_bench.hip measured 4.7-4.9 TB/s for scattered 400-B rows at this
    working set (profiles/r01_gather_ceiling.txt).  Launches are pre-bound (no wrapper time inside the HIP events)."""
    from jTransUP.hip import lib as L
    from jTransUP.hip import ops
    gen = torch.Generator(device=device); gen.manual_seed(3)
    nu, ni, ne = NU * scale, NI * scale, NE * scale
    free, _ = torch.cuda.mem_get_info(device)
    need = (nu + ni + ne) * D * 4
    if free < 1.5 * need:
        return {'skipped': 'needs %.1f GB of device memory' % (need / 1e9)}
    mk = lambda rows: torch.nn.functional.normalize(torch.randn(rows, D, generator=gen, device=device), dim=1)
    U, I, E = mk(nu), mk(ni), mk(ne + 1)
    P, Pn, R, Rn = mk(NR), mk(NR), mk(NR), mk(NR)
    i2e = torch.randint(0, ne, (ni,), generator=gen, device=device).to(torch.int32)
    u = torch.randint(0, nu, (REC_ROWS,), generator=gen, device=device)
    i = torch.randint(0, ni, (REC_ROWS,), generator=gen, device=device)
    h = torch.randint(0, ne, (KG_ROWS,), generator=gen, device=device)
    t = torch.randint(0, ne, (KG_ROWS,), generator=gen, device=device)
    r = torch.randint(0, NR, (KG_ROWS,), generator=gen, device=device)
    out = {'tables_GB': need / 1e9, 'rows_scale': scale}
    st = torch.cuda.current_stream(device).cuda_stream
    ws = ops.pref_workspace(P, Pn, R, Rn)
    s_rec = torch.empty(REC_ROWS, dtype=torch.float32, device=device)
    s_kg = torch.empty(KG_ROWS, dtype=torch.float32, device=device)
    rec = L.bind('ktup_score_ktup_fwd', U.data_ptr(), U.stride(0), I.data_ptr(), I.stride(0), E.data_ptr(), E.stride(0), i2e.data_ptr(),
                 ws.data_ptr(), NR, D, u.data_ptr(), i.data_ptr(), REC_ROWS, 0, ops.GUMBEL_OFF, None, 0, 0, s_rec.data_ptr(), st)
    kg = L.bind('ktup_score_transh_fwd', E.data_ptr(), E.stride(0), R.data_ptr(), R.stride(0), Rn.data_ptr(), Rn.stride(0), NR, D,
                h.data_ptr(), t.data_ptr(), r.data_ptr(), KG_ROWS, 0, s_kg.data_ptr(), st)
    for name, f, rows, bpr in (('ktup_rec_forward', rec, REC_ROWS, BYTES_REC), ('ktup_kg_forward', kg, KG_ROWS, BYTES_KG),
                               ('ktup_rec_forward_nontemporal', rec, REC_ROWS, BYTES_REC)):
        if only_rec and name != 'ktup_rec_forward':
            continue
        nt_before = L.set_option('nt_gather', 1) if name.endswith('nontemporal') else None
        for _ in range(3):
            f()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        torch.cuda.synchronize(device)
        for a, b in ev:
            a.record(); f(); b.record()
        torch.cuda.synchronize(device)
        ms = sorted(a.elapsed_time(b) for a, b in ev)[reps // 2]
        out[name] = {'ms_per_launch': ms, 'achieved_GBs': rows * bpr / (ms * 1e-3) / 1e9,
                     'frac_of_hbm_peak': rows * bpr / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS}
        if nt_before is not None:
            L.set_option('nt_gather', nt_before)
    out['note'] = 'algorithmic row bytes / median HIP-event time of the bound launch; tables HBM-resident, so traffic ~ algorithmic x 512/400'
    if only_rec:
        return out
    # K6 at config 5's width on HBM-resident tables: d = 256 rows are 1 KB and line-aligned (the pure gather runs at 5.8-6.1 TB/s there)
    del U, I, E, rec, kg
    torch.cuda.empty_cache()
    d2, sc2 = 256, 400
    nu, ni, ne = NU * sc2, NI * sc2, NE * sc2
    mk2 = lambda rows: torch.randn(rows, d2, generator=gen, device=device).mul_(1.0 / 16.0)
    U, I, E = mk2(nu), mk2(ni), mk2(ne + 1)
    P2 = [torch.nn.functional.normalize(torch.randn(NR, d2, generator=gen, device=device), dim=1) for _ in range(4)]
    i2e = torch.randint(0, ne, (ni,), generator=gen, device=device).to(torch.int32)
    u = torch.randint(0, nu, (REC_ROWS,), generator=gen, device=device)
    i = torch.randint(0, ni, (REC_ROWS,), generator=gen, device=device)
    ws2 = ops.pref_workspace(*P2)
    rec2 = L.bind('ktup_score_ktup_fwd', U.data_ptr(), U.stride(0), I.data_ptr(), I.stride(0), E.data_ptr(), E.stride(0), i2e.data_ptr(),
                  ws2.data_ptr(), NR, d2, u.data_ptr(), i.data_ptr(), REC_ROWS, 0, ops.GUMBEL_OFF, None, 0, 0, s_rec.data_ptr(), st)
    bpr2 = 12 * d2 + 24
    ramp_clocks(rec2, device)        # sustained rate: three warm-up launches measured the clock ramp (0.485 ms against 0.45 under load)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    torch.cuda.synchronize(device)
    for a, b in ev:
        a.record(); rec2(); b.record()
    torch.cuda.synchronize(device)
    ms = sorted(a.elapsed_time(b) for a, b in ev)[reps // 2]
    out['ktup_rec_forward_d256'] = {'ms_per_launch': ms, 'rows_per_launch': REC_ROWS, 'bytes_per_row': bpr2, 'tables_GB': (nu + ni + ne) * d2 * 4 / 1e9,
                                    'achieved_GBs': REC_ROWS * bpr2 / (ms * 1e-3) / 1e9, 'frac_of_hbm_peak': REC_ROWS * bpr2 / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                    'kernel': 'pref_fwd_wide_kernel<FwGeom<5,true>,false> (K6 at config 5 width; 1 KB line-aligned rows; four waves per 16-pair tile, three tiles per CU)'}
    return out


def roofline_hbm_resident(gs, live=None):
    """First-class companion of `roofline` for the case the north star means by "gather-bound": tables far larger than the
    caches.  Same schema; traffic LIVE (a rocprofv3 --pmc child pass over `--only gather_stress_rec`: K6 on the x1000 tables and
    nothing else), else from the committed gather-stress PMC pass when its stamp matches the kernel sources."""
    if 'ktup_rec_forward' not in gs:
        return {'skipped': gs.get('skipped', 'not run')}
    e = gs['ktup_rec_forward']
    traffic, tnote = live if live is not None else hbm_traffic('gather_stress_ktup_rec_forward')
    t = e['ms_per_launch'] * 1e-3
    return {'bound': 'hbm', 'kernel': 'pref_fwd_mc_kernel<McGeom<25,5,true,false>,false> on tables x%d rows (%.1f GB, uniform ids)'
                                      % (gs['rows_scale'], gs['tables_GB']),
            'achieved': e['achieved_GBs'], 'peak': HBM_PEAK_GBS, 'unit': 'GB/s', 'frac': e['frac_of_hbm_peak'],
            'traffic': traffic, 'traffic_source': tnote,
            'traffic_frac_of_hbm_peak': None if traffic is None else traffic / t / 1e9 / HBM_PEAK_GBS,
            'traffic_over_algorithmic': None if traffic is None else traffic / (REC_ROWS * BYTES_REC),
            'expected_traffic_over_algorithmic': 512.0 / 400.0,
            'with_nontemporal_row_loads': gs.get('ktup_rec_forward_nontemporal'),
            'scattered_row_ceiling_GBs': 4860.0, 'frac_of_scattered_row_ceiling': e['achieved_GBs'] / 4860.0,
            'ceiling_source': 'profiles/r03_gather_footprint.txt: pure gather of the same 2,150,400 rows from a 9.7 GB table, 4.68 TB/s default / 4.86 TB/s nontemporal',
            'ms_per_launch': e['ms_per_launch'], 'rows_per_launch': REC_ROWS, 'bytes_per_row': BYTES_REC,
            'kg_kernel': gs.get('ktup_kg_forward'),
            'note': '400-byte rows at their natural pitch cost four 128-byte lines; the ceiling is the pure gather microbenchmark '
                    '(tools/gather_bench.hip, profiles/r01_gather_ceiling.txt) at the same working set'}


def variants_bench(device, D_, i2e_d, X, reps=10, inner=8):
    """The other kernels of the path at the headline's sizes (716,800 pairs / 307,200 triples per launch): L1 distance (7 of
    the reference's recipes pass -L1_flag), the ST-Gumbel gate (transup.sh), TUP, TransE, TransR, BPRMF.  Each variant is
    captured into a HIP graph of `inner` launches and replayed, so the figure is kernel time, not Python time."""
    from jTransUP.hip import ops
    U, I, E, P, Pn, R, Rn = (D_[k] for k in ('U', 'I', 'E', 'P', 'Pn', 'R', 'Rn'))
    u, i, h, t, r = (X[k] for k in ('u', 'i', 'h', 't', 'r'))
    gen = torch.Generator(device=device); gen.manual_seed(5)
    M = torch.randn(NR, D * D, generator=gen, device=device) * 0.1
    U64 = F.normalize(torch.randn(NU, 64, generator=gen, device=device), dim=1)
    I64 = F.normalize(torch.randn(NI, 64, generator=gen, device=device), dim=1)
    ws = ops.pref_workspace(P, Pn, R, Rn)
    ws_tup = ops.pref_workspace(P, Pn)
    PH, OFF = ops.GUMBEL_PHILOX, ops.GUMBEL_OFF
    cases = [
        ('ktup_rec_soft_L2', lambda: ops.score_ktup(U, I, E, P, Pn, R, Rn, i2e_d, u, i, False, ws=ws), REC_ROWS, BYTES_REC),   # the headline kernel, for calibration
        ('ktup_rec_soft_L1', lambda: ops.score_ktup(U, I, E, P, Pn, R, Rn, i2e_d, u, i, True, ws=ws), REC_ROWS, BYTES_REC),
        ('ktup_rec_hard_L2', lambda: ops.score_ktup(U, I, E, P, Pn, R, Rn, i2e_d, u, i, False, PH, None, 7, 0, ws=ws), REC_ROWS, BYTES_REC),
        ('ktup_rec_hard_L1', lambda: ops.score_ktup(U, I, E, P, Pn, R, Rn, i2e_d, u, i, True, PH, None, 7, 0, ws=ws), REC_ROWS, BYTES_REC),
        ('tup_soft_L2', lambda: ops.score_tup(U, I, P, Pn, u, i, False, OFF, ws=ws_tup), REC_ROWS, 8 * D + 20),
        ('tup_hard_L1', lambda: ops.score_tup(U, I, P, Pn, u, i, True, PH, None, 7, 0, ws=ws_tup), REC_ROWS, 8 * D + 20),
        ('transh_L1', lambda: ops.score_transh(E, R, Rn, h, t, r, True), KG_ROWS, BYTES_KG),
        ('transe_L2', lambda: ops.score_transe(E, R, h, t, r, False), KG_ROWS, BYTES_KG),
        ('transe_L1', lambda: ops.score_transe(E, R, h, t, r, True), KG_ROWS, BYTES_KG),
        ('transr_L2', lambda: ops.score_transr(E, R, M, h, t, r, False), KG_ROWS, BYTES_KG),
        ('bprmf_d64', lambda: ops.score_bprmf(U64, I64, u, i), REC_ROWS, 8 * 64 + 20),
    ]
    # all-candidate evaluation, one batch of 512 queries (scores only; the ranking kernels add ~10 us)
    uq, hq, rq = u[:512].contiguous(), h[:512].contiguous(), r[:512].contiguous()
    i2e_rows = i2e_d[:I.shape[0]].contiguous()
    evals = [
        ('eval_ktup_soft_L2', lambda: ops.eval_ktup(U, I, E, P, Pn, R, Rn, i2e_rows, uq, False), 512 * NI),
        ('eval_ktup_soft_L1', lambda: ops.eval_ktup(U, I, E, P, Pn, R, Rn, i2e_rows, uq, True), 512 * NI),
        ('eval_tup_hard_L1', lambda: ops.eval_tup(U, I, P, Pn, uq, True, PH, None, 7, 0), 512 * NI),
        ('eval_tup_hard_L2', lambda: ops.eval_tup(U, I, P, Pn, uq, False, PH, None, 7, 0), 512 * NI),
        ('eval_transe_L2', lambda: ops.eval_transe(E, R, hq, rq, False, False), 512 * (NE + 1)),
        ('eval_transe_L1', lambda: ops.eval_transe(E, R, hq, rq, True, False), 512 * (NE + 1)),
        ('eval_transh_L2', lambda: ops.eval_transh(E, R, Rn, hq, rq, False, False), 512 * (NE + 1)),
        ('eval_transh_L1', lambda: ops.eval_transh(E, R, Rn, hq, rq, True, False), 512 * (NE + 1)),
        ('eval_transr_L2', lambda: ops.eval_transr(E, R, M, hq, rq, False, False), 512 * (NE + 1)),
        ('eval_bprmf_d64', lambda: ops.eval_bprmf(U64, I64, uq), 512 * NI),
    ]
    cases += [(name, f, pairs, 0) for name, f, pairs in evals]
    out = {}
    from jTransUP.hip.lib import capture as _cap
    with torch.no_grad():
        for name, f, rows, bpr in cases:
            f(); torch.cuda.synchronize(device)
            g = torch.cuda.CUDAGraph()
            with _cap(g):
                for _ in range(inner):
                    f()
            g.replay(); torch.cuda.synchronize(device)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                g.replay()
            b.record(); torch.cuda.synchronize(device)
            ms = a.elapsed_time(b) / (reps * inner)
            out[name] = {'ms_per_launch': round(ms, 5), 'rows_per_launch': rows, 'Grows_per_s': round(rows / ms / 1e6, 3)}
            if bpr:
                out[name]['frac_of_hbm_peak'] = round(rows * bpr / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 3)
    out['note'] = ('forward kernels, tables cache-resident (ml1m shape); frac = algorithmic bytes per row x rows / time / 8 TB/s; '
                   'time = graph replay of back-to-back launches, i.e. including the inter-kernel gap the HIP-event figure of the headline excludes')
    return out


def hbm_traffic(kind, tag=None):
    """HBM bytes per launch from the committed PMC passes (profiles/<tag>_hbm_traffic.json written by tools/collect_profiles.py:
    separate FETCH_SIZE / WRITE_SIZE runs of this same command, read side doubled per MI355X_MICROARCH.md).  The file is
    stamped with the kernel name and a hash of the kernel's sources; a stamp that does not match the tree means the counters
    were taken on another version of the kernel -> (None, reason) instead of a stale number."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, 'profiles', '*_hbm_traffic.json')))
    if tag:
        files = [f for f in files if os.path.basename(f).startswith(tag)]
    for path in reversed(files):
        try:
            with open(path) as f:
                rec = json.load(f)
            e = rec[kind]
        except Exception:      # noqa: BLE001
            continue
        stamp = rec.get('kernel_src_sha16')
        if stamp != kernel_src_sha16():
            return None, 'stale: %s was measured on kernel sources %s, the tree has %s' % (os.path.basename(path), stamp, kernel_src_sha16())
        return e['hbm_bytes_per_launch'], '%s (%s)' % (os.path.basename(path), e.get('kernel', '?'))
    return None, 'no profiles/*_hbm_traffic.json'


def _max_over_ranks(x, device, world):
    t = torch.tensor([x], dtype=torch.float64, device=device)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def _leg_steps(steps, warmup):
    """KTUP_BENCH_LEG_STEPS=<n>: a test hook (tests/test_bench_contract.py runs two ranks on ONE GPU over gloo, where a step of the
    N-GPU legs stages through the host and takes ~100 x what it takes over RCCL): n timed steps, n // 4 + 1 warm-up steps per leg."""
    n = int(os.environ.get('KTUP_BENCH_LEG_STEPS', '0') or 0)
    return (n, n // 4 + 1) if n > 0 else (steps, warmup)


def dp_train_leg(device, world, rank, steps=100, warmup=20):
    """BASELINE config 4 on N GPUs: the KTUP joint training step (ml1m shape, d=100, 7 rec : 3 kg, Adagrad + weight decay + clip)
    as data-parallel replicas -- every rank holds all tables, scores its slice of the global batch, ONE all-reduce of the flat
    gradient bucket (9.7 MB), then the identical clip + step (utils/fast_train.py JointStepper).  Weak scaling = global batch
    512 x N, strong = 512.  The comm / compute split: the same per-rank work without the exchange (a one-rank group: HIP-graph
    replay) and the bucket all-reduce alone."""
    steps, warmup = _leg_steps(steps, warmup)
    import types
    from jTransUP.models import jTransUP as jt
    from jTransUP.utils.fast_train import JointStepper
    from jTransUP.utils.fused_optim import FusedOptimizer
    solo = None
    if world > 1:
        groups = [dist.new_group([r]) for r in range(world)]          # every rank creates every group (collective call)
        solo = groups[rank]
    i_map = {i: i for i in range(NI)}
    new_map = {i: ((i * 4) % NE if i < ALIGNED else -1, i) for i in range(NI)}
    fl = types.SimpleNamespace(margin=1.0, kg_lambda=1.0, clipping_max_value=5.0)
    out = {'backend': dist.get_backend() if world > 1 else 'single process', 'world': world}

    def run(GB, group):
        torch.manual_seed(3)
        m = jt.jTransUPModel(False, D, NU, NI, NE, NR, i_map, new_map, False, False)
        opt = torch.optim.Adagrad(m.parameters(), lr=0.005, weight_decay=1e-5)
        tr = types.SimpleNamespace(fused=FusedOptimizer(opt), parameters=list(m.parameters()), model_target=-1, step=0)
        js = JointStepper(m, tr, fl, GB, group=group)
        gen = torch.Generator().manual_seed(5)                        # every rank draws the same global batches
        mk = lambda hi: torch.randint(0, hi, (steps + warmup, GB), generator=gen).to(device)
        u, pi, ni_, h, t, nh, nt, r = mk(NU), mk(NI), mk(NI), mk(NE), mk(NE), mk(NE), mk(NE), mk(NR)

        def fstep(s):
            if s % 10 < 7:
                js.rec_step(u[s], pi[s], ni_[s])
            else:
                js.kg_step(h[s], t[s], r[s], nh[s], nt[s], r[s])
        for s in range(warmup):
            fstep(s)
        if world == 1:
            ramp_clocks(lambda: [fstep(k) for k in range(10)], device)
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        for s in range(warmup, warmup + steps):
            fstep(s)
        torch.cuda.synchronize(device)
        if world > 1:
            dist.barrier()
        return _max_over_ranks(1e3 * (time.perf_counter() - t0) / steps, device, world), js

    for name, GB in (('weak', 512 * world), ('strong', 512)):
        if GB % world:
            continue
        ms, js = run(GB, None)
        leg = {'global_batch': GB, 'per_rank_batch': GB // world, 'ms_per_step': ms, 'scored_rows_per_s': 2 * GB / (ms * 1e-3),
               'bucket_MB': js.flat.numel() * 4 / 1e6}
        if world > 1:
            leg['ms_per_step_compute_only'], _ = run(GB // world, solo)      # same per-rank work, no exchange (graph replay)
            flat = js.flat
            for _ in range(5):
                dist.all_reduce(flat)
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            for _ in range(50):
                dist.all_reduce(flat)
            torch.cuda.synchronize(device)
            leg['ms_allreduce_only'] = _max_over_ranks(1e3 * (time.perf_counter() - t0) / 50, device, world)
        out[name] = leg
    out['note'] = ('replicas + ONE all-reduce of the flat gradient bucket per step; at ml1m scale every step touches ~20 % of the '
                   'rows, so an all-gather of (ids, row gradients) would move as many bytes as the dense bucket under weak scaling')
    return out


def config5_leg(device, world, rank, steps=100, warmup=10, batch=8192, full=True):
    """BASELINE config 5: KTUP at d=256 on 10 M users x 1 M items x 5 M entities, tables row-sharded over the N ranks
    (row % N), B = 8192 (u, pos, neg) per rank and step, through jTransUP/sharded_ktup.py: every buffer of the step has a
    fixed shape, so the step is graph replays with no host synchronisation -- device-side routing of the batch's distinct ids
    into fixed-capacity wire rows, (N > 1: an id, a row and a gradient all-to-all with EQUAL splits + one fp64 all-reduce), the fused
    KTUP forward / BPR / backward kernel with per-pair row gradients, the segment reduction run twice (norm, then clip +
    row-sparse Adagrad straight from registers).  `ms_per_step` is the host clock around `steps` steps, `ms_per_step_device` the
    time between two HIP events around the same steps.  With fewer than 8 ranks the same tables simply give bigger shards."""
    steps, warmup = _leg_steps(steps, warmup)
    if os.environ.get('KTUP_BENCH_LEG_STEPS'):
        full = False                                   # (the same test hook: tables of 1.25 M / 125 K / 625 K rows per rank)
    from jTransUP import parallel
    from jTransUP.sharded_ktup import ShardedKgStepper, ShardedKtupJoint, ShardedKtupStepper
    d, P, B = 256, 20, batch
    NUs, NIs, NEs = (10_000_000, 1_000_000, 5_000_000) if full else (1_250_000 * world, 125_000 * world, 625_000 * world)
    free, _ = torch.cuda.mem_get_info(device)
    need = 2.2 * (NUs + NIs + NEs) * d * 4 / world
    if free < need:
        return {'skipped': 'needs %.1f GB of device memory per rank' % (need / 1e9)}
    gen = torch.Generator(device=device); gen.manual_seed(3 + rank)

    def table(n):
        t = parallel.ShardedTable(n, d, rank=rank, world=world, device=device)
        t.weight.data.normal_(generator=gen)
        t.weight.data.mul_(1.0 / 16.0)                                 # rows of norm ~1 at d = 256
        return t
    Ut, It, Et = table(NUs), table(NIs), table(NEs)
    small = [torch.nn.Parameter(torch.nn.functional.normalize(torch.randn(P, d, generator=gen, device=device), dim=1)) for _ in range(4)]
    if world > 1:
        for p in small:
            dist.broadcast(p.data, src=0)
    item2ent = torch.randint(0, NEs, (NIs,), generator=torch.Generator(device=device).manual_seed(7), device=device).to(torch.int32)
    out = {'backend': dist.get_backend() if world > 1 else 'single process', 'world': world, 'batch_per_rank': B,
           'rows': {'users': NUs, 'items': NIs, 'entities': NEs}, 'd': d, 'tables_GB_per_rank': (NUs + NIs + NEs) * d * 4 / world / 1e9}

    def run(label, what='rec', kind='adagrad', warm=None, cycle=0, **kw):
        warm = warmup if warm is None else warm
        if os.environ.get('KTUP_BENCH_LEG_STEPS'):
            warm = min(warm, warmup)                   # (test hook: no 1,500-step Adam warm-up at ~0.1 s per gloo step)
        n = steps + warm + (steps + 2 * cycle if cycle else 0)
        rec = ShardedKtupStepper(Ut, It, Et, *small, item2ent, batch=B, kind=kind, lr=0.005, max_norm=5.0, orth=(what != 'rec'), **kw)
        rec.set_feed([torch.randint(0, hi, (n, B), generator=gen, device=device) for hi in (NUs, NIs, NIs)])   # device-fed: the step's own launches walk the columns
        st = rec
        if what != 'rec':       # the kg half of the joint schedule (knowledgable_recommendation.py:345-383) on the same entity shard
            kkw = {k: v for k, v in kw.items() if k != 'fused_apply'}
            kg = ShardedKgStepper(Et, small[2], small[3], batch=B, kind=kind, lr=0.005, max_norm=5.0, margin=1.0, kg_lambda=1.0,
                                  small_state=rec.small_state[2:4], opt_step=rec.opt_step, **kkw)
            ph, pt, oth = (torch.randint(0, NEs, (n, B), generator=gen, device=device) for _ in range(3))
            pr = torch.randint(0, P, (n, B), generator=gen, device=device)
            flip = torch.rand(n, B, generator=gen, device=device) < 0.5       # a corrupted triple keeps its head or its tail
            kg.set_feed([ph, pt, pr, torch.where(flip, oth, ph), torch.where(flip, pt, oth), pr])
            st = kg if what == 'kg' else ShardedKtupJoint(rec, kg, 0.7)
        for _ in range(warm):
            st.run()
        ramp_clocks(st.run, device, world=world)
        torch.cuda.synchronize(device)
        if world > 1:
            dist.barrier()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for _ in range(steps):
            st.run()
        e1.record()
        torch.cuda.synchronize(device)
        wall = _max_over_ranks(1e3 * (time.perf_counter() - t0) / steps, device, world)
        cyc = None
        if cycle and world == 1:         # the same steps in graphs of `cycle` steps (run_cycle): one graph launch per cycle, the next route joined between steps
            st.run_cycle(cycle); st.run_cycle(cycle)
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            for _ in range(steps // cycle):
                st.run_cycle(cycle)
            torch.cuda.synchronize(device)
            cyc = 1e3 * (time.perf_counter() - t0) / (steps // cycle * cycle)
        st.check()
        leg = {'ms_per_step': wall, 'ms_per_step_device': e0.elapsed_time(e1) / steps, 'scored_rows_per_s': 2 * B * world / (wall * 1e-3),
               'wire_rows_per_rank': rec.W if what != 'kg' else st.W, 'graph_segments': len(rec._graphs) if rec._graphs else 0}
        if cyc is not None:
            leg['ms_per_step_in_%d_step_graphs' % cycle] = cyc
        if what != 'rec':
            leg['what'] = {'kg': 'kg steps only (TransH on the entity shard: 2B scored triples per step)',
                           'joint': 'the 7 rec : 3 kg cycle of knowledgable_recommendation.py:320 over shared tables and Adagrad sums'}[what]
            del st
            return leg
        # train-step bytes per scored row = forward (12 d + 24 B ... = 3096 B at d = 256) + 3 gathered rows x 4 d x 3
        alg = 2 * B * (3096 + 3 * 4 * d * 3)
        # what a step must move at least on top of that: parameter + Adagrad state, read and written, of every distinct row
        moved = alg + st.W * d * 4 * 4
        leg['algorithmic_MB'] = alg / 1e6
        leg['hbm_frac_algorithmic'] = alg / (leg['ms_per_step_device'] * 1e-3) / 1e9 / HBM_PEAK_GBS
        leg['hbm_frac_with_optimizer_rows'] = moved / (leg['ms_per_step_device'] * 1e-3) / 1e9 / HBM_PEAK_GBS
        rec.close()
        del st
        return leg
    out.update(run('default', cycle=10))
    out['kg_step'] = run('kg', what='kg')
    out['joint'] = run('joint', what='joint')
    if world == 1:
        out['exchange_form'] = run('exchange', force_exchange=True)   # what ONE rank of a bigger job runs, minus the wire
        out['exchange_form']['note'] = ('the several-ranks route on one rank: the five segments AND the exchanges between them as ONE graph '
                                        '(device copies stand for the three all-to-alls; with RCCL the collectives are captured the same way), '
                                        'rows packed into the wire buffer, the requester reduction stores its rows, the next step\'s route on a second branch')
        out['exchange_form']['joint'] = run('exchange joint', what='joint', force_exchange=True)
    # the published recipe's optimizer (ktup.sh:1: Adam, l2_lambda 0) on the shards: row-sparse Adam with exact catch-up of the steps a row
    # was not touched for (include/ktup_hip.h ktup_adam_t); last, so that a failure here cannot take the figures above with it
    try:
        free, _ = torch.cuda.mem_get_info(device)
        if free > 2.3 * (NUs + NIs + NEs) * d * 4 / world:                # [m | v | last] rows: twice the tables
            # (1,500 untimed steps first: an Adam step costs what its rows have to catch up on, and that grows until every item and entity
            #  row has been touched once -- the steady state of a real run, the timed window of 100 steps right after 10 was not)
            out['joint_adam'] = run('joint adam', what='joint', kind='adam', warm=1500)
            out['joint_adam']['what'] = ('the 7 : 3 cycle with -optimizer_type Adam (row-sparse with catch-up = the dense Adam of utils/trainer.py:63-66), '
                                         'timed after 1,500 steps: every touched item / entity row then owes ~60-110 replayed steps')
        else:
            out['joint_adam'] = {'skipped': 'not enough free device memory for the Adam state'}
    except Exception as e:                                               # noqa: BLE001 -- reported, never fatal for the bench line
        out['joint_adam'] = {'error': '%s: %s' % (type(e).__name__, e)}
    out['note'] = ('top level: the rec step (the round-3 figure); kg_step / joint: the kg half and the 7 : 3 cycle.  One rank: ONE graph per step -- '
                   'fused step, norm walk, apply walk on one queue (the walks carry the small tables and the bookkeeping as extra workgroups) and, '
                   'on a second branch from the step\'s first launch to its last, the ROUTE OF THE NEXT STEP into the other of two buffer sets (two '
                   'graphs alternate); N > 1: the five segments, three equal-split all-to-alls and one fp64 all-reduce (small tables + norm + '
                   'overflow flag) as ONE graph where the collectives can be captured (RCCL), five graphs under gloo; round 3: 0.171, round 5: '
                   '0.129 ms per rec step')
    return out


def config4_sharded_leg(device, world, rank, steps=200, warmup=20):
    """BASELINE config 4 (KTUP, ml1m shape, d = 100, global batch 512, 7 rec : 3 kg) through the ROW-SHARDED steppers instead of
    replicas (-shard_tables at ml1m scale): the replicated route exchanges the dense 9.6 MB gradient bucket per step whatever the batch
    (dp_train_step), this one only the rows a step touches -- ~3,000 distinct rows of 400 B in, out and back over equal-split
    all-to-alls that use all links at once, plus the fp64 bucket of the four 20-row tables.  Exact for Adagrad / plain SGD without
    weight decay (what the row-sparse update can reproduce).  One rank: the same launches without the wire -- a latency chain of ~9
    launches on 64 pairs' worth of tiles, slower than the dense 2-launch step; the point of the leg is its curve over N."""
    steps, warmup = _leg_steps(steps, warmup)
    from jTransUP import parallel
    from jTransUP.sharded_ktup import ShardedKtupJoint
    if 512 % world:
        return {'skipped': 'global batch 512 is not divisible by %d ranks' % world}
    d, P, B = D, NR, 512 // world
    gen = torch.Generator(device=device); gen.manual_seed(3)          # the same tables on every rank's generator: shards of ONE model

    def table(n, pad_last=False):
        full = torch.nn.functional.normalize(torch.randn(n, d, generator=gen, device=device), dim=1)
        if pad_last:
            full[-1].zero_()                                       # the entity table's pad row (jTransUP.py:46,96): items without an entity
        return parallel.ShardedTable(n, d, rank=rank, world=world, device=device, init=lambda g: full[g.to(device)])
    Ut, It, Et = table(NU), table(NI), table(NE + 1, pad_last=True)
    small = [torch.nn.Parameter(torch.nn.functional.normalize(torch.randn(P, d, generator=gen, device=device), dim=1)) for _ in range(4)]
    # (4 i + i % 4, not the 4 i of the one-GPU legs: entity ids that are all multiples of 4 would all live on ONE of 2 or 4 owners of
    #  a row % N sharding and overflow its wire rows -- a real item -> entity map has no such pattern)
    ar = torch.arange(NI, device=device)
    item2ent = torch.where(ar < ALIGNED, (ar * 4 + ar % 4) % NE, torch.full((NI,), NE, device=device)).to(torch.int32)
    joint = ShardedKtupJoint.build(Ut, It, Et, *small, item2ent, batch=B, joint_ratio=0.7, margin=1.0, kg_lambda=1.0, kind='adagrad', lr=0.005,
                                   max_norm=5.0, ent_pad=NE)
    n = steps + warmup
    g2 = torch.Generator(device=device); g2.manual_seed(11 + rank)
    joint.rec.set_feed([torch.randint(0, hi, (n, B), generator=g2, device=device) for hi in (NU, NI, NI)])
    ph, pt, oth = (torch.randint(0, NE, (n, B), generator=g2, device=device) for _ in range(3))
    pr = torch.randint(0, P, (n, B), generator=g2, device=device)
    flip = torch.rand(n, B, generator=g2, device=device) < 0.5
    joint.kg.set_feed([ph, pt, pr, torch.where(flip, oth, ph), torch.where(flip, pt, oth), pr])
    for _ in range(warmup):
        joint.run()
    ramp_clocks(joint.run, device, world=world)
    torch.cuda.synchronize(device)
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        joint.run()
    torch.cuda.synchronize(device)
    wall = _max_over_ranks(1e3 * (time.perf_counter() - t0) / steps, device, world)
    joint.check()
    joint.close()
    return {'backend': dist.get_backend() if world > 1 else 'single process', 'world': world, 'global_batch': 512, 'per_rank_batch': B,
            'ms_per_step': wall, 'scored_rows_per_s': 2 * 512 / (wall * 1e-3), 'wire_rows_per_rank': {'rec': joint.rec.W, 'kg': joint.kg.W},
            'optimizer': 'row-sparse Adagrad, l2_lambda 0 (the replicated route of dp_train_step runs dense Adagrad with weight decay)',
            'note': 'strong scaling of the reference batch: B = 512 / N pairs or triples per rank and step'}


def key_figures(out):
    """The figures the rounds' targets are stated in, once more and compactly, as the LAST object of the JSON line (a reader who keeps
    only the line's tail still sees them); every value is copied from the leg that measured it."""
    def get(*path):
        v = out
        for k in path:
            if not isinstance(v, dict) or k not in v:
                return None
            v = v[k]
        return v
    kf = {
        'scoring_rows_per_s': out.get('value'), 'K6_frac_of_fp32_pipe': get('roofline', 'frac'),
        'eval_full_pass_ms': get('eval_all_item_hit10', 'full_pass_ms'),
        'eval_sweep_device_ms': get('eval_all_item_hit10', 'fused_pass', 'device_ms_scores_and_topk'),
        'eval_sweep_frac_of_fp32_peak': get('eval_all_item_hit10', 'fused_pass', 'gemm_frac_of_fp32_peak'),
        'train_step_b512_ms': {k: get('train_step_b512', 'ms_per_step_' + k) for k in ('gpu_resident', 'device_fed_x10', 'fused', 'torch')},
        'forward_b512_rows_per_s': get('forward_b512', 'scored_rows_per_s'),
        'cli_steps_per_s': get('cli_steps_per_s', 'steps_per_s'),
        'config5_ms': {'rec': get('config5_step', 'ms_per_step'), 'kg': get('config5_step', 'kg_step', 'ms_per_step'),
                       'joint': get('config5_step', 'joint', 'ms_per_step'), 'exchange_form': get('config5_step', 'exchange_form', 'ms_per_step'),
                       'exchange_form_joint': get('config5_step', 'exchange_form', 'joint', 'ms_per_step'),
                       'joint_adam': get('config5_step', 'joint_adam', 'ms_per_step')},
        'config5_rec_hbm_frac_algorithmic': get('config5_step', 'hbm_frac_algorithmic'),
        'K6_d256_hbm_resident_frac': get('roofline_hbm_resident', 'd256', 'frac_of_hbm_peak') or get('roofline_hbm_resident', 'frac'),
        'kg_pass_transe_ms': get('eval_kg_transe', 'full_pass_ms'),
        'dp_train_step_ms': get('dp_train_step', 'ms_per_step'),
    }
    return {k: v for k, v in kf.items() if v is not None}


def cli_throughput_leg(steps=3000, timeout_s=300):
    """The drop-in command line end to end (tools/cli_throughput.py): run_knowledgable_recommendation.py -model_type jtransup (d = 100, B = 512,
    joint_ratio 0.7, -device_sampling) on an ml1m-SHAPED dataset written in the reference's file formats, training steps per second over an
    interval between two periodic evaluations (one evaluation pass and a checkpoint included), in a process of its own.  Round 5's line did
    not carry this figure and a 1.7 x regression of it went unnoticed for two rounds."""
    import re
    import subprocess
    tool = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'tools', 'cli_throughput.py')
    try:
        r = subprocess.run([sys.executable, tool, str(steps), 'dev'], capture_output=True, text=True, timeout=timeout_s)
    except subprocess.TimeoutExpired:
        return {'error': 'timeout after %d s' % timeout_s}
    m = re.search(r'dev\s+sampling:\s+(\d+) steps/s', r.stdout)
    b = re.search(r'fastest of (\d+) intervals\s+(\d+) steps/s; per interval \[total, rec pass, kg pass, checkpoint \+ steps\] s: (.*)', r.stdout)
    if r.returncode != 0 or not m:
        return {'error': (r.stdout + r.stderr)[-400:]}
    out = {'steps_per_s': float(m.group(1)), 'scored_rows_per_s': float(m.group(1)) * 1024, 'steps_per_interval': steps,
           'what': 'run_knowledgable_recommendation.py jtransup d=100 B=512 -device_sampling, first interval after the step-0 evaluation '
                   '(evaluation passes + checkpoint included); round 3: 20,408, rounds 4-5: 11,450 / 11,765 (a full gc.collect() before every graph capture)'}
    if b:
        out['fastest_interval_steps_per_s'] = float(b.group(2))
        out['intervals_s_total_rec_kg_rest'] = b.group(3)
    return out


def roofline(rec_ms, kg_ms, step_ms=None, live_traffic=None):
    """The dominant kernel (K6, KTUP rec forward) against the ceiling that actually binds it.

    SURVEY 8(d)'s figure -- ALGORITHMIC bytes per launch / HIP-event time / 8 TB/s -- is kept as `hbm_algorithmic.frac_algorithmic`
    (north_star's ">= 70 % at ml1m shape" refers to it).  It is NOT an HBM measurement at this shape: the 9.7 MB of tables live in
    L2 / Infinity Cache, so the same formula exceeds 1 for the lighter kernels.  `bound` therefore comes from the counters: HBM
    traffic (live rocprofv3 pass of this very command when available, else the committed profile) below half the algorithmic
    bytes means the memory system is not what the kernel waits for, and the ceiling is the fp32 pipe that MFMA and VALU share
    ("mfma": useful flops per pair against 157.3 TF/s); `achieved / peak / unit / frac` are quoted against THAT ceiling.
    `step_algorithmic_over_peak` > 1 flags, in the line itself, that the whole step's algorithmic bytes / time exceeds the HBM peak
    (= cache-resident, not a bandwidth claim).  The honest HBM-bound companion is `roofline_hbm_resident` (tables x1000 rows)."""
    t = rec_ms * 1e-3
    ach = REC_ROWS * BYTES_REC / t / 1e9
    tf = REC_ROWS * FLOP_REC / t / 1e12
    t_hbm, t_fp32 = REC_ROWS * BYTES_REC / (HBM_PEAK_GBS * 1e9), REC_ROWS * FLOP_REC / (FP32_PEAK_TFLOPS * 1e12)
    if live_traffic is not None:
        traffic, tnote = live_traffic
    else:
        traffic, tnote = hbm_traffic('ktup_rec_forward')
    tables_bytes = (NU + NI + NE + 1 + 4 * NR) * D * 4
    ratio = None if traffic is None else traffic / (REC_ROWS * BYTES_REC)
    hbm_bound = (ratio >= 0.5) if ratio is not None else (tables_bytes > 256e6)      # no counters: Infinity Cache holds 256 MB
    out = {'bound': 'hbm' if hbm_bound else 'mfma',
           'kernel': 'pref_fwd_mc_kernel<McGeom<25,5,true,false>,false> (KTUP rec forward, K6)',
           'achieved': ach if hbm_bound else tf, 'peak': HBM_PEAK_GBS if hbm_bound else FP32_PEAK_TFLOPS,
           'unit': 'GB/s' if hbm_bound else 'TFLOP/s', 'frac': (ach / HBM_PEAK_GBS) if hbm_bound else (tf / FP32_PEAK_TFLOPS),
           'bound_decided_by': ('HBM traffic / algorithmic bytes = %.2f (%s)' % (ratio, tnote)) if ratio is not None else
                               ('no counters: tables are %.1f MB, %s the 256 MB Infinity Cache' % (tables_bytes / 1e6, 'beyond' if hbm_bound else 'inside')),
           'traffic': traffic, 'traffic_source': tnote,
           'traffic_frac_of_hbm_peak': None if traffic is None else traffic / t / 1e9 / HBM_PEAK_GBS,
           'traffic_over_algorithmic': ratio,
           'hbm_algorithmic': {'achieved': ach, 'peak': HBM_PEAK_GBS, 'unit': 'GB/s', 'frac_algorithmic': ach / HBM_PEAK_GBS,
                               'is': 'SURVEY 8(d): algorithmic bytes per launch / launch time / 8 TB/s -- cache-resident tables, not a bandwidth measurement'},
           'fp32': {'achieved_tflops': tf, 'peak_tflops': FP32_PEAK_TFLOPS, 'frac': tf / FP32_PEAK_TFLOPS, 'flop_per_row': FLOP_REC},
           'min_time_us': {'hbm_algorithmic': 1e6 * t_hbm, 'fp32': 1e6 * t_fp32},
           'bytes_per_row': BYTES_REC, 'rows_per_launch': REC_ROWS, 'ms_per_launch': rec_ms,
           'kg_kernel': {'kernel': 'transh_fwd_tile_kernel<25,true> (K3)', 'ms_per_launch': kg_ms,
                         'achieved': KG_ROWS * BYTES_KG / (kg_ms * 1e-3) / 1e9,
                         'frac_algorithmic': KG_ROWS * BYTES_KG / (kg_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                         'fp32_frac': KG_ROWS * FLOP_KG / (kg_ms * 1e-3) / 1e12 / FP32_PEAK_TFLOPS,
                         'note': 'algorithmic bytes; > 1 is possible because the entity table is cache-resident'}}
    if step_ms is not None:
        over = (REC_ROWS * BYTES_REC + KG_ROWS * BYTES_KG) / (step_ms * 1e-3) / 1e9 / HBM_PEAK_GBS
        out['step_algorithmic_over_peak'] = over
        out['step_algorithmic_over_peak_means'] = ('> 1: the step cannot be HBM-bound at this shape (tables are cache-resident)' if over > 1
                                                   else '<= 1')
    return out


def live_hbm_traffic(kernel_sub='pref_fwd_mc_kernel', timeout_s=150, child_args=('--steps', '5', '--warmup', '2', '--no-extras')):
    """HBM bytes per K6 launch measured NOW: two child runs of this very command under rocprofv3 (--pmc FETCH_SIZE, then --pmc
    WRITE_SIZE: separate passes, kernel trace only, from /tmp -- MI355X_MICROARCH.md), KB units, read side doubled (gfx950).
    -> (bytes, note) or None when rocprofv3 is missing, switched off (KTUP_BENCH_PMC=0) or a pass fails."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    if os.environ.get('KTUP_BENCH_PMC', '1') == '0' or os.environ.get('KTUP_BENCH_CHILD') or not shutil.which('rocprofv3'):
        return None
    tot = {}
    for counter in ('FETCH_SIZE', 'WRITE_SIZE'):
        d = tempfile.mkdtemp(prefix='ktup_pmc_', dir='/tmp')
        try:
            env = dict(os.environ, TMPDIR='/tmp', KTUP_BENCH_CHILD='1')
            cmd = ['rocprofv3', '--kernel-trace', '--pmc', counter, '--output-format', 'csv', '-d', d, '--', sys.executable,
                   os.path.join(ROOT, 'bench.py')] + list(child_args)
            r = subprocess.run(cmd, cwd='/tmp', env=env, capture_output=True, text=True, timeout=timeout_s)
            hits = glob.glob(os.path.join(d, '**', '*counter_collection.csv'), recursive=True)
            if r.returncode != 0 or not hits:
                return None
            per = {}
            with open(hits[0]) as f:
                for row in csv.DictReader(f):
                    if row['Counter_Name'] == counter and kernel_sub in row['Kernel_Name']:
                        per[row['Dispatch_Id']] = per.get(row['Dispatch_Id'], 0.0) + float(row['Counter_Value'])
            if not per:
                return None
            tot[counter] = sum(per.values()) / len(per) * 1024.0
        except Exception:      # noqa: BLE001
            return None
        finally:
            shutil.rmtree(d, ignore_errors=True)
    return int(2.0 * tot['FETCH_SIZE'] + tot['WRITE_SIZE']), 'live: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this command, read side doubled'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=200)       # a step is ~0.17 ms: 200 steps = 35 ms of timed work
    ap.add_argument('--warmup', type=int, default=50)       # long enough for the clocks to settle
    ap.add_argument('--full', action='store_true',
                    help='also the roofline, the CPU baselines, the side measurements and the N-GPU legs (a plain run times the headline only)')
    ap.add_argument('--no-extras', action='store_true', help='with --full: skip cpu_baseline / train-step / eval side measurements')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='after the timed steps, write the last step\'s scores as DIR/scores_rec.npy and DIR/scores_kg.npy (float32)')
    ap.add_argument('--only', default=None, choices=['gather_stress', 'gather_stress_rec'],
                    help='profiling hook: run only this side measurement (for a rocprofv3 pass) and print its JSON')
    args = ap.parse_args()
    extras = args.full and not args.no_extras

    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local = int(os.environ.get('LOCAL_RANK', '0'))
    if not torch.cuda.is_available():
        raise SystemExit('bench.py needs an MI355X (no CPU fallback: the HIP library is the product)')
    if world > 1:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        # "nccl" is RCCL on ROCm.  KTUP_BENCH_BACKEND=gloo is a test hook: it lets the world > 1 code path run with several
        # ranks sharing the one GPU of a single-GPU box (RCCL refuses duplicate devices).
        dist.init_process_group(os.environ.get('KTUP_BENCH_BACKEND', 'nccl'), rank=rank, world_size=world)
    local = local % torch.cuda.device_count()
    device = torch.device('cuda', local)
    torch.cuda.set_device(device)

    from jTransUP.hip import ops
    if args.only == 'gather_stress':
        print(json.dumps({'gather_stress_x1000': gather_stress_bench(device, reps=10)}))
        return
    if args.only == 'gather_stress_rec':             # the counter pass of roofline_hbm_resident: K6 on the x1000 tables, default loads only
        print(json.dumps({'gather_stress_x1000': gather_stress_bench(device, reps=5, only_rec=True)}))
        return
    W, i2e, idx = build_world(3 + rank, device)          # seed 3 like every recipe (swipe.sh); per-rank row shard
    D_ = {k: v.to(device) for k, v in W.items()}
    i2e_d = i2e.to(device, torch.int32)
    X = {k: v.to(device) for k, v in idx.items()}

    # The step = ktup_pref_prepare + ktup_score_ktup_fwd + ktup_score_transh_fwd through the C ABI on fixed buffers.
    # Launches are pre-bound (lib.bind): per-call Python marshalling (~50 us through the autograd wrappers) would leave the
    # GPU idle between kernels and the HIP events around a launch would then time the host, not the kernel.
    # The rec branch (prepare + K6) and the KG branch (K3) of a step are independent: they run on two HIP streams, so the
    # gather-bound K3 fills what the fp32-pipe-bound K6 leaves idle (121 us per step against 133 us back to back).
    from jTransUP.hip import lib as L
    stream = torch.cuda.current_stream(device).cuda_stream
    side = torch.cuda.Stream(device=device)
    ws = ops.pref_workspace(D_['P'], D_['Pn'], D_['R'], D_['Rn'])
    s_rec = torch.empty(REC_ROWS, dtype=torch.float32, device=device)
    s_kg = torch.empty(KG_ROWS, dtype=torch.float32, device=device)
    P_ = D_['P']
    prep = L.bind('ktup_pref_prepare', P_.data_ptr(), D_['Pn'].data_ptr(), D_['R'].data_ptr(), D_['Rn'].data_ptr(), P_.stride(0),
                  P_.shape[0], P_.shape[1], ws.data_ptr(), stream)
    rec = L.bind('ktup_score_ktup_fwd', D_['U'].data_ptr(), D_['U'].stride(0), D_['I'].data_ptr(), D_['I'].stride(0),
                 D_['E'].data_ptr(), D_['E'].stride(0), i2e_d.data_ptr(), ws.data_ptr(), P_.shape[0], D, X['u'].data_ptr(),
                 X['i'].data_ptr(), REC_ROWS, 0, ops.GUMBEL_OFF, None, 0, 0, s_rec.data_ptr(), stream)
    kg = L.bind('ktup_score_transh_fwd', D_['E'].data_ptr(), D_['E'].stride(0), D_['R'].data_ptr(), D_['R'].stride(0),
                D_['Rn'].data_ptr(), D_['Rn'].stride(0), D_['R'].shape[0], D, X['h'].data_ptr(), X['t'].data_ptr(),
                X['r'].data_ptr(), KG_ROWS, 0, s_kg.data_ptr(), side.cuda_stream)
    if args.full:
        with torch.no_grad():    # the bound launches must agree with the autograd wrappers the models use
            ref_rec = ops.score_ktup(D_['U'], D_['I'], D_['E'], D_['P'], D_['Pn'], D_['R'], D_['Rn'], i2e_d, X['u'], X['i'], False)
            ref_kg = ops.score_transh(D_['E'], D_['R'], D_['Rn'], X['h'], X['t'], X['r'], False)
            prep(); rec(); kg()
            torch.cuda.synchronize(device)
            assert torch.equal(ref_rec, s_rec) and torch.equal(ref_kg, s_kg), 'bound launches disagree with ops.*'

    def barrier():
        if world > 1:
            dist.barrier()

    # The events of the timed region exist (and have been recorded once: torch creates the HIP event at its first record) BEFORE the
    # ramp and the warm-up steps: whatever the host does between the warm-up and the timed region is idle time on the device, and the
    # chip answers an idle gap of a few hundred microseconds with ~25 ms of lowered clocks (per-step event timeline, round 6: period
    # 0.139 -> 0.155 -> 0.125 ms over the first 200 steps after a 0.4 ms gap, 0.1218 without one).
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
    _dump = bool(os.environ.get('KTUP_DUMP_EV'))
    evk = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)] if _dump else None
    for a_, b_ in ev:
        a_.record(); b_.record()
    torch.cuda.synchronize(device)
    # clock ramp (untimed, like the warm-up steps, whatever --warmup says): a fresh device / process needs load before it holds its
    # clocks -- 80 ms was not enough on a box's FIRST run (0.1375 ms per step against 0.123 on the second and third): run windows of 40
    # steps until two in a row are within 1 % of the best seen, at least 0.25 s, at most 2 s
    t_ramp, best_w, settled = time.perf_counter(), None, 0
    ramp_min_s = float(os.environ.get('KTUP_RAMP_MIN_S', '0.25'))
    ramp_win = int(os.environ.get('KTUP_RAMP_WIN', '40'))
    ramp_log = []
    while True:
        t_w = time.perf_counter()
        for _ in range(ramp_win):
            prep(); rec(); kg()
        torch.cuda.synchronize(device)
        w_ms = time.perf_counter() - t_w
        ramp_log.append(round(1e3 * w_ms / ramp_win, 4))
        settled = settled + 1 if (best_w is not None and w_ms <= 1.01 * best_w) else 0
        best_w = w_ms if best_w is None else min(best_w, w_ms)
        el = time.perf_counter() - t_ramp
        if (settled >= 2 and el > ramp_min_s) or el > max(2.0, 2 * ramp_min_s):
            break
    if os.environ.get('KTUP_RAMP_LOG'):
        print('ramp', len(ramp_log), ramp_log[:6], ramp_log[-12:], file=sys.stderr)
    for _ in range(args.warmup):
        prep(); rec(); kg()
    barrier(); torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    for s in range(args.steps):                         # the timed region: exactly K steps
        prep()
        ev[s][0].record(); rec(); ev[s][1].record()     # HIP events around the dominant kernel's launch, on its stream
        if _dump:
            evk[s][0].record(side)
        kg()
        if _dump:
            evk[s][1].record(side)
    torch.cuda.synchronize(device); barrier()
    dt = time.perf_counter() - t0
    if _dump:
        z = ev[0][0]
        for s in range(args.steps):
            print('ev', s, round(z.elapsed_time(ev[s][0]), 4), round(z.elapsed_time(ev[s][1]), 4), round(z.elapsed_time(evk[s][0]), 4),
                  round(z.elapsed_time(evk[s][1]), 4), file=sys.stderr)
    if args.dump_outputs:                               # the last timed step's scores, before anything else launches
        import numpy as np
        os.makedirs(args.dump_outputs, exist_ok=True)
        tag = '' if world == 1 else '_rank%d' % rank
        np.save(os.path.join(args.dump_outputs, 'scores_rec%s.npy' % tag), s_rec.cpu().numpy().astype(np.float32))
        np.save(os.path.join(args.dump_outputs, 'scores_kg%s.npy' % tag), s_kg.cpu().numpy().astype(np.float32))
    if args.full:
        ek = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(20)]
        for a_, b_ in ek:                               # the KG-branch kernel alone, timed after the region on its own stream
            a_.record(side); kg(); b_.record(side)
        torch.cuda.synchronize(device)
        eu = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(20)]
        for a_, b_ in eu:                               # ... and K6 alone (in the region it shares the chip with K3)
            a_.record(); rec(); b_.record()
        torch.cuda.synchronize(device)
        rec_alone_ms = sum(a.elapsed_time(b) for a, b in eu) / len(eu)
    tmax = torch.tensor([dt], device=device)
    if world > 1:
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
    dt = float(tmax.item())
    rows = (REC_ROWS + KG_ROWS) * world
    out = {
        'metric': 'scored (u,i)+(h,r,t) triples/sec at d=100 (KTUP forward scoring, ml1m shape)',
        'value': rows * args.steps / dt, 'unit': 'scored rows/s', 'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup,
        'ms_per_step': 1e3 * dt / args.steps, 'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None,
        'dtype': 'f32', 'data': 'synthetic',
        'config': {'workload': 'configs[3] KTUP (jtransup) ml1m shape d=100, soft gate, squared-L2, noshare: per GPU and step '
                               '716800 (u,i) pairs + 307200 (h,t,r) triples (= 2000 batches of 512 at joint_ratio 0.7), '
                               'tables replicated per GPU', 'rows_per_step_per_gpu': REC_ROWS + KG_ROWS,
                   'users': NU, 'items': NI, 'entities': NE, 'relations': NR, 'd': D},
        'roofline': None,
    }
    if args.full:
        rec_ms = sum(a.elapsed_time(b) for a, b in ev) / args.steps
        kg_ms = sum(a.elapsed_time(b) for a, b in ek) / len(ek)
        live = live_hbm_traffic() if (rank == 0 and world == 1 and extras) else None
        out['roofline'] = roofline(rec_ms, kg_ms, step_ms=1e3 * dt / args.steps, live_traffic=live)
        out['roofline']['ms_per_launch_alone'] = rec_alone_ms
        out['roofline']['note'] = ('ms_per_launch / achieved: HIP events around K6 inside the timed region, where the KG branch (K3) runs '
                                   'concurrently on a second stream; ms_per_launch_alone: the same launch with the chip to itself')
    if rank == 0 and world == 1 and extras:
        keep = {}
        out['eval_all_item_hit10'] = eval_bench(device, keep=keep)   # before the CPU baselines: their OpenMP pools disturb host-side timing
        out['train_step_b512'] = train_step_bench(device)
        out['forward_b512'] = forward_b512_bench(device, D_, i2e_d, X)
        out['variants'] = variants_bench(device, D_, i2e_d, X)
        out['gather_stress_x1000'] = gather_stress_bench(device)
        live_gs = live_hbm_traffic(child_args=('--only', 'gather_stress_rec'), timeout_s=240)
        out['roofline_hbm_resident'] = roofline_hbm_resident(out['gather_stress_x1000'], live=live_gs)
        out['roofline_hbm_resident']['d256'] = out['gather_stress_x1000'].get('ktup_rec_forward_d256')
        out['cpu_baseline'] = cpu_baseline(W, i2e, idx)
        out['train_step_b512']['cpu_baseline'] = cpu_train_step_baseline(out['cpu_baseline']['cores'])
        out['eval_kg_transe'] = eval_kg_bench(device)
        out['eval_tup_hard_gate'] = eval_tup_hard_bench(device)
        out['eval_ktup_l1'] = eval_ktup_l1_bench(device)
        out['eval_all_item_hit10']['cpu_baseline'] = cpu_eval_baseline(keep['m'], keep['users'], keep['gold'], keep['train'], keep['rows'])
        out['cli_steps_per_s'] = cli_throughput_leg()
    elif args.full and rank == 0:
        out['cpu_baseline'] = None
    if extras:
        # the N-GPU legs the scoring headline cannot show (it has no exchange step): config 4's data-parallel training step and
        # config 5's row-sharded step, each with its comm / compute split (every rank takes part; rank 0 reports)
        legs = {}

        def give_up():          # a rank stuck in a leg's collective must not take the headline line down with it
            if rank == 0:
                done = dict(out)
                for name in ('dp_train_step', 'config4_sharded_step', 'config5_step'):
                    done[name] = legs.get(name, {'error': 'timeout after %d s' % LEG_TIMEOUT_S})
                print(json.dumps(done), flush=True)
            os._exit(0)

        watchdog = threading.Timer(LEG_TIMEOUT_S, give_up)
        watchdog.daemon = True
        watchdog.start()
        for name, fn in (('dp_train_step', dp_train_leg), ('config4_sharded_step', config4_sharded_leg), ('config5_step', config5_leg)):
            try:
                t_leg = time.perf_counter()
                legs[name] = fn(device, world, rank)
                if isinstance(legs[name], dict):
                    legs[name]['leg_wall_s'] = round(time.perf_counter() - t_leg, 1)      # set-up + ramp + timed steps of the whole leg
            except Exception as e:      # noqa: BLE001 -- a leg must not take the headline line down with it
                legs[name] = {'error': '%s: %s' % (type(e).__name__, e)}
        watchdog.cancel()
        if rank == 0:
            out.update(legs)
    if rank == 0:
        out['key_figures'] = key_figures(out)          # LAST: what a truncated tail of the line still shows
        print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
