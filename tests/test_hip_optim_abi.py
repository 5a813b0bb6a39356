"""GPU parity of the dense optimizer launches (csrc/ktup_optim.hip) through the C ABI (jTransUP.hip.lib.call) against
tests/_optim_ref.py: fp64 from the same fp32 inputs, every element of p, g, state1 and state2 at C x 2^-24 x scale (derived in the
reference module, pinned on the CPU by tests/test_optim_ref_host.py), the squared norm at (4k + 8) x 2^-24.  Every case is one
launch from injected state (ktup_optim_clip_step) or the two launches ktup_optim_gradnorm + ktup_optim_step; the sequences are
test_workspace_reuse and test_graph_replay.  Exact facts asserted next to the tolerances: guard floats around every tensor
bit-identical; gradients bit-identical without clipping, g x 1.0f at coef == 1, exactly zero with zero_grads; arrays the kind
does not use untouched; ws[KTUP_OPTIM_WS_DOUBLES - 1] == 0 after every ktup_optim_clip_step.  Each case prints its largest
error / tolerance per buffer; test_zz_report prints the largest per kind.

Not covered: tensors near 2^32 elements (16 GiB per array; only the refusal of a claimed 2^32 is), a non-zero barrier-timeout
word (a timeout cannot be provoked deliberately), capacities other than this device's."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _optim_ref as R
from tests._optim_cases import (FOUR, GRID_LABELS, REUSE, SHAPES, STRIDE, VARIANTS, acc_case, adam_case, gnorm_case, graph_case,
                                grid_case, hyper_case, loss_case, refused_case, reuse_case, seed_of, stride_case, tail_weight_case,
                                tails_case, vid, zero_case, zero_grads_case)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
WS_DOUBLES = 784                                                      # KTUP_OPTIM_WS_DOUBLES
GNORM_DOUBLES, GNORM_SLOTS, GNORM_SET0 = 64, 16, 8                    # KTUP_GNORM_WS_DOUBLES, csrc/ktup_common.h
ROUTES = ('two', 'one')                                               # gradnorm + step / clip_step
WORST = {}                                                            # kind -> {buffer: largest error / tolerance of the module}


# ------------------------------------------------------------------------------------------------ launching
def lib():
    from jTransUP.hip import lib as L
    return L


def capacity(kind):
    cap = lib().load().ktup_optim_clip_step_capacity(kind)
    assert 8 <= cap <= 512 and cap % 4 == 0, cap                      # (a unit is a quarter chunk: tests/_optim_cases.grid_chunks)
    return cap


def stream():
    return torch.cuda.current_stream().cuda_stream


def arr(ctype, vals):
    vals = list(vals)
    return (ctype * max(len(vals), 1))(*vals)


class Device:
    """The flat buffers of a case on the GPU and the pointer arrays into them."""

    def __init__(self, c):
        self.c = c
        self.buf = {k: torch.from_numpy(c['bufs'][k]).to(DEV) for k in R.NAMES}

    def ptrs(self, name, null=(), shift=None):
        base = self.buf[name].data_ptr()
        vals = [None if i in null else base + 4 * s + (shift or {}).get(i, 0) for i, s in enumerate(self.c['starts'])]
        return arr(ctypes.c_void_p, vals)

    def download(self):
        torch.cuda.synchronize()
        return {k: self.buf[k].cpu().numpy() for k in R.NAMES}


def head(c, d, steps=None, steps_dev=None, **ptr_kw):
    h = c['hyper']
    pk = lambda name: ptr_kw.get(name, {})
    return (c['kind'], len(c['sizes']), d.ptrs('p', **pk('p')), d.ptrs('g', **pk('g')), d.ptrs('s1', **pk('s1')), d.ptrs('s2', **pk('s2')),
            arr(ctypes.c_int64, c['sizes']), arr(ctypes.c_int64, c['steps'] if steps is None else steps), steps_dev,
            arr(ctypes.c_int32, c['first'])) + tuple(float(h[k]) for k in ('lr', 'wd', 'momentum', 'beta1', 'beta2', 'eps', 'alpha'))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check(c, got, ref, k, extra_tol=None, note=''):
    """Tolerances (R.compare: every element, guards included) and the exact facts about gradients and unused arrays."""
    def report(worst, C):
        print('%-8s %s%s  ' % (R.KIND_NAMES[c['kind']], c['sizes'] if len(c['sizes']) <= 5 else '%d tensors' % len(c['sizes']), note)
              + '  '.join('%s %.3f of C = %g' % (n, worst[n], C[n]) for n in R.NAMES))
        w = WORST.setdefault(R.KIND_NAMES[c['kind']], dict.fromkeys(R.NAMES, 0.0))
        for n in R.NAMES:
            w[n] = worst[n] if not worst[n] <= w[n] else w[n]                    # (keeps a NaN)
    R.compare(c, got, ref, k, report=report, extra_tol=extra_tol)
    use = dict(zip(('s1', 's2'), R.uses(c['kind'], c['hyper'])))
    for t_in, t_got, out in zip(R.tensors_of(c), R.tensors_of(c, got), ref['outs']):
        if c['zero_grads']:
            assert not bits(t_got['g']).any()                                    # +0.0 everywhere
        elif float(c['max_norm']) <= 0.0 or ref['coef'] == 1.0:
            assert np.array_equal(bits(t_got['g']), bits(t_in['g']))             # untouched, or g x 1.0f
        for name in ('s1', 's2'):
            if not use[name]:
                assert np.array_equal(bits(t_got[name]), bits(t_in[name]))
        if np.array_equal(out['p'][0], t_in['p'].astype(np.float64)):            # the reference update is exactly 0
            assert np.array_equal(bits(t_got['p']), bits(t_in['p']))


def check_sumsq(got, want, k, what):
    bound = R.norm_bound(k) * want
    print('%s got %.17g want %.17g: error %.3g of the bound %.3g (k = %d)' % (what, got, want, abs(got - want), bound, k))
    assert abs(got - want) <= bound, what


def new_ws():
    return torch.zeros(WS_DOUBLES, dtype=torch.float64, device=DEV)


def check_ws(ws, ref, c, k):
    host = ws.cpu().numpy()
    assert host.view(np.uint64)[WS_DOUBLES - 1] == 0                             # no barrier timeout
    if float(c['max_norm']) > 0.0:
        check_sumsq(float(host[0]), ref['sumsq'], max(k, 1), 'ws[0]')
    # the barrier's scratch is back to zero: slot sums, slot tickets, the global ticket
    assert not host.view(np.uint64)[1:1 + 32 * 8 + 32 * 8 + 8].any()
    return host


def run(c, route, ws=None, steps=None, steps_dev=None, note=''):
    """One case through one route, compared with the reference.  Returns the reference."""
    L = lib()
    d = Device(c)
    mx = float(c['max_norm'])
    ref = R.expected(c)
    if route == 'two':
        k = R.float4_per_thread('gradnorm', c['sizes'])
        sumsq = torch.tensor([-3.0, -5.0, -9.0], dtype=torch.float64, device=DEV)
        L.call('ktup_optim_gradnorm', len(c['sizes']), d.ptrs('g'), arr(ctypes.c_int64, c['sizes']), sumsq.data_ptr() + 8, stream())
        L.call('ktup_optim_step', *head(c, d, steps, steps_dev), sumsq.data_ptr() + 8 if mx > 0.0 else None, mx, c['zero_grads'], stream())
        got = d.download()
        s = sumsq.cpu().numpy()
        assert s[0] == -3.0 and s[2] == -9.0
        if ref['sumsq'] == 0.0:
            assert s[1] == 0.0
        else:
            check_sumsq(float(s[1]), ref['sumsq'], k, 'gradnorm')
    else:
        k = R.float4_per_thread('clip_step', c['sizes'], capacity(c['kind']))
        ws = new_ws() if ws is None else ws
        L.call('ktup_optim_clip_step', *head(c, d, steps, steps_dev), ws.data_ptr(), None, mx, c['zero_grads'], None, 0, 0.0, None, None, stream())
        got = d.download()
        check_ws(ws, ref, c, k)
    check(c, got, ref, k, note=' ' + route + note)
    return ref


# ------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize('variant', FOUR, ids=vid)
@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('shape', list(SHAPES))
def test_tails_and_seams(shape, route, variant):
    """Single tensors at every tail length around a float4, a unit (1024) and a chunk (4096); lists in which a tensor with
    n % 4 != 0 is followed by another, with an empty tensor first / in the middle / last, and with twelve tensors."""
    run(tails_case(shape, variant), route)


@pytest.mark.parametrize('variant', FOUR, ids=vid)
@pytest.mark.parametrize('route', ROUTES)
def test_tail_carries_the_norm(route, variant):
    """n = 4099: the three tail gradients are 100 x the others and hold most of the norm -- a norm pass that dropped its scalar
    tail would move coef, and with it every output, far beyond tolerance."""
    c = tail_weight_case(variant)
    g = R.tensors_of(c)[0]['g'].astype(np.float64)
    assert float((g[-3:] ** 2).sum()) > 0.5 * float((g ** 2).sum())
    run(c, route)


@pytest.mark.parametrize('variant', VARIANTS, ids=vid)
@pytest.mark.parametrize('wd', [0.0, 1e-5, 0.1])
@pytest.mark.parametrize('clip', ['off', 'unit', 'below'])
@pytest.mark.parametrize('route', ROUTES)
def test_hyper_parameters(route, clip, wd, variant):
    """wd 0 / 1e-5 / 0.1; momentum 0 / 0.9 with first 0 / 1 (the buffer then holds the sentinel); max_norm <= 0, far above the
    norm (coef exactly 1) and below it."""
    run(hyper_case(variant, wd, clip), route)


@pytest.mark.parametrize('variant', VARIANTS, ids=vid)
@pytest.mark.parametrize('zero_state', [False, True])
@pytest.mark.parametrize('route', ROUTES)
def test_zero_gradient(route, zero_state, variant):
    """An all-zero gradient (clipping on: the norm is 0, coef 1), also with all-zero second moments: 0 / (0 + eps) = 0 and the
    parameters of Adagrad and of RMSprop without a live momentum buffer must come back bit-identical."""
    c = zero_case(variant, zero_state)
    ref = run(c, route)
    if zero_state and (variant[0] == R.ADAGRAD or (variant[0] == R.RMSPROP and (variant[1] == 0.0 or variant[2]))):
        assert all(np.array_equal(o['p'][0], t['p'].astype(np.float64)) for o, t in zip(ref['outs'], R.tensors_of(c)))


@pytest.mark.parametrize('variant', FOUR, ids=vid)
@pytest.mark.parametrize('clip', ['off', 'below'])
@pytest.mark.parametrize('route', ROUTES)
def test_zero_grads_stores_zeros(route, clip, variant):
    """zero_grads != 0: the update uses the (clipped) gradients and the arrays come back exactly zero, on both routes."""
    run(zero_grads_case(variant, clip), route, note=' zero_grads')


@pytest.mark.parametrize('variant', FOUR, ids=vid)
@pytest.mark.parametrize('label', GRID_LABELS)
def test_clip_step_grids(label, variant):
    """Grids of 4, 28, 32, 36 and 68 workgroups (fewer than the 32 barrier slots, exactly 32, no multiple of 32), the device's
    capacity and 4 below it, and the resident boundary: CS_UPT x capacity units (the update runs on the registers of the norm
    pass) and 4 more (it reads again)."""
    cap = capacity(variant[0])
    c = grid_case(label, variant, cap)
    units = 4 * R.n_chunks(c['sizes'])
    print('capacity', cap, 'units', units, 'grid', min(units, cap))
    run(c, 'one', note=' grid ' + label)


def test_workspace_reuse():
    """One workspace, zero-filled once, through launches of 4, capacity, 36, more-than-resident and 4 units of alternating kinds
    (and zero_grads): "every launch leaves them consistent for the next"."""
    ws = new_ws()
    for i in range(len(REUSE)):
        run(reuse_case(i, capacity(REUSE[i][1][0])), 'one', ws=ws, note=' launch %d on one workspace' % i)


@pytest.mark.parametrize('name', list(STRIDE))
def test_grid_stride_loops(name):
    """More chunks than the grid cap: 2049 for ktup_optim_step (2048 workgroups), 257 for ktup_optim_gradnorm (256)."""
    run(stride_case(name), 'two')


@pytest.mark.parametrize('name,n_slots', [('small', 1), ('small', 7), ('small', 16), ('chunks_1025', 7)])
def test_gradnorm_acc(name, n_slots):
    """The slots rise by the squared norm (pre-charged with known doubles: no clearing inside); nothing outside them changes.
    chunks_1025: more chunks than the grid cap of 1024."""
    c = acc_case(name)
    d = Device(c)
    before = (np.arange(24) + 0.5) * 0.01
    slots = torch.from_numpy(before.copy()).to(DEV)
    lib().call('ktup_optim_gradnorm_acc', len(c['sizes']), d.ptrs('g'), arr(ctypes.c_int64, c['sizes']), slots.data_ptr() + 32, n_slots, stream())
    got = d.download()
    after = slots.cpu().numpy()
    assert np.array_equal(after[:4], before[:4]) and np.array_equal(after[4 + n_slots:], before[4 + n_slots:])
    for name_ in R.NAMES:
        assert np.array_equal(bits(got[name_]), bits(c['bufs'][name_]))
    want = R.sum_squares(R.tensors_of(c))
    rise = float(np.sum(after[4:4 + n_slots] - before[4:4 + n_slots]))
    k = R.float4_per_thread('gradnorm_acc', c['sizes'])
    # (the pre-charge costs each slot's atomic adds a double rounding: 2^-53 per add of the slot's value, far below the bound)
    check_sumsq(rise, want, k, 'gradnorm_acc %d slots' % n_slots)
    if n_slots > 1 and R.n_chunks(c['sizes']) >= n_slots:
        assert bool((after[4:4 + n_slots] > before[4:4 + n_slots]).all())        # workgroup b adds to slot b mod n_slots


@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('dev_steps', [False, True])
def test_adam_step_counts(dev_steps, route):
    """Three tensors at step counts (1, 7, 100000), from the host array and from device memory (the host array is then wrong on
    purpose and must be ignored)."""
    c = adam_case()
    if dev_steps:
        sd = torch.tensor(c['steps'], dtype=torch.int64, device=DEV)
        run(c, route, steps=[3, 3, 3], steps_dev=sd.data_ptr(), note=' steps_dev')
    else:
        run(c, route)


def gnorm_workspace(set_, total, rng, steps_taken=10):
    """The tracked-norm workspace as a building kernel leaves it: word 0 steps, word 1 the set in use, that set's 16 slots a
    split of `total`, the idle set junk."""
    host = np.zeros(GNORM_DOUBLES)
    words = host.view(np.uint64)
    words[0], words[1] = steps_taken, set_
    host[2] = 123.0
    host[3:8] = rng.random(5)
    host[GNORM_SET0 + 2 * GNORM_SLOTS:] = rng.random(GNORM_DOUBLES - GNORM_SET0 - 2 * GNORM_SLOTS)
    w = rng.random(GNORM_SLOTS)
    used = slice(GNORM_SET0 + GNORM_SLOTS * set_, GNORM_SET0 + GNORM_SLOTS * (set_ + 1))
    idle = slice(GNORM_SET0 + GNORM_SLOTS * (1 - set_), GNORM_SET0 + GNORM_SLOTS * (2 - set_))
    host[used] = w / w.sum() * total
    host[idle] = 1e3 * (1.0 + rng.random(GNORM_SLOTS))
    return host, used, idle


def run_gnorm(c, host, used, idle, want_total):
    d = Device(c)
    ws, gn = new_ws(), torch.from_numpy(host.copy()).to(DEV)
    lib().call('ktup_optim_clip_step', *head(c, d), ws.data_ptr(), gn.data_ptr(), float(c['max_norm']), c['zero_grads'], None, 0, 0.0, None, None,
               stream())
    got = d.download()
    after, wsh = gn.cpu().numpy(), ws.cpu().numpy()
    fed = max(want_total, 0.0)
    assert abs(wsh[0] - fed) <= 1e-14 * fed and after[2] == wsh[0]                # ws[0] and double 2: the fed norm (16 doubles summed)
    assert wsh.view(np.uint64)[WS_DOUBLES - 1] == 0 and not wsh[1:].any()         # no norm pass, no barrier traffic
    assert after.view(np.uint64)[0] == host.view(np.uint64)[0] + 1 and after.view(np.uint64)[1] == host.view(np.uint64)[1]
    assert not after[idle].any()
    assert np.array_equal(after[used], host[used])
    rest = np.ones(GNORM_DOUBLES, dtype=bool)
    rest[0] = rest[2] = False
    rest[idle] = False
    assert np.array_equal(after[rest], host[rest])
    ref = R.expected(c, sumsq=float(wsh[0]))
    check(c, got, ref, None, note=' gnorm fed')
    return ref


@pytest.mark.parametrize('variant', FOUR, ids=vid)
@pytest.mark.parametrize('set_', [0, 1])
@pytest.mark.parametrize('zero_grads', [0, 1])
def test_gnorm_fed_directly(zero_grads, set_, variant):
    """The launch clips by the norm in the tracked-norm workspace -- 4 x the true squared norm, so coef is 0.25 and not the 0.5
    the gradients themselves would give --, writes ws[0] and double 2, counts the step, zeroes the idle set, leaves the used one."""
    c = gnorm_case(variant, zero_grads)
    total = 4.0 * R.sum_squares(R.tensors_of(c))
    host, used, idle = gnorm_workspace(set_, total, np.random.default_rng(seed_of('gnorm', set_, zero_grads)))
    ref = run_gnorm(c, host, used, idle, float(np.sum(host[used])))
    assert abs(ref['coef'] - 0.25) < 1e-3


def test_gnorm_tiny_negative_sum_clamps_to_zero():
    c = gnorm_case(FOUR[0], 0)
    host, used, idle = gnorm_workspace(1, 1.0, np.random.default_rng(3))
    host[used] = 0.0
    host[used.start], host[used.start + 5] = 1.0, -1.0 - 1e-12
    ref = run_gnorm(c, host, used, idle, -1e-12)
    assert ref['sumsq'] == 0.0 and ref['coef'] == 1.0


@pytest.mark.parametrize('n_slots', [1, 16])
@pytest.mark.parametrize('with_acc', [False, True])
@pytest.mark.parametrize('clip', ['off', 'below'])
def test_loss_slots(clip, with_acc, n_slots):
    """*loss_out = loss_scale x sum(slots), *loss_acc rises by the same amount, the slots are zero afterwards."""
    c = loss_case(clip)
    d = Device(c)
    rng = np.random.default_rng(seed_of('loss', clip, with_acc, n_slots))
    sl = np.full(n_slots + 8, 5.5, dtype=np.float32)
    sl[4:4 + n_slots] = rng.random(n_slots).astype(np.float32) * 3.0
    out = np.array([9.0, 9.0, 9.0, 9.0, 2.5, 9.0, 9.0, 9.0], dtype=np.float32)    # [1] = loss_out, [4] = loss_acc
    slots, outd, ws = torch.from_numpy(sl.copy()).to(DEV), torch.from_numpy(out.copy()).to(DEV), new_ws()
    scale = 0.25
    lib().call('ktup_optim_clip_step', *head(c, d), ws.data_ptr(), None, float(c['max_norm']), 0, slots.data_ptr() + 16, n_slots, scale,
               outd.data_ptr() + 4, outd.data_ptr() + 16 if with_acc else None, stream())
    got = d.download()
    ref = R.expected(c)
    k = R.float4_per_thread('clip_step', c['sizes'], capacity(c['kind']))
    check_ws(ws, ref, c, k)
    check(c, got, ref, k, note=' loss slots')
    sl2, out2 = slots.cpu().numpy(), outd.cpu().numpy()
    assert not bits(sl2[4:4 + n_slots]).any() and bool((sl2[:4] == 5.5).all()) and bool((sl2[4 + n_slots:] == 5.5).all())
    want = scale * float(np.sum(sl[4:4 + n_slots].astype(np.float64)))
    print('loss_out %.9g want %.9g' % (out2[1], want))
    assert abs(float(out2[1]) - want) <= (n_slots + 1) * R.U * want               # n - 1 fp32 adds and the product, all positive
    keep = [0, 2, 3, 5, 6, 7] + ([] if with_acc else [4])
    assert bool((out2[keep] == out[keep]).all())
    if with_acc:
        assert abs(float(out2[4]) - (2.5 + float(out2[1]))) <= 2 * R.U * (2.5 + float(out2[1]))


@pytest.mark.parametrize('clip', ['off', 'below'])
def test_loss_only_launch(clip):
    """n_tensors = 0 and loss slots only: one workgroup publishes the loss (with clipping on it also runs the barrier alone)."""
    sl = torch.tensor([1.5, 2.25, 0.5, 7.0], dtype=torch.float32, device=DEV)
    out = torch.tensor([9.0, 9.0], dtype=torch.float32, device=DEV)
    ws = new_ws()
    one = arr(ctypes.c_void_p, [None])
    lib().call('ktup_optim_clip_step', R.ADAM, 0, one, one, one, one, arr(ctypes.c_int64, [0]), arr(ctypes.c_int64, [1]), None,
               arr(ctypes.c_int32, [0]), 0.05, 0.0, 0.0, 0.9, 0.999, 1e-8, 0.99, ws.data_ptr(), None, 1.0 if clip == 'below' else 0.0, 0,
               sl.data_ptr(), 3, 2.0, out.data_ptr(), None, stream())
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [8.5, 9.0] and sl.cpu().tolist() == [0.0, 0.0, 0.0, 7.0]
    host = ws.cpu().numpy()
    assert not host[:1 + 32 * 8 + 32 * 8 + 8].any() and host.view(np.uint64)[WS_DOUBLES - 1] == 0


def test_graph_replay():
    """An Adam ktup_optim_clip_step with steps_dev (clipping on at coef == 1: the barrier runs, the gradients stay) captured with
    the increment of the counters and replayed five times = five reference steps, at the sum of the per-step bounds."""
    c = graph_case()
    L = lib()
    cap = capacity(c['kind'])
    k = R.float4_per_thread('clip_step', c['sizes'], cap)
    warm, d = Device(c), Device(c)
    ws = new_ws()
    counters = torch.tensor([s - 1 for s in c['steps']], dtype=torch.int64, device=DEV)
    scratch = counters.clone()

    def launch(dev, cnt):
        cnt.add_(1)
        L.call('ktup_optim_clip_step', *head(c, dev, steps=[1, 1, 1], steps_dev=cnt.data_ptr()), ws.data_ptr(), None, float(c['max_norm']), 0,
               None, 0, 0.0, None, None, stream())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch(warm, scratch)                                                     # loads the kernel outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch(d, counters)
    torch.cuda.synchronize()
    assert counters.cpu().tolist() == [s - 1 for s in c['steps']]                 # captured, not run
    for _ in range(5):
        graph.replay()
    got = d.download()
    assert counters.cpu().tolist() == [s + 4 for s in c['steps']]
    bufs = {n: c['bufs'][n].astype(np.float64) for n in R.NAMES}
    extra = [{n: np.zeros(s) for n in R.NAMES} for s in c['sizes']]
    for j in range(5):
        step = dict(c, steps=[s + j for s in c['steps']])
        ref = R.expected(step, bufs=bufs)
        assert ref['coef'] == 1.0
        C = R.constants(c['kind'], c['hyper'], False, k)
        if j < 4:
            for e, out, t in zip(extra, ref['outs'], R.tensors_of(c, bufs)):
                for n in ('p', 's1', 's2'):
                    e[n] += C[n] * R.U * out[n][1]
                    t[n][:] = out[n][0]
    check(c, got, ref, k, extra_tol=extra, note=' five replays')
    check_ws(ws, ref, c, k)


REFUSALS = ['13_tensors', 'grad_offset_4_bytes', 'sgd_state1', 'adagrad_state1', 'adam_state1', 'adam_state2', 'rmsprop_state1',
            'rmsprop_state2', 'adam_step_0', 'kind_4', 'gnorm_without_clipping', 'slots_without_loss_out', 'size_2^32',
            'clipping_without_sumsq']


ONE_ONLY, TWO_ONLY = ('gnorm_without_clipping', 'slots_without_loss_out', 'size_2^32'), ('clipping_without_sumsq',)
REFUSED = [(w, 'ktup_optim_step') for w in REFUSALS if w not in ONE_ONLY] + [(w, 'ktup_optim_clip_step') for w in REFUSALS if w not in TWO_ONLY]


@pytest.mark.parametrize('what,entry', REFUSED)
def test_refused_calls(what, entry):
    """Each returns an error code with ktup_last_error text, launches nothing, and leaves every buffer bit-identical."""
    L = lib()
    one = entry == 'ktup_optim_clip_step'
    variant = {'sgd_state1': (R.SGD, 0.9, 0), 'adagrad_state1': FOUR[1], 'rmsprop_state1': (R.RMSPROP, 0.0, 0), 'rmsprop_state2': FOUR[3],
               'size_2^32': FOUR[0]}.get(what, FOUR[2])
    c = refused_case(variant, 13 if what == '13_tensors' else 3)
    d = Device(c)
    kw, steps, kind, mx = {}, None, None, float(c['max_norm'])
    if what == 'grad_offset_4_bytes':
        kw['g'] = {'shift': {1: 4}}
    if what.endswith('_state1'):
        kw['s1'] = {'null': (1,)}
    if what.endswith('_state2'):
        kw['s2'] = {'null': (1,)}
    if what == 'adam_step_0':
        steps = [7, 0, 7]
    args = list(head(c, d, steps, None, **kw))
    if what == 'kind_4':
        args[0] = 4
    if what == 'size_2^32':
        args[6] = arr(ctypes.c_int64, [8, 1 << 32, 8])
    ws, gn = new_ws(), torch.zeros(GNORM_DOUBLES, dtype=torch.float64, device=DEV)
    sumsq = torch.ones(1, dtype=torch.float64, device=DEV)
    slots = torch.ones(4, dtype=torch.float32, device=DEV)
    if one:
        if what == 'gnorm_without_clipping':
            tail = (ws.data_ptr(), gn.data_ptr(), 0.0, 0, None, 0, 0.0, None, None)
        elif what == 'slots_without_loss_out':
            tail = (ws.data_ptr(), None, mx, 0, slots.data_ptr(), 4, 1.0, None, None)
        else:
            tail = (ws.data_ptr(), None, mx, 0, None, 0, 0.0, None, None)
    else:
        tail = (None if what == 'clipping_without_sumsq' else sumsq.data_ptr(), mx, 0)
    with pytest.raises(L.KtupError) as info:
        L.call(entry, *args, *tail, stream())
    text = L.load().ktup_last_error().decode()
    print(info.value.code, text)
    assert info.value.code not in (0, None) and len(text) > 10 and entry in text
    got = d.download()
    for n in R.NAMES:
        assert np.array_equal(bits(got[n]), bits(c['bufs'][n]))
    assert not ws.cpu().numpy().any() and not gn.cpu().numpy().any() and slots.cpu().tolist() == [1.0] * 4 and sumsq.item() == 1.0


def test_zz_report():
    """The largest error / tolerance of the module per kind and buffer (printed; every case asserted its own)."""
    for kind, w in sorted(WORST.items()):
        print('%-8s ' % kind + '  '.join('%s %.3f' % (n, w[n]) for n in R.NAMES))
    assert all(0.0 <= v <= 1.0 for w in WORST.values() for v in w.values())                    # false for a NaN as well
