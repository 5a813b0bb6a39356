"""Pins tests/_optim_ref.py on the CPU: (1) against fp64 torch.optim.{SGD, Adagrad, Adam, RMSprop} after clip_grad_norm_, with
injected state, to 1e-12; (2) its tolerance rule C x 2^-24 x scale against an emulation of update1 in torch fp32 operations at
1e6 elements per kind (largest ratios printed); (3) the generator's promises for every case tests/test_hip_optim_abi.py
launches, and its redraw counts."""
import math

import numpy as np
import pytest
import torch

from tests import _optim_ref as R

SIZES = [4099, 5, 0, 1023]


def _torch_step(c, first):
    """The same step by torch.optim in fp64: parameters, clipped gradients and the state arrays of every tensor."""
    kind, h = c['kind'], {k: float(v) for k, v in c['hyper'].items()}
    ts = R.tensors_of(c)
    params = [torch.nn.Parameter(torch.from_numpy(t['p'].astype(np.float64))) for t in ts]
    for q, t in zip(params, ts):
        q.grad = torch.from_numpy(t['g'].astype(np.float64))
    if kind == R.SGD:
        opt = torch.optim.SGD(params, lr=h['lr'], weight_decay=h['wd'], momentum=h['momentum'], foreach=False)
    elif kind == R.ADAGRAD:
        opt = torch.optim.Adagrad(params, lr=h['lr'], weight_decay=h['wd'], eps=h['eps'], foreach=False)
    elif kind == R.ADAM:
        opt = torch.optim.Adam(params, lr=h['lr'], weight_decay=h['wd'], betas=(h['beta1'], h['beta2']), eps=h['eps'], foreach=False)
    else:
        opt = torch.optim.RMSprop(params, lr=h['lr'], weight_decay=h['wd'], momentum=h['momentum'], alpha=h['alpha'], eps=h['eps'],
                                  foreach=False)
    use1, use2 = R.uses(kind, c['hyper'])
    for q, t, step in zip(params, ts, c['steps']):
        s1, s2 = (torch.from_numpy(t[k].astype(np.float64)) for k in ('s1', 's2'))
        if kind == R.SGD:
            if use1 and not first:
                opt.state[q] = {'momentum_buffer': s1}               # first: no buffer yet, torch clones the gradient
        elif kind == R.ADAGRAD:
            opt.state[q] = {'step': torch.tensor(3.0), 'sum': s1}
        elif kind == R.ADAM:
            opt.state[q] = {'step': torch.tensor(float(step - 1)), 'exp_avg': s1, 'exp_avg_sq': s2}
        else:
            st = {'step': torch.tensor(3.0), 'square_avg': s1}
            if use2:
                st['momentum_buffer'] = torch.zeros_like(s2) if first else s2      # torch's buffer starts at zero
            opt.state[q] = st
    if float(c['max_norm']) > 0.0:
        torch.nn.utils.clip_grad_norm_(params, float(c['max_norm']))
    opt.step()
    names = {R.SGD: ('momentum_buffer', None), R.ADAGRAD: ('sum', None), R.ADAM: ('exp_avg', 'exp_avg_sq'),
             R.RMSPROP: ('square_avg', 'momentum_buffer')}[kind]
    out = []
    for q in params:
        st = opt.state[q]
        out.append({'p': q.detach().numpy(), 'g': q.grad.numpy(),
                    's1': st[names[0]].numpy() if use1 else None, 's2': st[names[1]].numpy() if use2 else None})
    return out


def _close(a, b, scale, what):
    """Element by element: 1e-12 of the reference's own scale of that element (the sum of the magnitudes that form it: an entry
    that cancels is held to the size of what cancelled, not to the largest entry of the array), or of |b| where the array is not
    written (scale 0)."""
    assert bool((np.abs(a - b) <= 1e-12 * np.maximum(scale, np.abs(b))).all()), what


VARIANTS = [(R.SGD, 0.0, 0), (R.SGD, 0.9, 0), (R.SGD, 0.9, 1), (R.ADAGRAD, 0.0, 0), (R.ADAM, 0.0, 0),
            (R.RMSPROP, 0.0, 0), (R.RMSPROP, 0.9, 0), (R.RMSPROP, 0.9, 1)]


@pytest.mark.parametrize('kind,momentum,first', VARIANTS)
@pytest.mark.parametrize('wd', [0.0, 1e-5, 0.1])
@pytest.mark.parametrize('clip', ['off', 'unit', 'below'])
def test_reference_is_torch_optim_in_fp64(kind, momentum, first, wd, clip, monkeypatch):
    """Adam runs at step counts (1, 7, 100000, 7).  The reference rounds Adam's two bias terms to fp32, torch does not: that is
    the only intended difference, isolated here by ROUND_BIAS = False and bounded in the test below.  With `first` the buffers
    hold the sentinel (garbage) and the result must be torch's clone of the gradient (SGD) / its zero-started buffer (RMSprop)."""
    monkeypatch.setattr(R, 'ROUND_BIAS', False)
    c = R.case(kind, SIZES, 5, wd=wd, momentum=momentum, first=first, clip=clip, steps=[1, 7, 100000, 7], family='host')
    ref = R.expected(c)
    for t, out, n in zip(_torch_step(c, first), ref['outs'], c['sizes']):
        for name in R.NAMES:
            if t[name] is not None:
                _close(out[name][0], t[name], out[name][1], (name, n))


def test_adam_bias_rounding_is_bounded():
    """Rounding 1 - beta1^t and sqrt(1 - beta2^t) to fp32 moves the Adam update by at most 2 x 2^-24 (1 + 2^-23) of its size."""
    c = R.case(R.ADAM, SIZES, 6, wd=1e-5, clip='below', steps=[1, 7, 100000, 7], family='host')
    rounded = R.expected(c)
    try:
        R.ROUND_BIAS = False
        plain = R.expected(c)
    finally:
        R.ROUND_BIAS = True
    moved = False
    for a, b, t in zip(rounded['outs'], plain['outs'], R.tensors_of(c)):
        upd = np.abs(b['p'][0] - t['p'].astype(np.float64))
        diff = np.abs(a['p'][0] - b['p'][0])
        assert bool((diff <= 2.0 * R.U * (1.0 + 2.0 ** -23) * upd + 1e-18).all())
        moved = moved or bool(diff.any())
        for name in ('g', 's1', 's2'):
            assert np.array_equal(a[name][0], b[name][0])
    assert moved                                                      # (0.9 and 0.999 at t = 7 are not fp32 numbers)


def test_first_ignores_the_buffer():
    for kind in (R.SGD, R.RMSPROP):
        c = R.case(kind, [37], 8, momentum=0.9, first=1, family='host')
        a = R.expected(c)
        name = 's1' if kind == R.SGD else 's2'
        assert bool((R.tensors_of(c)[0][name] == R.SENTINEL).all())
        R.tensors_of(c)[0][name][:] = 123.0
        b = R.expected(c)
        for k in R.NAMES:
            assert np.array_equal(a['outs'][0][k][0], b['outs'][0][k][0])


# ----------------------------------------------------------------------------------------- fp32 emulation of update1
def _emulate(kind, c, coef32):
    """update1 in torch fp32 operations in the kernel's order; every fmaf is a rounded product and a rounded sum (no contraction)."""
    h = {k: torch.tensor(float(v), dtype=torch.float32) for k, v in c['hyper'].items()}
    t = R.tensors_of(c)[0]
    p, g, s1, s2 = (torch.from_numpy(t[k].copy()) for k in R.NAMES)
    first = bool(c['first'][0])
    mom = float(h['momentum'])
    g = g * coef32
    d = h['wd'] * p + g if float(h['wd']) != 0.0 else g
    one = torch.tensor(1.0, dtype=torch.float32)
    if kind == R.SGD:
        if mom != 0.0:
            s1 = d.clone() if first else h['momentum'] * s1 + d
            d = s1
        p = -h['lr'] * d + p
    elif kind == R.ADAGRAD:
        s1 = d * d + s1
        p = p - h['lr'] * (d / (torch.sqrt(s1) + h['eps']))
    elif kind == R.ADAM:
        bc1, bc2s = (torch.tensor(x, dtype=torch.float32) for x in R.bias_terms(c['hyper'], c['steps'][0]))
        s1 = s1 + (d - s1) * (one - h['beta1'])
        s2 = (one - h['beta2']) * (d * d) + h['beta2'] * s2
        denom = torch.sqrt(s2) / bc2s + h['eps']
        p = p - (h['lr'] / bc1) * (s1 / denom)
    else:
        s1 = (one - h['alpha']) * (d * d) + h['alpha'] * s1
        avg = torch.sqrt(s1) + h['eps']
        if mom > 0.0:
            s2 = d / avg if first else h['momentum'] * s2 + d / avg
            p = -h['lr'] * s2 + p
        else:
            p = p - h['lr'] * (d / avg)
    assert all(x.dtype == torch.float32 for x in (p, g, s1, s2))
    return {'p': p.numpy(), 'g': g.numpy(), 's1': s1.numpy(), 's2': s2.numpy()}


EMU_RATIOS = {}


@pytest.mark.parametrize('kind,momentum,first', VARIANTS)
@pytest.mark.parametrize('clip', ['unit', 'below'])
def test_tolerance_holds_for_fp32_arithmetic(kind, momentum, first, clip):
    """1e6 elements, wd = 0.1 (the weight-decay term is as large as the gradient: kappa up to 8), the exact norm (k = None).
    Inside the tolerance with no exception, and not looser than two orders of magnitude: the largest ratio of every output that
    has a tolerance is above 1e-2."""
    c = R.case(kind, [1000000], 21, wd=0.1, momentum=momentum, first=first, clip=clip, family='emulation')
    ref = R.expected(c)
    mx = torch.tensor(float(c['max_norm']), dtype=torch.float32)
    coef32 = mx / (torch.tensor(math.sqrt(ref['sumsq']), dtype=torch.float32) + torch.tensor(1e-6, dtype=torch.float32))
    coef32 = torch.minimum(coef32, torch.tensor(1.0, dtype=torch.float32))
    assert (float(coef32) < 1.0) == (ref['coef'] < 1.0)
    got = {k: c['bufs'][k].copy() for k in R.NAMES}
    emu = _emulate(kind, c, coef32)
    for k in R.NAMES:
        R.tensors_of(c, got)[0][k][:] = emu[k]
    seen = {}

    def report(worst, C):
        seen.update(worst)
        print(R.KIND_NAMES[kind], 'momentum', momentum, 'first', first, clip,
              ' '.join('%s %.3f (C %g)' % (k, worst[k], C[k]) for k in R.NAMES))
    R.compare(c, got, ref, None, report=report)
    EMU_RATIOS[(kind, momentum, first, clip)] = dict(seen)
    use1, use2 = R.uses(kind, c['hyper'])
    live = ['p'] + (['g'] if clip == 'below' else []) + (['s1'] if use1 else []) + (['s2'] if use2 else [])
    for k in live:
        assert seen[k] >= 1e-2, (k, seen[k])


# ----------------------------------------------------------------------------------------------- the comparator
def test_compare_rejects_nan_and_out_of_tolerance_elements():
    """R.compare is what every toleranced array of the GPU module goes through: it accepts the rounded reference, and one NaN,
    one infinity, one element just outside its tolerance, one changed guard float or one changed element of an array the kind does
    not write each make it fail -- wherever the element sits, the last tensor's tail included."""
    c = R.case(R.RMSPROP, [5, 4097], 9, momentum=0.9, family='host')
    ref = R.expected(c)
    C = R.constants(c['kind'], c['hyper'], True, 5)

    def rounded():
        got = {k: c['bufs'][k].copy() for k in R.NAMES}
        for t, out in zip(R.tensors_of(c, got), ref['outs']):
            for k in R.NAMES:
                t[k][:] = out[k][0].astype(np.float32)
        return got
    worst = R.compare(c, rounded(), ref, 5)
    assert all(0.0 <= worst[k] <= 1.0 for k in R.NAMES) and worst['p'] > 0.0
    for name in R.NAMES:
        for tensor, at in ((0, 1), (1, 4096)):
            for value in (np.nan, np.inf):
                got = rounded()
                R.tensors_of(c, got)[tensor][name][at] = value
                with pytest.raises(AssertionError):
                    R.compare(c, got, ref, 5)
            want, scale = ref['outs'][tensor][name]
            for factor, ok in ((0.5, True), (1.5, False)):
                got = rounded()
                got_t = R.tensors_of(c, got)[tensor][name]
                # half / one and a half tolerances off, on top of the rounding of `want` itself (at most half a unit of C >= 4)
                got_t[at] = np.float32(want[at] + factor * C[name] * R.U * scale[at])
                if ok:
                    R.compare(c, got, ref, 5)
                else:
                    with pytest.raises(AssertionError):
                        R.compare(c, got, ref, 5)
        got = rounded()
        got[name][c['starts'][1] + 4097] = 0.0                        # the first guard float behind the last tensor
        with pytest.raises(AssertionError):
            R.compare(c, got, ref, 5)
    plain = R.case(R.SGD, [5], 9, clip='off', family='host')          # no momentum, no clipping: g, s1 and s2 are not written
    pref = R.expected(plain)
    for name in ('g', 's1', 's2'):
        got = {k: plain['bufs'][k].copy() for k in R.NAMES}
        R.tensors_of(plain, got)[0]['p'][:] = pref['outs'][0]['p'][0].astype(np.float32)
        R.compare(plain, got, pref, 1)
        x = R.tensors_of(plain, got)[0][name]
        x[4] = np.nextafter(x[4], np.float32(9.0))
        with pytest.raises(AssertionError):
            R.compare(plain, got, pref, 1)


# ----------------------------------------------------------------------------------------------- generator
def test_generator_promises_hold_for_every_gpu_case():
    """Every case the GPU module launches is built here (the construction is host-only and deterministic), with the capacity
    taken as 512 and as 256; case() asserts check_case on each, and the redraw rounds stay far below their bound."""
    from tests import _optim_cases as G
    n = 0
    for cap in (512, 256):
        for make in G.all_case_builders(cap, cap_only=cap != 512):
            c = make()
            R.check_case(c)
            n += 1
    print('cases', n, 'redraw rounds', dict(R.ROUNDS))
    assert n > 250
    assert max(R.ROUNDS.values()) <= 6 <= R.MAX_ROUNDS


def test_float4_per_thread_and_layout():
    assert R.float4_per_thread('clip_step', [1], 512) == 1
    assert R.float4_per_thread('clip_step', [4096 * 128], 512) == 1
    assert R.float4_per_thread('clip_step', [4096 * 640], 512) == 5
    assert R.float4_per_thread('clip_step', [4096 * 641], 512) == 6
    assert R.float4_per_thread('gradnorm', [4096 * 256], None) == 4
    assert R.float4_per_thread('gradnorm', [4096 * 257], None) == 5
    assert R.float4_per_thread('gradnorm_acc', [4096 * 1025], None) == 5
    starts, total = R.layout([1, 0, 5, 4096])
    assert starts == [8, 20, 28, 44] and total == 44 + 4096 + 8
    c = R.case(R.ADAM, [1, 0, 5], 1, family='host')
    assert int(R.guard_mask(c).sum()) == c['total'] - 6
