"""fp64 reference of the dense optimizer launches of csrc/ktup_optim.hip (include/ktup_hip.h, K20): ktup_optim_gradnorm[_acc],
ktup_optim_step and ktup_optim_clip_step.  NOT a test module: tests/test_optim_ref_host.py pins it to fp64 torch.optim on the CPU,
tests/test_hip_optim_abi.py compares the kernels with it on the GPU.  numpy only, everything from the same fp32 inputs widened.

clip_and_step(kind, tensors, hyper, steps, first, max_norm, zero_grads, sumsq=None)
    sumsq = sum g^2 over all tensors (or the value handed in: a directly fed norm), coef = min(1, max_norm / (sqrt(sumsq) + 1e-6))
    for max_norm > 0 else 1, g' = g coef, d = g' + wd p (literally g' for wd == 0), then update1's rule of the kind.  Adam's
    1 - beta1^t and sqrt(1 - beta2^t) come from each tensor's own step count and are rounded to fp32 (the kernel's contract: the
    host, or the kernel for steps_dev, evaluates them in double and hands update1 a float); ROUND_BIAS = False leaves them in
    double (for the comparison with torch.optim only).  `first` is honoured for SGD and RMSprop momentum.
    Every output array comes as (want, scale).  scale is the same formula with each addition / subtraction replaced by the sum of
    the operands' magnitudes: a running bound of the absolute error in units of 2^-24 x (number of roundings).  An array the kind
    does not write has scale 0 (it must come back bit-identical).

Tolerance = C x 2^-24 x scale, C = constants(kind, clipped, k)[output].  Derivation (u = 2^-24, first order; e(x) counts units of
u relative to scale(x); a product adds the factors' counts + 1, a sum takes the larger count + 1 over the summed scales, a
positive quantity's sqrt halves the count + 1):
  coef    not clipped (max_norm <= 0, or coef == 1): exact, g' = g x 1.0f = g.  Clipped: (float)sqrt(sumsq), + 1e-6f, the
          division = 3 roundings, plus HALF the relative bound of sumsq (the square root), which is (4k + 8) u for a norm pass
          whose threads accumulate k float4 each and 0 for a squared norm handed in as doubles (gnorm): c = 3 + (2k + 4).
  g'      e_g = c + 1 (the product); scale |g'|.
  fma     an fmaf of the source counts as TWO roundings, its product and its sum: the bound then also holds for an evaluation
          without contraction (the fp32 emulation of tests/test_optim_ref_host.py), and for whichever of the plain a * b + c
          expressions the compiler does contract.
  d       wd p + g': E = max(e_g, 1) + 1 over sd = |g'| + |wd p|.  kappa = sd / |d| (>= 1) is the cancellation factor: relative
          to |d| the count is E kappa.  Wherever an output depends on d RELATIVELY -- through d^2 in a second moment and through
          the quotient d / (sqrt(.) + eps) -- its scale carries kappa, so that C stays a constant: scale(d^2) = |d| sd = kappa d^2
          with count 2E + 1, and a second moment m' = a d^2 + b m has scale(m') / m' <= kappa.
  SGD     buf' = mom buf + d (or d when first): E + 1.   p' = -lr (d or buf') + p: the product + 1, the sum + 1 -> E + 3.
  Adagrad sum' = d d + sum: 2E + 2.  den = sqrt(sum') + eps: relative (E + 1) kappa + 2.  q = d / den: E kappa + den + 1
          <= (2E + 4) kappa over |q|, i.e. count 2E + 4 over scale kappa |q|.  p' = p - lr q: + 2 -> 2E + 6.
  Adam    1 - beta1: 1.  exp_avg' = m + (d - m)(1 - beta1): E + 1, x: + 2, +: + 1 -> E + 4 over |m| + (sd + |m|)(1 - beta1).
          exp_avg_sq' = (1 - beta2)(d d) + beta2 v: 1 + (2E + 1) + 1 = 2E + 3 for the product, + 1 -> 2E + 4.
          denom = sqrt(v') / bc2s + eps: relative (E + 2) kappa + 3 <= (E + 5) kappa.  q = m' / denom: (E + 4) + (E + 5) + 1 =
          2E + 10 over kappa scale(m') / denom.  p' = p - (lr / bc1) q: lr / bc1 1, the product 1, the difference 1 -> 2E + 13.
  RMSprop square_avg' as Adam's: 2E + 4.  avg = sqrt(.) + eps: relative (E + 2) kappa + 2 <= (E + 4) kappa.  q = d / avg:
          E + (E + 4) + 1 = 2E + 5 over kappa |d| / avg.  No momentum: p' = p - lr q: + 2 -> 2E + 7.  Momentum: buf' = mom buf + q
          (or q when first): 2E + 6;  p' = -lr buf' + p: 2E + 8 (used for both forms).
Second-order terms (C^2 u^2) are ignored: C <= 80, so they are below 1e-5 of one unit.

Norm bound.  All terms are positive (condition number 1), so the relative error of the fp32 part is at most u times the number
of roundings one term passes through: 4 inside dot4 (a product and three fmas), one per `acc += dot4` of the k float4 a thread
accumulates, 6 in group_sum<64>; the four wave sums and everything across workgroups is added in double.  k + 10 <= 4k + 8 for
every k >= 1, and (4k + 8) u is the bound used here (a thread's scalar tail is at most three fmas in place of one dot4).
k = float4_per_thread(route, sizes, capacity): ceil(units / grid), units = 4 x chunks, grid = min(chunks, 256) for
ktup_optim_gradnorm, min(chunks, 1024) for ktup_optim_gradnorm_acc and min(units, capacity) for ktup_optim_clip_step (whose
resident form has k <= CS_UPT = 5).

Generator (case).  A flat fp32 buffer per array (p, g, s1, s2) holds every tensor of the list between GUARD sentinel floats,
each tensor starting at a multiple of 4 floats (16-byte alignment); everything outside the tensors is guard.  Knife edges are
kept out by construction and check_case asserts it on the fp64 reference before any launch:
  * kappa <= KAPPA_MAX = 8 for every element: parameters of offending elements are drawn again (never skipped), in at most
    MAX_ROUNDS rounds; ROUNDS holds the largest number of rounds any case of a family needed;
  * second moments (Adagrad sum, Adam exp_avg_sq, RMSprop square_avg) are positive and >= d^2, except where a case asks for
    all-zero state;
  * a clipped case has max_norm = 0.5 ||g|| and a coef == 1 case max_norm = 1000 ||g||: | ||g|| / max_norm - 1 | >= GAP = 0.25,
    far beyond any rounding of the norm, so fp32 and fp64 take the same branch of min(1, .)."""
import math

import numpy as np

SGD, ADAGRAD, ADAM, RMSPROP = 0, 1, 2, 3
KINDS = (SGD, ADAGRAD, ADAM, RMSPROP)
KIND_NAMES = {SGD: 'sgd', ADAGRAD: 'adagrad', ADAM: 'adam', RMSPROP: 'rmsprop'}
NAMES = ('p', 'g', 's1', 's2')
U = 2.0 ** -24
CHUNK = 4096
CS_UPT = 5
GUARD = 8
SENTINEL = np.float32(-7.25)
KAPPA_MAX = 8.0
GAP = 0.25
MAX_ROUNDS = 12
ROUND_BIAS = True
ROUNDS = {}                                      # family -> the largest number of redraw rounds one of its cases needed
DEFAULT_EPS = {SGD: 0.0, ADAGRAD: 1e-10, ADAM: 1e-8, RMSPROP: 1e-8}


def hyper(kind, lr=0.05, wd=0.0, momentum=0.0, beta1=0.9, beta2=0.999, eps=None, alpha=0.99):
    """The launch's seven floats, as the fp32 values the C ABI receives."""
    eps = DEFAULT_EPS[kind] if eps is None else eps
    return {k: np.float32(v) for k, v in dict(lr=lr, wd=wd, momentum=momentum, beta1=beta1, beta2=beta2, eps=eps, alpha=alpha).items()}


def uses(kind, h):
    """Which of (s1, s2) the kind reads and writes."""
    if kind == SGD:
        return (float(h['momentum']) != 0.0, False)
    if kind == ADAGRAD:
        return (True, False)
    if kind == ADAM:
        return (True, True)
    return (True, float(h['momentum']) > 0.0)


def bias_terms(h, t):
    bc1 = 1.0 - float(h['beta1']) ** float(t)
    bc2s = math.sqrt(1.0 - float(h['beta2']) ** float(t))
    if ROUND_BIAS:
        bc1, bc2s = float(np.float32(bc1)), float(np.float32(bc2s))
    return bc1, bc2s


def sum_squares(tensors):
    return float(sum(float(np.sum(t['g'].astype(np.float64) ** 2)) for t in tensors))


def clip_coef(sumsq, max_norm):
    if float(max_norm) <= 0.0:
        return 1.0
    return min(1.0, float(max_norm) / (math.sqrt(max(sumsq, 0.0)) + 1e-6))


def _d(gc, p, wd):
    if wd == 0.0:
        return gc, np.abs(gc)
    return gc + wd * p, np.abs(gc) + np.abs(wd * p)


def _kappa(d, sd):
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(sd > 0.0, sd / np.abs(d), 1.0)


def _update(kind, p, gc, s1, s2, h, bc1, bc2s, first):
    """update1 in fp64 on arrays: {name: (want, scale)} for p, s1, s2 (scale 0 = not written by this kind)."""
    lr, wd, mom = float(h['lr']), float(h['wd']), float(h['momentum'])
    eps = float(h['eps'])
    d, sd = _d(gc, p, wd)
    kap = _kappa(d, sd)
    zero = np.zeros_like(p)
    out = {'s1': (s1, zero), 's2': (s2, zero)}
    if kind == SGD:
        dd, cdd = d, sd
        if mom != 0.0:
            dd, cdd = (d, sd) if first else (mom * s1 + d, np.abs(mom * s1) + sd)
            out['s1'] = (dd, cdd)
        out['p'] = (p - lr * dd, np.abs(p) + lr * cdd)
    elif kind == ADAGRAD:
        n1 = s1 + d * d
        den = np.sqrt(n1) + eps
        out['s1'] = (n1, np.abs(s1) + np.abs(d) * sd)
        out['p'] = (p - lr * (d / den), np.abs(p) + lr * kap * np.abs(d) / den)
    elif kind == ADAM:
        b1, b2 = float(h['beta1']), float(h['beta2'])
        n1, c1 = s1 + (d - s1) * (1.0 - b1), np.abs(s1) + (sd + np.abs(s1)) * (1.0 - b1)
        n2, c2 = (1.0 - b2) * (d * d) + b2 * s2, (1.0 - b2) * np.abs(d) * sd + b2 * np.abs(s2)
        den = np.sqrt(n2) / bc2s + eps
        out['s1'], out['s2'] = (n1, c1), (n2, c2)
        out['p'] = (p - (lr / bc1) * (n1 / den), np.abs(p) + (lr / bc1) * kap * c1 / den)
    else:
        al = float(h['alpha'])
        n1, c1 = (1.0 - al) * (d * d) + al * s1, (1.0 - al) * np.abs(d) * sd + al * np.abs(s1)
        avg = np.sqrt(n1) + eps
        q, cq = d / avg, kap * np.abs(d) / avg
        out['s1'] = (n1, c1)
        if mom > 0.0:
            n2, c2 = (q, cq) if first else (mom * s2 + q, np.abs(mom * s2) + cq)
            out['s2'] = (n2, c2)
            out['p'] = (p - lr * n2, np.abs(p) + lr * c2)
        else:
            out['p'] = (p - lr * q, np.abs(p) + lr * cq)
    return out


def clip_and_step(kind, tensors, hyper, steps, first, max_norm, zero_grads, sumsq=None):
    """tensors: [{'p', 'g', 's1', 's2'}] fp32 arrays.  Returns {'sumsq', 'coef', 'outs': [{name: (want, scale)}]} in fp64."""
    if sumsq is None:
        sumsq = sum_squares(tensors)
    coef = clip_coef(sumsq, max_norm)
    outs = []
    for i, t in enumerate(tensors):
        p, g, s1, s2 = (t[k].astype(np.float64) for k in NAMES)
        gc = g * coef
        bc1, bc2s = bias_terms(hyper, steps[i]) if kind == ADAM else (1.0, 1.0)
        out = _update(kind, p, gc, s1, s2, hyper, bc1, bc2s, bool(first[i]))
        if zero_grads:
            out['g'] = (np.zeros_like(g), np.zeros_like(g))
        elif float(max_norm) > 0.0 and coef < 1.0:
            out['g'] = (gc, np.abs(gc))
        else:
            out['g'] = (g, np.zeros_like(g))                          # untouched, or g x 1.0f
        outs.append(out)
    return {'sumsq': sumsq, 'coef': coef, 'outs': outs}


def constants(kind, hyper, clipped, k):
    """C per output (module docstring).  clipped: coef < 1; k: float4 per thread of the norm pass, None for a norm handed in."""
    e_g = 0.0 if not clipped else 3.0 + (0.0 if k is None else (4.0 * k + 8.0) / 2.0) + 1.0
    E = max(e_g, 1.0) + 1.0
    if kind == SGD:
        C = {'s1': E + 1, 's2': 0.0, 'p': E + 3}
    elif kind == ADAGRAD:
        C = {'s1': 2 * E + 2, 's2': 0.0, 'p': 2 * E + 6}
    elif kind == ADAM:
        C = {'s1': E + 4, 's2': 2 * E + 4, 'p': 2 * E + 13}
    else:
        C = {'s1': 2 * E + 4, 's2': 2 * E + 6, 'p': 2 * E + 8}
    C['g'] = e_g
    return C


def n_chunks(sizes):
    return sum((int(n) + CHUNK - 1) // CHUNK for n in sizes)


def float4_per_thread(route, sizes, capacity=None):
    chunks = n_chunks(sizes)
    units = 4 * chunks
    if units == 0:
        return 0
    grid = {'gradnorm': min(chunks, 256), 'gradnorm_acc': min(chunks, 1024)}.get(route) or min(units, capacity)
    return -(-units // grid)


def norm_bound(k):
    """Relative bound of the squared norm a pass with k float4 per thread returns."""
    return (4.0 * k + 8.0) * U


# ------------------------------------------------------------------------------------------------------ generator
def layout(sizes):
    """Start of every tensor in the flat buffers and their total length."""
    starts, off = [], GUARD
    for n in sizes:
        starts.append(off)
        off += (int(n) + 3) // 4 * 4 + GUARD
    return starts, off


def tensors_of(c, bufs=None):
    bufs = c['bufs'] if bufs is None else bufs
    return [{k: bufs[k][s:s + n] for k in NAMES} for s, n in zip(c['starts'], c['sizes'])]


def guard_mask(c):
    m = np.ones(c['total'], dtype=bool)
    for s, n in zip(c['starts'], c['sizes']):
        m[s:s + n] = False
    return m


def case(kind, sizes, seed, wd=1e-5, momentum=0.0, first=0, clip='below', zero_grads=0, steps=None, zero_grad=False,
         zero_state=False, heavy_tail=False, lr=0.05, family='case'):
    """One launch's inputs.  clip: 'off' (max_norm 0), 'unit' (coef exactly 1) or 'below' (coef 0.5)."""
    sizes = [int(n) for n in sizes]
    rng = np.random.default_rng(seed)
    h = hyper(kind, lr=lr, wd=wd, momentum=momentum)
    starts, total = layout(sizes)
    c = {'kind': kind, 'sizes': sizes, 'hyper': h, 'starts': starts, 'total': total, 'zero_grads': int(zero_grads),
         'steps': list(steps) if steps is not None else [7] * len(sizes), 'first': [int(first)] * len(sizes), 'clip': clip,
         'zero_state': zero_state, 'family': family}
    bufs = {k: np.full(total, SENTINEL, dtype=np.float32) for k in NAMES}
    c['bufs'] = bufs
    ts = tensors_of(c)
    for t, n in zip(ts, sizes):
        t['p'][:] = (rng.standard_normal(n) * 0.1).astype(np.float32)
        t['g'][:] = 0.0 if zero_grad else (rng.standard_normal(n) * 0.01).astype(np.float32)
        if heavy_tail and n % 4:                                      # 100 x the others' size, whatever was drawn there
            t['g'][n - n % 4:] = np.where(t['g'][n - n % 4:] < 0, np.float32(-1.0), np.float32(1.0))
    norm = math.sqrt(sum_squares(ts))
    if clip == 'off':
        c['max_norm'] = np.float32(0.0)
    elif clip == 'unit':
        c['max_norm'] = np.float32(1000.0 * norm if norm > 0.0 else 1.0)
    else:
        assert clip == 'below' and norm > 0.0
        c['max_norm'] = np.float32(0.5 * norm)
    coef = clip_coef(norm * norm, c['max_norm'])
    wdf, rounds = float(h['wd']), 0
    for t, n in zip(ts, sizes):                                       # kappa: draw the offending parameters again
        for r in range(MAX_ROUNDS + 1):
            d, sd = _d(t['g'].astype(np.float64) * coef, t['p'].astype(np.float64), wdf)
            bad = ~(_kappa(d, sd) <= KAPPA_MAX)
            if not bad.any():
                break
            assert r < MAX_ROUNDS, 'kappa: out of redraw rounds'
            t['p'][bad] = (rng.standard_normal(int(bad.sum())) * 0.1).astype(np.float32)
        rounds = max(rounds, r)
        d2 = d * d
        second = np.zeros(n) if zero_state else (d2 + 1e-8) * (1.0 + 3.0 * rng.random(n))
        signed = rng.standard_normal(n) * 0.01
        junk = rng.standard_normal(n)
        use1, use2 = uses(kind, h)
        if kind == SGD:
            s1, s2 = (signed if use1 else junk), junk
        elif kind == ADAGRAD:
            s1, s2 = second, junk
        elif kind == ADAM:
            s1, s2 = signed, second
        else:
            s1, s2 = second, (signed * 100.0 if use2 else junk)
        t['s1'][:] = s1.astype(np.float32)
        t['s2'][:] = s2.astype(np.float32)
        if first and kind == SGD and use1:
            t['s1'][:] = SENTINEL
        if first and kind == RMSPROP and use2:
            t['s2'][:] = SENTINEL
    ROUNDS[family] = max(ROUNDS.get(family, 0), rounds)
    c['rounds'] = rounds
    check_case(c)
    return c


def second_moment_name(kind):
    return {ADAGRAD: 's1', ADAM: 's2', RMSPROP: 's1'}.get(kind)


def check_case(c):
    """The generator's promises, asserted on the fp64 reference."""
    ts = tensors_of(c)
    h = c['hyper']
    assert c['total'] % 4 == 0 and all(s % 4 == 0 and s >= GUARD for s in c['starts'])
    g = guard_mask(c)
    assert all(bool((c['bufs'][k][g] == SENTINEL).all()) for k in NAMES)
    sumsq = sum_squares(ts)
    norm, mx = math.sqrt(sumsq), float(c['max_norm'])
    if mx > 0.0 and norm > 0.0:
        assert abs(norm / mx - 1.0) >= GAP
    coef = clip_coef(sumsq, mx)
    assert (coef < 1.0) == (c['clip'] == 'below')
    name = second_moment_name(c['kind'])
    for t in ts:
        d, sd = _d(t['g'].astype(np.float64) * coef, t['p'].astype(np.float64), float(h['wd']))
        assert bool((_kappa(d, sd) <= KAPPA_MAX).all())
        if name is not None:
            m = t[name].astype(np.float64)
            if c['zero_state']:
                assert not m.any()
            else:
                assert bool((m > 0.0).all()) and bool((m >= d * d).all())
    assert c['rounds'] <= MAX_ROUNDS


def expected(c, sumsq=None, bufs=None):
    return clip_and_step(c['kind'], tensors_of(c, bufs), c['hyper'], c['steps'], c['first'], c['max_norm'], c['zero_grads'], sumsq)


def compare(c, got_bufs, ref, k, bufs=None, report=None, extra_tol=None):
    """Every element of every output array of every tensor against the reference at C x 2^-24 x scale; the guards bit-identical.
    Returns {name: largest |got - want| / tolerance} (0 for exact arrays, which are compared for equality).  Anything that is not
    finite fails, and so does every single element whose ratio is not <= 1 (the comparison is made per element, not on a maximum,
    which a NaN would slip through); a NaN ratio also makes the returned maximum NaN."""
    src = c['bufs'] if bufs is None else bufs
    C = constants(c['kind'], c['hyper'], ref['coef'] < 1.0, k)
    g = guard_mask(c)
    worst = {}
    for name in NAMES:
        assert np.array_equal(got_bufs[name][g].view(np.uint32), src[name][g].view(np.uint32)), 'guards of ' + name
        worst[name] = 0.0
        assert np.isfinite(got_bufs[name]).all(), 'not finite: ' + name
    bad = dict.fromkeys(NAMES, 0)
    for i, (got, out) in enumerate(zip(tensors_of(c, got_bufs), ref['outs'])):
        for name in NAMES:
            want, scale = out[name]
            tol = C[name] * U * scale
            if extra_tol is not None:
                tol = tol + extra_tol[i][name]
            exact = tol == 0.0
            if exact.any():
                assert np.array_equal(got[name][exact], want[exact].astype(np.float32)), (name, i, 'exact part')
            if (~exact).any():
                ratio = np.abs(got[name].astype(np.float64) - want)[~exact] / tol[~exact]
                worst[name] = float(np.fmax.reduce([worst[name], np.max(ratio)]) if np.isfinite(ratio).all() else np.nan)
                bad[name] += int((~(ratio <= 1.0)).sum())             # element by element: a NaN is not <= 1
    if report is not None:
        report(worst, C)
    for name in NAMES:
        assert bad[name] == 0 and worst[name] <= 1.0, (KIND_NAMES[c['kind']], name, bad[name], worst[name], C[name])
    return worst
