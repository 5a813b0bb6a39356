"""Pins tests/_shard_ref.py on the CPU: (1) reduce_ref and apply_ref against torch fp64 (index_add_, clip_grad_norm_, torch.optim with
injected state) to 1e-12; (2) check_route on routes computed in numpy; (3) every checker rejects a correct output with ONE defect;
(4) every case tests/test_hip_shard_abi.py launches keeps an fp32 emulation of the same sums and formulas inside the stated
tolerance; (5) the measured fp32 error of the Adam replay, which is that launch's tolerance."""
import numpy as np
import pytest
import torch

from tests import _optim_ref as O
from tests import _shard_cases as C
from tests import _shard_ref as R


def _close(a, b, what):
    assert bool((np.abs(a - b) <= 1e-12 * np.maximum(1.0, np.abs(b))).all()), what


def _boundary(rc):
    x = R.predict_xkeys(rc['skey'], rc['m'], rc['n'], rc['d'], rc['opt'])
    return sorted(set(x[x >= 0].tolist()))


def _gradient(rc):
    tot, mag, cnt = R.reduce_terms(rc['G'], rc['n_src'], rc['src_off'], rc['inverse'], rc['W'], rc['d'])
    return tot, (np.maximum(cnt - 1, 0)[:, None] * R.U * mag), cnt


# ------------------------------------------------------------------------------------------------ (1) the models are torch's
@pytest.mark.parametrize('name', ['padded', 'ktup', 'one_row_5S'])
def test_reduce_ref_is_index_add(name):
    rc = C.reduce_case(64, name)
    on = np.nonzero(rc['ids'] >= 0)[0]
    src = R.source_rows(rc['n'], rc['n_src'], rc['src_off'])
    want = torch.zeros(rc['W'], 64, dtype=torch.float64)
    want.index_add_(0, torch.from_numpy(rc['inverse'][on]), torch.from_numpy(rc['G'][src[on], :64].astype(np.float64)))
    _close(R.reduce_ref(rc['G'], rc['n_src'], rc['src_off'], rc['inverse'], rc['W'], 64), want.numpy(), name)
    assert rc['inverse'].max() == rc['W'] or name != 'padded'


@pytest.mark.parametrize('second', [False, True])
@pytest.mark.parametrize('clip', ['clip', 'unit', 'off'])
@pytest.mark.parametrize('kind', list(C.KINDS))
def test_apply_ref_is_torch_optim(kind, clip, second, monkeypatch):
    """The touched rows of all tables as ONE dense parameter each, the gradients of rows without an owner row and the small
    gradients (twice when they feed two tables: small_weight = 2) in the clipped norm; torch.optim with injected state."""
    monkeypatch.setattr(O, 'ROUND_BIAS', False)
    rc = C.reduce_case(64, 'each_side')
    d = 64
    c = C.apply_case(rc, kind, clip=clip, second=second, boundary=_boundary(rc))
    gsum, _, cnt = _gradient(rc)
    weight = 2.0 if second else 1.0
    sumsq = float((gsum ** 2).sum()) + weight * sum(float((s['g'].astype(np.float64) ** 2).sum()) for s in c['smalls'])
    c['max_norm'] = C.max_norm_of(clip, sumsq)
    touched = (c['ids'] >= 0) & (cnt > 0)
    ref = R.apply_ref(c, gsum, np.zeros_like(gsum), touched, sumsq, 0.0)
    h = R.hyper_of(c)
    params, groups = [], []
    wt = np.arange(rc['W']) % rc['T']
    for t in range(rc['T']):
        rows_w = np.nonzero((wt == t) & touched)[0]
        groups.append((c['tables'][t], None if c['states'] is None else c['states'][t], c['ids'][rows_w], gsum[rows_w], ref['tables'][t],
                       None if c['states'] is None else ref['states'][t]))
    for k, sm in enumerate(c['smalls']):
        for which in ('0', '1'):
            if sm['p' + which] is not None:
                groups.append((sm['p' + which], sm['s' + which], np.arange(sm['g'].shape[0]), sm['g'].astype(np.float64),
                               ref['small'][k]['p' + which], ref['small'][k]['s' + which]))
    for P, S, rows, g, _, _ in groups:
        q = torch.nn.Parameter(torch.from_numpy(P[rows, :d].astype(np.float64)))
        q.grad = torch.from_numpy(np.ascontiguousarray(g))
        params.append(q)
    rest = torch.nn.Parameter(torch.zeros(int((~touched).sum()), d, dtype=torch.float64))      # in the norm, never stepped
    rest.grad = torch.from_numpy(gsum[~touched])
    rule = R.rule_of(c)
    wd = h['wd'] if c['kind'] == R.ADAM else 0.0
    if rule == O.SGD:
        opt = torch.optim.SGD(params, lr=h['lr'], weight_decay=wd, foreach=False)
    elif rule == O.ADAGRAD:
        opt = torch.optim.Adagrad(params, lr=h['lr'], weight_decay=wd, eps=h['eps'], foreach=False)
    else:
        opt = torch.optim.Adam(params, lr=h['lr'], weight_decay=wd, betas=(h['beta1'], h['beta2']), eps=h['eps'], foreach=False)
    adam_rows = c['kind'] == R.ADAM
    for q, (P, S, rows, g, _, _) in zip(params, groups):
        if rule == O.ADAGRAD:
            opt.state[q] = {'step': torch.tensor(3.0), 'sum': torch.from_numpy((S[rows, d:2 * d] if adam_rows else S[rows, :d]).astype(np.float64))}
        elif rule == O.ADAM:
            opt.state[q] = {'step': torch.tensor(float(c['t'] - 1)), 'exp_avg': torch.from_numpy(S[rows, :d].astype(np.float64)),
                            'exp_avg_sq': torch.from_numpy(S[rows, d:2 * d].astype(np.float64))}
    if c['max_norm'] > 0.0:
        torch.nn.utils.clip_grad_norm_(params + [rest], c['max_norm'])
    opt.step()
    for q, (P, S, rows, g, ref_p, ref_s) in zip(params, groups):
        _close(ref_p[0][rows, :d], q.detach().numpy(), (kind, 'p'))
        untouched = np.setdiff1d(np.arange(P.shape[0]), rows)
        assert np.array_equal(ref_p[0][untouched, :d], P[untouched, :d].astype(np.float64)) and not ref_p[1][untouched].any()
        if rule == O.ADAGRAD:
            _close(ref_s[0][rows, d:2 * d] if adam_rows else ref_s[0][rows, :d], opt.state[q]['sum'].numpy(), (kind, 'sum'))
        elif rule == O.ADAM:
            _close(ref_s[0][rows, :d], opt.state[q]['exp_avg'].numpy(), (kind, 'exp_avg'))
            _close(ref_s[0][rows, d:2 * d], opt.state[q]['exp_avg_sq'].numpy(), (kind, 'exp_avg_sq'))
    assert np.array_equal(ref['loss_sum'], (c['loss_sum'] + c['loss_step']).astype(np.float32)) and ref['skipped'] == 5


@pytest.mark.parametrize('with_step', [False, True], ids=['catch_up', 'then_step_t'])
@pytest.mark.parametrize('rule,wd', [(0, 0.0), (0, 1e-2), (1, 1e-2), (2, 1e-2)], ids=['adam', 'adam_wd', 'adagrad_wd', 'sgd_wd'])
def test_lazy_rows_is_dense_torch_optim_over_the_owed_steps(rule, wd, with_step, monkeypatch):
    """R.lazy_rows against dense torch.optim.{Adam, Adagrad, SGD}(weight_decay = wd) in fp64: state injected at step `last`, K = 1, 3
    and 6 zero-gradient steps (row groups with their own `last`), then optionally step t with a gradient; 1e-12."""
    monkeypatch.setattr(O, 'ROUND_BIAS', False)
    rng = np.random.default_rng(C.seed_of('lazy', rule, wd, with_step))
    n, d, t = 9, 8, 41
    c = {'kind': R.ADAM, 'rule': rule, 'wd': wd, 'lr': 0.05, 'eps': 1e-6, 'beta1': 0.9, 'beta2': 0.999, 't': t}
    h = R.hyper_of(c)
    upto = t - 1 if with_step else t
    last = upto - np.asarray([1, 3, 6] * 3)
    p0, m0 = rng.standard_normal((n, d)).astype(np.float32), (0.3 * rng.standard_normal((n, d))).astype(np.float32)
    v0 = (0.05 + rng.random((n, d))).astype(np.float32)
    g = rng.standard_normal((n, d)).astype(np.float32) if with_step else None
    got = R.lazy_rows(c, p0, m0, v0, last, None if g is None else g.astype(np.float64), 0.5)
    for L in sorted(set(last.tolist())):
        rows = np.nonzero(last == L)[0]
        q = torch.nn.Parameter(torch.from_numpy(p0[rows].astype(np.float64)))
        if rule == 0:
            opt = torch.optim.Adam([q], lr=h['lr'], weight_decay=h['wd'] if wd else 0.0, betas=(h['beta1'], h['beta2']), eps=h['eps'], foreach=False)
            opt.state[q] = {'step': torch.tensor(float(L)), 'exp_avg': torch.from_numpy(m0[rows].astype(np.float64)),
                            'exp_avg_sq': torch.from_numpy(v0[rows].astype(np.float64))}
        elif rule == 1:
            opt = torch.optim.Adagrad([q], lr=h['lr'], weight_decay=h['wd'], eps=h['eps'], foreach=False)
            opt.state[q] = {'step': torch.tensor(float(L)), 'sum': torch.from_numpy(v0[rows].astype(np.float64))}
        else:
            opt = torch.optim.SGD([q], lr=h['lr'], weight_decay=h['wd'], foreach=False)
        for s in range(L + 1, t + 1):
            if s == t and not with_step:
                q.grad = torch.zeros_like(q)
            elif s == t:
                q.grad = torch.from_numpy(0.5 * g[rows].astype(np.float64))
            else:
                q.grad = torch.zeros_like(q)
            opt.step()
        _close(got[0][rows], q.detach().numpy(), (rule, 'p', L))
        if rule == 0:
            _close(got[1][rows], opt.state[q]['exp_avg'].numpy(), 'm')
            _close(got[2][rows], opt.state[q]['exp_avg_sq'].numpy(), 'v')
        elif rule == 1:
            _close(got[2][rows], opt.state[q]['sum'].numpy(), 'sum')
            assert np.array_equal(got[1][rows], m0[rows].astype(np.float64))


def test_skipped_step_books():
    rc = C.reduce_case(64, 'm_S_p1')
    for skip in ('count', 'value'):
        c = C.apply_case(rc, 'adagrad', skip=skip)
        c['max_norm'] = 0.0
        gsum, delta, cnt = _gradient(rc)
        ref = R.apply_ref(c, gsum, delta, (c['ids'] >= 0) & (cnt > 0), 1.0, 0.0)
        assert all(not tol.any() and np.array_equal(want, P.astype(np.float64)) for (want, tol), P in zip(ref['tables'], c['tables']))
        assert np.array_equal(ref['loss_sum'], c['loss_sum']) and ref['skipped'] == 6 and not ref['loss_step'].any()


# ------------------------------------------------------------------------------------------------ (2) check_route
def _model(rc):
    pa, pb = rc['pair'] if rc['pair'] else (None, None)
    return R.route_model(rc['ids'], rc['block'], rc['ent_off'], rc['world'], rc['cap'], pa, pb)


def _check(rc, out):
    pa, pb = rc['pair'] if rc['pair'] else (1, 2)
    R.check_route(rc['ids'], rc['block'], rc['ent_off'], rc['world'], rc['cap'], out['inverse'], out['send_ids'],
                  out['pair_map'] if rc['pair'] else None, out['counters'], out['sort_ws'], pa, pb)


@pytest.mark.parametrize('name', C.ROUTES + C.OVERFLOW + C.SCAN[:6], ids=str)
def test_check_route_accepts_a_numpy_route(name):
    rc = C.route_case(name)
    _check(rc, _model(rc))


@pytest.mark.parametrize('d,name', [(64, 'padded'), (100, 'ktup'), (256, 'consecutive')])
def test_geometry_cases_route_to_the_stated_rows(d, name):
    """world = 64, cap = 1: the wire row of (id, table) is id T + table whatever the arrival order; the sorted keys follow."""
    rc = C.reduce_case(d, name)
    out = R.route_model(rc['ids'], rc['n'], rc['ent_off'], rc['world'], rc['cap'], *(rc['pair'] or (None, None)))
    assert np.array_equal(out['inverse'], rc['inverse'])
    lay = R.sort_layout(rc['n'], rc['W'])
    assert np.array_equal(out['sort_ws'][lay['skey']:lay['skey'] + rc['m']], rc['skey'])


# ------------------------------------------------------------------------------------------------ (3) one defect each
def _route_defect(which):
    rc = C.route_case(('pair',))
    out = _model(rc)
    lay = R.sort_layout(len(rc['ids']), rc['world'] * sum(rc['cap']))
    inv = out['inverse']
    if which == 'swapped_rows':
        rows = np.unique(inv[rc['ids'] >= 0])
        a, b = rows[3], rows[4]
        out['inverse'] = np.where(inv == a, b, np.where(inv == b, a, inv))
    elif which == 'repeated_rank':
        e = np.nonzero(out['sort_ws'][lay['rank']:lay['rank'] + len(inv)] == 1)[0][0]
        out['sort_ws'][lay['rank'] + e] = 0
    elif which == 'start_W':
        out['sort_ws'][rc['world'] * sum(rc['cap'])] += 1
    elif which == 'send_ids_pad':
        free = np.nonzero(out['send_ids'] == -1)[0]
        out['send_ids'][free[len(free) // 2]] = 0
    return rc, out


@pytest.mark.parametrize('which', ['swapped_rows', 'repeated_rank', 'start_W', 'send_ids_pad'])
def test_check_route_rejects(which):
    rc, out = _route_defect(which)
    with pytest.raises(AssertionError):
        _check(rc, out)


def _reduced(rc, store):
    d, W = rc['d'], rc['W']
    before = np.full((W, rc['ld']), np.nan, np.float32)
    if not store:
        before[:, :d] = np.random.default_rng(3).standard_normal((W, d)).astype(np.float32)
    got = before.copy()
    cnt = np.bincount(rc['inverse'][rc['ids'] >= 0], minlength=W + 1)[:W]
    emu = R.emulate_reduce(rc['G'], rc['n_src'], rc['src_off'], rc['inverse'], W, d, None if store else before)
    rows = cnt > 0
    got[rows, :d] = emu[rows]
    return before, got


@pytest.mark.parametrize('store', [False, True])
@pytest.mark.parametrize('which', ['entry_missing', 'row_twice'])
def test_check_reduced_rejects(which, store):
    """One entry's contribution missing from a boundary row; one row's contribution added twice."""
    rc = C.reduce_case(64, 'stretch_p2')
    before, got = _reduced(rc, store)
    R.check_reduced(got, before, rc['G'], rc['n_src'], rc['src_off'], rc['inverse'], 64, store)
    b = _boundary(rc)[0]
    if which == 'entry_missing':
        e = np.nonzero(rc['inverse'] == b)[0][5]
        got[b, :64] -= rc['G'][e, :64]
    else:
        got[b, :64] += R.reduce_ref(rc['G'], rc['n_src'], rc['src_off'], rc['inverse'], rc['W'], 64)[b].astype(np.float32)
    with pytest.raises(AssertionError):
        R.check_reduced(got, before, rc['G'], rc['n_src'], rc['src_off'], rc['inverse'], 64, store)


@pytest.mark.parametrize('which', ['short_by_one_entry', 'full_where_dup_only'])
def test_check_sumsq_rejects(which):
    rc = C.reduce_case(64, 'consecutive')
    args = (rc['G'], rc['n_src'], rc['src_off'], rc['inverse'], rc['W'], 64)
    for dup in (0, 1):
        want, tol = R.sumsq_ref(*args, rc['n'], dup, _boundary(rc))
        R.check_sumsq(R.emulate_sumsq(*args, dup), want, tol)
    full, _ = R.sumsq_ref(*args, rc['n'], 0, _boundary(rc))
    with pytest.raises(AssertionError):
        if which == 'short_by_one_entry':
            smallest = min(float((rc['G'][e, :64].astype(np.float64) ** 2).sum()) for e in np.nonzero(rc['ids'] >= 0)[0])
            want, tol = R.sumsq_ref(*args, rc['n'], 0, _boundary(rc))
            R.check_sumsq(want - smallest, want, tol)
        else:
            want, tol = R.sumsq_ref(*args, rc['n'], 1, _boundary(rc))
            R.check_sumsq(full, want, tol)


def _applied(rc, c, form, sumsq=None):
    """The fp32 emulation of a whole apply launch, in check_apply's `got` layout."""
    d, W = c['d'], rc['W']
    gsum, delta, cnt = _gradient(rc)
    weight = 2.0 if any(s['p1'] is not None for s in c['smalls']) else 1.0
    if sumsq is None:
        sumsq = float((gsum ** 2).sum()) + weight * sum(float((s['g'].astype(np.float64) ** 2).sum()) for s in c['smalls'])
    c['max_norm'] = C.max_norm_of(c['clip'], sumsq)
    g32 = R.emulate_reduce(rc['G'], rc['n_src'], rc['src_off'], rc['inverse'], W, d)
    if form == 'buffer':                                               # ktup_shard_apply: the fp32 buffer IS the gradient
        gsum, delta, touched = g32.astype(np.float64), np.zeros_like(gsum), c['ids'] >= 0
    else:
        touched = (c['ids'] >= 0) & (cnt > 0)
    ref = R.apply_ref(c, gsum, delta, touched, sumsq, 0.0)
    skip = bool(c['skip_count']) or c['skip_value'] != 0.0
    coef = np.float32(ref['coef'])
    got = {'tables': [P.copy() for P in c['tables']], 'states': [S.copy() for S in c['states'] or []], 'small': []}
    adam = c['kind'] == R.ADAM
    wt = np.arange(W) % c['T']

    def step(P, S, rows, g):
        m = S[rows, :d] if adam else None
        v = S[rows, d:2 * d] if adam else (S[rows, :d] if S is not None else None)
        p, m, v = R.emulate_rule(c, P[rows, :d], g, m, v, coef)
        if adam:                                                       # rows that owe steps: the same recurrence in fp32
            last = S[rows, 2 * d].view(np.int32)
            st = np.nonzero(last < c['t'] - 1)[0]
            if len(st):
                rs = rows[st]
                p[st], m[st], v[st] = R.lazy_rows(c, P[rs, :d], S[rs, :d], S[rs, d:2 * d], last[st], g[st], float(coef), np.float32)
        P[rows, :d] = p
        if adam:
            S[rows, :d], S[rows, d:2 * d] = m, v
            S[rows, 2 * d] = np.full(len(rows), c['t'], np.int32).view(np.float32)
        elif S is not None:
            S[rows, :d] = v
    if not skip:
        for t in range(c['T']):
            rows_w = np.nonzero((wt == t) & touched)[0]
            step(got['tables'][t], got['states'][t] if got['states'] else None, c['ids'][rows_w], g32[rows_w])
    for sm in c['smalls']:
        res = {'g': np.zeros_like(sm['g'])}
        g = sm['g'] if sm['g64'] is None else sm['g64'].astype(np.float32)
        for which in ('0', '1'):
            res['p' + which] = None if sm['p' + which] is None else sm['p' + which].copy()
            res['s' + which] = None if sm['s' + which] is None else sm['s' + which].copy()
            if res['p' + which] is not None and not skip:
                step(res['p' + which], res['s' + which], np.arange(g.shape[0]), g)
        got['small'].append(res)
    grads = np.zeros((W, d), np.float32)
    got['grads_before'] = grads.copy()
    got['grads'], got['grads_zero'] = grads, np.ones((W, d), bool)
    got['loss_step'] = np.zeros_like(c['loss_step'])
    got['loss_sum'] = c['loss_sum'] if skip else c['loss_sum'] + c['loss_step']
    got['skipped'] = c['skipped'] + (1 if skip else 0)
    return ref, got


@pytest.mark.parametrize('which', ['row_not_zeroed', 'loss_on_skipped_step'])
def test_check_apply_rejects(which):
    rc = C.reduce_case(64, 'each_side')
    c = C.apply_case(rc, 'adagrad', skip='count' if which == 'loss_on_skipped_step' else None)
    ref, got = _applied(rc, c, 'fused')
    R.check_apply(c, ref, got)
    if which == 'row_not_zeroed':
        got['grads'][17, 3] = np.float32(1e-30)
    else:
        got['loss_sum'] = c['loss_sum'] + c['loss_step']
    with pytest.raises(AssertionError):
        R.check_apply(c, ref, got)


# ------------------------------------------------------------------------------------------------ (4) every case, emulated in fp32
@pytest.mark.parametrize('case', C.CASES, ids=C.case_id)
def test_every_reduce_case_keeps_fp32_inside_the_tolerance(case):
    rc = C.reduce_case(*case)
    d, name = case[0], C.case_id(case)
    assert rc['m'] == int((rc['ids'] >= 0).sum()) and (np.diff(rc['skey']) >= 0).all()
    worst = []
    for store in (False, True):
        before, got = _reduced(rc, store)
        worst.append(R.check_reduced(got, before, rc['G'], rc['n_src'], rc['src_off'], rc['inverse'], d, store))
    args = (rc['G'], rc['n_src'], rc['src_off'], rc['inverse'], rc['W'], d)
    smalls = C.small_grads(rc, 2)
    for dup in (0, 1):
        G = C.dup_only_G(rc) if dup else rc['G']
        a = (G,) + args[1:]
        want, tol = R.sumsq_ref(*a, rc['n'], dup, _boundary(rc), smalls, 2.0, None, rc['opt'])
        worst.append(R.check_sumsq(R.emulate_sumsq(*a, dup, smalls, 2.0), want, tol))
    print('d %4d %-28s fp32 emulation / tolerance: rows %.3f store %.3f sumsq %.3f dup_only %.3f' % ((d, name) + tuple(worst)))


@pytest.mark.parametrize('form', ['fused', 'buffer'])
@pytest.mark.parametrize('case', C.CASES, ids=C.case_id)
def test_every_apply_case_keeps_fp32_inside_the_tolerance(case, form):
    """Every reduce case with every option set the GPU test runs."""
    rc = C.reduce_case(*case)
    for kind, clip, skip, n_small, second, g64, slots, stale in C.APPLY_OPTIONS:
        c = C.apply_case(rc, kind, clip=clip, skip=skip, n_small=n_small, second=second, g64=g64, slots=slots, boundary=_boundary(rc),
                         stale=stale)
        ref, got = _applied(rc, c, form)
        print('%-28s %-10s %-6s clip %-8s skip %-5s fp32 emulation / tolerance %.3f'
              % (C.case_id(case), kind, form, clip, skip, R.check_apply(c, ref, got)))


# ------------------------------------------------------------------------------------------------ (5) the Adam replay's tolerance
def test_adam_replay_fp32_error_is_the_tolerance():
    """Measured here (printed): the largest |fp32 - fp64| of the step-by-step replay over the catch-up cases of
    tests/test_hip_shard_abi.py.  The GPU test allows 4 x these figures (R.replay_tolerance computes them from the same case).
    Measured: gap 3: p 1.34e-06 absolute, m 6.7e-07, v 8.15e-07 relative; gap 20: p 1.30e-06, m 7.95e-07, v 8.0e-07.  Under weight
    decay 1e-2 (m absolute there, R._measured), gap 3 / gap 20: Adam p 7.96e-07 / 9.85e-07, m 9.45e-09 / 9.82e-09, v 1.15e-06 /
    1.44e-06; Adagrad p 1.76e-06 / 1.58e-06, v 9.03e-07 / 1.02e-06, m not written; SGD p 4.61e-07 / 6.74e-07, m and v not written."""
    for gap in C.CATCHUP_GAPS:
        for rule, wd in ((0, 0.0), (0, 1e-2), (1, 1e-2), (2, 1e-2)):      # under weight decay: every owed step on wd * p (R.lazy_rows)
            c = C.catchup_case(gap, rule=rule, wd=wd)
            tol = R.replay_tolerance(c)
            want = dict(zip('pmv', R.replay_expected(c)))
            fig = {k: float(tol[k].max()) / 4 if k == 'p' or (k == 'm' and wd) else float((tol[k] / np.maximum(np.abs(want[k]), 1e-300)).max()) / 4
                   for k in 'pmv'}
            print('gap %3d rule %d wd %g: fp32 replay error  p %.3g (abs)  m %.3g (%s)  v %.3g (relative)'
                  % (gap, rule, wd, fig['p'], fig['m'], 'abs' if wd else 'relative', fig['v']))
            assert 0 < fig['p'] < 1e-5 and (fig['m'] > 0) == (rule == 0) and (fig['v'] > 0) == (rule != 2) and fig['m'] < 1e-5 and fig['v'] < 1e-5
