"""Pins tests/_loss_ref.py on the CPU: (1) the reference against torch fp64 autograd of oracle.cpu_ref.{bpr_loss, margin_loss,
norm_loss, orthogonal_loss} per element at 1e-12 of scale (on inputs without exact ties: torch's clamp passes a gradient AT the
edge, the kernels' header does not; the ties are pinned separately); (2) the comparator; (3) the builders' promises for every
case tests/test_hip_loss_abi.py launches; (4) the tolerances against an fp32 numpy emulation of the kernels' summation
(lane-strided chunks, xor-shuffle tree, 4-way block sum, workgroup partials added in two different orders, the gradient adds of
a cell in two orders) at the widest rung of each path.  Largest error / tolerance of (4), as printed by test_tolerance_sanity:
    float4 G64x4 d = 1024, 513 rows:  norm value 0.057  gT 0.822   orth value 0.015  gRel 0.085  gNrm 0.129
    float  G64x4 d =  255, 513 rows:  norm value 0.063  gT 0.778   orth value 0.004  gRel 0.118  gNrm 0.241
    margin n = 65537: value 0.038
gT is high because most of its cells receive ONE add: two roundings (the product 1.5 x, the add onto g0), and among thousands of
cells some come near both bounds at once.  The values are low because the bound adds 513 rows' worst cases with one sign while
the errors add like a random walk (1 / sqrt(513) = 0.044 of it), orth more so since its row bound E D also assumes every
product of w . r rounds the same way."""
import numpy as np
import pytest
import torch

from oracle import cpu_ref as O
from tests import _loss_ref as R


def _rel(got, want, scale, what):
    err = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64))
    assert np.all(err <= 1e-12 * np.maximum(np.asarray(scale, dtype=np.float64), 1e-300)), (what, float(np.max(err)))


# ------------------------------------------------------------------------------------------------ (1) against autograd
@pytest.mark.parametrize('d,how,mode,n', [(7, '', 'ids', 40), (64, 'pitch4', 'null', 33), (260, '', 'heavy', 9), (129, '', 'ids', 5)])
def test_regularisers_match_autograd(d, how, mode, n):
    c = R.reg_case('x', d, how, n, mode)
    T, W = c['T'].view().copy(), c['W'].view().copy()
    T[:3], W[:3] = R.drawn_rows(np.random.default_rng(d), 3, d), W[3:6]       # no exact edge rows here (see the module docstring)
    s = R.check_rows(T)
    assert not (s == 1.0).any()
    gl, g0, gw0 = c['gloss'], c['G'].view(), c['GW'].view()
    rows = np.arange(c['n']) if c['ids'] is None else c['ids']
    Tt, Wt = torch.from_numpy(T.astype(np.float64)).requires_grad_(True), torch.from_numpy(W.astype(np.float64)).requires_grad_(True)
    idx = torch.from_numpy(np.asarray(rows, dtype=np.int64))
    vn = O.norm_loss(Tt[idx])
    gn, = torch.autograd.grad(vn * float(np.float32(gl)), Tt)
    vo = O.orthogonal_loss(Tt[idx], Wt[idx])
    gr, gw = torch.autograd.grad(vo * float(np.float32(gl)), (Tt, Wt))
    vec4 = c['vec4_bwd']
    rn = R.norm_ref(T, c['ids'], c['n'], gl, g0, vec4, slot0=2.5)
    ro = R.orth_ref(T, W, c['ids'], c['n'], gl, g0, gw0, vec4, slot0=2.5)
    _rel(rn['value'][0] - 2.5, vn.item(), vn.item() + 2.5, 'norm value')
    _rel(ro['value'][0] - 2.5, vo.item(), vo.item() + 2.5, 'orth value')
    occ = R._scatter(T.shape, rows, np.ones((len(rows), d)))
    for got, want, base, scale in ((rn['gT'][0], gn, g0, 2 * np.abs(T) * occ), (ro['gR'][0], gr, g0, None), (ro['gW'][0], gw, gw0, None)):
        want = want.numpy() + base.astype(np.float64)
        _rel(got, want, np.abs(base) + (scale if scale is not None else np.abs(want) + np.abs(got) + 1.0), 'gradient')
    # the tolerances are positive exactly where an add lands, and rows no id names are exact
    named = np.zeros(len(T), dtype=bool); named[rows] = True
    assert not rn['gT'][1][~named].any() and not ro['gR'][1][~named].any() and not ro['gW'][1][~named].any()
    if float(gl) != 0.0:
        assert (ro['gW'][1][named] > 0).all()
    else:
        assert not rn['gT'][1].any() and not ro['gR'][1].any()


@pytest.mark.parametrize('kind,param', [('bpr', 1.0), ('bpr', -1.0), ('margin', 0.5)])
@pytest.mark.parametrize('n', [1, 257, 65537])
def test_pair_losses_match_autograd(kind, param, n):
    c = R.pair_case(kind, param, n)
    p, q = (torch.from_numpy(c[k].astype(np.float64)).requires_grad_(True) for k in ('pos', 'neg'))
    v = O.bpr_loss(p, q, param) if kind == 'bpr' else O.margin_loss(p, q, param)
    gp, gq = torch.autograd.grad(v * float(np.float32(c['gloss'])), (p, q))
    ref = R.pair_ref(kind, c['pos'], c['neg'], param, c['gloss'], slot0=2.5)
    _rel(ref['value'][0] - 2.5, v.item(), abs(v.item()) + 2.5, 'value')
    _rel(ref['gpos'][0], gp.numpy(), np.abs(gp.numpy()), 'gpos')
    _rel(ref['gneg'][0], gq.numpy(), np.abs(gq.numpy()), 'gneg')
    assert ref['value'][1] > 0 and (kind == 'margin' or float(c['gloss']) == 0.0) == (not ref['gpos'][1].any())


def test_ties_follow_the_header():
    """pos = 1, neg = 2, margin = 1: value 0, gradient exactly 0 (tolerance 0); rows with s == 1: value 0, gradient row exact."""
    ref = R.pair_ref('margin', np.array([1.0, 5.0], dtype=np.float32), np.array([2.0, 1.0], dtype=np.float32), 1.0, 0.75)
    assert ref['value'][0] == 5.0 and ref['gpos'][0].tolist() == [0.0, 0.75] and not ref['gpos'][1].any()
    for d in (1, 4, 50):
        rows = R.edge_rows(d)
        T = np.stack([r for r, _ in rows])
        g0 = np.full(T.shape, 0.3, dtype=np.float32)
        ref = R.norm_ref(T, None, len(T), 1.0, g0, False)
        for i, (row, active) in enumerate(rows):
            s32 = np.float32(0.0)
            for x in row[::-1]:
                s32 = np.float32(s32 + x * x)
            assert (float(s32) > 1.0) == active and (float((row.astype(np.float64) ** 2).sum()) == float(s32))
            assert bool(ref['gT'][1][i].any()) == active
            if not active:
                assert np.array_equal(ref['gT'][0][i], g0[i].astype(np.float64))
        assert ref['value'][0] == 2.0 ** -10 + 2.0 ** -22


# ------------------------------------------------------------------------------------------------ (2) the comparator
def test_comparator():
    want, tol = np.array([1.0, 2.0, 3.0]), np.array([1e-3, 0.0, 1e-3])
    assert R.compare(np.array([1.0005, 2.0, 3.0], dtype=np.float32), want, tol) == pytest.approx(0.5, rel=1e-3)
    for bad in ([1.0015, 2.0, 3.0], [np.nan, 2.0, 3.0], [1.0, 2.0, np.inf], [1.0, np.float32(2.0) + np.float32(2.0 ** -22), 3.0]):
        with pytest.raises(AssertionError):
            R.compare(np.array(bad, dtype=np.float32), want, tol)
    with pytest.raises(AssertionError):
        R.compare(np.array([1.0], dtype=np.float32), np.array([np.nan]), np.array([1.0]))
    with pytest.raises(AssertionError):
        R.compare(np.array([1.0], dtype=np.float32), np.array([1.0]), np.array([np.nan]))
    assert R.compare(np.float32(2.0), 2.0, 0.0) == 0.0
    R.same_bits(np.array([0.0, R.SENTINEL], dtype=np.float32), np.array([0.0, R.SENTINEL], dtype=np.float32))
    with pytest.raises(AssertionError):                                   # guards by bits: -0.0 is not 0.0
        R.same_bits(np.array([-0.0], dtype=np.float32), np.array([0.0], dtype=np.float32))
    t = R.Table(np.ones((3, 5), dtype=np.float32), 7, 1)
    assert t.guard().sum() == len(t.flat) - 15 and (t.flat[t.guard()] == R.SENTINEL).all() and len(t.flat) % 4 == 0
    assert t.start % 4 == 1 and t.guard()[t.start + 5] and t.guard()[t.start + 6] and not t.guard()[t.start + 7]


# ------------------------------------------------------------------------------------------------ (3) the builders
def test_every_regulariser_case_keeps_its_promises():
    specs = R.rung_cases() + R.seam_cases() + R.serial_cases()
    reached, hows = set(), set()
    for spec in specs:
        c = R.reg_case(*spec)
        R.check_reg_case(c)
        reached.add((c['name'], c['d']))
        hows.add(c['how'])
        s = (c['T'].view().astype(np.float64) ** 2).sum(1)
        assert sorted({1.0, 1.0 + 2.0 ** -10 + 2.0 ** -22} & set(s.tolist())) == [1.0, 1.0 + 2.0 ** -10 + 2.0 ** -22]
    want = {(name, d) for table in (R.F4_RUNGS, R.F1_RUNGS) for name, ds in table.items() for d in ds}
    assert want <= reached and hows == {'', 'pitch1', 'pitch4', 'offset', 'grad'}
    assert {g for g in R.GLOSS} == {R.reg_case(*spec)['gloss'] for spec in specs if spec[3] < 100}
    for d, how in R.REFUSED_D:
        c = R.reg_case('refused', d, how, 5, 'ids', 8)
        assert R.rung(d, c['vec4_fwd']) is None and R.rung(d, c['vec4_bwd']) is None
    assert R.rung(1024, True) == (4, 64, 4) and R.rung(256, False) == (1, 64, 4) and R.rung(1028, True) is None


def test_hinge_margin_of_drawn_rows():
    """(d + 8) u s <= 7e-4 |s - 1| for rows drawn at every d of the ladder tables and at 1024, 200 rows per width."""
    worst = 0.0
    for d in sorted({d for t in (R.F4_RUNGS, R.F1_RUNGS) for ds in t.values() for d in ds}):
        x = R.drawn_rows(np.random.default_rng(d), 200, d).astype(np.float64)
        s = (x * x).sum(1)
        worst = max(worst, float(((d + 8) * R.U * s / np.abs(s - 1.0)).max()))
    print('largest (d + 8) u s / |s - 1| = %.3g' % worst)
    assert worst <= R.EDGE_CLEAR


def test_every_pair_case_keeps_its_promises():
    for kind, param in R.PAIR_KINDS:
        for n in R.PAIR_N:
            c = R.pair_case(kind, param, n)
            assert len(c['pos']) == n and c['pos'].dtype == np.float32
            if kind == 'margin':
                R.check_pair(c['pos'], c['neg'], param)
                if n > 3 and param == 1.0:
                    assert c['pos'][3] == 1.0 and c['neg'][3] == 2.0
            elif n >= 255:
                x = param * (c['pos'].astype(np.float64) - c['neg'].astype(np.float64))
                assert x.min() < -25 and x.max() > 25 and np.abs(x).max() < 30.001 and np.abs(x).min() < 0.5
    assert {R.pair_case(k, p, n)['gloss'] for k, p in R.PAIR_KINDS for n in R.PAIR_N} == set(R.GLOSS)


# ------------------------------------------------------------------------------------------------ (4) tolerance sanity
F = np.float32


def emu_row_sum(X, Y, w, g, cpl):
    """sum_j X Y per row as a G-lane group forms it: chunk c = lane + j G, dot4 as a chain from .w down (product and add rounded
    separately), CPL chunks per lane in order, then the xor tree.  fp32 throughout."""
    n, d = X.shape
    width = g * cpl * w
    Xp, Yp = np.zeros((n, width), dtype=F), np.zeros((n, width), dtype=F)
    Xp[:, :d], Yp[:, :d] = X, Y
    P = (Xp * Yp).reshape(n, cpl, g, w)
    lane = np.zeros((n, g), dtype=F)
    for j in range(cpl):
        chunk = P[:, j, :, w - 1]
        for k in range(w - 2, -1, -1):
            chunk = P[:, j, :, k] + chunk
        lane = lane + chunk
    m = g // 2
    while m >= 1:
        lane = lane + lane[:, np.arange(g) ^ m]
        m //= 2
    assert lane.dtype == F
    return lane[:, 0]


def emu_scalar_sum(v, g, slot0, reverse):
    """Row values -> thread partials (row-strided trips) -> wave tree -> 4-way block sum -> one atomic per workgroup."""
    n, gpb = len(v), 256 // g
    _, grid = R.reduce_sum_count(n, g)
    part = np.zeros((grid, 256), dtype=F)
    for row in range(n):
        b, grp = (row // gpb) % grid, row % gpb
        part[b, grp * g] = part[b, grp * g] + v[row]
    waves = part.reshape(grid, 4, 64)
    m = 32
    while m >= 1:
        waves = waves + waves[:, :, np.arange(64) ^ m]
        m //= 2
    red = waves[:, :, 0]
    tot = ((red[:, 0] + red[:, 1]) + red[:, 2]) + red[:, 3]
    out = F(slot0)
    for b in (range(grid - 1, -1, -1) if reverse else range(grid)):
        out = F(out + tot[b])
    return out


def emu_cells(g0, rows, add, reverse):
    out = g0.copy()
    order = range(len(rows) - 1, -1, -1) if reverse else range(len(rows))
    for i in order:
        out[rows[i]] = out[rows[i]] + add[i]
    assert out.dtype == F
    return out


@pytest.mark.parametrize('name,d', [('f4/G64x4', 1024), ('f1/G64x4', 255)])
def test_tolerance_sanity(name, d):
    """The largest cases in fp32 emulation against the fp64 reference: every ratio below 1 (the tolerance holds for a rounding
    at every counted place) and not below 0.001 (it is not loose beyond what the module docstring explains)."""
    c = R.reg_case(name, d, '', 513, 'ids', 64)
    R.check_reg_case(c)
    T, W, g0, gw0, rows, gl = c['T'].view(), c['W'].view(), c['G'].view(), c['GW'].view(), c['ids'], F(c['gloss'])
    w, g, cpl = R.rung(d, c['vec4_bwd'])
    assert (w, g, cpl) == ((4, 64, 4) if d % 4 == 0 else (1, 64, 4)) and float(gl) != 0.0
    X, Y = T[rows], W[rows]
    worst = {}
    s = emu_row_sum(X, X, w, g, cpl)
    act = (s - F(1.0)) > 0
    v = np.maximum(s - F(1.0), F(0.0))
    rn = R.norm_ref(T, rows, len(rows), gl, g0, c['vec4_bwd'], slot0=2.5)
    add = np.where(act[:, None], (F(2.0) * gl) * X, F(0.0)).astype(F)
    dot, nr = emu_row_sum(X, Y, w, g, cpl), s
    vo = dot * dot / nr
    c1, c2 = (gl * F(2.0) * dot / nr)[:, None], (gl * F(2.0) * dot * dot / (nr * nr))[:, None]
    add_r, add_w = (-c2) * X + c1 * Y, c1 * X
    ro = R.orth_ref(T, W, rows, len(rows), gl, g0, gw0, c['vec4_bwd'], slot0=2.5)
    for rev in (False, True):
        for key, got, (want, tol) in (('norm value', emu_scalar_sum(v, g, 2.5, rev), rn['value']), ('gT', emu_cells(g0, rows, add, rev), rn['gT']),
                                      ('orth value', emu_scalar_sum(vo, g, 2.5, rev), ro['value']),
                                      ('gRel', emu_cells(g0, rows, add_r.astype(F), rev), ro['gR']),
                                      ('gNrm', emu_cells(gw0, rows, add_w.astype(F), rev), ro['gW'])):
            worst[key] = max(worst.get(key, 0.0), R.compare(got, want, tol, key))
    print(name, d, '  '.join('%s %.3f' % kv for kv in worst.items()))
    assert all(0.001 <= r < 1.0 for r in worst.values()), worst


def test_tolerance_sanity_margin():
    c = R.pair_case('margin', 0.5, 65537)
    arg = (c['pos'] - c['neg']) + F(0.5)
    t = np.maximum(arg, F(0.0))
    _, grid = R.pair_sum_count(len(t))
    part = np.zeros((grid, 256), dtype=F)
    idx = np.arange(len(t))
    for trip in range(-(-len(t) // (grid * 256))):
        sel = idx[trip * grid * 256:(trip + 1) * grid * 256]
        np.add.at(part, ((sel // 256) % grid, sel % 256), t[sel])                  # one element per thread and trip: plain fp32 adds
    waves = part.reshape(grid, 4, 64)
    m = 32
    while m >= 1:
        waves = waves + waves[:, :, np.arange(64) ^ m]
        m //= 2
    red = waves[:, :, 0]
    tot = ((red[:, 0] + red[:, 1]) + red[:, 2]) + red[:, 3]
    want, tol = R.pair_ref('margin', c['pos'], c['neg'], 0.5, 1.0, slot0=2.5)['value']
    worst = 0.0
    for order in (range(grid), range(grid - 1, -1, -1)):
        out = F(2.5)
        for b in order:
            out = F(out + tot[b])
        worst = max(worst, R.compare(out, want, tol, 'margin value'))
    print('margin value %.4f' % worst)
    assert 0.001 <= worst < 1.0
