"""GPU parity of the loss / regulariser launches (csrc/ktup_loss.hip, K8-K10) through the C ABI (jTransUP.hip.lib.call) against
tests/_loss_ref.py: fp64 from the same fp32 inputs, every element of every output at the tolerances derived there (pinned on the
CPU by tests/test_loss_ref_host.py).  Every case runs all entries of its family: _fwd (onto a slot preloaded with garbage), _bwd
and _fused (onto a slot holding 2.5 and onto non-zero gradient tables), and the fused value against the fwd value.  Exact facts
next to the tolerances: sentinel floats around every buffer and in the pitch padding of every table bit-identical, rows no id
names bit-identical, inactive rows / exact ties bit-identical, gneg == -gpos by bits, inputs unchanged.  Each case prints its
largest error / tolerance; test_zz_report prints the largest per entry.

Regulariser cases: every rung of both ladders of ktup_rows.h (tests/_loss_ref.py RUNG_CASES), the float path reached by d % 4,
by pitch d + 1, by a 4-byte base offset and by misaligned gradient tables alone; row counts 1, 256/G - 1, 256/G, 256/G + 1; the
second trip of both capped grids; ids and ids = NULL; a row listed more than 64 times.

Recorded on the MI355X (182 cases, about 700 launches, 4.2 s): largest error / tolerance per entry
    ktup_loss_bpr_fwd 0.371  _bwd 0.768  _fused 0.768        ktup_loss_margin_fwd 0.088  _bwd exact  _fused 0.088
    ktup_reg_norm_fwd 0.135  _bwd 0.984  _fused 0.984        ktup_reg_orth_fwd    0.054  _bwd 0.492  _fused 0.677
and the libm measurement gpos 1.294, single-element value 0.719 (units of 2^-23 of the element; allowances 3 and 2).  The norm
gradient comes near its bound because most cells receive ONE add = two roundings (the product 1.5 x at gloss 0.75, the add onto
g0), and a ids = NULL case has 2.8e5 such cells, some of which sit near both bounds at once; the fp32 emulation of
tests/test_loss_ref_host.py gives 0.82 on 3e4 cells.  With gloss 1 or -2 the product is exact and the same cells stay below 0.5.
Scratch mutants of csrc/ (arithmetic only, never committed) and the tests that failed, [old] = tests/test_hip_loss.py:
  1 `s - 1 > 0` -> `>=` in NormFused          every_rung, grid_seams, serial_mode, graph_replay (the s == 1 rows)       [old: none]
  2 c2 without one factor of dot               every_rung, grid_seams, serial_mode, graph_replay      [old: goldens, fused entries]
  3 float load: out-of-range chunk = chunk 0   every_rung at d = 65, 100, 129, 255 only, serial_mode d = 65, perpendicular [old: none]
  4 `part += v` on every lane                  every value of the row kernels, sums_in_row_order      [old: goldens, fused, gathered]
  5 mean scale dropped in pair_loss_fused      pair_losses (bpr, n > 1)                               [old: fused entries n > 1]
  6 sigmoid(-x) -> sigmoid(x) in the gradient  pair_losses (bpr), bpr_libm_allowance                  [old: goldens, sizes, fused]
  7 float4 G64x4 OrthFwd skips its last chunk  every_rung at d = 1024 only                                               [old: none]
  8 serial flag ignored in row_reduce_kernel   sums_in_row_order only                                                    [old: none]

Not covered: a zero Rel row in orth (NaN in the kernel and in the reference alike)."""
import math

import numpy as np
import pytest
import torch

from tests import _loss_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
WORST = {}                                                            # entry -> largest error / tolerance of the module
MEASURED = {}                                                         # the libm measurement of test_bpr_libm_allowance
GARBAGE, PRELOAD = 123.5, 2.5


def lib():
    from jTransUP.hip import lib as L
    return L


def stream():
    return torch.cuda.current_stream().cuda_stream


class Dev:
    """A flat fp32 buffer on the GPU (16-byte aligned base) and float-indexed pointers into it."""

    def __init__(self, flat):
        self.before = np.array(flat, dtype=np.float32, copy=True)
        self.t = torch.from_numpy(self.before.copy()).to(DEV)
        assert self.t.data_ptr() % 16 == 0

    def ptr(self, start=0):
        return self.t.data_ptr() + 4 * start

    def host(self):
        torch.cuda.synchronize()
        return self.t.cpu().numpy()


def note(entry, what, ratio):
    prev = WORST.get(entry, 0.0)
    WORST[entry] = ratio if not ratio <= prev else prev                                     # (keeps a NaN)
    return '%s %s %.3f' % (entry.replace('ktup_', ''), what, ratio)


def check_slot(entry, dev, want, tol):
    h = dev.host()
    R.same_bits(np.delete(h, 4), np.delete(dev.before, 4), entry + ' slot guards')
    return note(entry, 'value', R.compare(h[4], want, tol, entry + ' value'))


def check_table(entry, what, dev, table, want, tol):
    h = dev.host()
    g = table.guard()
    R.same_bits(h[g], dev.before[g], entry + ' guards of ' + what)
    return note(entry, what, R.compare(table.view(h), want, tol, entry + ' ' + what))


def unchanged(*devs):
    for d in devs:
        R.same_bits(d.host(), d.before, 'an input')


# ------------------------------------------------------------------------------------------------ regularisers
def run_reg(c, serial=False):
    """All six regulariser entries on one case.  Returns the raw fp32 outputs (for the bit-for-bit comparison of serial runs)."""
    L = lib()
    T, W, G, GW, n, d, ld, gl = c['T'], c['W'], c['G'], c['GW'], c['n'], c['d'], c['ld'], c['gloss']
    dT, dW, dgl = Dev(T.flat), Dev(W.flat), Dev(R.scalar_slot(gl))
    ids = None if c['ids'] is None else torch.from_numpy(c['ids']).to(DEV)
    idp = None if ids is None else ids.data_ptr()
    tp, wp, st = dT.ptr(T.start), dW.ptr(W.start), stream()
    out, raw = [], []
    kw = dict(serial=serial)
    # ---- norm
    rf = R.norm_ref(T.view(), c['ids'], n, gl, G.view(), c['vec4_fwd'], **kw)
    rb = R.norm_ref(T.view(), c['ids'], n, gl, G.view(), c['vec4_bwd'], slot0=PRELOAD, **kw)
    slot = Dev(R.scalar_slot(GARBAGE))
    L.call('ktup_reg_norm_fwd', tp, ld, d, idp, n, slot.ptr(4), st)
    out.append(check_slot('ktup_reg_norm_fwd', slot, *rf['value']))
    fwd_value = float(slot.host()[4])
    if not serial:
        g = Dev(G.flat)
        L.call('ktup_reg_norm_bwd', tp, ld, d, idp, n, dgl.ptr(4), g.ptr(G.start), st)
        out.append(check_table('ktup_reg_norm_bwd', 'gT', g, G, *rb['gT']))
    slot2, g2 = Dev(R.scalar_slot(PRELOAD)), Dev(G.flat)
    L.call('ktup_reg_norm_fused', tp, ld, d, idp, n, dgl.ptr(4), slot2.ptr(4), g2.ptr(G.start), st)
    out.append(check_slot('ktup_reg_norm_fused', slot2, *rb['value']))
    out.append(check_table('ktup_reg_norm_fused', 'gT', g2, G, *rb['gT']))
    assert abs((float(slot2.host()[4]) - PRELOAD) - fwd_value) <= rf['value'][1] + rb['value'][1]
    raw += [slot.host(), slot2.host(), g2.host()]
    # ---- orth
    of = R.orth_ref(T.view(), W.view(), c['ids'], n, gl, G.view(), GW.view(), c['vec4_fwd'], **kw)
    ob = R.orth_ref(T.view(), W.view(), c['ids'], n, gl, G.view(), GW.view(), c['vec4_bwd'], slot0=PRELOAD, **kw)
    slot = Dev(R.scalar_slot(GARBAGE))
    L.call('ktup_reg_orth_fwd', tp, ld, wp, ld, d, idp, n, slot.ptr(4), st)
    out.append(check_slot('ktup_reg_orth_fwd', slot, *of['value']))
    fwd_value = float(slot.host()[4])
    if not serial:
        g, gw = Dev(G.flat), Dev(GW.flat)
        L.call('ktup_reg_orth_bwd', tp, ld, wp, ld, d, idp, n, dgl.ptr(4), g.ptr(G.start), gw.ptr(GW.start), st)
        out.append(check_table('ktup_reg_orth_bwd', 'gRel', g, G, *ob['gR']))
        out.append(check_table('ktup_reg_orth_bwd', 'gNrm', gw, GW, *ob['gW']))
    slot2, g2, gw2 = Dev(R.scalar_slot(PRELOAD)), Dev(G.flat), Dev(GW.flat)
    L.call('ktup_reg_orth_fused', tp, ld, wp, ld, d, idp, n, dgl.ptr(4), slot2.ptr(4), g2.ptr(G.start), gw2.ptr(GW.start), st)
    out.append(check_slot('ktup_reg_orth_fused', slot2, *ob['value']))
    out.append(check_table('ktup_reg_orth_fused', 'gRel', g2, G, *ob['gR']))
    out.append(check_table('ktup_reg_orth_fused', 'gNrm', gw2, GW, *ob['gW']))
    assert abs((float(slot2.host()[4]) - PRELOAD) - fwd_value) <= of['value'][1] + ob['value'][1]
    raw += [slot.host(), slot2.host(), g2.host(), gw2.host()]
    unchanged(dT, dW, dgl)
    if ids is not None:
        assert np.array_equal(ids.cpu().numpy(), c['ids'])
    print(c['name'], 'd', d, c['how'], 'n', n, c['mode'], 'gloss', gl, '|', '  '.join(out))
    return raw


RUNGS, SEAMS, SERIAL = R.rung_cases(), R.seam_cases(), R.serial_cases()


@pytest.mark.parametrize('spec', RUNGS, ids=R.case_id)
def test_regularisers_every_rung(spec):
    """Every (V, G, CPL) of both ladders at both ends of its width range, 256/G + 1 rows by ids and by ids = NULL; per rung also
    1, 256/G - 1 and 256/G rows and a row listed more than 64 times.  The tables hold the three exact hinge rows (two inactive
    at s == 1, one active one ulp-scale above) and drawn rows on both sides."""
    c = R.reg_case(*spec)
    R.check_reg_case(c)
    run_reg(c)


@pytest.mark.parametrize('spec', SEAMS, ids=R.case_id)
def test_regularisers_grid_seams(spec):
    """128 x (256/G) + 1 rows: the second trip of launch_rows_reduce's 128 workgroups (_fwd, _fused); 2048 x (256/G) + 1 rows: the
    second trip of launch_rows' 2048 (_bwd).  By ids into a 64-row table (every row hundreds of times) and by ids = NULL."""
    c = R.reg_case(*spec)
    R.check_reg_case(c)
    run_reg(c)


@pytest.fixture
def deterministic():
    L = lib()
    old = L.set_option('deterministic', 1)
    try:
        yield
    finally:
        L.set_option('deterministic', old)


@pytest.mark.parametrize('spec', SERIAL, ids=R.case_id)
def test_regularisers_serial_mode(spec, deterministic):
    """Library option `deterministic`: one lane group walks all rows.  _fwd and _fused of both regularisers meet the reference
    (whose scalar-sum count is then trips = n, grid = 1), and two runs agree in every bit of the values and gradient tables."""
    assert lib().get_option('deterministic') == 1
    c = R.reg_case(*spec)
    R.check_reg_case(c)
    a, b = run_reg(c, serial=True), run_reg(c, serial=True)
    for x, y in zip(a, b):
        R.same_bits(x, y, 'second serial run')


@pytest.mark.parametrize('d', [8, 7])
def test_serial_mode_sums_in_row_order(d, deterministic):
    """Row values that are exact in fp32 and a sum whose result depends on the order: 2^24 - 1 (a one-hot 4096) followed by forty
    rows of value 1 (two ones).  In row order the running sum reaches 2^24 and every further + 1 is a tie that rounds back to
    2^24; any other grouping adds the ones among themselves first and ends near 2^24 + 39."""
    L = lib()
    T = np.zeros((2, d), dtype=np.float32)
    T[0, 2], T[1, 0], T[1, d - 1] = 4096.0, 1.0, 1.0
    ids_np = np.array([0] + [1] * 40, dtype=np.int64)
    want = np.float32(0.0)
    for r in ids_np:
        want = np.float32(want + np.float32((T[r].astype(np.float64) ** 2).sum() - 1.0))
    assert float(want) == 2.0 ** 24
    tab, g0 = R.Table(T), R.Table(np.zeros((2, d), dtype=np.float32))
    dT, dgl, ids, st = Dev(tab.flat), Dev(R.scalar_slot(0.0)), torch.from_numpy(ids_np).to(DEV), stream()
    slot, slot2, g = Dev(R.scalar_slot(GARBAGE)), Dev(R.scalar_slot(0.0)), Dev(g0.flat)
    L.call('ktup_reg_norm_fwd', dT.ptr(tab.start), d, d, ids.data_ptr(), len(ids_np), slot.ptr(4), st)
    L.call('ktup_reg_norm_fused', dT.ptr(tab.start), d, d, ids.data_ptr(), len(ids_np), dgl.ptr(4), slot2.ptr(4), g.ptr(g0.start), st)
    assert float(slot.host()[4]) == 2.0 ** 24 and float(slot2.host()[4]) == 2.0 ** 24
    unchanged(g, dT)                                                  # gloss 0: every add is 0.0


@pytest.mark.parametrize('d,how', [(4, ''), (7, ''), (260, ''), (100, 'grad')])
def test_regularisers_empty_batch(d, how):
    """n = 0: _fwd stores 0, _fused leaves its slot alone, no gradient cell changes; null table pointers are accepted."""
    L = lib()
    c = R.reg_case('n0', d, how, 0, 'null', table_rows=8)
    G, GW, ld = c['G'], c['GW'], c['ld']
    st, dgl = stream(), Dev(R.scalar_slot(1.0))
    for null in (False, True):
        dT, dW, g, gw = Dev(c['T'].flat), Dev(c['W'].flat), Dev(G.flat), Dev(GW.flat)
        tp, wp, gp, gwp = (None,) * 4 if null else (dT.ptr(c['T'].start), dW.ptr(c['W'].start), g.ptr(G.start), gw.ptr(GW.start))
        glp = None if null else dgl.ptr(4)
        for entry, args in (('ktup_reg_norm_fwd', (tp, ld, d, None, 0)), ('ktup_reg_orth_fwd', (tp, ld, wp, ld, d, None, 0))):
            slot = Dev(R.scalar_slot(GARBAGE))
            L.call(entry, *args, slot.ptr(4), st)
            assert slot.host().tolist() == R.scalar_slot(0.0).tolist()
        slot = Dev(R.scalar_slot(PRELOAD))
        L.call('ktup_reg_norm_bwd', tp, ld, d, None, 0, glp, gp, st)
        L.call('ktup_reg_orth_bwd', tp, ld, wp, ld, d, None, 0, glp, gp, gwp, st)
        L.call('ktup_reg_norm_fused', tp, ld, d, None, 0, glp, None if null else slot.ptr(4), gp, st)
        L.call('ktup_reg_orth_fused', tp, ld, wp, ld, d, None, 0, glp, None if null else slot.ptr(4), gp, gwp, st)
        unchanged(dT, dW, g, gw, slot, dgl)


def test_orth_exactly_perpendicular_rows():
    """w . r == 0 exactly in fp32 under any summation order (integer products +-1 that cancel): the value is exactly 0, c1 and c2
    are exactly 0 and both gradient tables come back bit-identical, on the float4 and on the float path."""
    L = lib()
    for d, shift in ((8, 0), (8, 1), (260, 0), (129, 0)):
        Rel, Nrm = np.zeros((3, d), dtype=np.float32), np.zeros((3, d), dtype=np.float32)
        for r in range(3):
            Rel[r, [r, d - 1 - r]] = 1.0
            Nrm[r, r], Nrm[r, d - 1 - r] = 1.0, -1.0
            Rel[r, 3], Nrm[r, 4] = 0.5, 3.0                                                    # |r|^2 = 2.25, w not parallel to r
        assert not (Rel.astype(np.float64) * Nrm).sum(1).any() and (np.abs(Rel * Nrm).sum(1) == 2.0).all()
        tr, tw = R.Table(Rel, None, shift), R.Table(Nrm, None, shift)
        g0 = R.Table(np.full((3, d), 0.3, dtype=np.float32), None, shift)
        dT, dW, dgl, st = Dev(tr.flat), Dev(tw.flat), Dev(R.scalar_slot(0.75)), stream()
        slot, g, gw = Dev(R.scalar_slot(GARBAGE)), Dev(g0.flat), Dev(g0.flat)
        ids = torch.tensor([0, 1, 2, 2, 0], dtype=torch.int64, device=DEV)
        L.call('ktup_reg_orth_fwd', dT.ptr(tr.start), d, dW.ptr(tw.start), d, d, ids.data_ptr(), 5, slot.ptr(4), st)
        assert R.bits(slot.host()).tolist() == R.bits(R.scalar_slot(0.0)).tolist()
        L.call('ktup_reg_orth_bwd', dT.ptr(tr.start), d, dW.ptr(tw.start), d, d, ids.data_ptr(), 5, dgl.ptr(4), g.ptr(g0.start), gw.ptr(g0.start), st)
        unchanged(g, gw)
        slot = Dev(R.scalar_slot(PRELOAD))
        L.call('ktup_reg_orth_fused', dT.ptr(tr.start), d, dW.ptr(tw.start), d, d, ids.data_ptr(), 5, dgl.ptr(4), slot.ptr(4), g.ptr(g0.start),
               gw.ptr(g0.start), st)
        unchanged(g, gw, slot, dT, dW)


@pytest.mark.parametrize('d,how', R.REFUSED_D)
def test_regularisers_refuse_more_than_256_chunks(d, how):
    """d = 257 and 322 on the float path, 1028 on the float4 path, 260 at a 4-byte offset (float path): every entry answers
    KTUP_ERR_UNSUPPORTED, launches nothing and writes nothing -- not even _fwd's zero."""
    L = lib()
    c = R.reg_case('refused', d, how, 5, 'ids', table_rows=8)
    assert R.rung(d, c['vec4_bwd']) is None and R.rung(d, c['vec4_fwd']) is None
    T, W, G, GW, ld = c['T'], c['W'], c['G'], c['GW'], c['ld']
    dT, dW, g, gw, dgl, slot = Dev(T.flat), Dev(W.flat), Dev(G.flat), Dev(GW.flat), Dev(R.scalar_slot(1.0)), Dev(R.scalar_slot(GARBAGE))
    ids = torch.from_numpy(c['ids']).to(DEV)
    tp, wp, gp, gwp, idp, st = dT.ptr(T.start), dW.ptr(W.start), g.ptr(G.start), gw.ptr(GW.start), ids.data_ptr(), stream()
    calls = (('ktup_reg_norm_fwd', (tp, ld, d, idp, 5, slot.ptr(4))), ('ktup_reg_norm_bwd', (tp, ld, d, idp, 5, dgl.ptr(4), gp)),
             ('ktup_reg_norm_fused', (tp, ld, d, idp, 5, dgl.ptr(4), slot.ptr(4), gp)),
             ('ktup_reg_orth_fwd', (tp, ld, wp, ld, d, idp, 5, slot.ptr(4))),
             ('ktup_reg_orth_bwd', (tp, ld, wp, ld, d, idp, 5, dgl.ptr(4), gp, gwp)),
             ('ktup_reg_orth_fused', (tp, ld, wp, ld, d, idp, 5, dgl.ptr(4), slot.ptr(4), gp, gwp)))
    for entry, args in calls:
        with pytest.raises(L.KtupError) as info:
            L.call(entry, *args, st)
        assert info.value.code == L.ERR_UNSUPPORTED and entry in L.load().ktup_last_error().decode()
        unchanged(dT, dW, g, gw, dgl, slot)


# ------------------------------------------------------------------------------------------------ pair losses
def run_pair(c):
    L = lib()
    kind, param, n, gl = c['kind'], c['param'], c['n'], c['gloss']
    vp, vn = R.vector(c['pos']), R.vector(c['neg'])
    dp, dn, dgl, st = Dev(vp.flat), Dev(vn.flat), Dev(R.scalar_slot(gl)), stream()
    pp, npn = (dp.ptr(vp.start), dn.ptr(vn.start)) if n else (None, None)
    junk = R.vector(np.full(n, 9.75, dtype=np.float32))
    rf, rb = R.pair_ref(kind, c['pos'], c['neg'], param, gl), R.pair_ref(kind, c['pos'], c['neg'], param, gl, slot0=PRELOAD)
    out = []
    slot = Dev(R.scalar_slot(GARBAGE))
    L.call('ktup_loss_%s_fwd' % kind, pp, npn, n, param, slot.ptr(4), st)
    out.append(check_slot('ktup_loss_%s_fwd' % kind, slot, *rf['value']))
    for entry in ('ktup_loss_%s_bwd' % kind, 'ktup_loss_%s_fused' % kind):
        gp, gn, slot2 = Dev(junk.flat), Dev(junk.flat), Dev(R.scalar_slot(PRELOAD))
        if entry.endswith('_bwd'):
            L.call(entry, pp, npn, n, param, dgl.ptr(4), gp.ptr(junk.start), gn.ptr(junk.start), st)
            unchanged(slot2)
        else:
            L.call(entry, pp, npn, n, param, dgl.ptr(4), slot2.ptr(4), gp.ptr(junk.start), gn.ptr(junk.start), st)
            out.append(check_slot(entry, slot2, *rb['value']))
            assert abs((float(slot2.host()[4]) - PRELOAD) - float(slot.host()[4])) <= rf['value'][1] + rb['value'][1]
        out.append(check_table(entry, 'gpos', gp, junk, rb['gpos'][0][None, :], rb['gpos'][1][None, :]))
        out.append(check_table(entry, 'gneg', gn, junk, rb['gneg'][0][None, :], rb['gneg'][1][None, :]))
        if n:
            R.same_bits(junk.view(gn.host()), -junk.view(gp.host()), 'gneg == -gpos')
    unchanged(dp, dn, dgl)
    print(kind, param, 'n', n, 'gloss', gl, '|', '  '.join(out))


@pytest.mark.parametrize('n', R.PAIR_N)
@pytest.mark.parametrize('kind,param', R.PAIR_KINDS)
def test_pair_losses(kind, param, n):
    """n around the workgroup (256) and the 1024 elements a fwd / fused workgroup takes per trip, 65537 (second trip of the 64
    fwd / fused workgroups) and 262145 (second trip of the 1024 bwd workgroups); BPR as a mean with targets +1 and -1 over
    arguments -30 .. 30, margin as a sum with exact ties (gradient exactly 0)."""
    run_pair(R.pair_case(kind, param, n))


def test_bpr_libm_allowance():
    """The measurement behind BPR_GRAD_ULPS / BPR_VALUE_ULPS (tests/_loss_ref.py): arguments x = k / 256 over -32 .. 32 with
    pos - neg exact in fp32, so that nothing but device expf / log1pf and the handful of roundings after them separates the
    kernel from fp64.  gpos of one ktup_loss_bpr_bwd call per target; single-element ktup_loss_bpr_fwd calls at x = k / 8."""
    L = lib()
    rng = np.random.default_rng(5)
    k = np.arange(-32 * 256, 32 * 256 + 1)
    neg = (rng.integers(-1024, 1025, len(k)) / 256.0).astype(np.float32)
    pos = (neg.astype(np.float64) + k / 256.0).astype(np.float32)
    assert np.array_equal(pos.astype(np.float64) - neg.astype(np.float64), k / 256.0)
    assert np.array_equal((pos - neg).astype(np.float64), k / 256.0)                         # the fp32 difference is exact
    dp, dn, st = torch.from_numpy(pos).to(DEV), torch.from_numpy(neg).to(DEV), stream()
    gl = torch.ones(1, device=DEV)
    worst_g = worst_v = 0.0
    for target in (1.0, -1.0):
        gp, gn = torch.empty_like(dp), torch.empty_like(dp)
        L.call('ktup_loss_bpr_bwd', dp.data_ptr(), dn.data_ptr(), len(k), target, gl.data_ptr(), gp.data_ptr(), gn.data_ptr(), st)
        want = R.pair_ref('bpr', pos, neg, target, 1.0)['gpos'][0]
        err = np.abs(gp.cpu().numpy().astype(np.float64) - want) / (R.ULP * np.abs(want))
        assert np.isfinite(err).all()
        worst_g = max(worst_g, float(err.max()))
        sel = np.arange(0, len(k), 32)
        vals = torch.full((len(sel),), GARBAGE, device=DEV)
        for j, i in enumerate(sel):
            L.call('ktup_loss_bpr_fwd', dp.data_ptr() + 4 * int(i), dn.data_ptr() + 4 * int(i), 1, target, vals.data_ptr() + 4 * j, st)
        x = target * k[sel] / 256.0
        want = np.maximum(-x, 0.0) + np.log1p(np.exp(-np.abs(x)))
        err = np.abs(vals.cpu().numpy().astype(np.float64) - want) / (R.ULP * want)
        assert np.isfinite(err).all()
        worst_v = max(worst_v, float(err.max()))
    MEASURED.update(gpos=worst_g, value=worst_v)
    print('measured libm error in units of 2^-23 of the element: gpos %.3f (allowance %d), single-element value %.3f (allowance %d)'
          % (worst_g, R.BPR_GRAD_ULPS, worst_v, R.BPR_VALUE_ULPS))
    assert worst_g <= 8.0 and worst_v <= 8.0                                                 # more would be a finding, not a number
    assert math.ceil(2.0 * worst_g) <= R.BPR_GRAD_ULPS and math.ceil(2.0 * worst_v) <= R.BPR_VALUE_ULPS


# ------------------------------------------------------------------------------------------------ graph replay
def test_graph_replay_of_the_step_plan_sequence():
    """ktup_loss_margin_fused + ktup_reg_orth_fused + ktup_reg_norm_fused captured on one stream (the order of utils/step_plans.py),
    replayed three times after scores, tables, gradient tables, loss slots and gloss were changed in place: every replay meets
    the reference for the contents it ran on."""
    L = lib()
    n, d, rows = 300, 68, 40
    ids_np = np.random.default_rng(1).integers(0, 30, 77).astype(np.int64)
    ids = torch.from_numpy(ids_np).to(DEV)

    def contents(seed):
        rng = np.random.default_rng(seed)
        pos, neg = R.pair_scores(rng, n, 'margin', 1.0)
        T, W = R.reg_tables(rng, rows, d)
        E, _ = R.reg_tables(rng, rows, d)
        R.check_rows(T), R.check_rows(E)
        g = [(rng.standard_normal((rows, d)) * 0.1).astype(np.float32) for _ in range(3)]
        return dict(pos=R.vector(pos), neg=R.vector(neg), T=R.Table(T), W=R.Table(W), E=R.Table(E), gT=R.Table(g[0]), gW=R.Table(g[1]),
                    gE=R.Table(g[2]), gl=R.scalar_slot(R.GLOSS[seed % 4]), slots=np.array([0.5, 1.5, 2.5, R.SENTINEL], dtype=np.float32),
                    gp=R.vector(np.full(n, 9.75, dtype=np.float32)), gn=R.vector(np.full(n, 9.75, dtype=np.float32)))

    first = contents(0)
    dev = {k: Dev(v if isinstance(v, np.ndarray) else v.flat) for k, v in first.items()}
    p = lambda k: dev[k].ptr(first[k].start if not isinstance(first[k], np.ndarray) else 0)

    def launch():
        st = stream()
        L.call('ktup_loss_margin_fused', p('pos'), p('neg'), n, 1.0, dev['gl'].ptr(4), dev['slots'].ptr(0), p('gp'), p('gn'), st)
        L.call('ktup_reg_orth_fused', p('T'), d, p('W'), d, d, ids.data_ptr(), len(ids_np), dev['gl'].ptr(4), dev['slots'].ptr(1), p('gT'), p('gW'), st)
        L.call('ktup_reg_norm_fused', p('E'), d, d, ids.data_ptr(), len(ids_np), dev['gl'].ptr(4), dev['slots'].ptr(2), p('gE'), st)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()                                                                              # loads the kernels outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with L.capture(graph):
        launch()
    torch.cuda.synchronize()
    for seed in (1, 2, 3):
        c = contents(seed)
        for k, v in c.items():
            flat = v if isinstance(v, np.ndarray) else v.flat
            dev[k].before = flat.copy()
            dev[k].t.copy_(torch.from_numpy(flat))
        graph.replay()
        gl = float(c['gl'][4])
        m = R.pair_ref('margin', c['pos'].view()[0], c['neg'].view()[0], 1.0, gl, slot0=0.5)
        o = R.orth_ref(c['T'].view(), c['W'].view(), ids_np, len(ids_np), gl, c['gT'].view(), c['gW'].view(), True, slot0=1.5)
        e = R.norm_ref(c['E'].view(), ids_np, len(ids_np), gl, c['gE'].view(), True, slot0=2.5)
        h = dev['slots'].host()
        assert h[3] == R.SENTINEL
        out = [note('graph', name, R.compare(h[i], *ref['value'], 'replay ' + name)) for i, (name, ref) in enumerate((('margin', m), ('orth', o), ('norm', e)))]
        out.append(check_table('graph', 'gpos', dev['gp'], c['gp'], m['gpos'][0][None, :], m['gpos'][1][None, :]))
        out.append(check_table('graph', 'gneg', dev['gn'], c['gn'], m['gneg'][0][None, :], m['gneg'][1][None, :]))
        out.append(check_table('graph', 'gRel', dev['gT'], c['gT'], *o['gR']))
        out.append(check_table('graph', 'gNrm', dev['gW'], c['gW'], *o['gW']))
        out.append(check_table('graph', 'gT', dev['gE'], c['gE'], *e['gT']))
        unchanged(dev['pos'], dev['neg'], dev['T'], dev['W'], dev['E'], dev['gl'])
        print('replay', seed, 'gloss', gl, '|', '  '.join(out))


def test_zz_report():
    """The largest error / tolerance of the module per entry (printed; every case asserted its own) and the libm measurement."""
    for entry, w in sorted(WORST.items()):
        print('%-24s %.3f' % (entry, w))
    print('libm', MEASURED)
    assert all(0.0 <= w <= 1.0 for w in WORST.values())                                       # false for a NaN as well
