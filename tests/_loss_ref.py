"""fp64 reference of the twelve loss / regulariser entry points of csrc/ktup_loss.hip (include/ktup_hip.h, K8-K10):
ktup_loss_{bpr,margin}_{fwd,bwd,fused} and ktup_reg_{norm,orth}_{fwd,bwd,fused}.  NOT a test module: tests/test_loss_ref_host.py
pins it on the CPU, tests/test_hip_loss_abi.py compares the kernels with it on the GPU.  numpy only, everything from the same fp32
inputs widened.

pair_ref(kind, pos, neg, param, gloss)           value (mean for BPR, sum for margin), gpos, gneg
norm_ref / orth_ref(tables, ids, n, gloss, g0)   value, table-shaped gradients = g0 + every occurrence's add
Each output comes as (want, tol); tol == 0 marks an element that must match exactly (fp32(want), compared for equality).
Ties follow the header: an example (margin) or a row (norm) is active iff its argument is > 0; the builders keep every fp64
argument so far from 0 that its fp32 evaluation takes the same side (check_pair / check_rows assert it), and the exact ties they
add evaluate to exactly 0 in fp32 under any summation order.

Tolerance = (number of roundings) x 2^-24 x scale, u = 2^-24, first order; an fmaf counts as two roundings (as tests/_optim_ref.py).
  row sums   A lane holds CPL chunks of W floats (ktup_rows.h: W = 4 or 1, G lanes per row).  Per chunk 2W roundings (W products,
             W adds or fmas) and one for `s += `, then log2 G shuffle adds:  E = CPL (2W + 1) + log2 G  (e_row).  A sum of
             non-negative terms is off by at most E u times itself; a signed one (w.r) by E u times D = sum |w_j r_j|.
  scalar sum every row kernel value and every pair loss goes thread partial -> group_sum<64> (6) -> the 4-way block sum (3) -> one
             atomic per workgroup in any order (grid):  NS = trips + 6 + 3 + grid, trips = the per-thread loop count, all terms
             non-negative, hence NS u V.  A slot preloaded with s0 (the _fused entries) adds grid u |s0|.
  norm value row term v = max(s - 1, 0): E u s from the sum and u v from the subtraction -> sum over ACTIVE rows of E s + v.
  norm grad  an occurrence adds 2 gloss x (2 gloss exact, one product); m adds onto a cell that held g0 round m times, each at most
             u (|g0| + sum |add|):  (m + 1) u (|g0| + sum |add|), m = the number of adds of non-zero scale the cell receives (0: exact).
  orth value v = a^2 / b, a = w.r, b = r.r:  2 |a| E D / b + (E + 2) v  per row  (E for b, one each for the square and the quotient).
  orth grad  c1 = 2 g a / b is off by (2E + 2) u S1, S1 = |2g| D / b;  c2 = 2 g a^2 / b^2 by (4E + 4) u S2, S2 = |2g| |a| D / b^2.
             gNrm add c1 r: (2E + 3) over S1 |r|.   gRel add fma(-c2, r, c1 w): (4E + 6) over S1 |w| + S2 |r|.  Then the m atomic
             adds as for norm: (C + m) u (|g0| + sum of the occurrences' scales).
  margin     argument (pos - neg) + margin: two roundings, u (|pos| + |neg| + |arg|) per ACTIVE example (not relative to the
             argument: the difference cancels); the gradient is gloss or 0, exact.
  bpr        x = target (pos - neg): one rounding of the difference, which moves the term by |x| sigmoid(-x) u and the gradient by
             |x| sigmoid(x) u of itself.  Everything after it -- expf, log1pf, 1 + e, the quotient, the products with gloss / n --
             is covered by the MEASURED allowance below, in units of 2^-23 of the element (one fp32 ulp at most).

Measured allowance (the one constant not derived: device expf / log1pf).  tests/test_hip_loss_abi.py::test_bpr_libm_allowance
runs the 16385 arguments x = k / 256, -32 <= x <= 32, with pos - neg exact in fp32, through ktup_loss_bpr_bwd (gpos is
element-wise, no atomics) and every 32nd of them through a single-element ktup_loss_bpr_fwd call, for both targets.  Largest
error on the MI355X, in units of 2^-23 of the element:
    gpos   1.294   -> BPR_GRAD_ULPS  = 3
    value  0.719   -> BPR_VALUE_ULPS = 2
(twice the measurement rounded up to whole ulps; the test fails if a later measurement exceeds 8 or half the allowance).

Not in the reference: a zero Rel row in orth (0 / 0 = NaN here as in the kernel; the builders never make one)."""
import math

import numpy as np

U = 2.0 ** -24
ULP = 2.0 ** -23
GUARD = 8
SENTINEL = np.float32(-7.25)
BPR_GRAD_ULPS = 3
BPR_VALUE_ULPS = 2
GLOSS = (1.0, 0.75, -2.0, 0.0)
NORMS = (0.25, 0.9, 1.1, 4.0)
EDGE_CLEAR = 7e-4                                   # (d + 8) u s <= EDGE_CLEAR |s - 1| for every drawn row, d <= 1024
PAIR_CLEAR = 2.0 ** -10                             # |pos - neg + margin| >= PAIR_CLEAR max(|pos|, |neg|, |margin|)
LADDER = ((16, 16, 1), (32, 32, 1), (64, 64, 1), (128, 64, 2), (256, 64, 4))        # (chunks <=, G, CPL), ktup_rows.h


# ------------------------------------------------------------------------------------------------ dispatch model
def can_vec4(d, offsets, lds):
    """ktup_rows.h can_vec4: offsets = float offsets of every listed pointer from a 16-byte boundary."""
    return d % 4 == 0 and all(o % 4 == 0 for o in offsets) and all(l % 4 == 0 for l in lds)


def rung(d, vec4):
    """(W, G, CPL) of the instantiation launch_rows / launch_rows_reduce pick, None above 256 chunks (KTUP_ERR_UNSUPPORTED)."""
    w = 4 if vec4 else 1
    for lim, g, cpl in LADDER:
        if d // w <= lim:
            return w, g, cpl
    return None


def e_row(w, g, cpl):
    return cpl * (2 * w + 1) + int(math.log2(g))


def reduce_sum_count(n, g, serial=False):
    """NS and the grid of launch_rows_reduce (128 workgroups at most; serial: one lane group of one workgroup walks all rows)."""
    gpb = 256 // g
    grid = 1 if serial else min(max(-(-n // gpb), 1), 128)
    trips = n if serial else -(-n // (grid * gpb))
    return trips + 6 + 3 + grid, grid


def pair_sum_count(n):
    grid = min(max(-(-n // 1024), 1), 64)
    return -(-n // (grid * 256)) + 6 + 3 + grid, grid


# ------------------------------------------------------------------------------------------------ pair losses
def sigmoid(x):
    return np.exp(-np.logaddexp(0.0, -x))


def pair_ref(kind, pos, neg, param, gloss, slot0=0.0):
    """kind 'bpr' (param = target, MEAN) or 'margin' (param = margin, SUM).  {'value', 'gpos', 'gneg'}: (want, tol)."""
    p, q = pos.astype(np.float64), neg.astype(np.float64)
    n, param, gloss = len(p), float(np.float32(param)), float(np.float32(gloss))
    zero = np.zeros(n)
    if n == 0:
        return {'value': (slot0, 0.0), 'gpos': (zero, zero), 'gneg': (zero, zero)}
    ns, grid = pair_sum_count(n)
    diff = p - q
    if kind == 'margin':
        arg = diff + param
        act = arg > 0.0
        v = float(arg[act].sum())
        tol = U * (float((np.abs(p) + np.abs(q) + np.abs(arg))[act].sum()) + (ns + 1) * v)
        g, gtol = np.where(act, gloss, 0.0), zero
    else:
        x = param * diff
        term = np.maximum(-x, 0.0) + np.log1p(np.exp(-np.abs(x)))
        v = float(term.mean())
        tol = U * float((np.abs(x) * sigmoid(-x)).sum()) / n + (2 * BPR_VALUE_ULPS + ns + 2) * U * v
        g = -gloss / n * param * sigmoid(-x)
        gtol = (np.abs(x) * sigmoid(x) * U + BPR_GRAD_ULPS * ULP) * np.abs(g)
    tol += U * grid * abs(slot0)
    return {'value': (slot0 + v, tol), 'gpos': (g, gtol), 'gneg': (-g, gtol)}


# ------------------------------------------------------------------------------------------------ regularisers
def _rows(ids, n):
    return np.arange(n, dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64)


def _scatter(shape, rows, vals):
    out = np.zeros(shape)
    np.add.at(out, rows, vals)
    return out


def _cells(g0, rows, add, scale, c):
    """Table-shaped gradient g0 + adds and its tolerance (c + m) u (|g0| + sum scale), exact where no non-zero add lands."""
    g0 = g0.astype(np.float64)
    m = _scatter(g0.shape, rows, (scale != 0.0).astype(np.float64))         # (by scale: an add may cancel to 0 in fp64 only)
    tol = np.where(m > 0, (c + m) * U * (np.abs(g0) + _scatter(g0.shape, rows, scale)), 0.0)
    return g0 + _scatter(g0.shape, rows, add), tol


def norm_ref(T, ids, n, gloss, g0, vec4, serial=False, slot0=0.0):
    """T: (rows x d) fp32 table, g0: the gradient table before the call.  {'value', 'gT'}: (want, tol)."""
    rows, gloss = _rows(ids, n), float(np.float32(gloss))
    if n == 0:
        return {'value': (slot0, 0.0), 'gT': (g0.astype(np.float64), np.zeros(g0.shape))}
    w, g, cpl = rung(T.shape[1], vec4)
    e = e_row(w, g, cpl)
    ns, grid = reduce_sum_count(n, g, serial)
    x = T.astype(np.float64)[rows]
    s = (x * x).sum(1)
    act = s > 1.0
    v = np.where(act, s - 1.0, 0.0)
    total = float(v.sum())
    tol = U * (float((e * s + v)[act].sum()) + ns * total + grid * abs(slot0))
    add = 2.0 * gloss * x * act[:, None]
    return {'value': (slot0 + total, tol), 'gT': _cells(g0, rows, add, np.abs(add), 1)}


def orth_ref(R, W, ids, n, gloss, g0r, g0w, vec4, serial=False, slot0=0.0):
    """R = Rel, W = Nrm tables.  {'value', 'gR', 'gW'}: (want, tol)."""
    rows, gloss = _rows(ids, n), float(np.float32(gloss))
    if n == 0:
        return {'value': (slot0, 0.0), 'gR': (g0r.astype(np.float64), np.zeros(g0r.shape)),
                'gW': (g0w.astype(np.float64), np.zeros(g0w.shape))}
    wd, g, cpl = rung(R.shape[1], vec4)
    e = e_row(wd, g, cpl)
    ns, grid = reduce_sum_count(n, g, serial)
    a, w = R.astype(np.float64)[rows], W.astype(np.float64)[rows]
    dot, dabs, nr = (a * w).sum(1), np.abs(a * w).sum(1), (a * a).sum(1)
    v = dot * dot / nr
    total = float(v.sum())
    tol = U * (float((2.0 * np.abs(dot) * e * dabs / nr + (e + 2) * v).sum()) + ns * total + grid * abs(slot0))
    c1, c2 = (2.0 * gloss * dot / nr)[:, None], (2.0 * gloss * dot * dot / (nr * nr))[:, None]
    s1, s2 = (abs(2.0 * gloss) * dabs / nr)[:, None], (abs(2.0 * gloss) * np.abs(dot) * dabs / (nr * nr))[:, None]
    return {'value': (slot0 + total, tol),
            'gR': _cells(g0r, rows, c1 * w - c2 * a, s1 * np.abs(w) + s2 * np.abs(a), 4 * e + 6),
            'gW': _cells(g0w, rows, c1 * a, s1 * np.abs(a), 2 * e + 3)}


# ------------------------------------------------------------------------------------------------ comparator
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def compare(got, want, tol, what=''):
    """Every element of got (fp32) against want at tol; tol == 0 elements must equal fp32(want).  Returns the largest
    error / tolerance over the elements with tol > 0 (0.0 if there are none).  A non-finite element fails, and so does every
    single element whose ratio is not <= 1 (per element: a NaN is not <= 1)."""
    got = np.atleast_1d(np.asarray(got, dtype=np.float32)).astype(np.float64)
    want, tol = np.broadcast_to(np.asarray(want, dtype=np.float64), got.shape), np.broadcast_to(np.asarray(tol, dtype=np.float64), got.shape)
    assert np.isfinite(got).all(), 'not finite: ' + what
    assert np.isfinite(want).all() and np.isfinite(tol).all() and (tol >= 0.0).all(), 'reference not finite: ' + what
    exact = tol == 0.0
    assert np.array_equal(got[exact], want[exact].astype(np.float32).astype(np.float64)), 'exact part of ' + what
    if exact.all():
        return 0.0
    ratio = np.abs(got - want)[~exact] / tol[~exact]
    bad = int((~(ratio <= 1.0)).sum())
    worst = float(ratio.max())
    assert bad == 0 and worst <= 1.0, (what, bad, worst)
    return worst


def same_bits(got, before, what=''):
    assert np.array_equal(bits(got), bits(before)), 'changed: ' + what


# ------------------------------------------------------------------------------------------------ buffers with guards
class Table:
    """A (rows x d) fp32 table at pitch ld inside a flat buffer: GUARD sentinels, `shift` more (0: 16-byte aligned, 1: a 4-byte
    offset), the rows with sentinels in the pitch padding, sentinels up to a multiple of 4 and GUARD more."""

    def __init__(self, data, ld=None, shift=0):
        self.rows, self.d = data.shape
        self.ld = self.d if ld is None else ld
        self.shift = shift
        self.start = GUARD + shift
        total = self.start + self.rows * self.ld
        self.flat = np.full((total + 3) // 4 * 4 + GUARD, SENTINEL, dtype=np.float32)
        self.view()[:] = data

    def view(self, flat=None):
        f = self.flat if flat is None else flat
        return f[self.start:self.start + self.rows * self.ld].reshape(self.rows, self.ld)[:, :self.d]

    def guard(self):
        m = np.ones(self.flat.shape, dtype=bool)
        self.view(m)[:] = False
        return m

    def like(self, data):
        return Table(data, self.ld, self.shift)


def scalar_slot(value):
    """One float between sentinels: index 4 of 9."""
    a = np.full(9, SENTINEL, dtype=np.float32)
    a[4] = value
    return a


def vector(data, shift=0):
    return Table(np.asarray(data, dtype=np.float32).reshape(1, -1), None, shift)


# ------------------------------------------------------------------------------------------------ builders
def edge_rows(d):
    """Rows whose squared norm is exact in fp32 under any summation order: (row, active)."""
    out = []
    one = np.zeros(d, dtype=np.float32); one[d // 2] = 1.0
    out.append((one, False))                                                       # s = 1
    up = np.zeros(d, dtype=np.float32); up[d - 1] = np.float32(1.0 + 2.0 ** -11)
    out.append((up, True))                                                         # s = 1 + 2^-10 + 2^-22
    if d >= 4:
        half = np.zeros(d, dtype=np.float32); half[[0, 1, d - 2, d - 1]] = 0.5
        out.append((half, False))                                                  # s = 4 x 0.25 = 1
    return out


def drawn_rows(rng, rows, d, norms=NORMS):
    """Normal vectors rescaled to squared norms cycling through `norms`."""
    x = rng.standard_normal((rows, d))
    want = np.array([norms[i % len(norms)] for i in range(rows)])
    return (x * np.sqrt(want / (x * x).sum(1))[:, None]).astype(np.float32)


def reg_tables(rng, rows, d):
    """Rel-like table (edge rows first, then drawn rows; every |r|^2 in [0.1, 10]) and a Nrm-like table of unit-ish rows."""
    edges = [e for e, _ in edge_rows(d)][:rows]
    T = np.concatenate([np.stack(edges), drawn_rows(rng, rows - len(edges), d)]) if rows > len(edges) else np.stack(edges)
    W = drawn_rows(rng, rows, d, norms=(1.0, 0.5, 2.0))
    return T, W


def check_rows(T, with_edges=True):
    """The builders' promises for a table, asserted: every squared norm either one of the exact edge values or clear of 1 by
    the fp32 summation bound over EDGE_CLEAR; every |r|^2 in [0.1, 10]; both sides of the hinge present (tables of >= 4 rows)."""
    x = T.astype(np.float64)
    d = T.shape[1]
    s = (x * x).sum(1)
    edge = (s == 1.0) | (s == 1.0 + 2.0 ** -10 + 2.0 ** -22)
    for row, e in zip(T, edge):
        if e:                                                                      # exact in fp32 in any order: <= 4 non-zeros, dyadic
            assert int((row != 0).sum()) <= 4 and set(np.abs(row[row != 0]).tolist()) <= {1.0, 0.5, float(np.float32(1.0 + 2.0 ** -11))}
    clear = (d + 8) * U * s <= EDGE_CLEAR * np.abs(s - 1.0)
    assert bool((edge | clear).all()), 'a row too close to the hinge'
    assert bool(((s >= 0.1) & (s <= 10.0)).all())
    if len(T) >= 4:
        assert bool((s > 1.0).any()) and bool((s <= 1.0).any())
    return s


def pair_scores(rng, n, kind, param):
    """Scores whose every decision is clear.  margin: |pos - neg + margin| >= PAIR_CLEAR max(|pos|, |neg|, |margin|), redrawn (never
    skipped), with exact ties (pos 1, neg 2, margin 1) at every 7th place from index 3; bpr: arguments across -30 .. 30."""
    if kind == 'bpr':
        pos = (rng.standard_normal(n) * 2.0).astype(np.float32)
        neg = (pos.astype(np.float64) - rng.uniform(-30.0, 30.0, n)).astype(np.float32)
        return pos, neg
    pos, neg = (rng.standard_normal(n) * 2.0).astype(np.float32), (rng.standard_normal(n) * 2.0).astype(np.float32)
    for _ in range(20):
        bad = ~_pair_clear(pos, neg, param)
        if not bad.any():
            break
        pos[bad] = (rng.standard_normal(int(bad.sum())) * 2.0).astype(np.float32)
    if float(param) == 1.0:
        pos[3::7], neg[3::7] = 1.0, 2.0
    check_pair(pos, neg, param)
    return pos, neg


def _pair_clear(pos, neg, param):
    p, q = pos.astype(np.float64), neg.astype(np.float64)
    arg = p - q + float(param)
    return np.abs(arg) >= PAIR_CLEAR * np.maximum(np.maximum(np.abs(p), np.abs(q)), abs(float(param)))


def check_pair(pos, neg, param):
    """Margin inputs: every argument an exact tie (0 in fp64 AND in fp32) or clear by PAIR_CLEAR, and then the fp32 argument
    (pos - neg) + margin of the kernel takes the fp64 argument's side."""
    arg = pos.astype(np.float64) - neg.astype(np.float64) + float(param)
    arg32 = (pos - neg) + np.float32(param)
    assert arg32.dtype == np.float32
    tie = arg == 0.0
    assert bool((tie | _pair_clear(pos, neg, param)).all())
    assert bool((arg32[tie] == 0.0).all()) and bool(((arg32 > 0) == (arg > 0)).all())


# ------------------------------------------------------------------------------------------------ the cases of the GPU module
# d -> how the case reaches its path: '' (d alone decides), 'pitch1' (ld = d + 1), 'offset' (every table at a 4-byte offset),
# 'grad' (only the gradient tables at a 4-byte offset: _bwd / _fused on float, _fwd on float4), 'pitch4' (ld = d + 4: float4)
F4_RUNGS = {'f4/G16': (4, 64), 'f4/G32': (68, 128), 'f4/G64x1': (132, 256), 'f4/G64x2': (260, 512), 'f4/G64x4': (516, 1024)}
F1_RUNGS = {'f1/G16': (1, 7, 16), 'f1/G32': (17, 32), 'f1/G64x1': (33, 50, 64), 'f1/G64x2': (65, 128), 'f1/G64x4': (129, 255, 256)}
F1_HOW = {16: 'pitch1', 32: 'offset', 64: 'grad', 128: 'pitch1', 256: 'offset'}
RUNG_CASES = [(name, d, 'pitch4' if d in (64, 260) else '') for name, ds in F4_RUNGS.items() for d in ds] \
    + [(name, d, F1_HOW.get(d, '')) for name, ds in F1_RUNGS.items() for d in ds] + [('f1/G64x2', 100, 'grad'), ('f1/G16', 8, 'offset')]
SEAM_D = (('f4/G16', 4, ''), ('f4/G32', 68, ''), ('f4/G64x1', 132, ''), ('f1/G16', 7, ''), ('f1/G32', 17, ''), ('f1/G64x1', 33, ''))
SERIAL_D = (('f4/G16', 4, ''), ('f4/G32', 68, ''), ('f4/G64x4', 516, ''), ('f1/G64x2', 65, ''))
REFUSED_D = ((257, ''), (322, ''), (1028, ''), (260, 'offset'))          # 260 floats a row on the float path: 260 chunks


def seed_of(*key):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(repr(key))) % (2 ** 31)


def group_rows(name):
    return 256 // int(name.split('G')[1].split('x')[0])


def reg_case(name, d, how, n, mode, table_rows=None):
    """One regulariser case: tables T (Rel) and W (Nrm) with their gradient tables G / GW (non-zero contents), ids and gloss.
    mode: 'null' (ids = NULL: rows 0 .. n-1), 'ids' (drawn from the first three quarters of the table, duplicates likely),
    'heavy' (as 'ids' with row 5 listed 70 more times)."""
    rng = np.random.default_rng(seed_of('reg', name, d, how, n, mode))
    rows = table_rows or (64 if n <= 60 else n + 2)
    ld = d + {'pitch1': 1, 'pitch4': 4}.get(how, 0)
    tshift, gshift = (1 if how == 'offset' else 0), (1 if how in ('offset', 'grad') else 0)
    T, W = reg_tables(rng, rows, d)
    if mode == 'null':
        ids = None
    else:
        ids = rng.integers(0, max(rows * 3 // 4, 1), n).astype(np.int64)
        if mode == 'heavy':
            ids = np.concatenate([ids, np.full(70, 5, dtype=np.int64)])
            rng.shuffle(ids)
    c = {'name': name, 'd': d, 'how': how, 'ld': ld, 'n': n if ids is None else len(ids), 'ids': ids, 'mode': mode,
         'gloss': GLOSS[seed_of(name, d, n, mode) % 3] if n > 1 else GLOSS[(d + len(mode)) % 4],
         'T': Table(T, ld, tshift), 'W': Table(W, ld, tshift),
         'G': Table((rng.standard_normal((rows, d)) * 0.1).astype(np.float32), ld, gshift),
         'GW': Table((rng.standard_normal((rows, d)) * 0.1).astype(np.float32), ld, gshift)}
    c['vec4_fwd'] = can_vec4(d, [tshift], [ld])
    c['vec4_bwd'] = can_vec4(d, [tshift, gshift], [ld])
    return c


def check_reg_case(c):
    """Promises of a regulariser case: hinge margins (check_rows), the path its label names, duplicates where asked for."""
    check_rows(c['T'].view())
    r = rung(c['d'], c['vec4_bwd'])
    if r is not None:
        w, g, cpl = r
        assert 'f%d/G%d' % (w, g) + ('x%d' % cpl if g == 64 else '') == c['name'], (c['name'], r)
        assert c['vec4_fwd'] == (c['vec4_bwd'] or c['how'] == 'grad')
    if c['how'] == 'pitch4':
        assert c['vec4_bwd'] and c['ld'] == c['d'] + 4
    if c['mode'] == 'heavy':
        assert int((c['ids'] == 5).sum()) >= 64
    if c['ids'] is not None:
        assert int(c['ids'].max()) < c['T'].rows and c['T'].rows - len(set(c['ids'].tolist())) >= 1      # an unnamed row exists
    else:
        assert c['n'] < c['T'].rows


def rung_cases():
    """Specs (the arguments of reg_case); the tables are built inside the test."""
    out = []
    firsts = set()
    for name, d, how in RUNG_CASES:
        gpb = group_rows(name)
        out.append((name, d, how, gpb + 1, 'ids', None))
        out.append((name, d, how, gpb + 1, 'null', None))
        if name not in firsts:                                            # one d per rung: the other row counts and the heavy row
            firsts.add(name)
            out += [(name, d, how, n, 'ids', None) for n in sorted({1, gpb - 1, gpb})]
            out.append((name, d, how, 1, 'null', None))
            out.append((name, d, how, gpb + 1, 'heavy', None))
    return out


def seam_cases():
    out = []
    for name, d, how in SEAM_D:
        gpb = group_rows(name)
        out.append((name, d, how, 128 * gpb + 1, 'ids', 64))
        out.append((name, d, how, 128 * gpb + 1, 'null', None))
        out.append((name, d, how, 2048 * gpb + 1, 'ids', 64))
        out.append((name, d, how, 2048 * gpb + 1, 'null', None))
    return out


def serial_cases():
    return [(name, d, how, 3 * group_rows(name) + 1, 'heavy', None) for name, d, how in SERIAL_D]


def case_id(spec):
    name, d, how, n, mode = spec[:5]
    return '%s-d%d%s-n%d-%s' % (name.replace('/', '_'), d, '-' + how if how else '', n, mode)


PAIR_N = (0, 1, 255, 256, 257, 1023, 1024, 1025, 65537, 262145)
PAIR_KINDS = (('bpr', 1.0), ('bpr', -1.0), ('margin', 1.0), ('margin', 0.5))


def pair_case(kind, param, n):
    rng = np.random.default_rng(seed_of('pair', kind, param, n))
    pos, neg = pair_scores(rng, n, kind, param)
    return {'kind': kind, 'param': param, 'n': n, 'pos': pos, 'neg': neg, 'gloss': GLOSS[(n + int(param * 2)) % 4]}
