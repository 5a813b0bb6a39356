"""fp64 models and checkers of the sharded step's launches (csrc/ktup_shard_step.hip + the segment walk of csrc/ktup_segreduce.hip;
include/ktup_hip.h "row-sharded tables").  NOT a test module: tests/test_shard_ref_host.py pins it on the CPU (torch fp64, defect
rejection, an fp32 emulation of every generated case), tests/test_hip_shard_abi.py compares the kernels with it on the GPU.  numpy
only; the per-element update rules and their constants are those of tests/_optim_ref.py (the kernels evaluate the same formulas).

ROUTE.  Slots inside an (owner, table) block are handed out in atomic arrival order, so check_route asserts invariants (its
docstring), never equality with route_model, which is one admissible outcome (first appearance in entry order).

REDUCE.  reduce_terms gives, per wire row, the fp64 sum of its entries' source rows, the sum of their magnitudes and the entry
count k.  u = 2^-24 throughout.
  row element  k fp32 terms summed in any order: every one of the k - 1 additions rounds a partial sum that is at most sum |terms|:
               |error| <= (k - 1) u sum |terms|.  k = 1: no addition at all (0 + g is exact) -- bit-identical (stored), or the ONE
               correctly rounded add old + g (accumulated).  Accumulating onto `old` is one more term: k u (|old| + sum |terms|).
  squared norm Every thread keeps an fp32 chain `ss`; a wave sums 64 chains in 6 butterfly steps; the four wave sums, the workgroups
               and the slots are joined in double (3 joins, no fp32 rounding worth counting: 1e-14 of the scale is allowed for them).
               Operations on one chain: a lane group walks `chunk` sorted entries and closes at most `chunk` rows, CPL
               (float4 columns per lane) additions each; with dup_only it also subtracts CPL squares per entry; lane group 0
               also closes the rows joined across the workgroup's chunks, at most 2 x (256 / GL) of them.  Each added term has
               at most 5 roundings of its own (dot4: a product and three fmas; a boundary add's 2 old v + v^2 per component and
               the sum of four).  So
                   C_norm = CPL x (chunk x (1 + dup_only) + 2 x 256 / GL) + 5 + 6 + 3          (norm_constant)
               in units of u x scale, scale = the sum of the ABSOLUTE terms: sum |row|^2 for rows finished in registers,
               (sum_e |g_e|)^2 for a boundary row (its adds 2 old v + v^2 telescope to |row|^2, and sum (2 |old| |v| + v^2) <=
               (sum |v|)^2), plus sum_e |g_e|^2 over the entries of shared rows for dup_only -- NOT the (small) difference.
               On top, the squared row inherits the row's own summation error: d(row^2) = 2 |row| (k - 1) u sum |terms| per
               element; a boundary row's atomics round k' <= k - 1 times more, each moving the telescoped sum by 2 u row^2:
               4 (k - 1) u (sum |terms|)^2 covers both there.  Small gradients: a thread of the extra workgroups takes
               ks = ceil(N / (blocks x 256)) fmas of weight x v x v (3 roundings each): (3 ks + 9) u weight sum v^2.
               For a LISTED row this part of the bound is weak: with k entries it allows ~4 (k - 1) u of the row's (sum |g|)^2, a
               few percent of the norm for one row of 5 S entries -- which entries a workgroup's partial holds depends on the
               arrival order, so the partials' own magnitudes cannot be stated.  What holds such a row is the direct comparison
               of its sum in gwire after the norm call, at (k - 1) u sum |terms| per element.
  apply        per element C x u x scale of tests/_optim_ref.py (constants / _update: the same update1 formulas, the clip
               coefficient's (4k + 8) / 2 replaced by HALF the relative bound of the squared norm actually handed in), plus the
               reduced gradient's own bound delta = coef (k - 1) u sum |terms| carried through the rule to first order:
               max |f(g +- delta) - f(g)| (f smooth; delta <= 1e-3 |g| here, the second-order term is ignored as there).
  replay       The steps a row owes (lazy_rows: the Adam zero-gradient replay; under weight decay every owed step on wd * p for
               rules 0 / 1 / 2), in ktup_shard_adam_catchup and, for rows with last < t - 1, inside the two apply launches, have
               no derived bound: the series form, __expf-seeded bias corrections, rcp / rsq, a closed form for SGD.  They are held
               to 4 x the error of an fp32 emulation of the step-by-step recurrence over the same rows (_measured), printed by
               tests/test_shard_ref_host.py; lazy_rows itself is pinned to dense torch.optim over the owed steps there.

GEOMETRY of the two fused walks (ktup_shard_reduce_norm / _apply / _store): chunk = 8 sorted entries per lane group below 73,728
entries (option shard_chunk overrides, rounded up to 4), GL = 16 / 32 / 64 lanes for d <= 64 / 128 / above, 256 / GL groups per
workgroup: a workgroup's stretch is S = chunk x 256 / GL entries.  A row is listed (boundary) by workgroup b at its head when it
continues the previous stretch and at its tail when it continues into the next; predict_xkeys models exactly that."""
import math

import numpy as np

from tests import _optim_ref as O

U = 2.0 ** -24
TILE, MAX_TILES = 1024, 1024                     # csrc/ktup_shard_step.hip: counters per scan tile, tiles the scatter launch scans
SUMSQ_SLOTS = 16                                 # KTUP_SHARD_SUMSQ_SLOTS
SGD, ADAGRAD, ADAM = 0, 1, 2                     # KTUP_OPT_*


# ------------------------------------------------------------------------------------------------ wire layout and route
def wire(world, cap):
    cap = [int(c) for c in cap]
    toff = np.concatenate([[0], np.cumsum(cap)]).astype(np.int64)
    return cap, toff, int(toff[-1]), int(world) * int(toff[-1])


def tables_of(n, block, ent_off):
    """Table of every entry: the number of i in 1 .. T - 1 with (e mod block) >= ent_off[i]."""
    ent_off = np.asarray(ent_off, np.int64)
    T = len(ent_off) - 1
    return np.searchsorted(ent_off[1:T], np.arange(n, dtype=np.int64) % int(block), side='right').astype(np.int64)


def sort_layout(n, W):
    """Offsets (int32 words) of start / rank / perm / skey / tile totals in sort_ws and its length (route_impl)."""
    o_rank = (W + 2) & ~1
    return {'start': 0, 'rank': o_rank, 'perm': o_rank + n, 'skey': o_rank + 2 * n, 'tiles': o_rank + 3 * n,
            'len': o_rank + 3 * n + (W + TILE - 1) // TILE}


def route_model(ids, block, ent_off, world, cap, pair_a=None, pair_b=None):
    """One admissible route: slots in order of first appearance.  Overflowing ids take slot 0 of their block, as the kernel's."""
    ids = np.asarray(ids, np.int64)
    n, T = len(ids), len(cap)
    cap, toff, capsum, W = wire(world, cap)
    tab = tables_of(n, block, ent_off)
    counters = np.zeros(world * T + 1, np.int32)
    send = np.full(W, -1, np.int64)
    inverse = np.full(n, W, np.int64)
    seen = {}
    for e in range(n):
        g = int(ids[e])
        if g < 0:
            continue
        t = int(tab[e])
        if (t, g) not in seen:
            p = g % world if world > 1 else 0
            slot = int(counters[p * T + t])
            counters[p * T + t] += 1
            if slot >= cap[t]:
                counters[world * T] += 1
                slot = 0
            else:
                send[p * capsum + toff[t] + slot] = g // world if world > 1 else g
            seen[(t, g)] = p * capsum + toff[t] + slot
        inverse[e] = seen[(t, g)]
    pair_map = None
    if pair_a is not None:
        pair_map = np.full(W + 1, -7, np.int32)
        shift = int(ent_off[pair_b]) - int(ent_off[pair_a])
        for e in np.nonzero((tab == pair_a) & (ids >= 0))[0]:
            pair_map[inverse[e]] = inverse[e + shift]
    lay = sort_layout(n, W)
    ws = np.zeros(lay['len'], np.int32)
    on = ids >= 0
    hist = np.bincount(inverse[on], minlength=W)[:W]
    prefix = np.concatenate([[0], np.cumsum(hist)])
    ws[:W] = prefix[:W]
    ws[W] = int(on.sum())
    fill = np.zeros(W, np.int64)
    for e in range(n):
        if not on[e]:
            ws[lay['rank'] + e] = -1
            continue
        w = inverse[e]
        ws[lay['rank'] + e] = fill[w]
        pos = prefix[w] + fill[w]
        fill[w] += 1
        ws[lay['perm'] + pos] = e
        ws[lay['skey'] + pos] = w
    return {'inverse': inverse, 'send_ids': send, 'pair_map': pair_map, 'counters': counters, 'sort_ws': ws}


def check_route(ids, block, ent_off, world, cap, inverse, send_ids, pair_map, counters, sort_ws, pair_a=1, pair_b=2):
    """The invariants of ktup_shard_route's outputs (W = world x sum(cap)); raises AssertionError.
    counters[p T + t] = distinct non-negative ids of table t owned by p; the first that many slots of block (p, t) of send_ids hold
    exactly {id // world}, the others -1; inverse[e] = W exactly for padding, otherwise a row of block (id % world, t) whose
    send_ids is id // world; pair_map[inverse[e]] = inverse of the partner entry; sort_ws: start[W] = m, rank = -1 exactly for
    padding, a row's ranks a permutation of 0 .. count - 1, perm[0 .. m) a permutation of the live entries placed at (exclusive
    prefix of the histogram at inverse[e]) + rank[e], skey[k] = inverse[perm[k]] non-decreasing.  start[0 .. W) itself is scratch in
    either scan form and is not looked at.  Overflow (more distinct ids than cap[t] somewhere): counters[world T] = the surplus, every
    inverse still in [0, W], the block's slots hold distinct members of its id set."""
    ids = np.asarray(ids, np.int64)
    n, T = len(ids), len(cap)
    cap, toff, capsum, W = wire(world, cap)
    inverse, send_ids, counters, sort_ws = (np.asarray(a) for a in (inverse, send_ids, counters, sort_ws))
    assert len(inverse) == n and len(send_ids) >= W and len(counters) >= world * T + 1
    tab = tables_of(n, block, ent_off)
    on = ids >= 0
    owner = ids % world if world > 1 else np.zeros(n, np.int64)
    local = ids // world if world > 1 else ids
    surplus, over = 0, np.zeros((world, T), bool)
    for p in range(world):
        for t in range(T):
            want = set(local[on & (owner == p) & (tab == t)].tolist())
            assert int(counters[p * T + t]) == len(want), ('counter', p, t, int(counters[p * T + t]), len(want))
            seg = send_ids[p * capsum + toff[t]:p * capsum + toff[t + 1]]
            k = min(len(want), cap[t])
            have = seg[:k].tolist()
            assert len(set(have)) == k and set(have) <= want, ('send_ids block', p, t)
            assert (seg[k:] == -1).all(), ('unused slots of send_ids must be -1', p, t)
            over[p, t] = len(want) > cap[t]
            surplus += max(0, len(want) - cap[t])
    assert int(counters[world * T]) == surplus, ('overflow word', int(counters[world * T]), surplus)
    assert (inverse[~on] == W).all(), 'padding entries must map to row W'
    inv = inverse[on].astype(np.int64)
    lo = owner[on] * capsum + toff[tab[on]]
    assert ((inv >= lo) & (inv < lo + np.asarray(cap, np.int64)[tab[on]])).all(), 'an entry outside its (owner, table) block'
    fits = ~over[owner[on], tab[on]]
    assert (send_ids[inv[fits]] == local[on][fits]).all(), 'send_ids[inverse[e]] is not the entry\'s local row'
    key = tab[on] * (1 << 57) + ids[on]                                 # one wire row per (table, id), also under overflow
    order = np.argsort(key, kind='stable')
    same = key[order][1:] == key[order][:-1]
    assert (inv[order][1:][same] == inv[order][:-1][same]).all(), 'one (table, id) in two wire rows'
    if pair_map is not None:
        pair_map = np.asarray(pair_map)
        ea = np.nonzero(on & (tab == pair_a))[0]
        partner = ea + (int(ent_off[pair_b]) - int(ent_off[pair_a]))
        assert (pair_map[inverse[ea]] == inverse[partner]).all(), 'pair_map'
    lay = sort_layout(n, W)
    assert len(sort_ws) >= lay['len']
    m = int(on.sum())
    assert int(sort_ws[W]) == m, ('start[W]', int(sort_ws[W]), m)
    rank = sort_ws[lay['rank']:lay['rank'] + n].astype(np.int64)
    perm = sort_ws[lay['perm']:lay['perm'] + n].astype(np.int64)
    skey = sort_ws[lay['skey']:lay['skey'] + n].astype(np.int64)
    assert ((rank == -1) == ~on).all(), 'rank must be -1 exactly for padding'
    hist = np.bincount(inv, minlength=W)
    rk = rank[on]
    order = np.lexsort((rk, inv))
    first = np.concatenate([[0], np.cumsum(hist)])[inv[order]]
    assert (rk[order] == np.arange(m) - first).all(), 'the ranks of a row are not a permutation of 0 .. count - 1'
    pos = np.concatenate([[0], np.cumsum(hist)])[inv] + rk
    assert (perm[pos] == np.nonzero(on)[0]).all(), 'perm does not place an entry at prefix + rank'
    assert (skey[:m] == inverse[perm[:m]]).all() and (np.diff(skey[:m]) >= 0).all(), 'skey'


def ktup_entries_model(u, pos, neg, item2ent, ent_pad):
    """[u | pos ; neg | item2ent[pos ; neg]] (5B; 3B without item2ent), an entity < 0 or == ent_pad becoming padding."""
    items = np.concatenate([pos, neg]).astype(np.int64)
    if item2ent is None:
        return np.concatenate([np.asarray(u, np.int64), items])
    ent = np.asarray(item2ent, np.int64)[items]
    ent = np.where((ent < 0) | (ent == ent_pad), -1, ent)
    return np.concatenate([np.asarray(u, np.int64), items, ent])


def kg_entries_model(ph, pt, pr, nh, nt, nr):
    """entries = [ph ; pt ; nh ; nt] with a twin (nh == ph, nt == pt) as -1; rels = [pr ; nr]."""
    return (np.concatenate([ph, pt, np.where(nh == ph, -1, nh), np.where(nt == pt, -1, nt)]).astype(np.int64),
            np.concatenate([pr, nr]).astype(np.int64))


# ------------------------------------------------------------------------------------------------ geometry of the walks
def fused_chunk(n_entries, opt=0):
    if opt > 0:
        return (opt + 3) & ~3
    ch = n_entries // 8192
    return (min(max(ch, 8), 64) + 3) & ~3


def fused_gl(d):
    nch = d // 4
    return 16 if nch <= 16 else 32 if nch <= 32 else 64


def fused_cpl(d):
    nch = d // 4
    return 1 if nch <= 64 else 2 if nch <= 128 else 4


def stretch(n_entries, d, opt=0):
    return fused_chunk(n_entries, opt) * (256 // fused_gl(d))


def fused_grid(n_entries, d, opt=0):
    return -(-n_entries // stretch(n_entries, d, opt))


def list_len(n_entries, d, opt=0):
    return 2 * fused_grid(n_entries, d, opt)


def predict_xkeys(skey, m, n_entries, d, opt=0):
    """xkeys after ktup_shard_reduce_norm: [2 b], [2 b + 1] = the row workgroup b shares with b - 1 / b + 1, else -1."""
    S = stretch(n_entries, d, opt)
    out = np.full(list_len(n_entries, d, opt), -1, np.int32)
    for b in range(len(out) // 2):
        w0, w1 = b * S, min(m, (b + 1) * S)
        if w0 >= m:
            break
        if w0 > 0 and skey[w0 - 1] == skey[w0]:
            out[2 * b] = skey[w0]
        if w1 < m and skey[w1] == skey[w1 - 1]:
            out[2 * b + 1] = skey[w1 - 1]
    return out


def norm_constant(n_entries, d, dup_only, opt=0):
    """C_norm of the module docstring."""
    return fused_cpl(d) * (fused_chunk(n_entries, opt) * (2 if dup_only else 1) + 2 * (256 // fused_gl(d))) + 5 + 6 + 3


# ------------------------------------------------------------------------------------------------ reduce
def source_rows(n_entries, n_src, src_off):
    e = np.arange(n_entries, dtype=np.int64)
    return np.where(e < n_src, e, e - src_off)


def reduce_terms(G, n_src, src_off, inverse, n_wire_rows, d=None):
    """(sum, sum of magnitudes, entry count) per wire row in fp64; rows of G no live entry names are never looked at."""
    inverse = np.asarray(inverse, np.int64)
    d = G.shape[1] if d is None else d
    on = np.nonzero(inverse < n_wire_rows)[0]
    rows = G[source_rows(len(inverse), n_src, src_off)[on], :d].astype(np.float64)
    tot, mag = np.zeros((n_wire_rows, d)), np.zeros((n_wire_rows, d))
    np.add.at(tot, inverse[on], rows)
    np.add.at(mag, inverse[on], np.abs(rows))
    return tot, mag, np.bincount(inverse[on], minlength=n_wire_rows)


def reduce_ref(G, n_src, src_off, inverse, n_wire_rows=None, d=None):
    """The fp64 index_add of the source rows: entry e reads row e of G for e < n_src, row e - src_off otherwise."""
    inverse = np.asarray(inverse, np.int64)
    W = int(inverse.max()) if n_wire_rows is None else n_wire_rows       # (padding maps to row W itself)
    return reduce_terms(G, n_src, src_off, inverse, W, d)[0]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check_reduced(got, before, G, n_src, src_off, inverse, d, store):
    """gwire (W x ld, fp32) after ktup_shard_reduce_rows (store = False: before + sum) or after ktup_shard_zero_shared_rows +
    ktup_shard_reduce_store (store = True) against reduce_terms.  Exact facts: pitch columns and (store) rows without an entry
    bit-identical to `before`; a row with one entry bit-identical to its source row (store) or to the one fp32 add before + g.
    Returns the largest error / tolerance over the rows with two or more entries."""
    W = got.shape[0]
    tot, mag, cnt = reduce_terms(G, n_src, src_off, inverse, W, d)
    assert np.array_equal(_bits(got[:, d:]), _bits(before[:, d:])), 'pitch columns written'
    one, many, none = cnt == 1, cnt >= 2, cnt == 0
    if store:
        assert np.array_equal(_bits(got[none, :d]), _bits(before[none, :d])), 'a row without entries was written'
        assert np.array_equal(got[one, :d], tot[one].astype(np.float32)), 'a single-entry row is not its source row'
        want, tol = tot, (cnt[:, None] - 1) * U * mag
    else:
        old = before[:, :d].astype(np.float64)
        assert np.array_equal(_bits(got[none, :d]), _bits(before[none, :d])), 'a row without entries changed'
        assert np.array_equal(got[one, :d], before[one, :d] + tot[one].astype(np.float32)), 'a single-entry row is not old + g'
        want, tol = old + tot, cnt[:, None] * U * (np.abs(old) + mag)
    if not many.any():
        return 0.0
    err = np.abs(got[many, :d].astype(np.float64) - want[many])
    ratio = err / np.maximum(tol[many], 1e-300)
    assert np.isfinite(got[many, :d]).all() and (err <= tol[many]).all(), ('reduced rows', float(ratio.max()))
    return float(ratio.max())


def sumsq_ref(G, n_src, src_off, inverse, W, d, n_entries, dup_only, boundary=(), smalls=(), small_weight=1.0, fold=None, opt=0):
    """(want, tolerance) of what ktup_shard_reduce_norm adds to the sum of squares; `boundary`: the wire rows predict_xkeys lists."""
    inverse = np.asarray(inverse, np.int64)
    tot, mag, cnt = reduce_terms(G, n_src, src_off, inverse, W, d)
    rows = cnt >= 2 if dup_only else cnt >= 1
    is_b = np.zeros(W, bool)
    is_b[[int(b) for b in boundary]] = True
    want = float((tot[rows] ** 2).sum())
    term = np.where(is_b[:, None], mag ** 2, tot ** 2)[rows].sum()
    own = (np.where(is_b[:, None], 4.0 * mag * mag, 2.0 * np.abs(tot) * mag) * (cnt[:, None] - 1))[rows].sum()
    if dup_only:
        on = np.nonzero(inverse < W)[0]
        on = on[cnt[inverse[on]] >= 2]
        sq = float((G[source_rows(len(inverse), n_src, src_off)[on], :d].astype(np.float64) ** 2).sum())
        want -= sq
        term += sq
    tol = U * (norm_constant(n_entries, d, dup_only, opt) * term + own) + 1e-14 * term
    N = sum(int(s.size) for s in smalls)
    if N:
        blocks = min(-(-N // 2048), 64)
        ks = -(-N // (blocks * 256))
        sv = float(sum((s.astype(np.float64) ** 2).sum() for s in smalls))
        want += float(small_weight) * sv
        tol += (3 * ks + 9) * U * float(small_weight) * sv
    if fold is not None:
        want += float(np.sum(fold))
        tol += 1e-15 * float(np.abs(fold).sum())
    return want, tol


def check_sumsq(got, want, tol, what='sumsq'):
    assert math.isfinite(got) and abs(got - want) <= tol, (what, got, want, abs(got - want), tol)
    return abs(got - want) / tol if tol > 0 else 0.0


def check_xkeys(got, want):
    """Exactly the predicted list (equal keys adjacent, the rest -1) at the predicted length."""
    got = np.asarray(got)
    assert got.shape == want.shape and np.array_equal(got, want), ('xkeys', got.tolist(), want.tolist())
    live = got[got >= 0]
    for k in set(live.tolist()):
        idx = np.nonzero(got == k)[0]
        assert (np.diff(idx) == 1).all(), 'equal keys must be adjacent'


# ------------------------------------------------------------------------------------------------ apply
def adam_pitch(d):
    return 2 * d + 4                                                    # KTUP_SHARD_ADAM_STATE_PITCH


def clip_coef(sumsq, max_norm):
    return O.clip_coef(sumsq, max_norm)


def hyper_of(c):
    return {'lr': float(np.float32(c['lr'])), 'wd': float(np.float32(c.get('wd', 0.0))), 'momentum': 0.0,
            'beta1': float(np.float32(c.get('beta1', 0.9))), 'beta2': float(np.float32(c.get('beta2', 0.999))),
            'eps': float(np.float32(c['eps'])), 'alpha': 0.0}


def rule_of(c):
    """The dense rule (tests/_optim_ref.py kind) a case's rows take: plain SGD / Adagrad, or ktup_adam_t's rule 0 / 1 / 2."""
    if c['kind'] == ADAM:
        return {0: O.ADAM, 1: O.ADAGRAD, 2: O.SGD}[c['rule']]
    return {SGD: O.SGD, ADAGRAD: O.ADAGRAD}[c['kind']]


def _rows_update(c, p, g, delta, m, v, coef, C):
    """One rule on a block of rows in fp64: {'p', 'm', 'v'} -> (want, tol); m / v None where the kind has no such half."""
    h = hyper_of(c)
    if c['kind'] != ADAM:
        h['wd'] = 0.0
    rule = rule_of(c)
    bc1, bc2s = O.bias_terms(h, c['t']) if rule == O.ADAM else (1.0, 1.0)
    zero = np.zeros_like(p)
    s1, s2 = (m, v) if rule == O.ADAM else (v, zero)

    def f(gg):
        return O._update(rule, p, gg * coef, zero if s1 is None else s1, zero if s2 is None else s2, h, bc1, bc2s, False)
    mid, hi, lo = f(g), f(g + delta), f(g - delta)
    out = {}
    names = {O.SGD: (('p', 'p'),), O.ADAGRAD: (('p', 'p'), ('s1', 'v')), O.ADAM: (('p', 'p'), ('s1', 'm'), ('s2', 'v'))}[rule]
    for name, key in names:
        want, scale = mid[name]
        prop = np.maximum(np.abs(hi[name][0] - want), np.abs(lo[name][0] - want))
        out[key] = (want, C[name] * U * scale + prop)
    return out


def apply_ref(c, gsum, gdelta, touched, sumsq, sumsq_tol):
    """What ktup_shard_apply / ktup_shard_reduce_apply leave behind, as {buffer: (want fp64 or exact array, tol or None)}.
    c: the case (tests/_shard_cases.apply_case); gsum / gdelta: W x d fp64 gradient per wire row and its absolute error bound;
    touched: the wire rows the launch steps (ids >= 0 and, for the fused walk, at least one entry).  tol None = compared exactly.
    Skip (skip_count or skip_value non-zero): nothing moves, the books: loss_step := 0, loss_sum unchanged, skipped + 1."""
    d, T = c['d'], c['T']
    skip = bool(c['skip_count']) or c['skip_value'] != 0.0
    coef = clip_coef(sumsq, c['max_norm'])
    clipped = coef < 1.0
    h = hyper_of(c)
    rel = (sumsq_tol / sumsq / U) if (clipped and sumsq > 0) else 0.0
    C = O.constants(rule_of(c), h, clipped, (rel - 8.0) / 4.0)
    adam = c['kind'] == ADAM
    cap, toff, capsum, W = wire(c['n_blocks'], c['cap'])
    out = {'tables': [], 'states': [], 'small': []}
    wt = np.searchsorted(toff[1:T], np.arange(W) % capsum, side='right')
    for t in range(T):
        P = c['tables'][t]
        want_p, tol_p = P.astype(np.float64), np.zeros(P.shape)
        S = c['states'][t] if c['states'] is not None else None
        want_s = None if S is None else S.copy()                      # fp32 bits; the touched rows' halves are replaced below
        tol_s = None if S is None else np.zeros(S.shape)
        ws64 = None if S is None else S.astype(np.float64)
        rows_w = np.nonzero((wt == t) & touched)[0] if not skip else np.zeros(0, np.int64)
        if len(rows_w):
            r = c['ids'][rows_w]
            assert len(set(r.tolist())) == len(r), 'owner-side ids must be distinct per table'
            m = ws64[r, :d] if adam else None
            v = ws64[r, d:2 * d] if adam else (ws64[r, :d] if S is not None else None)
            up = _rows_update(c, want_p[r, :d], gsum[rows_w], gdelta[rows_w], m, v, coef, C)
            want_p[r, :d], tol_p[r, :d] = up['p']
            if adam:
                for key, sl in (('m', slice(0, d)), ('v', slice(d, 2 * d))):
                    if key in up:
                        ws64[r, sl], tol_s[r, sl] = up[key]
            elif S is not None:
                ws64[r, :d], tol_s[r, :d] = up['v']
            if adam:                                                  # rows that owe steps: the replay, then step t (lazy_rows)
                last = S[r, 2 * d].view(np.int32)
                st = np.nonzero(last < c['t'] - 1)[0]
                if len(st):
                    rs, g = r[st], gsum[rows_w][st]
                    dd = gdelta[rows_w][st] + np.abs(g) * C['g'] * U      # + the clip coefficient's own error
                    (want_p[rs, :d], tol_p[rs, :d]), (ws64[rs, :d], tol_s[rs, :d]), (ws64[rs, d:2 * d], tol_s[rs, d:2 * d]) = \
                        lazy_tolerance(c, P[rs, :d], S[rs, :d], S[rs, d:2 * d], last[st], g, dd, coef)
        out['tables'].append((want_p, tol_p))
        if S is not None:
            stamp = None
            if adam:
                stamp = S[:, 2 * d].view(np.int32).copy()
                if len(rows_w):
                    stamp[c['ids'][rows_w]] = c['t']
            out['states'].append((ws64, tol_s, stamp))
    for k, sm in enumerate(c['smalls']):
        g = sm['g64'] if sm.get('g64') is not None else sm['g'].astype(np.float64)
        res = {}
        for which in ('0', '1'):
            P = sm.get('p' + which)
            if P is None:
                continue
            S = sm.get('s' + which)
            want_p, tol_p = P.astype(np.float64), np.zeros(P.shape)
            ws64 = None if S is None else S.astype(np.float64)
            tol_s = None if S is None else np.zeros(S.shape)
            stamp = None
            if not skip:
                m = ws64[:, :d] if adam else None
                v = ws64[:, d:2 * d] if adam else (ws64[:, :d] if S is not None else None)
                up = _rows_update(c, want_p, g, np.zeros_like(g), m, v, coef, C)
                want_p, tol_p = up['p']
                if adam:
                    for key, sl in (('m', slice(0, d)), ('v', slice(d, 2 * d))):
                        if key in up:
                            ws64[:, sl], tol_s[:, sl] = up[key]
                elif S is not None:
                    ws64[:, :d], tol_s[:, :d] = up['v']
            if adam:
                stamp = S[:, 2 * d].view(np.int32).copy()
                if not skip:
                    stamp[:] = c['t']
            res['p' + which] = (want_p, tol_p)
            res['s' + which] = None if S is None else (ws64, tol_s, stamp)
        out['small'].append(res)
    n_loss = c['n_loss']
    out['loss_step'] = np.zeros(n_loss, np.float32)
    out['loss_sum'] = c['loss_sum'].copy() if skip else (c['loss_sum'] + c['loss_step']).astype(np.float32)   # one fp32 add
    out['skipped'] = c['skipped'] + (1 if skip else 0)
    out['coef'], out['C'] = coef, C
    return out


def _cmp(got, want, tol, what, worst):
    got64 = got.astype(np.float64)
    exact = tol == 0.0
    assert np.array_equal(got[exact], want[exact].astype(np.float32)), (what, 'an element the launch must not move')
    if (~exact).any():
        assert np.isfinite(got[~exact]).all(), (what, 'not finite')
        ratio = np.abs(got64 - want)[~exact] / tol[~exact]
        worst[0] = max(worst[0], float(ratio.max()))
        assert (ratio <= 1.0).all(), (what, float(ratio.max()))


def check_apply(c, ref, got):
    """got: {'tables': [fp32 arrays], 'states': [...], 'small': [{'p0', 's0', 'p1', 's1', 'g'}], 'grads': the gradient buffer
    (gwire of the fused form), 'grads_zero': bool mask of the elements that must be +0.0 (the others bit-identical to
    'grads_before'), 'loss_step', 'loss_sum', 'skipped'}.  Every element of every buffer is compared.  Returns the largest ratio."""
    d = c['d']
    worst = [0.0]
    for t, (want, tol) in enumerate(ref['tables']):
        _cmp(got['tables'][t][:, :d], want[:, :d], tol[:, :d], 'table %d' % t, worst)
        assert np.array_equal(_bits(got['tables'][t][:, d:]), _bits(c['tables'][t][:, d:])), 'table pitch columns'
    for t, (want, tol, stamp) in enumerate(ref['states']):
        _check_state(c, got['states'][t], c['states'][t], want, tol, stamp, 'state %d' % t, worst)
    for k, res in enumerate(ref['small']):
        for which in ('0', '1'):
            if 'p' + which in res:
                want, tol = res['p' + which]
                _cmp(got['small'][k]['p' + which], want, tol, 'small p%s[%d]' % (which, k), worst)
                if res['s' + which] is not None:
                    want, tol, stamp = res['s' + which]
                    _check_state(c, got['small'][k]['s' + which], c['smalls'][k]['s' + which], want, tol, stamp, 'small state', worst)
        assert not _bits(got['small'][k]['g']).any(), 'a consumed small gradient is not zero-filled'
    zero = got['grads_zero']
    assert not _bits(got['grads'])[zero].any(), 'a consumed gradient row is not zero-filled'
    assert np.array_equal(_bits(got['grads'])[~zero], _bits(got['grads_before'])[~zero]), 'an unconsumed gradient element changed'
    assert not _bits(got['loss_step']).any(), 'loss_step must be cleared'
    assert np.array_equal(_bits(got['loss_sum']), _bits(ref['loss_sum'])), ('loss_sum', got['loss_sum'], ref['loss_sum'])
    assert int(got['skipped']) == ref['skipped'], ('skipped_steps', int(got['skipped']), ref['skipped'])
    return worst[0]


def _check_state(c, got, before, want, tol, stamp, what, worst):
    d = c['d']
    n = 2 * d if c['kind'] == ADAM else d
    _cmp(got[:, :n], want[:, :n], tol[:, :n], what, worst)
    if stamp is not None:
        assert np.array_equal(got[:, 2 * d].view(np.int32), stamp), (what, 'the rows\' step stamps')
        assert np.array_equal(_bits(got[:, 2 * d + 1:]), _bits(before[:, 2 * d + 1:])), (what, 'padding words')
    else:
        assert np.array_equal(_bits(got[:, n:]), _bits(before[:, n:])), (what, 'pitch columns')


# ------------------------------------------------------------------------------------------------ fp32 emulations (host test)
def emulate_reduce(G, n_src, src_off, inverse, W, d, before=None):
    """The same sums in fp32, one entry after the other in entry order (one of the orders the bound covers)."""
    out = np.zeros((W, d), np.float32)
    src = source_rows(len(inverse), n_src, src_off)
    for e in np.nonzero(np.asarray(inverse) < W)[0]:
        out[inverse[e]] += G[src[e], :d]
    return out if before is None else (before[:, :d] + out).astype(np.float32)


def emulate_sumsq(G, n_src, src_off, inverse, W, d, dup_only, smalls=(), small_weight=1.0, fold=None):
    """fp32 rows (emulate_reduce), fp32 dot4 per float4, fp32 sums across a row; rows joined in double (as the workgroups are)."""
    inverse = np.asarray(inverse)
    rows = emulate_reduce(G, n_src, src_off, inverse, W, d)
    cnt = np.bincount(inverse[inverse < W], minlength=W)
    f32 = np.float32

    def sq(a):
        q = a.reshape(a.shape[0], a.shape[1] // 4, 4)
        return (((q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1]) + q[..., 2] * q[..., 2]) + q[..., 3] * q[..., 3]).sum(axis=1, dtype=f32)
    use = cnt >= 2 if dup_only else cnt >= 1
    tot = float(sq(rows[use]).astype(np.float64).sum())
    if dup_only:
        on = np.nonzero(inverse < W)[0]
        on = on[cnt[inverse[on]] >= 2]
        tot -= float(sq(G[source_rows(len(inverse), n_src, src_off)[on], :d]).astype(np.float64).sum())
    for s in smalls:
        tot += float((f32(small_weight) * s.ravel() * s.ravel()).sum(dtype=f32))
    if fold is not None:
        tot += float(np.sum(fold))
    return tot


def emulate_rule(c, p, g, m, v, coef):
    """update of one block of rows in fp32 numpy operations, the kernel's expressions (up1 / adam_step1 / lazy_step1)."""
    f32 = np.float32
    h = hyper_of(c)
    lr, eps, wd, b1, b2 = (f32(h[k]) for k in ('lr', 'eps', 'wd', 'beta1', 'beta2'))
    rule = rule_of(c)
    g = (f32(coef) * g).astype(f32)
    if c['kind'] == ADAM and float(wd) != 0.0:
        g = (wd * p + g).astype(f32)
    if rule == O.SGD:
        return (p - lr * g).astype(f32), m, v
    if rule == O.ADAGRAD:
        v = (g * g + v).astype(f32)
        return (p - lr * (g / (np.sqrt(v) + eps))).astype(f32), m, v
    bc1, bc2s = (f32(x) for x in O.bias_terms(h, c['t']))
    m = (m + (g - m) * (f32(1.0) - b1)).astype(f32)
    v = ((f32(1.0) - b2) * (g * g) + b2 * v).astype(f32)
    return (p - (lr / bc1) * (m / (np.sqrt(v) / bc2s + eps))).astype(f32), m, v


def adam_replay_ref(p, m, v, last, t, lr, eps, b1, b2, replay, dtype=np.float64):
    """The dense zero-gradient steps last + 1 .. t of a block of rows (last: per row, 0 = never written: the row rests), the
    recurrence of tests/test_hip_sharded_ktup.py::test_adam_flush_replays_the_untouched_steps; beyond `replay` steps only m and
    v keep decaying.  dtype = float32 gives the emulation the replay's tolerance is measured with."""
    f = dtype
    p, m, v = p.astype(f), m.astype(f), v.astype(f)
    last = np.asarray(last, np.int64)
    for s in range(int(last[last > 0].min()) + 1 if (last > 0).any() else t + 1, t + 1):
        on = (last > 0) & (last < s)
        m[on] = m[on] * f(b1)
        v[on] = v[on] * f(b2)
        mv = on & (s - last <= replay)
        p[mv] = p[mv] - f(lr / (1.0 - b1 ** s)) * m[mv] / (np.sqrt(v[mv]) / f(math.sqrt(1.0 - b2 ** s)) + f(eps))
    return p, m, v


def replay_expected(c, dtype=np.float64):
    d = c['d']
    if c.get('wd'):                                                     # weight decay: every owed step on wd * p (lazy_rows)
        return lazy_rows(c, c['p'], c['S'][:, :d], c['S'][:, d:2 * d], c['last'], None, 1.0, dtype)
    return adam_replay_ref(c['p'], c['S'][:, :d], c['S'][:, d:2 * d], np.where(c['last'] >= c['t'], 0, c['last']), c['t'], c['lr'], c['eps'],
                           c['beta1'], c['beta2'], c['replay'], dtype)


MEASURE_MIN = 4096


def _measured(ref, emu, wd, onto=None):
    """Per element, 4 x the largest fp32 error over the block: p absolute; v relative to the element; m relative without weight
    decay and absolute under it (there m = (1 - beta1) sum of beta1^k (wd p) terms beside the decaying old m and may pass through
    zero: a relative figure is then set by the one element nearest zero).  0 everywhere for an array the rule does not write.
    onto: the (want_p, want_m, want_v) the tolerance arrays are laid over (default: ref itself)."""
    out = []
    for i, (r, e) in enumerate(zip(ref, emu)):
        err = np.abs(e.astype(np.float64) - r)
        base = r if onto is None else onto[i]
        if i == 0 or (i == 1 and wd):
            out.append(np.full(base.shape, 4.0 * float(err.max())))
        else:
            out.append(4.0 * float((err / np.maximum(np.abs(r), 1e-300)).max()) * np.abs(base))
    return out


def replay_tolerance(c):
    """{'p', 'm', 'v'}: per-element tolerance of the catch-up, 4 x the fp32 replay's error against the fp64 one (_measured)."""
    return dict(zip('pmv', _measured(replay_expected(c), replay_expected(c, np.float32), c.get('wd'))))


def lazy_rows(c, p, m, v, last, g, coef, dtype=np.float64):
    """include/ktup_hip.h, "Row-sparse ADAM" / "WEIGHT DECAY": a row whose state was written at step `last` first takes the dense
    optimizer's steps last + 1 .. upto on a ZERO gradient -- i.e. on wd * p under weight decay, for rule 0 (Adam: m <- m + (g - m)
    (1 - beta1), v <- (1 - beta2) g^2 + beta2 v, p <- p - lr / (1 - beta1^s) m / (sqrt(v) / sqrt(1 - beta2^s) + eps)), rule 1
    (Adagrad, its sum in v: v <- v + g^2, p <- p - lr g / (sqrt(v) + eps)) and rule 2 (SGD: p <- p - lr g) --, then, if g is given,
    step t on coef * g + wd * p with the bias corrections ktup_shard_step_count rounds to float (upto = t - 1); g None: the catch-up
    to upto = t.  Without weight decay a row never written (last = 0, m = v = 0) rests.  Per-row `last`; dtype float32 is the
    emulation the tolerance is measured with (4 x its error against float64; module docstring)."""
    f = dtype
    h = hyper_of(c)
    rule = c['rule']
    lr, eps, wd, b1, b2 = h['lr'], h['eps'], (h['wd'] if c.get('wd') else 0.0), h['beta1'], h['beta2']
    p, m, v = p.astype(f), m.astype(f), v.astype(f)
    last = np.asarray(last, np.int64)
    t = int(c['t'])
    upto = t if g is None else t - 1

    def one(on, gg, c1, bc2s):
        if rule == 0:
            m[on] = m[on] + (gg - m[on]) * f(1.0 - b1)
            v[on] = f(1.0 - b2) * (gg * gg) + f(b2) * v[on]
            p[on] = p[on] - f(c1) * (m[on] / (np.sqrt(v[on]) / f(bc2s) + f(eps)))
        elif rule == 1:
            v[on] = v[on] + gg * gg
            p[on] = p[on] - f(lr) * (gg / (np.sqrt(v[on]) + f(eps)))
        else:
            p[on] = p[on] - f(lr) * gg
    live = last < upto if wd != 0.0 else (last > 0) & (last < upto)
    for s in range(int(last[live].min()) + 1 if live.any() else upto + 1, upto + 1):
        on = live & (last < s)
        one(on, f(wd) * p[on], lr / (1.0 - b1 ** s), math.sqrt(1.0 - b2 ** s))
    if g is not None:
        bc1, bc2s = O.bias_terms(h, t) if rule == 0 else (1.0, 1.0)
        on = np.ones(len(last), bool)
        gg = f(coef) * g.astype(f)
        one(on, gg + f(wd) * p if wd != 0.0 else gg, lr / bc1, bc2s)
    return p, m, v


def lazy_tolerance(c, p, m, v, last, g, delta, coef):
    """(want, tol) for p, m, v of stale rows: want = lazy_rows in float64; tol = 4 x the largest error of the float32 emulation over
    these rows (_measured; an array the rule does not write has tolerance 0: bit-identical) + what the gradient's own
    bound `delta` moves the result by (|f(g +- delta) - f(g)|, first order)."""
    ref = lazy_rows(c, p, m, v, last, g, coef)
    # The figure is a maximum and must not rest on a handful of elements (at d = 4 a table has 24 stale elements): it is taken over
    # at least MEASURE_MIN elements -- the block itself and seeded copies of it scaled down by factors in [0.5, 1) (same `last`, same
    # formulas, magnitudes never above the block's own).
    K = max(1, -(-MEASURE_MIN // max(p.size, 1)))
    rng = np.random.default_rng(20261021)
    F = np.concatenate([np.ones(p.shape, np.float32)] + [rng.uniform(0.5, 1.0, size=p.shape).astype(np.float32) for _ in range(K - 1)])
    tile = lambda a: np.concatenate([a.astype(np.float32)] * K)
    big = (tile(p) * F, tile(m) * F, tile(v) * F * F, np.concatenate([last] * K), None if g is None else (tile(g) * F).astype(np.float64))
    wide = _measured(lazy_rows(c, *big, coef), lazy_rows(c, big[0], big[1], big[2], big[3], None if g is None else big[4].astype(np.float32),
                                                         coef, np.float32), c.get('wd'), ref)
    out = [[r, t] for r, t in zip(ref, wide)]
    if g is not None and np.any(delta):
        hi, lo = lazy_rows(c, p, m, v, last, g + delta, coef), lazy_rows(c, p, m, v, last, g - delta, coef)
        for i in range(3):
            out[i][1] = out[i][1] + np.maximum(np.abs(hi[i] - out[i][0]), np.abs(lo[i] - out[i][0]))
    return out
