"""Seeded case generators of the sharded-step parity suite (tests/_shard_ref.py has the models; tests/test_shard_ref_host.py runs
every case through an fp32 emulation on the CPU, tests/test_hip_shard_abi.py through the kernels).  numpy only.

Geometry without a hand-written sort_ws: route with world = 64 and cap = [1] * T over ids 0 .. 63 -- the slot is always 0, so id i
of table t sits in wire row i T + t whatever the arrival order, and the sorted order is fixed by the multiplicities alone.  A
LAYOUT is a list of per-row entry counts (rows in sorted order) + a number of padding entries; layouts(S, chunk) writes them
relative to the walk's stretch S and chunk (tests/_shard_ref.py GEOMETRY)."""
import zlib

import numpy as np

from tests import _shard_ref as R

T_GEO, WORLD_GEO = 4, 64
DS = (4, 64, 68, 100, 128, 132, 256, 260, 512, 516, 1024)            # one per template rung and edge
FULL_DS = (64, 100, 256)                                              # the whole layout list; the others take EDGE
LAYOUTS = ('m1', 'm_chunk', 'm_chunk_p1', 'm_S', 'm_S_p1', 'singles', 'one_row_5S', 'ends_on_edge', 'each_side', 'whole_stretch',
           'stretch_p2', 'three_stretches', 'consecutive', 'first_last', 'padded', 'ktup')
EDGE = ('m_S_p1', 'stretch_p2', 'first_last', 'padded')


def seed_of(*key):
    return zlib.crc32(repr(key).encode()) & 0x7fffffff


def split(rng, m):
    """Row counts of 1 .. 5 entries that sum to m."""
    out = []
    while m > 0:
        k = int(min(m, rng.integers(1, 6)))
        out.append(k)
        m -= k
    return out


def layout(name, S, c, rng):
    """(per-row entry counts in sorted order, padding entries)."""
    sp = lambda m: split(rng, m)
    return {
        'm1': lambda: ([1], 0),
        'm_chunk': lambda: (sp(c), 0),
        'm_chunk_p1': lambda: (sp(c - 2) + [3], 0),                   # the last row has two entries before the chunk edge, one after
        'm_S': lambda: (sp(S), 0),
        'm_S_p1': lambda: (sp(S - 1) + [2], 0),                       # one entry on each side of the stretch edge
        'singles': lambda: ([1] * min(T_GEO * WORLD_GEO, 2 * S + 3), 0),
        'one_row_5S': lambda: ([5 * S], 0),
        'ends_on_edge': lambda: (sp(S - 6) + [6] + sp(9), 0),         # ends exactly on the edge: no boundary at all
        'each_side': lambda: (sp(S - 1) + [2] + sp(7), 0),
        'whole_stretch': lambda: (sp(S) + [S] + sp(5), 0),            # one aligned stretch: interior, not listed
        'stretch_p2': lambda: (sp(S - 1) + [S + 2] + sp(5), 0),       # the middle workgroup lists it on both sides
        'three_stretches': lambda: ([3, 3 * S + 5, 2, 4], 0),
        'consecutive': lambda: (sp(S - 2) + [4] + sp(S - 4) + [4] + sp(S - 4) + [4, 3], 0),
        'first_last': lambda: ([S + 1] + sp(S - 3) + [6], 0),         # the first row and the last row are both boundary rows
        'padded': lambda: (sp(S - 1) + [2] + sp(S - 4) + [5], 2 * S + 7),       # m < n_entries: trailing workgroups exit early
    }[name]()


def layouts_of(d):
    return LAYOUTS if d in FULL_DS else EDGE


# (d, layout, shard_chunk option, pitched G / gwire): every layout at 64, 100, 256, the edge layouts elsewhere, chunk 4 and 12, pitches
CASES = [(d, name, 0, False) for d in DS for name in layouts_of(d)] + \
        [(64, 'stretch_p2', 4, False), (256, 'consecutive', 12, False), (100, 'padded', 0, True), (256, 'stretch_p2', 0, True),
         (64, 'ktup', 12, True)]
# (kind, clip, skip, n_small, second summand table, small_g64, sumsq slots, stale) of the apply launches; stale: some touched rows carry
# last = t - 2, t - 4, t - 7 and owe the launch the steps in between (the Adam zero-gradient replay; under weight decay rules 0, 1, 2)
APPLY_OPTIONS = [('sgd', 'clip', None, 2, True, False, 1, False), ('adagrad', 'unit', None, 4, False, False, 16, False),
                 ('adam', 'clip', None, 2, True, True, 16, False), ('adam_wd', 'off', None, 0, False, False, 1, False),
                 ('adagrad_wd', 'clip', 'count', 2, True, False, 16, False), ('sgd_wd', 'negative', None, 1, False, True, 1, False),
                 ('adagrad', 'clip', 'value', 2, False, False, 1, False), ('sgd_wd', 'clip', None, 3, True, False, 16, False),
                 ('adagrad_wd', 'unit', None, 1, True, True, 1, False), ('adam', 'clip', None, 1, False, False, 1, True),
                 ('adam_wd', 'clip', None, 2, True, False, 16, True), ('adagrad_wd', 'off', None, 0, False, False, 1, True),
                 ('sgd_wd', 'unit', None, 1, True, False, 16, True)]


def case_id(c):
    return '%d-%s%s%s' % (c[0], c[1], '-chunk%d' % c[2] if c[2] else '', '-pitched' if c[3] else '')


def reduce_case(d, name, opt=0, pitched=False):
    """Entries, the wire rows they must get, the sorted order, and G (NaN in rows no live entry may read and in pitch columns)."""
    rng = np.random.default_rng(seed_of('reduce', d, name, opt, pitched))
    if name == 'ktup':
        return _ktup_case(d, rng, opt, pitched)
    T, world = T_GEO, WORLD_GEO
    # (the chunk of fewer than 73,728 entries does not depend on their number)
    c = R.fused_chunk(1, opt)
    S = c * (256 // R.fused_gl(d))
    counts, n_pad = layout(name, S, c, rng)
    assert len(counts) <= T * world, (name, len(counts))
    rows = np.sort(rng.choice(T * world, size=len(counts), replace=False))          # the wire rows in use, ascending
    seg = [[] for _ in range(T)]
    for w, k in zip(rows, counts):
        seg[w % T] += [w // T] * k
    for t in rng.integers(0, T, size=n_pad):
        seg[t].append(-1)
    ids = np.concatenate([rng.permutation(np.asarray(s, np.int64)) for s in seg]).astype(np.int64)
    ent_off = np.concatenate([[0], np.cumsum([len(s) for s in seg])]).astype(np.int64)
    n = len(ids)
    tab = R.tables_of(n, n, ent_off)
    inverse = np.where(ids >= 0, ids * T + tab, T * world)
    return _finish(d, name, opt, pitched, rng, ids, ent_off, T, world, inverse, n, 0, None)


def _ktup_case(d, rng, opt, pitched):
    """The KTUP re-read layout: entries [u | pos ; neg | item2ent[pos ; neg]] (5B), G = [GU ; GV] (3B rows): n_src = 3B, src_off = 2B."""
    B, T, world = 100, 3, WORLD_GEO
    u = rng.choice(6, size=B)                                             # hot users: rows that cross stretch edges
    items = rng.integers(0, 64, size=2 * B)
    i2e = np.where(np.arange(64) % 5 == 0, -1, (np.arange(64) * 7) % 64)
    ids = np.concatenate([u, items, i2e[items]]).astype(np.int64)
    ent_off = np.asarray([0, B, 3 * B, 5 * B], np.int64)
    tab = R.tables_of(5 * B, 5 * B, ent_off)
    inverse = np.where(ids >= 0, ids * T + tab, T * world)
    return _finish(d, 'ktup', opt, pitched, rng, ids, ent_off, T, world, inverse, 3 * B, 2 * B, (1, 2))


def _finish(d, name, opt, pitched, rng, ids, ent_off, T, world, inverse, n_src, src_off, pair):
    n = len(ids)
    n_src = n if n_src == 0 else n_src
    W = T * world
    ld = d + 4 if pitched else d
    G = np.full((n_src, ld), np.nan, np.float32)
    G[:, :d] = (rng.standard_normal((n_src, d)) * rng.uniform(0.2, 3.0, size=(n_src, 1))).astype(np.float32)
    src = R.source_rows(n, n_src, src_off)
    read = np.zeros(n_src, bool)
    read[src[ids >= 0]] = True
    G[~read, :d] = np.nan                                                 # a padding entry's row is never read
    order = np.argsort(inverse, kind='stable')
    m = int((ids >= 0).sum())
    return {'d': d, 'name': name, 'opt': opt, 'T': T, 'world': world, 'cap': [1] * T, 'W': W, 'ids': ids, 'ent_off': ent_off, 'n': n,
            'inverse': inverse, 'skey': inverse[order][:m].astype(np.int32), 'm': m, 'G': G, 'ld': ld, 'n_src': n_src,
            'src_off': src_off, 'pair': pair}


def dup_only_G(c):
    """G with NaN also in the rows of entries that are alone on their wire row (dup_only never reads them)."""
    G = c['G'].copy()
    cnt = np.bincount(c['inverse'][c['ids'] >= 0], minlength=c['W'] + 1)
    src = R.source_rows(c['n'], c['n_src'], c['src_off'])
    shared = np.zeros(c['n_src'], bool)
    on = np.nonzero(c['ids'] >= 0)[0]
    shared[src[on[cnt[c['inverse'][on]] >= 2]]] = True
    G[~shared, :c['d']] = np.nan
    return G


def small_grads(c, n_small, rows=3):
    rng = np.random.default_rng(seed_of('small', c['d'], c['name'], n_small))
    return [(0.5 * rng.standard_normal((rows, c['d']))).astype(np.float32) for _ in range(n_small)]


# ------------------------------------------------------------------------------------------------ apply
KINDS = {'sgd': (R.SGD, 0, 0.0), 'adagrad': (R.ADAGRAD, 0, 0.0), 'adam': (R.ADAM, 0, 0.0), 'adam_wd': (R.ADAM, 0, 1e-2),
         'adagrad_wd': (R.ADAM, 1, 1e-2), 'sgd_wd': (R.ADAM, 2, 1e-2)}
SENTINEL = np.float32(-7.25)


def apply_case(rc, kind, clip='clip', skip=None, n_small=2, second=True, g64=False, slots=1, boundary=(), n_loss=3, stale=False):
    """Tables, states, owner-side ids and the step's scalars for a reduce case.  ids: distinct local rows per table, -1 on one LISTED
    (boundary) row -- its sum must still leave gwire --, on two rows with entries that the walk finishes in registers and on a few
    rows without entries.  Adam states carry last = t - 1 on every row (as the catch-up launch of a step leaves the rows it touches)
    except where `stale` asks for older stamps: those rows owe the steps last + 1 .. t - 1 to the apply launch itself."""
    d, T, W = rc['d'], rc['T'], rc['W']
    rng = np.random.default_rng(seed_of('apply', d, rc['name'], kind, clip, skip, n_small, second, g64))
    k, rule, wd = KINDS[kind]
    pitched = rc['ld'] > d
    n_rows, t = rc['world'] + 6, (537 if stale else 37)
    sp = R.adam_pitch(d) if k == R.ADAM else d
    c = {'kind': k, 'rule': rule, 'wd': wd, 'lr': 0.05, 'eps': 1e-6, 'beta1': 0.9, 'beta2': 0.999, 't': t, 'replay': 110, 'd': d, 'T': T,
         'cap': rc['cap'], 'n_blocks': rc['world'], 'n_loss': n_loss, 'skipped': 5, 'slots': slots,
         'skip_count': 1 if skip == 'count' else 0, 'skip_value': 2.5 if skip == 'value' else 0.0}
    c['tables'], c['states'] = [], ([] if k != R.SGD else None)
    ids = np.full(W, -1, np.int64)
    for tt in range(T):
        P = np.full((n_rows, d + 4 if pitched else d), np.nan, np.float32)
        P[:, :d] = rng.standard_normal((n_rows, d)).astype(np.float32)
        c['tables'].append(P)
        ids[tt::T] = rng.permutation(n_rows)[:rc['world']]
        if k != R.SGD:
            c['states'].append(_state(rng, n_rows, d, sp, k == R.ADAM, t, pitched))
    cnt = np.bincount(rc['inverse'][rc['ids'] >= 0], minlength=W + 1)[:W]
    listed = set(int(b) for b in boundary)
    inner = [int(w) for w in np.nonzero(cnt > 0)[0] if int(w) not in listed]       # rows the walk finishes in registers
    drop = sorted(listed)[:1] + inner[len(inner) // 2:len(inner) // 2 + 2] + [int(x) for x in np.nonzero(cnt == 0)[0][:3]]
    ids[drop] = -1
    c['ids'] = ids
    if stale and k == R.ADAM:                                         # touched rows (and two others, which must rest) with older stamps
        for tt in range(T):
            rows = [int(ids[w]) for w in np.nonzero(cnt > 0)[0] if w % T == tt and ids[w] >= 0][:6]
            rows += [int(x) for x in np.setdiff1d(np.arange(n_rows), ids[tt::T])[:2]]
            stamp = c['states'][tt][:, 2 * d].view(np.int32).copy()
            stamp[rows] = t - 1 - np.asarray([1, 3, 6] * 3)[:len(rows)]
            c['states'][tt][:, 2 * d] = stamp.view(np.float32)
    c['smalls'] = []
    for g in small_grads(rc, n_small):
        sm = {'g': g, 'g64': None, 'p0': rng.standard_normal(g.shape).astype(np.float32), 's0': None, 'p1': None, 's1': None}
        if g64:                                                       # the all-reduced bucket: fp32-representable doubles, NOT sm['g']
            sm['g64'] = (2.0 * g).astype(np.float64)
        if second:
            sm['p1'] = rng.standard_normal(g.shape).astype(np.float32)
        if k != R.SGD:
            sm['s0'] = _state(rng, g.shape[0], d, sp, k == R.ADAM, t, False)
            if second:
                sm['s1'] = _state(rng, g.shape[0], d, sp, k == R.ADAM, t, False)
        c['smalls'].append(sm)
    c['loss_step'] = rng.standard_normal(max(n_loss, 1)).astype(np.float32)[:n_loss]
    c['loss_sum'] = (10 * rng.standard_normal(max(n_loss, 1))).astype(np.float32)[:n_loss]
    c['clip'] = clip
    return c


def _state(rng, n_rows, d, pitch, adam, t, pitched):
    S = np.full((n_rows, pitch + (4 if pitched else 0)), SENTINEL, np.float32)
    if adam:
        S[:, :d] = (0.3 * rng.standard_normal((n_rows, d))).astype(np.float32)
        S[:, d:2 * d] = (0.05 + rng.uniform(0.0, 2.0, size=(n_rows, d))).astype(np.float32)
        S[:, 2 * d] = np.full(n_rows, t - 1, np.int32).view(np.float32)
    else:
        S[:, :d] = (0.05 + rng.uniform(0.0, 2.0, size=(n_rows, d))).astype(np.float32)
    return S


def max_norm_of(clip, sumsq):
    """'clip': coef = 0.5; 'unit': far above the norm (coef exactly 1); 'off': no clipping.  | norm / max_norm - 1 | >= 0.5 either
    way: no rounding of the norm moves the branch of min(1, .)."""
    norm = float(np.sqrt(sumsq))
    return float(np.float32({'clip': 0.5 * norm, 'unit': 1000.0 * norm, 'off': 0.0, 'negative': -1.0}[clip]))     # (the ABI takes a float)


# ------------------------------------------------------------------------------------------------ route
def _route(ids_per_table, pads, world, cap, rng, blocks=1, pair=None):
    seg = [np.concatenate([np.asarray(s, np.int64), np.full(p, -1, np.int64)]) for s, p in zip(ids_per_table, pads)]
    seg = [rng.permutation(s) for s in seg]
    ent_off = np.concatenate([[0], np.cumsum([len(s) for s in seg])]).astype(np.int64)
    ids = np.concatenate(seg) if seg else np.zeros(0, np.int64)
    return {'ids': ids.astype(np.int64), 'block': int(ent_off[-1]), 'ent_off': ent_off, 'world': world, 'cap': list(cap), 'pair': pair}


def route_case(name):
    rng = np.random.default_rng(seed_of('route', name))
    kind = name[0]
    if kind == 'grid':                                                # T in 1 .. 4, world in {1, 2, 3, 64}
        _, T, world = name
        per = [rng.integers(0, 300, size=int(rng.integers(40, 200))) for _ in range(T)]
        cap = [int(np.bincount(np.unique(s) % world, minlength=world).max()) + 3 for s in per]      # distinct ids per owner, + 3 spare
        return _route(per, [int(rng.integers(0, 9)) for _ in range(T)], world, cap, rng)
    if kind == 'owner':                                               # the owner side: world = 1, block = capsum, the same row asked by many peers
        T, peers, wcap = 3, 7, [5, 9, 4]
        blocks = []
        for _ in range(peers):
            for t in range(T):
                k = int(rng.integers(0, wcap[t] + 1))
                blocks.append(np.concatenate([rng.choice(12, size=k, replace=False), np.full(wcap[t] - k, -1)]).astype(np.int64))
        ids = np.concatenate(blocks)
        return {'ids': ids, 'block': sum(wcap), 'ent_off': np.asarray([0, 5, 14, 18], np.int64), 'world': 1, 'cap': [12, 12, 12], 'pair': None}
    if kind == 'heavy':                                               # 10 distinct ids over 5,000 entries
        return _route([rng.choice(rng.choice(10 ** 6, size=10, replace=False), size=5000)], [0], 3, [10], rng)
    if kind == 'distinct':
        return _route([rng.permutation(3000)[:1500], rng.permutation(3000)[:700]], [3, 0], 2, [800, 400], rng)
    if kind == 'all_padding':
        return _route([[], []], [300, 212], 3, [4, 4], rng)
    if kind == 'one_entry':
        return _route([[41]], [0], 2, [1], rng)
    if kind == 'same_id_two_tables':
        return _route([[5, 5, 9], [5, 9, 9, 5]], [1, 0], 2, [2, 2], rng)
    if kind == 'big_ids':                                             # ids near 2^40
        base = (1 << 40) - 50
        return _route([base + rng.integers(0, 100, size=600), base + rng.integers(0, 100, size=300)], [5, 5], 3, [40, 40], rng)
    if kind == 'exact_fit':                                           # distinct == cap in every (owner, table)
        return _route([np.repeat(np.arange(3 * 17), 3), np.repeat(np.arange(3 * 5), 2)], [2, 2], 3, [17, 5], rng)
    if kind == 'overflow':                                            # ('overflow', surplus)
        surplus = name[1]
        return _route([np.repeat(np.arange(2 * (9 + surplus)), 2), np.arange(10)], [3, 0], 2, [9, 8], rng)
    if kind == 'pair':                                                # pair_map: items (table 1) -> entities (table 2)
        items = rng.integers(0, 90, size=400)
        i2e = np.where(np.arange(90) % 4 == 0, -1, (np.arange(90) * 11) % 70)
        ids = np.concatenate([rng.integers(0, 50, size=200), items, i2e[items]]).astype(np.int64)
        return {'ids': ids, 'block': 1000, 'ent_off': np.asarray([0, 200, 600, 1000], np.int64), 'world': 3, 'cap': [30, 40, 40],
                'pair': (1, 2)}
    if kind == 'scan':                                                # ('scan', world, cap): W = world x cap picks the scan path
        _, world, cap = name
        n = min(4096, max(1, world * cap))
        distinct = rng.choice(min(world * cap, 1 << 20), size=min(n, world * cap, 2500), replace=False) if world * cap > 3 else np.arange(world * cap)
        ids = rng.choice(distinct, size=n)
        return _route([ids], [0 if world * cap <= 3 else 37], world, [cap], rng)
    raise KeyError(name)


# W = 1, 3, 1023, 1024, 1025, 4 x 1024 + 2 (tile tail, W % 4 != 0); 262,145 (two tile totals per thread); 1,048,580 (seg_scan_wide)
SCAN = [('scan', 1, 1), ('scan', 3, 1), ('scan', 3, 341), ('scan', 64, 16), ('scan', 25, 41), ('scan', 2, 2049), ('scan', 5, 52429),
        ('scan', 20, 52429)]
ROUTES = ([('grid', T, world) for T in (1, 2, 3, 4) for world in (1, 2, 3, 64)] +
          [('owner',), ('heavy',), ('distinct',), ('all_padding',), ('one_entry',), ('same_id_two_tables',), ('big_ids',), ('exact_fit',),
           ('pair',)])
OVERFLOW = [('overflow', 1), ('overflow', 23)]


def ktup_batches(B=48, n_batches=3, with_ent=True):
    rng = np.random.default_rng(seed_of('ktup_batches', B, n_batches, with_ent))
    n_items, ent_pad = 120, 77
    i2e = ((np.arange(n_items) * 13) % 90).astype(np.int32)
    i2e[::6] = -1
    i2e[1::9] = ent_pad
    return {'u': rng.integers(0, 70, size=(n_batches, B)).astype(np.int64), 'pos': rng.integers(0, n_items, size=(n_batches, B)).astype(np.int64),
            'neg': rng.integers(0, n_items, size=(n_batches, B)).astype(np.int64), 'item2ent': i2e if with_ent else None, 'ent_pad': ent_pad,
            'B': B, 'n_batches': n_batches, 'world': 3, 'cap': [40, 60, 60] if with_ent else [40, 60]}


def kg_batches(B=40, n_batches=2):
    rng = np.random.default_rng(seed_of('kg_batches', B, n_batches))
    ph, pt = (rng.integers(0, 150, size=(n_batches, B)).astype(np.int64) for _ in range(2))
    head = rng.random((n_batches, B)) < 0.5                              # a corrupted triple keeps its head or its tail
    nh = np.where(head, rng.integers(0, 150, size=(n_batches, B)), ph).astype(np.int64)
    nt = np.where(head, pt, rng.integers(0, 150, size=(n_batches, B))).astype(np.int64)
    pr, nr = (rng.integers(0, 11, size=(n_batches, B)).astype(np.int64) for _ in range(2))
    return {'ph': ph, 'pt': pt, 'pr': pr, 'nh': nh, 'nt': nt, 'nr': nr, 'B': B, 'n_batches': n_batches, 'world': 2, 'cap': [90]}


# ------------------------------------------------------------------------------------------------ Adam catch-up
CATCHUP_GAPS = (3, 20)                                # a short replay (step by step) and one of the series form (>= 8 steps, old states)


def catchup_case(gap, n=64, d=100, rule=0, wd=0.0):
    """Rows whose states were written 1 .. 59 steps after step 2000 (old: the bias corrections move slowly), some never (last = 0:
    they rest) and some already at the step the catch-up runs to (they must come back bit-identical).  Under weight decay (wd > 0,
    rule 0 Adam / 1 Adagrad / 2 SGD) every row owes its steps on wd * p; the never-written rows are then stamped t - 2 instead, so that
    no row owes two thousand steps."""
    rng = np.random.default_rng(seed_of('catchup', gap, n, d))
    b1, b2 = float(np.float32(0.9)), float(np.float32(0.999))
    p = rng.standard_normal((n, d)).astype(np.float32)
    m = (1e-2 * rng.standard_normal((n, d))).astype(np.float32)
    v = ((m.astype(np.float64) ** 2) * (0.2 + 3 * rng.random((n, d))) + 1e-12).astype(np.float32)
    last = (2000 + rng.integers(1, 60, size=n)).astype(np.int32)
    t = int(last.max()) + gap
    last[::9] = 0
    last[4::11] = t
    m[last == 0] = 0
    v[last == 0] = 0
    if wd > 0.0:
        last[last == 0] = t - 2
    S = np.full((n, R.adam_pitch(d)), SENTINEL, np.float32)
    S[:, :d], S[:, d:2 * d] = m, v
    S[:, 2 * d] = last.view(np.float32)
    return {'p': p, 'S': S, 'last': last, 't': t, 'd': d, 'n': n, 'lr': float(np.float32(0.01)), 'eps': float(np.float32(1e-8)), 'beta1': b1, 'beta2': b2,
            'replay': 110, 'rule': rule, 'wd': float(np.float32(wd))}
