"""Host model of the device negative samplers (K19), written from their contract in include/ktup_hip.h -- not from the kernels.

Draw t of row b is the word at position offset + b * 4096 + t of the samplers' Philox stream (tests/philox_host.py, SAMPLER_TAG),
mapped to [0, n) by (x * n) >> 32.

rec  row b tries draws 0 .. 4095 and takes the first item that is not its positive and not rated by its user; failing that it scans
     the items from draw 4095 upwards, wrapping; failing that too it takes the stand-in pos + 1 (0 past the end) and counts a failure.
     unique_in_batch: the tries are rounds -- in round t every open row proposes its draw t (if admissible); an item owned since an
     earlier round stays with its owner, and among the proposers of one round the lowest row wins it.  Rows still open after round
     4095 are served in row order by the same scan, over items that are admissible AND unowned; then the stand-in and a failure.
kg   the coin is the top bit of draw 0 (set: the head is corrupted); the entity comes from draws 1 .. 4095, first one that differs
     from the original and does not make a known triple; then the scan from the last draw; then the stand-in orig + 1, and a failure.
feed the batch is rows [cursor, cursor + B) of the columns, the negatives those of (seed, offset); cursor += B, offset += B * 4096.

Every function returns (ids..., fail_count); a dict passed as `stats` receives 'scan_rows', the rows that ran out of tries (those
the scan served are scan_rows - fail_count).  Vectorised over rows; the tries are taken in slabs so that only open rows cost work."""
import numpy as np

from tests.philox_host import SAMPLER_TAG, words_at

TRIES = 4096
_SLABS = (0, 2, 16, 128, 1024, TRIES)


def bounded(w, n):
    return ((np.asarray(w, dtype=np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def raw_draws(seed, offset, rows, t0, t1):
    """uint32 words of draws t0 .. t1 - 1 of the given rows: (len(rows), t1 - t0)."""
    rows = np.asarray(rows, dtype=np.uint64)
    base = np.uint64(int(offset) & (2 ** 64 - 1)) + rows * np.uint64(TRIES)
    return words_at(seed, base[:, None] + np.arange(t0, t1, dtype=np.uint64)[None, :], SAMPLER_TAG)


def draws(seed, offset, rows, t0, t1, n):
    return bounded(raw_draws(seed, offset, rows, t0, t1), n)


def _rated(bitmap, users, items):
    """bitmap: (n_users, words) uint32 or None; users (k,) against items (k, m) or (k,)."""
    if bitmap is None:
        return np.zeros(np.shape(items), dtype=bool)
    u = users[:, None] if np.ndim(items) == 2 else users
    return ((bitmap[u, items >> 5] >> (items & 31).astype(np.uint32)) & np.uint32(1)).astype(bool)


def _first_true(ok):
    """index of the first True per row, -1 if none."""
    idx = ok.argmax(axis=1)
    return np.where(ok[np.arange(ok.shape[0]), idx], idx, -1)


def _scan_order(start, n):
    return (start[:, None] + np.arange(n, dtype=np.int64)[None, :]) % n


def rec(seed, offset, u, pos, n_items, bitmap=None, unique=False, stats=None):
    u, pos = np.asarray(u, dtype=np.int64), np.asarray(pos, dtype=np.int64)
    stats = {} if stats is None else stats
    if unique:
        return _rec_unique(seed, offset, u, pos, n_items, bitmap, stats)
    n = u.size
    neg = np.full(n, -1, dtype=np.int64)
    for t0, t1 in zip(_SLABS[:-1], _SLABS[1:]):
        rows = np.flatnonzero(neg < 0)
        if rows.size == 0:
            break
        c = draws(seed, offset, rows, t0, t1, n_items)
        ok = (c != pos[rows, None]) & ~_rated(bitmap, u[rows], c)
        k = _first_true(ok)
        hit = k >= 0
        neg[rows[hit]] = c[hit, k[hit]]
    fail = 0
    rows = np.flatnonzero(neg < 0)
    stats['scan_rows'] = int(rows.size)
    if rows.size:
        c = _scan_order(draws(seed, offset, rows, TRIES - 1, TRIES, n_items)[:, 0], n_items)
        ok = (c != pos[rows, None]) & ~_rated(bitmap, u[rows], c)
        k = _first_true(ok)
        hit = k >= 0
        neg[rows[hit]] = c[hit, k[hit]]
        lost = rows[~hit]
        neg[lost] = np.where(pos[lost] + 1 < n_items, pos[lost] + 1, 0)
        fail = int(lost.size)
    return neg, fail


def _rec_unique(seed, offset, u, pos, n_items, bitmap, stats):
    n = u.size
    neg = np.full(n, -1, dtype=np.int64)
    owned = np.zeros(n_items, dtype=bool)
    SLAB = 64
    for t0 in range(0, TRIES, SLAB):
        rows = np.flatnonzero(neg < 0)                    # ascending: the first proposer of an item in a round is its lowest row
        if rows.size == 0:
            break
        c_all = draws(seed, offset, rows, t0, t0 + SLAB, n_items)
        ok_all = (c_all != pos[rows, None]) & ~_rated(bitmap, u[rows], c_all)
        live = np.ones(rows.size, dtype=bool)
        for k in range(SLAB):
            idx = np.flatnonzero(live & ok_all[:, k])
            if idx.size:
                c = c_all[idx, k]
                free = ~owned[c]
                idx, c = idx[free], c[free]
                items, first = np.unique(c, return_index=True)
                win = idx[first]
                neg[rows[win]] = items
                owned[items] = True
                live[win] = False
            if not live.any():
                break
    fail = 0
    rows = np.flatnonzero(neg < 0)
    stats['scan_rows'] = int(rows.size)
    if rows.size:
        start = draws(seed, offset, rows, TRIES - 1, TRIES, n_items)[:, 0]
        for b, s0 in zip(rows.tolist(), start.tolist()):  # in row order: a row's pick is taken from the rows after it
            c = (s0 + np.arange(n_items, dtype=np.int64)) % n_items
            ok = (c != pos[b]) & ~owned[c]
            if bitmap is not None:
                ok &= ~_rated(bitmap, np.full(n_items, u[b], dtype=np.int64), c)
            k = np.flatnonzero(ok)
            if k.size:
                neg[b] = c[k[0]]
                owned[neg[b]] = True
            else:
                neg[b] = pos[b] + 1 if pos[b] + 1 < n_items else 0
                fail += 1
    return neg, fail


def triple_keys(h, r, t, n_ent, n_rel):
    h, r, t = (np.asarray(x).astype(np.uint64) for x in (h, r, t))
    return (h * np.uint64(n_rel) + r) * np.uint64(n_ent) + t


def _known(keys, k):
    if keys is None:
        return np.zeros(k.shape, dtype=bool)
    if keys.size == 0:
        return np.zeros(k.shape, dtype=bool)
    i = np.searchsorted(keys, k)
    return keys[np.minimum(i, keys.size - 1)] == k


def coin(seed, offset, rows):
    """True where the HEAD is corrupted: the top bit of draw 0."""
    return (raw_draws(seed, offset, rows, 0, 1)[:, 0] >> np.uint32(31)).astype(bool)


def kg(seed, offset, h, t, r, n_ent, n_rel, keys=None, stats=None):
    """keys: ascending uint64 keys of the known triples, or None for no filter -> (neg_h, neg_t, fail)."""
    h, t, r = (np.asarray(x, dtype=np.int64) for x in (h, t, r))
    n = h.size
    head = coin(seed, offset, np.arange(n))
    orig = np.where(head, h, t)
    pick = np.full(n, -1, dtype=np.int64)

    def admissible(rows, c):                                                # c: (len(rows), m)
        hh, tt, rr = (np.broadcast_to(x[rows, None], c.shape) for x in (h, t, r))
        hd = np.broadcast_to(head[rows, None], c.shape)
        k = triple_keys(np.where(hd, c, hh), rr, np.where(hd, tt, c), n_ent, n_rel)
        return (c != orig[rows, None]) & ~_known(keys, k)

    for t0, t1 in zip((1,) + _SLABS[1:-1], _SLABS[1:]):
        rows = np.flatnonzero(pick < 0)
        if rows.size == 0:
            break
        c = draws(seed, offset, rows, t0, t1, n_ent)
        k = _first_true(admissible(rows, c))
        hit = k >= 0
        pick[rows[hit]] = c[hit, k[hit]]
    fail = 0
    rows = np.flatnonzero(pick < 0)
    if stats is not None:
        stats['scan_rows'] = int(rows.size)
    if rows.size:
        c = _scan_order(draws(seed, offset, rows, TRIES - 1, TRIES, n_ent)[:, 0], n_ent)
        k = _first_true(admissible(rows, c))
        hit = k >= 0
        pick[rows[hit]] = c[hit, k[hit]]
        lost = rows[~hit]
        pick[lost] = np.where(orig[lost] + 1 < n_ent, orig[lost] + 1, 0)
        fail = int(lost.size)
    return np.where(head, pick, h), np.where(head, t, pick), fail


def feed_rec(seed, offset, cursor, col_u, col_i, B, n_items, bitmap=None, unique=False):
    """-> (u2, i2, cursor', offset', fail)"""
    u, pos = np.asarray(col_u)[cursor:cursor + B], np.asarray(col_i)[cursor:cursor + B]
    neg, fail = rec(seed, offset, u, pos, n_items, bitmap, unique)
    return np.concatenate([u, u]), np.concatenate([pos, neg]), cursor + B, offset + B * TRIES, fail


def feed_kg(seed, offset, cursor, col_h, col_t, col_r, B, n_ent, n_rel, keys=None):
    """-> (h2, t2, r2, cursor', offset', fail)"""
    h, t, r = (np.asarray(x)[cursor:cursor + B] for x in (col_h, col_t, col_r))
    nh, nt, fail = kg(seed, offset, h, t, r, n_ent, n_rel, keys)
    return np.concatenate([h, nh]), np.concatenate([t, nt]), np.concatenate([r, r]), cursor + B, offset + B * TRIES, fail
