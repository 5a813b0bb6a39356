"""The negative samplers and feed launches (csrc/ktup_sample.hip) against a host model, id for id.

Given (seed, offset) and their inputs the kernels are deterministic integer functions, and include/ktup_hip.h says which: draw t of
row b is position offset + b * 4096 + t of the samplers' Philox stream, then the scan, then the stand-in and a failure count.
tests/sampler_host.py writes that contract down in numpy; here every id and the failure counter must equal the model's -- over the
LDS and the global-memory uniqueness paths, the scan and fail paths of both samplers, the wide coarse index of ktup_feed_kg, and
offsets whose Philox block index carries into the second counter word.

The CPU tests check the model itself: its outputs keep the constraints, and its draws are uniform by a chi-square over 3,240 bins
(mean 3,239, sd = sqrt(2 * 3239) = 80.5, accepted within 5 sd) -- for the rec draw and for the kg entity draw on each side of the
coin, which a stand-in that never returns the last id, or an entity drawn from the coin's own word, would fail."""
import numpy as np
import pytest
import torch

from tests import sampler_host as SH

DEV = 'cuda'
KG_STREAM = 1 << 62
OFFSETS = [777, 2 ** 34 - 3 * 4096, 2 ** 40 + 12345, KG_STREAM]
gpu = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ inputs
def _bitmap(n_users, n_items, rated):
    bits = np.zeros((n_users, (n_items + 31) // 32), dtype=np.uint32)
    for u, items in rated.items():
        for i in items:
            bits[u, i >> 5] |= np.uint32(1 << (i & 31))
    return bits


def _rec_world(seed, n, n_users, n_items, n_rated):
    """Random users with n_rated items each; rows (u, pos) with pos rated by u."""
    rng = np.random.RandomState(seed)
    rated = {u: set(rng.choice(n_items, size=n_rated, replace=False).tolist()) for u in range(n_users)}
    u = rng.randint(0, n_users, size=n)
    pos = np.array([sorted(rated[int(x)])[rng.randint(n_rated)] for x in u], dtype=np.int64)
    return rated, u.astype(np.int64), pos


def _lone_item_users(rated, u, pos, n_users, n_items, k=12):
    """k more users (ids n_users ..) who rated everything but one item each, a different one per user, with one row each: 4096 tries
    miss a lone item among 5,000 with probability 0.44, and then the scan has to find it."""
    lone = [311 * j + 13 for j in range(k)]
    for user in range(n_users):
        rated[user] = set(rated.get(user, ())) | set(lone)                   # nobody else may take a lone item (batch-unique mode)
    for j in range(k):
        rated[n_users + j] = set(range(n_items)) - {lone[j]}
    return rated, np.concatenate([u, n_users + np.arange(k)]), np.concatenate([pos, np.arange(k) * 3]), n_users + k


def _nearly_full_world():
    """70 items (3 bitmap words): user 0 rated all but item 41, user 1 everything, users 2 .. 9 thirty items each; rows of user 1
    with pos = 69 take the stand-in that wraps to 0."""
    n, nu, ni = 700, 10, 70
    rated, u, pos = _rec_world(5, n, nu, ni, 30)
    rated[0] = set(range(ni)) - {41}
    rated[1] = set(range(ni))
    rng = np.random.RandomState(6)
    pos[u == 0] = rng.choice(sorted(rated[0]), size=int((u == 0).sum()))
    pos[u == 1] = rng.randint(0, ni, size=int((u == 1).sum()))
    pos[np.flatnonzero(u == 1)[:5]] = ni - 1
    return n, nu, ni, rated, u, pos


def _kg_world(seed, n_ent, n_rel, n_known, n):
    rng = np.random.RandomState(seed)
    total = n_ent * n_ent * n_rel
    keys = np.sort(rng.choice(total, size=n_known, replace=False)).astype(np.uint64)
    rows = rng.choice(n_known, size=n)                                        # the batch: known triples, as in training
    k = keys[rows].astype(np.int64)
    t, hr = k % n_ent, k // n_ent
    return keys, hr // n_rel, t, hr % n_rel                                   # keys, h, t, r


def _triples(keys, n_ent, n_rel):
    k = keys.astype(np.int64)
    return [(int(a), int(b), int(c)) for a, b, c in zip(k // n_ent // n_rel, k % n_ent, k // n_ent % n_rel)]   # (h, t, r)


# ------------------------------------------------------------------------------------------------ CPU: the model itself
def _chi_square(ids, bins):
    counts = np.bincount(ids, minlength=bins).astype(np.float64)
    assert counts.size == bins
    e = ids.size / float(bins)
    return float(((counts - e) ** 2 / e).sum())


CHI_LO, CHI_HI = 3239 - 5 * (2 * 3239) ** 0.5, 3239 + 5 * (2 * 3239) ** 0.5


def test_model_keeps_the_constraints():
    for unique in (False, True):
        rated, u, pos = _rec_world(1, 300, 20, 400, 60)
        bits = _bitmap(20, 400, rated)
        neg, fail = SH.rec(11, 4242, u, pos, 400, bits, unique)
        assert fail == 0 and neg.min() >= 0 and neg.max() < 400
        assert all(g != p and g not in rated[int(x)] for x, p, g in zip(u, pos, neg))
        assert not unique or len(set(neg.tolist())) == neg.size
    # more rows than admissible items: each admissible item once, the other rows get the stand-in and are counted
    bits = _bitmap(2, 40, {0: set(range(30))})
    neg, fail = SH.rec(1, 0, np.zeros(64, np.int64), np.zeros(64, np.int64), 40, bits, True)
    assert fail == 54 and sorted(neg[neg >= 30].tolist()) == list(range(30, 40)) and (neg[neg < 30] == 1).all()
    # a user who rated everything but one item: the scan finds it; one who rated everything: stand-in, wrapping at the end
    bits = _bitmap(2, 70, {0: set(range(70)) - {41}, 1: set(range(70))})
    neg, fail = SH.rec(2, 9, np.array([0, 0, 1, 1]), np.array([3, 69, 3, 69]), 70, bits, False)
    assert neg.tolist() == [41, 41, 4, 0] and fail == 2
    keys, h, t, r = _kg_world(3, 50, 4, 3000, 500)
    known = set(keys.tolist())
    nh, nt, fail = SH.kg(9, KG_STREAM, h, t, r, 50, 4, keys)
    assert fail == 0 and ((nh != h) != (nt != t)).all()
    assert all(int(k) not in known for k in SH.triple_keys(nh, r, nt, 50, 4))
    # everything known: no admissible entity -> orig + 1, wrapping
    allk = np.arange(6 * 6 * 2, dtype=np.uint64)
    nh, nt, fail = SH.kg(9, 0, np.array([5, 2]), np.array([5, 3]), np.array([1, 0]), 6, 2, allk)
    assert fail == 2 and [(int(a), int(b)) for a, b in zip(nh, nt)] in ([(0, 5), (3, 3)], [(0, 5), (2, 4)], [(5, 0), (3, 3)], [(5, 0), (2, 4)])


def test_model_rec_draws_are_uniform():
    rng = np.random.RandomState(0)
    n, ni = 400000, 3240
    neg, fail = SH.rec(0x1234abcd, 2 ** 34 - 4096 * 1000, np.zeros(n, np.int64), rng.randint(0, ni, size=n), ni, None, False)
    chi = _chi_square(neg, ni)
    assert fail == 0 and CHI_LO < chi < CHI_HI, chi


def test_model_kg_entity_draws_are_uniform_on_each_coin_side():
    rng = np.random.RandomState(1)
    n, ne = 820000, 3240                                                     # each side keeps its first 4e5 draws
    h, t = rng.randint(0, ne, size=n), rng.randint(0, ne, size=n)
    nh, nt, fail = SH.kg(0x5eed, KG_STREAM, h, t, np.zeros(n, np.int64), ne, 1, None)
    head = nh != h
    assert fail == 0 and ((nt != t) != head).all() and 0.495 < head.mean() < 0.505     # 5 sd of a fair coin over 8e5 rows is 0.0028
    for side, ids in ((True, nh[head]), (False, nt[~head])):
        ids = ids[:400000]
        assert ids.size == 400000
        chi = _chi_square(ids, ne)
        assert CHI_LO < chi < CHI_HI, (side, chi)


# ------------------------------------------------------------------------------------------------ GPU
def dv(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _sampler(seed, n_users=0, n_items=0, rated=None, with_bitmap=True, kg=None):
    from jTransUP.utils.device_sampler import DeviceSampler
    s = DeviceSampler(DEV, seed=seed)
    if n_items:
        s.set_rating_dicts(n_users, n_items, [rated] if with_bitmap else None)
        if with_bitmap:                                                       # the bitmap the model reads is built here, not by the sampler
            assert np.array_equal(s.bitmap.cpu().numpy().view(np.uint32), _bitmap(n_users, n_items, rated))
    if kg is not None:
        n_ent, n_rel, keys = kg
        s.set_triples(n_ent, n_rel, None if keys is None else [_triples(keys, n_ent, n_rel)])
        if keys is not None:
            assert np.array_equal(s.keys.cpu().numpy().view(np.uint64), keys)
    return s


def _fails(s):
    n = int(s.fail.item())
    s.fail.zero_()
    return n


def _check_rec(s, offset, u, pos, n_items, bits, unique, scan_hits=None):
    s.offsets['rec'] = offset
    got = s.sample_rec(dv(u), dv(pos), unique_in_batch=unique).cpu().numpy()
    got_fail = _fails(s)
    stats = {}
    want, want_fail = SH.rec(s.seed, offset, u, pos, n_items, bits, unique, stats)
    np.testing.assert_array_equal(got, want)
    assert got_fail == want_fail
    assert s.offsets['rec'] == offset + u.size * 4096
    if scan_hits is not None:                                                 # rows that ran out of tries and were served by the scan
        assert stats['scan_rows'] - want_fail >= scan_hits, (stats, want_fail)
    return want_fail


@gpu
@pytest.mark.parametrize('offset', OFFSETS)
def test_rec_sampler_equals_the_model(offset):
    n, nu, ni, rated, u, pos = _nearly_full_world()
    bits = _bitmap(nu, ni, rated)
    assert bits.shape[1] == 3
    fails = _check_rec(_sampler(3, nu, ni, rated), offset, u, pos, ni, bits, False)
    assert fails == int((u == 1).sum())                                       # the user who rated everything
    assert _check_rec(_sampler(3, nu, ni, rated, with_bitmap=False), offset, u, pos, ni, None, False) == 0
    # among 70 items the tries always find the lone admissible one; among 5,000 some rows need the scan
    rated, u, pos = _rec_world(7, 20, 4, 5000, 50)
    rated, u, pos, nu = _lone_item_users(rated, u, pos, 4, 5000)
    assert _check_rec(_sampler(3, nu, 5000, rated), offset, u, pos, 5000, _bitmap(nu, 5000, rated), False, scan_hits=1) == 0


@gpu
@pytest.mark.parametrize('offset', OFFSETS)
def test_unique_rec_sampler_lds_path_equals_the_model(offset):
    # 512 rows over 600 items, 100 of them rated by each user: rows collide for many rounds
    rated, u, pos = _rec_world(2, 512, 30, 600, 100)
    assert _check_rec(_sampler(4, 30, 600, rated), offset, u, pos, 600, _bitmap(30, 600, rated), True) == 0
    # 64 rows, 10 admissible items: exhaustion, the row-order scan and 54 failures
    rated = {0: set(range(30))}
    z = np.zeros(64, np.int64)
    assert _check_rec(_sampler(1, 2, 40, rated), offset, z, z, 40, _bitmap(2, 40, rated), True) == 54
    # 5,000 items, twelve users with one admissible item each: rows whose 4096 rounds miss it are served by the scan, no failure
    rated, u, pos = _rec_world(7, 200, 4, 5000, 50)
    rated, u, pos, nu = _lone_item_users(rated, u, pos, 4, 5000)
    assert _check_rec(_sampler(3, nu, 5000, rated), offset, u, pos, 5000, _bitmap(nu, 5000, rated), True, scan_hits=1) == 0


@gpu
@pytest.mark.parametrize('n,n_items,n_rated', [(1025, 3000, 300), (300, 8001, 500), (1100, 1050, 0)])
def test_unique_rec_sampler_global_path_equals_the_model(n, n_items, n_rated):
    """n > 1024 or n_items > 8000: owner[] in global memory (rec_unique_rounds).  (1100, 1050): more rows than items, so the rounds
    run out and thread 0 serves the rest.  The same batch through ktup_feed_rec, which promises to leave the scratch all-ones."""
    from jTransUP.hip import lib as L
    from jTransUP.hip.ops import _p, _stream
    nu = 25
    rated, u, pos = _rec_world(n, n, nu, n_items, max(n_rated, 1))
    if not n_rated:
        rated = {}
    if n_items == 8001:                                                       # rows the scan serves without a failure
        rated, u, pos, nu = _lone_item_users(rated, u, pos, nu, n_items)
        n = u.size
    bits = _bitmap(nu, n_items, rated)
    s = _sampler(8, nu, n_items, rated)
    offset = 2 ** 34 - 7 * 4096 - 5
    fails = _check_rec(s, offset, u, pos, n_items, bits, True, scan_hits=1 if n_items == 8001 else None)
    assert (fails > 0) == (n > n_items)
    want_u2, want_i2, cur, off, want_fail = SH.feed_rec(s.seed, offset, 3, np.concatenate([[0, 0, 0], u]), np.concatenate([[0, 0, 0], pos]),
                                                         n, n_items, bits, True)
    col_u, col_i = dv(np.concatenate([[0, 0, 0], u])), dv(np.concatenate([[0, 0, 0], pos]))
    cursor, offset_dev = torch.tensor([3], dtype=torch.int64, device=DEV), torch.tensor([offset], dtype=torch.int64, device=DEV)
    u2, i2 = torch.zeros(2 * n, dtype=torch.int64, device=DEV), torch.zeros(2 * n, dtype=torch.int64, device=DEV)
    ws = s.rec_workspace()
    assert bool((ws == -1).all())
    L.call('ktup_feed_rec', _p(col_u), _p(col_i), n + 3, n, _p(cursor), _p(offset_dev), n_items, _p(s.bitmap), s.words, s.seed, 1, _p(u2),
           _p(i2), _p(ws), _p(s.fail), _stream(s.device))
    np.testing.assert_array_equal(u2.cpu().numpy(), want_u2)
    np.testing.assert_array_equal(i2.cpu().numpy(), want_i2)
    assert _fails(s) == want_fail == fails
    assert cursor.tolist() == [cur] and offset_dev.tolist() == [off]
    assert bool((ws == -1).all())


def _check_kg(s, offset, h, t, r, n_ent, n_rel, keys, scan_hits=None):
    s.offsets['kg'] = offset
    nh, nt = s.sample_kg(dv(h), dv(t), dv(r))
    got_fail = _fails(s)
    stats = {}
    want_h, want_t, want_fail = SH.kg(s.seed, offset, h, t, r, n_ent, n_rel, keys, stats)
    np.testing.assert_array_equal(nh.cpu().numpy(), want_h)
    np.testing.assert_array_equal(nt.cpu().numpy(), want_t)
    assert got_fail == want_fail
    if scan_hits is not None:
        assert stats['scan_rows'] - want_fail >= scan_hits, (stats, want_fail)
    return want_fail


@gpu
@pytest.mark.parametrize('offset', OFFSETS)
def test_kg_sampler_equals_the_model(offset):
    keys, h, t, r = _kg_world(1, 500, 7, 22000, 1500)
    assert _check_kg(_sampler(9, kg=(500, 7, keys)), offset, h, t, r, 500, 7, keys) == 0
    assert _check_kg(_sampler(9, kg=(500, 7, None)), offset, h, t, r, 500, 7, None) == 0
    # 6 entities, 2 relations, all but three of the 72 triples known: most rows run out of tries, scan, and many fail -- with
    # originals at the last entity, whose stand-in wraps to 0
    rng = np.random.RandomState(2)
    keys = np.setdiff1d(np.arange(72, dtype=np.uint64), np.array([7, 40, 71], dtype=np.uint64))
    h, t, r = rng.randint(0, 6, size=200), rng.randint(0, 6, size=200), rng.randint(0, 2, size=200)
    h[:20] = 5; t[:20] = 5
    fails = _check_kg(_sampler(9, kg=(6, 2, keys)), offset, h, t, r, 6, 2, keys)
    assert 0 < fails < 200
    # 5,000 entities: head 3 is linked to every tail but 4321 and every head but 1234 to tail 7, so a row (3, 7) has one admissible
    # entity on either side of the coin -- 4096 tries miss it with probability 0.44, and the scan finds it
    ne = 5000
    c = np.arange(ne, dtype=np.uint64)
    keys = np.unique(np.concatenate([SH.triple_keys(3, 0, c[c != 4321], ne, 1), SH.triple_keys(c[c != 1234], 0, 7, ne, 1)]))
    h, t, r = np.full(40, 3), np.full(40, 7), np.zeros(40, np.int64)
    assert _check_kg(_sampler(9, kg=(ne, 1, keys)), offset, h, t, r, ne, 1, keys, scan_hits=1) == 0


@gpu
def test_feed_launches_equal_the_model():
    """ktup_feed_kg with 70,001 of the 72,000 possible triples known: its coarse index holds every 18th key (3,889 entries, a partial
    last block) and nearly every candidate is a known key, so the membership test lands on, below and above coarse entries.  Two
    launches each (B = 32), kg and rec (plain and batch-unique); cursor and counter end where the model says."""
    from jTransUP.hip import lib as L
    from jTransUP.hip.ops import _p, _stream
    B, ne, nr = 32, 120, 5
    rng = np.random.RandomState(3)
    total = ne * ne * nr
    forced = np.array([0, 17, 18, 36000, total - 1])                          # (key 0 unknown: candidates below the smallest key)
    rest = rng.choice(total, size=2100, replace=False)
    unknown = np.concatenate([forced, rest[~np.isin(rest, forced)][:1999 - forced.size]])
    keys = np.setdiff1d(np.arange(total, dtype=np.uint64), unknown.astype(np.uint64))
    assert keys.size == 70001 and -(-keys.size // 4096) == 18
    s = _sampler(21, kg=(ne, nr, keys))
    n_rows = 100
    cols = [rng.randint(0, ne, size=n_rows), rng.randint(0, ne, size=n_rows), rng.randint(0, nr, size=n_rows)]
    dcols = [dv(c) for c in cols]
    i64 = dict(dtype=torch.int64, device=DEV)
    cursor, offset = 5, 2 ** 34 - 40 * 4096
    cur_dev, off_dev = torch.tensor([cursor], **i64), torch.tensor([offset], **i64)
    h2, t2, r2 = (torch.zeros(2 * B, **i64) for _ in range(3))
    for launch in range(2):
        want = SH.feed_kg(s.seed, offset, cursor, cols[0], cols[1], cols[2], B, ne, nr, keys)
        L.call('ktup_feed_kg', _p(dcols[0]), _p(dcols[1]), _p(dcols[2]), n_rows, B, _p(cur_dev), _p(off_dev), ne, nr, _p(s.keys),
               s.keys.numel(), s.seed, _p(h2), _p(t2), _p(r2), _p(s.fail), _stream(s.device))
        for got, w in zip((h2, t2, r2), want[:3]):
            np.testing.assert_array_equal(got.cpu().numpy(), w)
        cursor, offset = want[3], want[4]
        assert cur_dev.tolist() == [cursor] and off_dev.tolist() == [offset] and _fails(s) == want[5]
    assert cursor == 5 + 2 * B and offset == 2 ** 34 - 40 * 4096 + 2 * B * 4096
    # the same batch through ktup_negsample_kg (plain binary search of the key list): the two membership tests agree
    _check_kg(s, 2 ** 34 - 40 * 4096, cols[0][5:5 + B], cols[1][5:5 + B], cols[2][5:5 + B], ne, nr, keys)

    nu, ni = 12, 90
    rated, _, _ = _rec_world(4, 1, nu, ni, 40)
    bits = _bitmap(nu, ni, rated)
    s = _sampler(22, nu, ni, rated)
    col_u, col_i = rng.randint(0, nu, size=n_rows), rng.randint(0, ni, size=n_rows)
    du, di = dv(col_u), dv(col_i)
    u2, i2 = torch.zeros(2 * B, **i64), torch.zeros(2 * B, **i64)
    for unique in (0, 1):
        cursor, offset = 1, 2 ** 40 + 99
        cur_dev, off_dev = torch.tensor([cursor], **i64), torch.tensor([offset], **i64)
        for launch in range(2):
            want = SH.feed_rec(s.seed, offset, cursor, col_u, col_i, B, ni, bits, bool(unique))
            L.call('ktup_feed_rec', _p(du), _p(di), n_rows, B, _p(cur_dev), _p(off_dev), ni, _p(s.bitmap), s.words, s.seed, unique,
                   _p(u2), _p(i2), _p(s.rec_workspace()), _p(s.fail), _stream(s.device))
            np.testing.assert_array_equal(u2.cpu().numpy(), want[0])
            np.testing.assert_array_equal(i2.cpu().numpy(), want[1])
            cursor, offset = want[2], want[3]
            assert cur_dev.tolist() == [cursor] and off_dev.tolist() == [offset] and _fails(s) == want[4] == 0
