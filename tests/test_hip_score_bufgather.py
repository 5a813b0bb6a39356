"""The buffer-load gather of the soft-gate K5-K7 forward (option fwd_buf_gather, ktup_score_pref_mc.hip): the lanes that load a tile's ids
form each row's byte offset once, the row loads are buffer loads at 32-bit offsets, and a tile with a row that ends past byte 2^32 - 1 of
its table falls back, as a whole, to 64-bit pointers.  No floating-point operation changes, so everything here is compared bit for bit
(torch.equal) against fwd_buf_gather = 0, the pointer kernel:
  * d in {64, 100, 128} x P in {3, 20} (fp32 and split stage 2), KTUP and TUP, squared L2 and L1, n in {1, 16, 17, 512, 70,001}: 70,001
    pairs give every wave more than one tile, so the offsets and the tile's flag travel through the prefetch path, with a ragged last
    tile; ~10 % of the items map to the pad row.  n <= 512 is also checked against the CPU oracle at tests/test_hip_score.py's tolerances;
  * the guard: a table that is a pitched view of an uninitialised allocation, 3 rows at a pitch of 2^29 + 4 floats, so row 2 starts past
    4 GB; 48 pairs = three tiles: rows {0, 1} only (fast), rows 1 and 2 mixed (falls back as a whole), row 2 only.  For U, for I, and for
    E through item2ent, one large table at a time; and once with 70,001 pairs, where the flag of a far tile arrives through the prefetch;
  * the edge: 2 rows at a pitch of 2^30 - 16 floats, d = 100: row 1 starts 64 bytes below 4 GB and ends above it (a guard that looked at
    the row's start alone would wrap);
  * an inf / nan row of one pair stays in that pair (the zeroing of the chunks past the row survives the new loads)."""
import numpy as np
import pytest
import torch

from oracle import cpu_ref as O

pytestmark = pytest.mark.gpu
DEV = 'cuda'
RT, AT = 1e-4, 1e-5                      # tests/test_hip_score.py


def close(got, want, rtol=RT, atol=AT):
    np.testing.assert_allclose(got.detach().cpu().numpy(), want.detach().cpu().numpy(), rtol=rtol, atol=atol)


def rand_world(seed, nu, ni, ne, nr, d):
    gen = torch.Generator().manual_seed(seed)
    mk = lambda r: O.make_table(r, d, gen)
    W = dict(U=mk(nu), I=mk(ni), E=torch.cat([mk(ne), torch.zeros(1, d)]), P=mk(nr), Pn=mk(nr), R=mk(nr), Rn=mk(nr))
    i2e = torch.randint(0, ne, (ni,), generator=gen)
    i2e[torch.rand(ni, generator=gen) < 0.1] = ne          # ~10 % of items map to the pad row
    return W, i2e, gen


def scores(D, i2e_d, u, i, l1, buf):
    """(KTUP, TUP) scores with option fwd_buf_gather set to `buf` for the two launches."""
    from jTransUP.hip import lib as L
    from jTransUP.hip import ops
    old = L.set_option('fwd_buf_gather', buf)
    try:
        with torch.no_grad():
            return (ops.score_ktup(D['U'], D['I'], D['E'], D['P'], D['Pn'], D['R'], D['Rn'], i2e_d, u, i, l1).cpu(),
                    ops.score_tup(D['U'], D['I'], D['P'], D['Pn'], u, i, l1).cpu())
    finally:
        L.set_option('fwd_buf_gather', old)


def test_option_is_on_by_default():
    from jTransUP.hip import lib as L
    assert L.get_option('fwd_buf_gather') == 1


@pytest.mark.parametrize('P', [3, 20])
@pytest.mark.parametrize('d', [64, 100, 128])
def test_buffer_gather_same_bits_as_pointer_gather(d, P):
    nu, ni, ne = 700, 400, 900
    W, i2e, gen = rand_world(11 + d + P, nu, ni, ne, P, d)
    D = {k: v.to(DEV) for k, v in W.items()}
    i2e_d = i2e.to(DEV, torch.int32)
    for n in (1, 16, 17, 512, 70001):
        u = torch.randint(0, nu, (n,), generator=gen); i = torch.randint(0, ni, (n,), generator=gen)
        ud, idv = u.to(DEV), i.to(DEV)
        for l1 in (False, True):
            new, old = scores(D, i2e_d, ud, idv, l1, 1), scores(D, i2e_d, ud, idv, l1, 0)
            for k in range(2):
                assert torch.equal(new[k], old[k]), 'fwd_buf_gather changes bits at d = %d, P = %d, n = %d, l1 = %s, %s' % (d, P, n, l1, ('KTUP', 'TUP')[k])
            if n <= 512:
                close(new[0], O.score_ktup_rec(W['U'], W['I'], W['E'], W['P'], W['Pn'], W['R'], W['Rn'], i2e, u, i, l1))
                close(new[1], O.score_tup(W['U'], W['I'], W['P'], W['Pn'], u, i, l1))


def pitched(rows, pitch):
    """`rows` (r x d, CPU) as a view with a row pitch of `pitch` floats of an uninitialised device allocation: only these rows are written."""
    r, d = rows.shape
    t = torch.empty((r - 1) * pitch + d, dtype=torch.float32, device=DEV).as_strided((r, d), (pitch, 1))
    t.copy_(rows.to(DEV))
    return t


def tile_rows(n, lo_hi_by_tile, gen):
    """One row id per pair: tile k (16 pairs) draws from lo_hi_by_tile[k % len]; both ends of a two-row range are present in the tile."""
    out = torch.empty(n, dtype=torch.int64)
    for k in range((n + 15) // 16):
        lo, hi = lo_hi_by_tile[k % len(lo_hi_by_tile)]
        m = min(16, n - 16 * k)
        ids = torch.randint(lo, hi + 1, (m,), generator=gen)
        ids[0] = lo; ids[m - 1] = hi
        out[16 * k:16 * k + m] = ids
    return out


@pytest.mark.parametrize('which', ['U', 'I', 'E'])
@pytest.mark.parametrize('P', [3, 20])
def test_rows_past_4gb_fall_back_per_tile(which, P):
    d, pitch = 100, (1 << 29) + 4                            # row 2 starts at byte 2^32 + 32
    nu, ni, ne = 300, 200, 400
    W, i2e, gen = rand_world(31 + P, nu, ni, ne, P, d)
    plan = [(0, 1), (1, 2), (2, 2)]                          # fast; mixed: falls back as a whole; far only
    D = {k: v.to(DEV) for k, v in W.items() if k != which}
    if which == 'E':
        W['E'] = W['E'][:3].contiguous()
        i2e = torch.arange(ni) % 3
    else:
        W[which] = W[which][:3].contiguous()
    D[which] = pitched(W[which], pitch)
    for n in (48, 70001):                                    # 70,001: a far tile's flag arrives with the prefetched offsets
        rows = tile_rows(n, plan, gen)
        u = rows if which == 'U' else torch.randint(0, nu, (n,), generator=gen)
        if which == 'I':
            i = rows
        elif which == 'E':
            i = rows + 3 * torch.randint(0, ni // 3 - 1, (n,), generator=gen)      # item2ent[i] = i % 3 = the planned entity row
        else:
            i = torch.randint(0, ni, (n,), generator=gen)
        i2e_d, ud, idv = i2e.to(DEV, torch.int32), u.to(DEV), i.to(DEV)
        for l1 in (False, True):
            new, old = scores(D, i2e_d, ud, idv, l1, 1), scores(D, i2e_d, ud, idv, l1, 0)
            for k in range(2):
                assert torch.equal(new[k], old[k]), 'pitched %s, n = %d, l1 = %s, %s' % (which, n, l1, ('KTUP', 'TUP')[k])
            if n == 48:
                close(new[0], O.score_ktup_rec(W['U'], W['I'], W['E'], W['P'], W['Pn'], W['R'], W['Rn'], i2e, u, i, l1))
                close(new[1], O.score_tup(W['U'], W['I'], W['P'], W['Pn'], u, i, l1))
    del D
    torch.cuda.empty_cache()


@pytest.mark.parametrize('which', ['U', 'I', 'E'])
def test_row_that_straddles_4gb_is_not_fast(which):
    d, P, pitch, n = 100, 20, (1 << 30) - 16, 64             # row 1: bytes [2^32 - 64, 2^32 + 336)
    nu, ni, ne = 300, 200, 400
    W, i2e, gen = rand_world(47, nu, ni, ne, P, d)
    D = {k: v.to(DEV) for k, v in W.items() if k != which}
    if which == 'E':
        W['E'] = W['E'][:2].contiguous()
        i2e = torch.arange(ni) % 2
    else:
        W[which] = W[which][:2].contiguous()
    D[which] = pitched(W[which], pitch)
    rows = tile_rows(n, [(0, 0), (0, 1), (1, 1)], gen)
    u = rows if which == 'U' else torch.randint(0, nu, (n,), generator=gen)
    i = rows if which != 'U' else torch.randint(0, ni, (n,), generator=gen)
    if which == 'E':
        i = rows + 2 * torch.randint(0, ni // 2 - 1, (n,), generator=gen)
    i2e_d, ud, idv = i2e.to(DEV, torch.int32), u.to(DEV), i.to(DEV)
    for l1 in (False, True):
        new, old = scores(D, i2e_d, ud, idv, l1, 1), scores(D, i2e_d, ud, idv, l1, 0)
        for k in range(2):
            assert torch.equal(new[k], old[k]), 'straddling row of %s, l1 = %s, %s' % (which, l1, ('KTUP', 'TUP')[k])
        close(new[0], O.score_ktup_rec(W['U'], W['I'], W['E'], W['P'], W['Pn'], W['R'], W['Rn'], i2e, u, i, l1))
        close(new[1], O.score_tup(W['U'], W['I'], W['P'], W['Pn'], u, i, l1))
    del D
    torch.cuda.empty_cache()


@pytest.mark.parametrize('P', [16, 20])
@pytest.mark.parametrize('d', [64, 100, 128])
def test_buffer_gather_keeps_inf_and_nan_inside_their_pair(d, P):
    """The inf / nan test of tests/test_hip_score_split.py with fwd_buf_gather = 1: pair 5 gathers a user row holding inf, pair 37 an item
    row holding nan; every other pair keeps the bits of the clean run, and the two pairs themselves are not finite."""
    nu, ni, ne, n = 300, 200, 400, 100
    W, i2e, gen = rand_world(23 + d + P, nu, ni, ne, P, d)
    u = torch.randint(1, nu, (n,), generator=gen); i = torch.randint(1, ni, (n,), generator=gen)
    u[5] = 0; i[37] = 0
    D = {k: v.to(DEV) for k, v in W.items()}
    i2e_d, ud, idv = i2e.to(DEV, torch.int32), u.to(DEV), i.to(DEV)
    bad = {k: v.clone() for k, v in D.items()}
    bad['U'][0, d // 3] = float('inf')
    bad['I'][0, :] = float('nan')
    keep = torch.ones(n, dtype=torch.bool); keep[5] = False; keep[37] = False
    for l1 in (False, True):
        clean, dirty = scores(D, i2e_d, ud, idv, l1, 1), scores(bad, i2e_d, ud, idv, l1, 1)
        for k in range(2):
            assert torch.equal(clean[k][keep], dirty[k][keep]), 'an inf / nan row leaked into another pair'
            assert not torch.isfinite(dirty[k][5]) and not torch.isfinite(dirty[k][37])
            assert torch.isfinite(clean[k]).all()
