"""What the tests of the link-prediction list pass (ktup_eval_kg_topk) share, on the host: the fp64 scores of evaluateHead /
evaluateTail (transE.py:65-105, transH.py:73-121) from fp32 tables, the CSR filter lists, and the referee of
tests/test_hip_cfkg_pass.py, which decides whether a returned list is A right list for the fp64 scores.

With tol(s) = 1e-4 |s| + 1e-5 a returned list is right if
  * it has the reference list's length and padding (ids -1, scores 0.0),
  * its ids are distinct, unfiltered candidates in range,
  * its returned scores agree with the fp64 scores of its own ids within tol,
  * its scores are non-decreasing, equal scores ordered by lower j first,
  * no unfiltered candidate left out has an fp64 score below the list's last fp64 score by more than tol.
That tolerance is about 60 times the arithmetic's error, so `exact_fraction` stands beside it: the share of keys whose list is
exactly the fp64 list as an id sequence."""
import numpy as np


def tol(s):
    return 1e-4 * np.abs(s) + 1e-5


def scores64(E, R, N, C, q, r, l1, head):
    """(len(q), len(C)) fp64 distances from fp32 (or any) numpy tables; N None = TransE, else w = N[r] (no unit norm assumed)."""
    E, R, C = (np.asarray(t, dtype=np.float64) for t in (E, R, C))
    sgn = -1.0 if head else 1.0
    eq, rr = E[q], R[r]
    if N is None:
        c = eq + sgn * rr
        z = c[:, None, :] - C[None, :, :]
    else:
        w = np.asarray(N, dtype=np.float64)[r]
        c = (eq - (w * eq).sum(1, keepdims=True) * w) + sgn * rr
        we = w @ C.T                                                      # (nq, n_cand)
        z = c[:, None, :] - C[None, :, :] + we[:, :, None] * w[:, None, :]
    return np.abs(z).sum(2) if l1 else (z * z).sum(2)


def filters(rng, nq, n_cand):
    """CSR filter lists per key in candidate space: random sizes, key 0 without a list entry, key 1 filtered completely, key 2 a row
    of -1 (nothing is filtered by it).  -> int64 offsets, int32 ids, per key the set of filtered j."""
    sizes = rng.randint(0, max(2, n_cand // 4) + 1, size=nq)
    sizes[0] = 0
    if nq > 1:
        sizes[1] = n_cand
    if nq > 2:
        sizes[2] = 3
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    flat = rng.randint(0, n_cand, size=int(off[-1])).astype(np.int32)
    if nq > 1:
        flat[off[1]:off[2]] = np.arange(n_cand, dtype=np.int32)
    if nq > 2:
        flat[off[2]:off[3]] = -1
    banned = [set(int(x) for x in flat[off[b]:off[b + 1]] if x >= 0) for b in range(nq)]
    return off, flat, banned


def _allowed(ref_row, banned_b):
    ok = np.isfinite(ref_row)
    if banned_b is not None and len(banned_b):
        ok[np.fromiter(banned_b, dtype=np.int64)] = False
    return ok


def list64(ref, banned, topn):
    """The fp64 list: per key the first topn unfiltered candidates by (score, j), -1 padded."""
    nq, n_cand = ref.shape
    out = np.full((nq, topn), -1, dtype=np.int32)
    for b in range(nq):
        ok = _allowed(ref[b], None if banned is None else banned[b])
        idx = np.nonzero(ok)[0]
        order = idx[np.lexsort((idx, ref[b, idx]))][:topn]
        out[b, :len(order)] = order
    return out


def exact_fraction(ids, ref, banned, topn):
    want = list64(ref, banned, topn)
    return float((ids == want).all(1).mean()) if len(ids) else 1.0


def referee(ids, scores, ref, banned, topn, what):
    """ids / scores: (nq, topn) of the pass (scores may be None); ref: (nq, n_cand) fp64 scores; banned: per key the set of filtered
    j, or None.  Every row, every slot is judged."""
    nq, n_cand = ref.shape
    assert ids.shape == (nq, topn) and ids.dtype == np.int32, what
    for b in range(nq):
        ok = _allowed(ref[b], None if banned is None else banned[b])
        n = min(topn, int(ok.sum()))
        row = ids[b]
        assert (row[n:] == -1).all() and (row[:n] >= 0).all() and (row[:n] < n_cand).all(), (what, b, row, n)
        got = row[:n].astype(np.int64)
        assert len(set(got.tolist())) == n, (what, b, 'repeated ids', row)
        assert ok[got].all(), (what, b, 'a filtered candidate', row)
        mine = ref[b, got]
        if scores is not None:
            assert (scores[b, n:] == 0.0).all(), (what, b, 'padding scores')
            sc = scores[b, :n]
            assert (np.abs(sc.astype(np.float64) - mine) <= tol(mine)).all(), (what, b, sc, mine)
            assert (sc[1:] >= sc[:-1]).all(), (what, b, 'scores not ascending', sc)
            same = sc[1:] == sc[:-1]
            assert (got[1:][same] > got[:-1][same]).all(), (what, b, 'equal scores: lower j first', row, sc)
        else:
            assert (mine[1:] >= mine[:-1] - tol(mine[:-1])).all(), (what, b, 'fp64 scores of the list not ascending', mine)
        if n:
            out = ok.copy()
            out[got] = False
            last = mine[-1]
            assert not (ref[b, out] < last - tol(last)).any(), (what, b, 'a better candidate was left out',
                                                                np.nonzero(out & (ref[b] < last - tol(last)))[0])
