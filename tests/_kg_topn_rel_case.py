"""What the tests of the relation-bucketed link-prediction list pass (ktup_eval_kg_topk_rel) share, on the host: the fp64 scores of
evaluateHead / evaluateTail for TransR / CKE (transR.py:80-128, CKE.py:155-203) and TransD (transD.py:78-134) from fp32 tables.  The
CSR filter lists, the referee, the exact-list share and the tolerance are those of tests/_kg_topn_case.py.

    TransR   c = M_r E[q] + sgn R[r],                            z = c - M_r e
    TransD   a = Ep[q], b = Rp[r], c = E[q] + (E[q].a) b + sgn R[r],   z = c - e - (e.a) b     (the QUERY's row a projects every candidate)
with sgn = +1 for tails, -1 for heads; distance = sum |z_k| (l1) or sum z_k^2."""
import numpy as np

from tests._kg_topn_case import exact_fraction, filters, list64, referee, tol  # noqa: F401  (re-exported)


def scores64_transr(E, R, M, q, r, l1, head):
    """(len(q), len(E)) fp64 distances; M: (n_rel, d * d), row-major d x d matrices."""
    E, R, M = (np.asarray(t, dtype=np.float64) for t in (E, R, M))
    d = E.shape[1]
    sgn = -1.0 if head else 1.0
    Mr = M.reshape(-1, d, d)[r]                                            # (nq, d, d)
    c = np.matmul(Mr, E[q][:, :, None])[:, :, 0] + sgn * R[r]
    pe = np.matmul(E[None, :, :], Mr.transpose(0, 2, 1))                   # (nq, n_ent, d): M_r e for every key and entity
    z = c[:, None, :] - pe
    return np.abs(z).sum(2) if l1 else (z * z).sum(2)


def scores64_transd(E, R, Ep, Rp, q, r, l1, head):
    """(len(q), len(E)) fp64 distances."""
    E, R, Ep, Rp = (np.asarray(t, dtype=np.float64) for t in (E, R, Ep, Rp))
    sgn = -1.0 if head else 1.0
    a, b, eq = Ep[q], Rp[r], E[q]
    c = eq + (eq * a).sum(1, keepdims=True) * b + sgn * R[r]
    s = a @ E.T                                                            # (nq, n_ent): e . a, a the query's row
    z = c[:, None, :] - E[None, :, :] - s[:, :, None] * b[:, None, :]
    return np.abs(z).sum(2) if l1 else (z * z).sum(2)
