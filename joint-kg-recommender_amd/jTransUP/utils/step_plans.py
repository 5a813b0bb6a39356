"""The launch plans of the GPU-resident training steps (utils/fast_train.py, utils/fast_train_dot.py): ONE function per entry point
of include/ktup_hip.h that more than one stepper binds, so that an argument list is typed out once.  Each takes tensors and plain
values and returns `lib.bind` launchers (zero-argument callables with the arguments marshalled).

Common arguments: `ids` -- the persistent [pos ; neg] id arrays of the step kind, (u2, i2) for rec and (h2, t2, r2[, ht4]) for kg;
`loss` -- the 8 loss slots; `g(t)` -- the pointer of table t's gradient buffer (the steppers' `_g`: `t.grad`, or the kept-aside view of a
table that has not joined the optimizer step yet); `gnorm` -- pointer of the tracked-gradient-norm workspace or None; `st` -- the stream.
A table a model does not have is None: its pointers are NULL, its pitch 0, its pad row -1."""
from jTransUP.hip import lib as L


def _p(t):
    return None if t is None else t.data_ptr()


def _ld(t):
    return 0 if t is None else t.stride(0)


def _opt(g):
    return lambda t: None if t is None else g(t)


def rec_step(U, I, P, Pn, ids, B, l1, gate, target, inv, loss, g, gnorm, st, E=None, i2e=None, ent_pad=-1, R=None, Rn=None):
    """ktup_train_rec_step: TUP on (U, I, P, Pn); with the entity side (E, i2e, ent_pad) and the relation tables (R, Rn) KTUP.
    `gate` = (mode, pointer) of the preference gate, `inv` = 1 / world."""
    u2, i2 = ids
    n_pref, d = P.shape
    g = _opt(g)
    return L.bind('ktup_train_rec_step', _p(U), U.stride(0), _p(I), I.stride(0), _p(E), _ld(E), _p(i2e), ent_pad, _p(P), _p(Pn), _p(R),
                  _p(Rn), P.stride(0), n_pref, d, _p(u2), _p(i2), B, l1, gate[0], gate[1], 0, 0, target, inv, 1, _p(loss), g(U), g(I), g(E),
                  g(P), g(Pn), g(R), g(Rn), gnorm, st)


def kg_step(E, R, Rn, ids, B, l1, margin, scale, loss, g, gnorm, st):
    """ktup_train_kg_step: TransH with the normal table Rn (all three regularisers), TransE with Rn = None (the two row norms).
    `scale` multiplies the gradients (kg_lambda of the joint drivers)."""
    transh = Rn is not None
    g = _opt(g)
    return L.bind('ktup_train_kg_step', int(transh), _p(E), E.stride(0), _p(R), R.stride(0), _p(Rn), _ld(Rn), E.shape[1], _p(ids[0]),
                  _p(ids[1]), _p(ids[2]), B, l1, margin, scale, 7 if transh else 6, _p(loss), g(E), g(R), g(Rn), gnorm, st)


def transr_step(E, R, M, ids, B, l1, margin, scale, loss, g, st):
    """ktup_train_transr_step (no tracked norm: the kernel has no such argument)."""
    return L.bind('ktup_train_transr_step', _p(E), E.stride(0), _p(R), R.stride(0), _p(M), M.stride(0), min(R.shape[0], M.shape[0]),
                  E.shape[1], _p(ids[0]), _p(ids[1]), _p(ids[2]), B, l1, margin, scale, 6, 0, _p(loss), g(E), g(R), g(M), st)


def transd_step(E, R, Ep, Rp, ids, B, l1, margin, scale, loss, g, gnorm, st):
    """ktup_train_transd_step."""
    return L.bind('ktup_train_transd_step', _p(E), E.stride(0), _p(R), R.stride(0), _p(Ep), Ep.stride(0), _p(Rp), Rp.stride(0), E.shape[1],
                  _p(ids[0]), _p(ids[1]), _p(ids[2]), B, l1, margin, scale, 6, _p(loss), g(E), g(R), g(Ep), g(Rp), gnorm, st)


def dot_step(U, I, ids, B, target, inv, loss, g, st, E=None, i2e=None, ent_pad=-1, bias=None):
    """ktup_train_dot_step: <user row, item row> (+ the item's entity row: E, i2e, ent_pad -- CKE) (+ `bias` = (global bias, user bias
    table, item bias table) -- FM, coFM; of those only the item bias has a gradient under a BPR loss)."""
    gb, bu, bi = bias if bias is not None else (None, None, None)
    g = _opt(g)
    return L.bind('ktup_train_dot_step', _p(U), U.stride(0), _p(I), I.stride(0), _p(E), _ld(E), _p(i2e), ent_pad, _p(gb), _p(bu), _p(bi),
                  U.shape[1], _p(ids[0]), _p(ids[1]), B, target, inv, _p(loss), g(U), g(I), g(E), g(bi), st)


# model kind -> (forward entry, backward entry, tables after (E, R), the forward takes the relation count, orthogonalLoss(R, Rn) rows)
KG_SEQUENCE = {
    'transe': ('ktup_score_transe_fwd', 'ktup_score_transe_bwd', 0, True, False),
    'transh': ('ktup_score_transh_fwd', 'ktup_score_transh_bwd', 1, True, True),
    'transr': ('ktup_score_transr_fwd', 'ktup_score_transr_bwd', 1, True, False),      # its forward also takes the bucket workspace `rws`
    'transd': ('ktup_score_transd_fwd', 'ktup_score_transd_bwd', 2, False, False)}


def kg_sequence(kind, tabs, ids, B, l1, margin, score, gscore, loss, up, g, st, rws=None):
    """The multi-launch KG step, in order: score forward of [pos ; neg], marginLoss value + gradient, score backward,
    (TransH) orthogonalLoss on the step's relation rows, normLoss on its entity rows and on its relation rows.  `tabs` = (E, R) + the
    kind's own tables, `ids` = (h2, t2, r2, ht4), `up` the upstream device scalar every loss gradient is multiplied by (one, or
    kg_lambda), `rws` TransR's workspace of the relation-bucketed forward."""
    fwd, bwd, extra, counted, orth = KG_SEQUENCE[kind]
    if len(tabs) != 2 + extra:
        raise L.KtupError('%s takes %d tables, got %d' % (kind, 2 + extra, len(tabs)))
    E, R = tabs[:2]
    h2, t2, r2, ht4 = ids
    d = E.shape[1]
    rows = ()
    for t in tabs:
        rows += (_p(t), t.stride(0))
    n_rel = (min(t.shape[0] for t in tabs[1:]),) if counted else ()
    batch = (d, _p(h2), _p(t2), _p(r2), 2 * B, l1)
    calls = [
        L.bind(fwd, *(rows + n_rel + batch + (_p(score),) + ((_p(rws),) if kind == 'transr' else ()) + (st,))),
        L.bind('ktup_loss_margin_fused', _p(score[:B]), _p(score[B:]), B, margin, _p(up), _p(loss[0:]), _p(gscore[:B]), _p(gscore[B:]), st),
        L.bind(bwd, *(rows + batch + (_p(gscore),) + tuple(g(t) for t in tabs) + (st,)))]
    if orth:
        Rn = tabs[2]
        calls.append(L.bind('ktup_reg_orth_fused', _p(R), R.stride(0), _p(Rn), Rn.stride(0), d, _p(r2), 2 * B, _p(up), _p(loss[1:]),
                            g(R), g(Rn), st))
    calls += [L.bind('ktup_reg_norm_fused', _p(E), E.stride(0), d, _p(ht4), 4 * B, _p(up), _p(loss[2:]), g(E), st),
              L.bind('ktup_reg_norm_fused', _p(R), R.stride(0), d, _p(r2), 2 * B, _p(up), _p(loss[3:]), g(R), st)]
    return calls
