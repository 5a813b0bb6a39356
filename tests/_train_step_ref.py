"""fp64 reference of the fused training-step entry points (include/ktup_hip.h, "the B = 512 training step in two launches"):
ktup_train_rec_step, ktup_train_kg_step and their stored-row forms.  NOT a test module: tests/test_train_step_ref_host.py pins
it to oracle/cpu_ref.py on the CPU, tests/test_hip_train_step.py compares the kernels with it on the GPU.

Everything is plain torch in fp64 on the CPU, computed from the same fp32 inputs the kernels get, through the oracle's own
functions (score_tup, score_ktup_rec, score_transe, score_transh, bpr_loss, margin_loss, orthogonal_loss, norm_loss; the hard gate
is the oracle's st_gumbel_softmax, reached through the `uniform` argument of the score functions).

Case construction (rec_case / kg_case).  fp32 and fp64 legitimately disagree at knife edges, so a case holds none.  That is
asserted on the fp64 reference before a case is handed out; a case that violates a condition is drawn again with the next seed,
never pruned, and more than MAX_DRAWS seeds is an error of the construction.  While a case is built, the uniforms of offending
hard-gate rows and offending kg triples are drawn again from the same generator (one triple in a few hundred falls into the hinge
band and the largest batch holds 16387: no seed could ever pass as a whole); these inner rounds are capped at MAX_DRAWS too --
running out of them is loud for the gate and costs a seed for kg -- and counted: DRAWS holds the seeds and ROUNDS the inner
rounds of every family, and the tests assert that both stay small.  The conditions:
  * row norms: every user, item, entity, relation and preference row is a normalised row times 0.8 or 1.25 (|x|^2 = 0.64 or
    1.5625: both sides of normLoss's threshold, | |x|^2 - 1 | >= 1e-2); item 0, its entity and user 0 -- the rows the dead slots
    of a partial tile gather -- are times 3, so that a dead slot that leaks ON ONE SIDE is visible.  A leak on both sides is not:
    the positive and the negative half of a dead slot gather the same user 0, item 0 and uniform row 0 (fetch_ids and the gate of
    pref_bwd_wide_kernel), score alike, and their BPR gradients +g and -g cancel in every table gradient whatever row 0 holds;
  * margin (kg): min_k |pos_k - neg_k + margin| >= 10 x the score tolerance of tests/test_hip_score.py (rtol 1e-4, atol 1e-5) of
    both scores, and from B = 4 on active and inactive triples both occur;
  * L1: no coordinate of any z within 1e-7 of zero (tests/test_hip_score.py _l1_knife_edge) -- except the deliberate exact zero
    of kg_exact_zero_case;
  * hard gate: the best perturbed logit of every pair leads the second by >= 10 x (2e-5 + 2e-6 |best|), the redo margin of
    gate_argmax (tests/test_hip_gate_stream.py)."""
import torch

from oracle import cpu_ref as O

MAX_DRAWS = 20
SMALL = {'nu': 7, 'nitems': 11, 'ne': 9}            # rows collide; the entity table has one more row, the pad
DRAWS = {}                                       # family -> the largest number of seeds one of its cases needed
ROUNDS = {}                                      # family -> the largest number of inner rounds (offending rows / triples drawn again)


def _note(family, draws, rounds=0):
    DRAWS[family] = max(DRAWS.get(family, 0), draws)
    ROUNDS[family] = max(ROUNDS.get(family, 0), rounds)


def _rows(n, d, ld, gen, flip=0):
    """n normalised rows times 0.8 / 1.25 in turn, in a table of pitch ld whose columns beyond d hold junk."""
    t = torch.randn(n, ld, generator=gen)
    x = torch.nn.functional.normalize(t[:, :d], dim=1)
    scale = torch.where((torch.arange(n) + flip) % 2 == 0, 0.8, 1.25).unsqueeze(1)
    t[:, :d] = x * scale
    return t


def _d(t, d):
    return t[:, :d].double()


def assert_row_norms(*tables):
    for t in tables:
        n2 = (t.double() ** 2).sum(1)
        n2 = n2[n2 > 0]                                              # the pad row is zero
        assert float((n2 - 1.0).abs().min()) >= 1e-2
        assert n2.numel() < 2 or (bool((n2 > 1).any()) and bool((n2 < 1).any()))


def score_tol(s):
    return 1e-5 + 1e-4 * s.abs()


# ---------------------------------------------------------------------------------------------------- rec step
def _rec_scores(c, T, u, i, uni):
    """Scores of the pairs (u, i) from the fp64 tables T through the oracle."""
    if c['ktup']:
        return O.score_ktup_rec(T['U'], T['I'], T['E'], T['P'], T['Pn'], T['R'], T['Rn'], c['i2e'], u, i, c['l1'], uni)
    return O.score_tup(T['U'], T['I'], T['P'], T['Pn'], u, i, c['l1'], uni)


def rec_tables(c):
    d = c['d']
    names = ('U', 'I', 'E', 'P', 'Pn', 'R', 'Rn') if c['ktup'] else ('U', 'I', 'P', 'Pn')
    return {k: _d(c[k], d) for k in names}


def _rec_z_and_logits(c):
    """fp64 z of every pair (2B x d) and its perturbed logits (hard gate; else None), from the oracle's helpers."""
    T = rec_tables(c)
    u2, i2 = torch.cat([c['u'], c['u']]), torch.cat([c['pi'], c['ni']])
    uni = None if c['uni'] is None else c['uni'].double()
    u_e = T['U'][u2]
    if c['ktup']:
        v_e = T['I'][i2] + T['E'][c['i2e'][i2]]
        A = T['P'] + T['R']
        _, r_e, nrm = O.ktup_preferences(u_e, v_e, T['P'], T['Pn'], T['R'], T['Rn'], uni)
    else:
        v_e = T['I'][i2]
        A = T['P']
        _, r_e, nrm = O.tup_preferences(u_e, v_e, T['P'], T['Pn'], uni)
    z = O.projection_transH(u_e, nrm) + r_e - O.projection_transH(v_e, nrm)
    pert = None if uni is None else torch.matmul(u_e + v_e, A.t()) / 2 + O.gumbel_noise(uni)
    return z, pert


def _gate_offenders(c):
    _, pert = _rec_z_and_logits(c)
    if c['n_pref'] < 2:
        return torch.zeros(pert.shape[0], dtype=torch.bool)
    top = pert.topk(2, dim=1).values
    return (top[:, 0] - top[:, 1]) < 10.0 * (2e-5 + 2e-6 * top[:, 0].abs())


def rec_case(d, n_pref, B, ktup, hard, l1, seed, pitch=(0, 0, 0), sizes=SMALL, family='rec'):
    """A rec-step case that meets the module's conditions: fp32 tables (pitches d + pitch[0..2] for U, I, E), ids, uniforms."""
    nu, ni, ne = sizes['nu'], sizes['nitems'], sizes['ne']
    for draw in range(MAX_DRAWS):
        gen = torch.Generator().manual_seed(1000003 * seed + draw)
        c = {'d': d, 'n_pref': n_pref, 'B': B, 'ktup': ktup, 'hard': hard, 'l1': bool(l1), 'nu': nu, 'nitems': ni, 'ne': ne,
             'ldu': d + pitch[0], 'ldi': d + pitch[1], 'lde': d + pitch[2]}
        c['U'], c['I'] = _rows(nu, d, c['ldu'], gen), _rows(ni, d, c['ldi'], gen, 1)
        c['E'] = _rows(ne + 1, d, c['lde'], gen)
        c['E'][ne] = 0.0                                            # the pad row of nn.Embedding(padding_idx)
        c['P'], c['Pn'] = _rows(n_pref, d, d, gen), _rows(n_pref, d, d, gen, 1)
        c['R'], c['Rn'] = _rows(n_pref, d, d, gen, 1), _rows(n_pref, d, d, gen)
        i2e = torch.randint(0, ne, (ni,), generator=gen)
        i2e[3], i2e[ni - 1] = ne, ne                                # two items without an entity
        i2e[0] = 2                                                  # item 0 -- what a dead slot gathers -- has a real one
        c['i2e'] = i2e
        for t, row in ((c['U'], 0), (c['I'], 0), (c['E'], 2)):
            t[row, :d] *= 3.0 / float(t[row, :d].norm())
        c['u'] = torch.randint(0, nu, (B,), generator=gen)
        c['pi'], c['ni'] = torch.randint(0, ni, (B,), generator=gen), torch.randint(0, ni, (B,), generator=gen)
        c['pi'][0] = 3                                              # a pair on the pad row; B > 1: one on item 0's rows
        if B > 1:
            c['ni'][1] = 0
        c['uni'] = torch.rand(2 * B, n_pref, generator=gen) if hard else None
        assert_row_norms(c['U'][:, :d], c['I'][:, :d], c['E'][:, :d], c['P'], c['Pn'], c['R'], c['Rn'])
        rounds = 0
        if hard:
            for rounds in range(MAX_DRAWS + 1):
                bad = _gate_offenders(c)
                if not bool(bad.any()):
                    break
                if rounds == MAX_DRAWS:
                    raise AssertionError('hard gate: close calls survive %d draws of the uniforms' % MAX_DRAWS)
                c['uni'][bad] = torch.rand(int(bad.sum()), n_pref, generator=gen)
        if l1:
            z, _ = _rec_z_and_logits(c)
            if float(z.abs().min()) < 1e-7:
                continue
        _note(family, draw + 1, rounds)
        return c
    raise AssertionError('no admissible rec case in %d draws: the construction is wrong' % MAX_DRAWS)


def rec_loss_terms(c, T, target, orth):
    """(mean_k -logsigmoid(target (pos_k - neg_k)), orthogonalLoss(pref, pref_norm) or None) as fp64 graph nodes."""
    uni = c['uni']
    B = c['B']
    up, un = (None, None) if uni is None else (uni[:B].double(), uni[B:].double())
    pos, neg = _rec_scores(c, T, c['u'], c['pi'], up), _rec_scores(c, T, c['u'], c['ni'], un)
    return O.bpr_loss(pos, neg, target), (O.orthogonal_loss(T['P'], T['Pn']) if orth else None)


def rec_reference(c, target, gscale, orth):
    """What ONE ktup_train_rec_step adds: ([loss0, loss1], {table: gradient}).  The loss values are NOT scaled by gscale (the
    header); the gradients are those of (mean + orth) x gscale; the pad entity row receives nothing."""
    T = {k: v.clone().requires_grad_(True) for k, v in rec_tables(c).items()}
    bpr, ol = rec_loss_terms(c, T, target, orth)
    total = bpr if ol is None else bpr + ol
    (gscale * total).backward()
    g = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in T.items()}
    if c['ktup']:
        g['E'][c['ne']] = 0.0
    return [float(bpr.detach()), 0.0 if ol is None else float(ol.detach())], g


def rec_rows_reference(c, target, gscale, orth):
    """The stored-row form: autograd with the GATHERED rows as leaves.  GU row k (B x d) = the user-row gradient of example k
    from both its pairs, GV row k (2B x d) = the item(-plus-entity) row gradient of pair k; sumsq as the header defines it:
    sum |GU row|^2 + sum |GV row|^2 x (1 + [the pair's item has an entity row]).  -> (losses, {'GU','GV','P','Pn','R','Rn'}, sumsq)"""
    B, d = c['B'], c['d']
    T0 = rec_tables(c)
    u2, i2 = torch.cat([c['u'], c['u']]), torch.cat([c['pi'], c['ni']])
    ue = T0['U'][u2].clone().requires_grad_(True)
    ve = (T0['I'][i2] + T0['E'][c['i2e'][i2]] if c['ktup'] else T0['I'][i2]).clone().requires_grad_(True)
    T = {k: T0[k].clone().requires_grad_(True) for k in T0 if k not in ('U', 'I', 'E')}
    T['U'], T['I'] = ue, ve
    sub = dict(c)
    if c['ktup']:                                                   # the gathered row already holds the entity's: add a zero row
        T['E'] = torch.zeros(1, d, dtype=torch.float64)
        sub['i2e'] = torch.zeros(2 * B, dtype=torch.int64)
    k = torch.arange(B)
    sub['u'], sub['pi'], sub['ni'] = k, k, k + B
    uni = c['uni']
    up, un = (None, None) if uni is None else (uni[:B].double(), uni[B:].double())
    pos = _rec_scores(sub, T, k, k, up)
    neg = _rec_scores(sub, T, k + B, k + B, un)
    bpr = O.bpr_loss(pos, neg, target)
    ol = O.orthogonal_loss(T['P'], T['Pn']) if orth else None
    (gscale * (bpr if ol is None else bpr + ol)).backward()
    out = {'GU': ue.grad[:B] + ue.grad[B:], 'GV': ve.grad}
    for name in ('P', 'Pn', 'R', 'Rn'):
        if name in T:
            out[name] = T[name].grad
    has_e = (c['i2e'][i2] != c['ne']).double() if c['ktup'] else torch.zeros(2 * B, dtype=torch.float64)
    sumsq = float((out['GU'] ** 2).sum() + ((out['GV'] ** 2).sum(1) * (1.0 + has_e)).sum())
    return [float(bpr.detach()), 0.0 if ol is None else float(ol.detach())], out, sumsq


def scatter_rec_rows(c, rows):
    """The table gradients the stored rows stand for: index_add by id (the entity row takes its item's; the pad row nothing)."""
    d = c['d']
    i2 = torch.cat([c['pi'], c['ni']])
    g = {'U': torch.zeros(c['nu'], d, dtype=torch.float64).index_add_(0, c['u'], rows['GU']),
         'I': torch.zeros(c['nitems'], d, dtype=torch.float64).index_add_(0, i2, rows['GV'])}
    if c['ktup']:
        g['E'] = torch.zeros(c['ne'] + 1, d, dtype=torch.float64).index_add_(0, c['i2e'][i2], rows['GV'])
        g['E'][c['ne']] = 0.0
    return g


def reg_rows_reference(c, GU, GV, gP, scale_rows, scale_pref):
    """ktup_train_rec_reg_rows on top of preset fp64 GU / GV / gP: ([loss0, loss1] added, GU, GV, gP afterwards)."""
    d = c['d']
    i2 = torch.cat([c['pi'], c['ni']])
    ue = _d(c['U'], d)[c['u']].clone().requires_grad_(True)
    ve = _d(c['I'], d)[i2].clone().requires_grad_(True)
    pr = c['P'].double().clone().requires_grad_(True)
    rows_term = scale_rows * (O.norm_loss(ue) + O.norm_loss(ve))
    pref_term = scale_pref * O.norm_loss(pr)
    (rows_term + pref_term).backward()
    return [float(rows_term.detach()), float(pref_term.detach())], GU + ue.grad, GV + ve.grad, gP + pr.grad


# ---------------------------------------------------------------------------------------------------- kg step
def kg_tables(c):
    d = c['d']
    return {k: _d(c[k], d) for k in (('E', 'R', 'N') if c['transh'] else ('E', 'R'))}


def _kg_scores(c, T, h, t, r):
    if c['transh']:
        return O.score_transh(T['E'], T['R'], T['N'], h, t, r, c['l1'])
    return O.score_transe(T['E'], T['R'], h, t, r, c['l1'])


def _kg_z(c, T, h, t, r):
    if c['transh']:
        n_e = T['N'][r]
        return O.projection_transH(T['E'][h], n_e) + T['R'][r] - O.projection_transH(T['E'][t], n_e)
    return T['E'][h] + T['R'][r] - T['E'][t]


def kg_conditions(c, margin, skip_z_of=None):
    """The margin and L1 conditions of a kg case on the fp64 reference: None if they hold, else what fails."""
    T = kg_tables(c)
    B = c['B']
    h2, t2, r2 = torch.cat([c['h'], c['nh']]), torch.cat([c['t'], c['nt']]), torch.cat([c['r'], c['r']])
    s = _kg_scores(c, T, h2, t2, r2)
    pos, neg = s[:B], s[B:]
    m = pos - neg + margin
    if bool((m.abs() < 10.0 * (score_tol(pos) + score_tol(neg))).any()):
        return 'a margin term within ten score tolerances of its hinge'
    if B >= 4 and not (bool((m > 0).any()) and bool((m < 0).any())):
        return 'no active or no inactive triple'
    if c['l1']:
        z = _kg_z(c, T, h2, t2, r2).abs()
        if skip_z_of is not None:
            z[skip_z_of] = 1.0
        if float(z.min()) < 1e-7:
            return 'an L1 coordinate within 1e-7 of zero'
    return None


def _kg_triple_state(c, margins):
    """Per triple: (offending: a margin term within ten score tolerances of its hinge, or (L1) a coordinate of z within 1e-7 of
    zero; active under every margin; inactive under every margin)."""
    T = kg_tables(c)
    B = c['B']
    h2, t2, r2 = torch.cat([c['h'], c['nh']]), torch.cat([c['t'], c['nt']]), torch.cat([c['r'], c['r']])
    s = _kg_scores(c, T, h2, t2, r2)
    pos, neg = s[:B], s[B:]
    bad = torch.zeros(B, dtype=torch.bool)
    for m in margins:
        bad |= (pos - neg + m).abs() < 10.0 * (score_tol(pos) + score_tol(neg))
    if c['l1']:
        near = _kg_z(c, T, h2, t2, r2).abs().min(dim=1).values < 1e-7
        bad |= near[:B] | near[B:]
    return bad, (pos - neg + min(margins)) > 0, (pos - neg + max(margins)) < 0


def _plant_triple(c, slot, want_active, margins, gen):
    """Put a triple of the wanted kind into `slot`: the first admissible one of 64 candidates (an inactive triple is one in four to
    one in ten, depending on width and distance: waiting for it one draw at a time took up to 17 rounds)."""
    n = 64
    cand = dict(c, B=n, keeps_head=torch.zeros(n, dtype=torch.bool))
    for k in ('h', 't', 'r', 'nh', 'nt'):
        cand[k] = torch.zeros(n, dtype=torch.int64)
    _draw_triples(cand, torch.arange(n), gen)
    bad, active, inactive = _kg_triple_state(cand, margins)
    ok = ((active if want_active else inactive) & ~bad).nonzero().flatten()
    if ok.numel():
        for k in ('h', 't', 'r', 'nh', 'nt', 'keeps_head'):
            c[k][slot] = cand[k][ok[0]]


def _draw_triples(c, idx, gen):
    """(Re-)draw the triples `idx` and their twins: a twin keeps its head or its tail and takes a uniform entity at the other end."""
    n, ne = idx.numel(), c['ne']
    h, t = torch.randint(0, ne, (n,), generator=gen), torch.randint(0, ne, (n,), generator=gen)
    t = torch.where(t == h, (t + 1) % ne, t)
    other = torch.randint(0, ne, (n,), generator=gen)
    head = torch.rand(n, generator=gen) < 0.5                       # which end the twin corrupts
    c['h'][idx], c['t'][idx], c['r'][idx] = h, t, torch.randint(0, c['nr'], (n,), generator=gen)
    c['keeps_head'][idx] = ~head
    c['nh'][idx], c['nt'][idx] = torch.where(head, other, h), torch.where(head, t, other)


def kg_case(d, B, transh, l1, seed, margins=(1.0,), pitch=(0, 0, 0), ne=9, nr=4, family='kg'):
    """A kg-step case that meets the conditions for every margin in `margins`.  Triple k's twin keeps its head or its tail.  A
    hinge band of ten tolerances catches one triple in a few hundred and the grid-stride cases hold 16387, so -- like the hard gate's
    uniforms -- the OFFENDING triples are drawn again (whole triples, from the same generator) while the case is built, and a
    batch of four or more whose triples are all active or all inactive gets a triple of the missing kind planted in slot 0
    (inactive) or 1 (active); at most MAX_DRAWS such rounds (counted in ROUNDS), then the case is checked as a whole
    (kg_conditions) and a case that fails costs a seed."""
    for draw in range(MAX_DRAWS):
        gen = torch.Generator().manual_seed(1000003 * seed + draw)
        c = {'d': d, 'B': B, 'transh': bool(transh), 'l1': bool(l1), 'ne': ne, 'nr': nr,
             'lde': d + pitch[0], 'ldr': d + pitch[1], 'ldn': d + pitch[2]}
        c['E'], c['R'], c['N'] = _rows(ne, d, c['lde'], gen), _rows(nr, d, c['ldr'], gen, 1), _rows(nr, d, c['ldn'], gen)
        for k in ('h', 't', 'r', 'nh', 'nt'):
            c[k] = torch.zeros(B, dtype=torch.int64)
        c['keeps_head'] = torch.zeros(B, dtype=torch.bool)
        _draw_triples(c, torch.arange(B), gen)
        for rounds in range(MAX_DRAWS + 1):
            bad, active, inactive = _kg_triple_state(c, margins)
            lacks = [] if B < 4 else [(0, False)] * (not bool(inactive.any())) + [(1, True)] * (not bool(active.any()))
            done = not bool(bad.any()) and not lacks
            if done or rounds == MAX_DRAWS:
                break
            if bool(bad.any()):
                _draw_triples(c, bad.nonzero().flatten(), gen)
            for slot, want_active in lacks:                             # both kinds must occur: planted, not waited for
                _plant_triple(c, slot, want_active, margins, gen)
        assert_row_norms(c['E'][:, :d], c['R'][:, :d])
        if done and all(kg_conditions(c, m) is None for m in margins):
            _note(family, draw + 1, rounds)
            return c
    raise AssertionError('no admissible kg case in %d draws: the construction is wrong' % MAX_DRAWS)


def kg_exact_zero_case(d, transh, l1, seed, margin=1.0):
    """B = 5 whose triple 0 is (e, r0, e) with an all-zero relation row r0: z is EXACTLY zero in fp32 and fp64 alike, and torch's
    sign(0) = 0 makes its margin gradient exactly 0 under L1.  Its twin is (a, r0, b) on two entities of its own with
    b = a + 0.5 / d in every coordinate with random signs -- a score of 0.5 (L1) or less (L2), so the triple is ACTIVE at margin 1 -- and entity e
    is used by no other triple: gE[e] must come out exactly 0.  Entities 9, 10, 11 and relation 4 are appended to the small
    tables for it."""
    for draw in range(MAX_DRAWS):
        c = kg_case(d, 5, transh, l1, 7919 * seed + draw, margins=(margin,), family='kg_zero')
        gen = torch.Generator().manual_seed(seed + draw)
        extra = _rows(3, d, c['lde'], gen)
        sign = torch.where(torch.rand(d, generator=gen) < 0.5, -1.0, 1.0)
        extra[2, :d] = extra[1, :d] + (0.5 / d) * sign
        c['E'] = torch.cat([c['E'], extra])
        c['R'] = torch.cat([c['R'], torch.zeros(1, c['ldr'])])
        c['N'] = torch.cat([c['N'], _rows(1, d, c['ldn'], gen)])
        c['ne'], c['nr'] = c['ne'] + 3, c['nr'] + 1
        e, a, b, r0 = c['ne'] - 3, c['ne'] - 2, c['ne'] - 1, c['nr'] - 1
        c['h'][0], c['t'][0], c['r'][0], c['nh'][0], c['nt'][0] = e, e, r0, a, b
        c['zero_entity'] = e
        skip = torch.zeros(10, dtype=torch.bool)
        skip[0] = True
        T = kg_tables(c)
        z0 = _kg_z(c, T, c['h'][:1], c['t'][:1], c['r'][:1])
        assert float(z0.abs().max()) == 0.0
        s = _kg_scores(c, T, torch.tensor([e, a]), torch.tensor([e, b]), torch.tensor([r0, r0]))
        assert float(s[0] - s[1] + margin) > 0.1                    # active
        if kg_conditions(c, margin, skip_z_of=skip) is None:
            _note('kg_zero', draw + 1)
            return c
    raise AssertionError('no admissible exact-zero case in %d draws' % MAX_DRAWS)


def _kg_total(c, T, h2, t2, r2, ent_rows, margin, regs):
    """The four loss slots as graph nodes (None where `regs` switches one off); ent_rows: the 4B entity rows of normLoss."""
    B = c['B']
    s = _kg_scores(c, T, h2, t2, r2)
    terms = [O.margin_loss(s[:B], s[B:], margin), None, None, None]
    if (regs & 1) and c['transh']:
        terms[1] = O.orthogonal_loss(T['R'][r2], T['N'][r2])
    if regs & 2:
        terms[2] = O.norm_loss(ent_rows)
    if regs & 4:
        terms[3] = O.norm_loss(T['R'][r2])
    return terms


def kg_reference(c, margin, gscale, regs):
    """What ONE ktup_train_kg_step adds: ([4 loss slots], {'E','R'(,'N')}: gradients x gscale)."""
    T = {k: v.clone().requires_grad_(True) for k, v in kg_tables(c).items()}
    h2, t2, r2 = torch.cat([c['h'], c['nh']]), torch.cat([c['t'], c['nt']]), torch.cat([c['r'], c['r']])
    terms = _kg_total(c, T, h2, t2, r2, T['E'][torch.cat([c['h'], c['t'], c['nh'], c['nt']])], margin, regs)
    (gscale * sum(t for t in terms if t is not None)).backward()
    return [0.0 if t is None else float(t.detach()) for t in terms], {k: v.grad for k, v in T.items()}


def kg_rows_ids(c, mark):
    """ent_ids = [ph ; pt ; nh ; nt] of ktup_train_kg_step_rows with the kept end of every twin marked `mark` (-1 or ent_pad)."""
    nh = torch.where(c['keeps_head'], torch.full_like(c['nh'], mark), c['nh'])
    nt = torch.where(c['keeps_head'], c['nt'], torch.full_like(c['nt'], mark))
    return torch.cat([c['h'], c['t'], nh, nt])


def kg_rows_reference(c, margin, gscale, regs):
    """The stored-row form: the 4B gathered entity rows are the leaves, and a twin's kept end IS the positive's leaf -- its
    gradient lands in the positive's stored row and its own row is not written.  -> (losses, GE (4B x d), written (4B bool),
    {'R'(,'N')}, sumsq = sum of |row|^2 over the stored rows)."""
    B = c['B']
    T0 = kg_tables(c)
    k = torch.arange(B)
    Eg = T0['E'][torch.cat([c['h'], c['t'], c['nh'], c['nt']])].clone().requires_grad_(True)
    T = {n: T0[n].clone().requires_grad_(True) for n in T0 if n != 'E'}
    T['E'] = Eg
    nh_idx = torch.where(c['keeps_head'], k, 2 * B + k)
    nt_idx = torch.where(c['keeps_head'], 3 * B + k, B + k)
    h2, t2, r2 = torch.cat([k, nh_idx]), torch.cat([B + k, nt_idx]), torch.cat([c['r'], c['r']])
    terms = _kg_total(c, T, h2, t2, r2, Eg[torch.cat([k, B + k, nh_idx, nt_idx])], margin, regs)
    (gscale * sum(t for t in terms if t is not None)).backward()
    written = torch.cat([torch.ones(2 * B, dtype=torch.bool), ~c['keeps_head'], c['keeps_head']])
    GE = Eg.grad
    assert float(GE[~written].abs().max() if bool((~written).any()) else 0.0) == 0.0
    small = {n: T[n].grad for n in T if n != 'E'}
    return [0.0 if t is None else float(t.detach()) for t in terms], GE, written, small, float((GE ** 2).sum())


def scatter_kg_rows(c, GE):
    ids = torch.cat([c['h'], c['t'], c['nh'], c['nt']])
    return torch.zeros(c['ne'], c['d'], dtype=torch.float64).index_add_(0, ids, GE)
