"""fp64 reference of ktup_train_transr_step (include/ktup_hip.h, "the TransR training step in one launch").  NOT a test module:
tests/test_transr_step_ref_host.py pins it to the closed forms of the header on the CPU, tests/test_hip_transr_step.py compares the
kernel with it on the GPU.

Everything is torch autograd in fp64 on the CPU of oracle.cpu_ref.score_transr, margin_loss and norm_loss, from the same fp32
inputs the kernel gets.  Cases are built like tests/_train_step_ref.py kg_case (its row generator, tolerances and counters are
reused): entity and relation rows are normalised rows times 0.8 / 1.25 (both sides of normLoss's threshold), the projection rows
are Xavier-scale random matrices (uniform in +-sqrt(6 / (d + d)), not the identity), and a case holds no knife edge:
  * no hinge argument pos - neg + margin within 10 score tolerances (rtol 1e-4, atol 1e-5 of both scores) of 0;
  * under L1 no coordinate of any y within 1e-7 of 0;
  * from B = 4 on active and inactive examples both occur.
The RELATION ids of a case are given by the caller (the arrangements are what the tests are about), so the entities of offending
examples are drawn again from the same generator, and an example of the missing kind is planted, for at most MAX_DRAWS rounds per
seed and MAX_DRAWS seeds; running out is an error of the construction.  All of this happens before any launch."""
import math

import torch

from oracle import cpu_ref as O
from tests._train_step_ref import MAX_DRAWS, DRAWS, ROUNDS, _note, _rows, _d, assert_row_norms, score_tol

NE = 9                                           # rows collide


def tables(c):
    d = c['d']
    return {'E': _d(c['E'], d), 'R': _d(c['R'], d), 'M': c['M'][:, :d * d].double()}


def ids(c):
    """[pos ; neg] id arrays of the launch."""
    return torch.cat([c['h'], c['nh']]), torch.cat([c['t'], c['nt']]), torch.cat([c['r'], c['nr']])


def _y(T, h, t, r):
    d = T['E'].shape[1]
    return torch.einsum('bij,bj->bi', T['M'][r].view(-1, d, d), T['E'][h] - T['E'][t]) + T['R'][r]


def _state(c, margins):
    """Per example: (offending, active under every margin, inactive under every margin)."""
    T = tables(c)
    B = c['B']
    h2, t2, r2 = ids(c)
    s = O.score_transr(T['E'], T['R'], T['M'], h2, t2, r2, c['l1'])
    pos, neg = s[:B], s[B:]
    bad = torch.zeros(B, dtype=torch.bool)
    for m in margins:
        bad |= (pos - neg + m).abs() < 10.0 * (score_tol(pos) + score_tol(neg))
    if c['l1']:
        near = _y(T, h2, t2, r2).abs().min(dim=1).values < 1e-7
        bad |= near[:B] | near[B:]
    return bad, (pos - neg + min(margins)) > 0, (pos - neg + max(margins)) < 0


def conditions(c, margins):
    """None if the case holds no knife edge and both kinds of example (B >= 4), else what fails."""
    bad, active, inactive = _state(c, margins)
    if bool(bad.any()):
        return 'a hinge argument within ten score tolerances of 0, or an L1 coordinate within 1e-7 of 0'
    if c['B'] >= 4 and len(margins) == 1 and not c.get('all_inactive') and not (bool(active.any()) and bool(inactive.any())):
        return 'no active or no inactive example'
    return None


def _draw_entities(c, idx, gen):
    """(Re-)draw the entities of the examples `idx`: a twin keeps its head or its tail and takes a uniform entity at the other end."""
    n, ne = idx.numel(), c['ne']
    h, t = torch.randint(0, ne, (n,), generator=gen), torch.randint(0, ne, (n,), generator=gen)
    t = torch.where(t == h, (t + 1) % ne, t)
    other = torch.randint(0, ne, (n,), generator=gen)
    head = torch.rand(n, generator=gen) < 0.5
    c['h'][idx], c['t'][idx] = h, t
    c['nh'][idx], c['nt'][idx] = torch.where(head, other, h), torch.where(head, t, other)


def _plant(c, slot, want_active, margins, gen):
    """Entities for example `slot` (its relations stay) that make it active / inactive: the first admissible of 64 candidates."""
    n = 64
    cand = dict(c, B=n)
    for k in ('h', 't', 'nh', 'nt'):
        cand[k] = torch.zeros(n, dtype=torch.int64)
    cand['r'], cand['nr'] = c['r'][slot].repeat(n), c['nr'][slot].repeat(n)
    _draw_entities(cand, torch.arange(n), gen)
    bad, active, inactive = _state(cand, margins)
    ok = ((active if want_active else inactive) & ~bad).nonzero().flatten()
    if ok.numel():
        for k in ('h', 't', 'nh', 'nt'):
            c[k][slot] = cand[k][ok[0]]


def rel_ids(B, n_rel, kind, seed=0):
    """The relation arrangements of the tests.  'random': uniform ids; 'skip': relation 0 has no example; 'edge': one relation with
    exactly 16 examples, one with 17, and with n_rel >= 3 the rest on the others (tile edges: a wave tile is 8 examples, two are
    16); 'major': one relation holds more than half of the batch."""
    gen = torch.Generator().manual_seed(977 * seed + 31 * B + n_rel)
    if kind == 'random' or n_rel == 1:
        return torch.randint(0, n_rel, (B,), generator=gen)
    if kind == 'skip':
        return torch.randint(1, n_rel, (B,), generator=gen)
    if kind == 'major':
        r = torch.randint(0, n_rel, (B,), generator=gen)
        r[torch.randperm(B, generator=gen)[:B // 2 + 1]] = n_rel - 1
        return r
    if kind == 'edge':
        assert B >= 33 and n_rel >= 2
        r = torch.randint(2, n_rel, (B,), generator=gen) if n_rel > 2 else torch.zeros(B, dtype=torch.int64)
        perm = torch.randperm(B, generator=gen)
        r[perm[:16]] = 1
        if n_rel > 2:
            r[perm[16:33]] = 0
        else:
            assert B == 33
        return r
    raise ValueError(kind)


def case(d, B, n_rel, l1, seed, r=None, nr=None, margins=(1.0,), pitch=(0, 0, 0), all_inactive=False, family='transr'):
    """A TransR step case: fp32 tables E (NE x (d + pitch[0])), R (n_rel x (d + pitch[1])), M (n_rel x (d^2 + pitch[2])) whose pitch
    gaps hold junk, relation ids `r` (default: uniform) and twin relation ids `nr` (default: r; anything else makes strays).
    all_inactive: every example must be inactive (needs a negative margin the caller picked for it)."""
    r = rel_ids(B, n_rel, 'random', seed) if r is None else r.clone()
    nr = r.clone() if nr is None else nr.clone()
    assert r.numel() == B and nr.numel() == B and int(r.max()) < n_rel and int(nr.max()) < n_rel
    for draw in range(MAX_DRAWS):
        gen = torch.Generator().manual_seed(1000003 * seed + draw)
        c = {'d': d, 'B': B, 'n_rel': n_rel, 'l1': bool(l1), 'ne': NE, 'r': r, 'nr': nr, 'all_inactive': all_inactive,
             'lde': d + pitch[0], 'ldr': d + pitch[1], 'ldm': d * d + pitch[2]}
        c['E'], c['R'] = _rows(NE, d, c['lde'], gen), _rows(n_rel, d, c['ldr'], gen, 1)
        bound = math.sqrt(6.0 / (d + d))
        c['M'] = (torch.rand(n_rel, c['ldm'], generator=gen) * 2.0 - 1.0) * bound
        for k in ('h', 't', 'nh', 'nt'):
            c[k] = torch.zeros(B, dtype=torch.int64)
        _draw_entities(c, torch.arange(B), gen)
        done = False
        for rounds in range(MAX_DRAWS + 1):
            bad, active, inactive = _state(c, margins)
            if all_inactive:
                bad = bad | ~inactive
                lacks = []
            else:
                lacks = [] if B < 4 else [(0, False)] * (not bool(inactive.any())) + [(1, True)] * (not bool(active.any()))
            done = not bool(bad.any()) and not lacks
            if done or rounds == MAX_DRAWS:
                break
            if bool(bad.any()):
                _draw_entities(c, bad.nonzero().flatten(), gen)
            for slot, want_active in lacks:
                _plant(c, slot, want_active, margins, gen)
        assert_row_norms(c['E'][:, :d], c['R'][:, :d])
        if done and conditions(c, margins) is None:
            _note(family, draw + 1, rounds)
            return c
    raise AssertionError('no admissible TransR case in %d draws: the construction is wrong' % MAX_DRAWS)


def loss_terms(c, T, margin, regs):
    """The loss slots 0, 2, 3 as graph nodes (None where `regs` switches one off)."""
    B = c['B']
    h2, t2, r2 = ids(c)
    s = O.score_transr(T['E'], T['R'], T['M'], h2, t2, r2, c['l1'])
    terms = [O.margin_loss(s[:B], s[B:], margin), None, None, None]
    if regs & 2:
        terms[2] = O.norm_loss(T['E'][torch.cat([c['h'], c['t'], c['nh'], c['nt']])])
    if regs & 4:
        terms[3] = O.norm_loss(T['R'][r2])
    return terms


def touched_rows(c, margin, regs):
    """{'E', 'R', 'M'}: bool per table row -- does the step add anything to that row of the gradient?  A row is touched by a triple of
    an ACTIVE example (fp64 hinge argument > 0; entity rows of both ends, the relation's row of R and of M) and by its regulariser
    where `regs` has it on and |row|^2 > 1.  Everything else must keep its content bit for bit.  (This is not "the reference's row is
    zero": an example whose twin is the same triple is active with a hinge argument of exactly `margin`, and its two halves add +x
    and -x to the same rows -- zero in the reference, but touched, and x - x onto a non-zero cell need not give the cell back.)"""
    T = tables(c)
    B = c['B']
    h2, t2, r2 = ids(c)
    s = O.score_transr(T['E'], T['R'], T['M'], h2, t2, r2, c['l1'])
    act = (s[:B] - s[B:] + margin) > 0
    act2 = torch.cat([act, act])
    out = {'E': torch.zeros(c['ne'], dtype=torch.bool), 'R': torch.zeros(c['n_rel'], dtype=torch.bool),
           'M': torch.zeros(c['n_rel'], dtype=torch.bool)}
    out['E'][h2[act2]] = True
    out['E'][t2[act2]] = True
    out['R'][r2[act2]] = True
    out['M'][r2[act2]] = True
    if regs & 2:
        used = torch.zeros(c['ne'], dtype=torch.bool)
        used[torch.cat([h2, t2])] = True
        out['E'] |= used & ((T['E'] ** 2).sum(1) > 1)
    if regs & 4:
        used = torch.zeros(c['n_rel'], dtype=torch.bool)
        used[r2] = True
        out['R'] |= used & ((T['R'] ** 2).sum(1) > 1)
    return out


def reference(c, margin, gscale, regs):
    """What ONE ktup_train_transr_step adds: ([4 loss slots, unscaled], {'E', 'R', 'M'}: gradients x gscale)."""
    T = {k: v.clone().requires_grad_(True) for k, v in tables(c).items()}
    terms = loss_terms(c, T, margin, regs)
    (gscale * sum(t for t in terms if t is not None)).backward()
    return [0.0 if t is None else float(t.detach()) for t in terms], {k: v.grad for k, v in T.items()}


# ---------------------------------------------------------------------------------------------------- the cases of the GPU test
NSPLITS = (0, 1, 3)
PITCHES = ((0, 0, 0), (4, 4, 4), (4, 0, 4), (0, 4, 0))
REGS = (6, 0, 2, 4)
GSCALES = (1.0, 0.37)
KINDS = ('random', 'skip', 'major')


def grid_specs():
    """d x l1 x B x n_rel in full; the relation arrangement, nsplit, the pitches, regs and gscale rotate over the grid at strides
    chosen so that every value of each meets every d and both distances."""
    out = []
    idx = 0
    for d in (64, 100, 128):
        for l1 in (0, 1):
            for B in (1, 15, 16, 17, 67, 300):
                for n_rel in (1, 4, 7):
                    out.append(dict(d=d, l1=l1, B=B, n_rel=n_rel, kind=KINDS[idx % 3] if n_rel > 1 else 'random', nsplit=NSPLITS[(idx // 3) % 3],
                                    pitch=PITCHES[idx % 4], regs=REGS[(idx // 2) % 4], gscale=GSCALES[(idx // 5) % 2], seed=idx + 1))
                    idx += 1
    return out


def edge_specs():
    """Tile edges: a relation with exactly 16 examples and one with 17 (B = 33 on two relations, B = 67 and 300 with the rest spread
    over the others), under every nsplit; and at B = 300 a relation with more than half of the batch under every nsplit."""
    out = []
    idx = 0
    for d in (64, 100, 128):
        for l1 in (0, 1):
            for nsplit in NSPLITS:
                B, n_rel = ((33, 2), (67, 4), (67, 7))[idx % 3]
                out.append(dict(d=d, l1=l1, B=B, n_rel=n_rel, kind='edge', nsplit=nsplit, pitch=PITCHES[idx % 4], regs=REGS[idx % 4],
                                gscale=GSCALES[idx % 2], seed=500 + idx))
                idx += 1
    for l1 in (0, 1):
        for nsplit in NSPLITS:
            for kind in ('edge', 'major'):
                out.append(dict(d=100, l1=l1, B=300, n_rel=7, kind=kind, nsplit=nsplit, pitch=PITCHES[idx % 4], regs=6,
                                gscale=GSCALES[idx % 2], seed=500 + idx))
                idx += 1
    return out


def spec_id(s):
    return 'd%d-%s-B%d-R%d-%s-ns%d-p%d%d%d-regs%d-g%s' % ((s['d'], 'L1' if s['l1'] else 'L2', s['B'], s['n_rel'], s['kind'], s['nsplit'])
                                                          + tuple(s['pitch']) + (s['regs'], s['gscale']))


_CACHE = {}


def spec_case(s):
    """The (cached: built once, shared, never modified) case of a spec."""
    key = spec_id(s)
    if key not in _CACHE:
        _CACHE[key] = case(s['d'], s['B'], s['n_rel'], s['l1'], s['seed'], r=rel_ids(s['B'], s['n_rel'], s['kind'], s['seed']), pitch=s['pitch'])
    return _CACHE[key]


def stray_case(d, l1, seed=71):
    """B = 40 on 4 relations with three examples whose twin names another relation."""
    B, n_rel = 40, 4
    r = rel_ids(B, n_rel, 'random', seed)
    nr = r.clone()
    for k in (3, 17, 39):
        nr[k] = (r[k] + 1 + k % 3) % n_rel
    assert int((nr != r).sum()) == 3
    return case(d, B, n_rel, l1, seed, r=r, nr=nr, pitch=(4, 4, 4), family='transr_stray')


def inactive_case(d, l1, seed=83):
    """B = 20 with every example inactive: margin -1e4 is below every pos - neg the small tables can produce."""
    return case(d, 20, 4, l1, seed, margins=(INACTIVE_MARGIN,), all_inactive=True, family='transr_inactive')


INACTIVE_MARGIN = -1.0e4
