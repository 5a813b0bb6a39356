"""fp64 reference of ktup_train_transd_step (include/ktup_hip.h, "the TransD training step in one launch").  NOT a test module:
tests/test_transd_step_ref_host.py pins it to the reference's goldens (tests/golden/transd.npz) on the CPU,
tests/test_hip_transd_step.py compares the kernel with it on the GPU.

Everything is torch autograd in fp64 on the CPU over the closed forms of the header -- alpha = h . h_p, beta = t . t_p,
v = (h - t) + r + (alpha - beta) r_p, s = sum |v| or sum v^2 -- with oracle.cpu_ref's margin_loss and norm_loss, from the same fp32
inputs the kernel gets.  Cases are built like tests/_transr_step_ref.py's (the row generator, the score tolerance and the counters
of tests/_train_step_ref.py are reused): all four tables hold normalised rows times 0.8 / 1.25 in turn, so | |x|^2 - 1 | >= 0.36
for every regularised row (asserted: >= 1e-2), and a case holds no knife edge:
  * no hinge argument s+ - s- + margin within 10 score tolerances (rtol 1e-4, atol 1e-5 of both scores) of 0: the kernel's scores
    are held to one such tolerance each, so fp32 cannot put an example on the other side of the hinge;
  * under L1 no coordinate of any v within L1_CLEAR = 2e-6 of 0.  The fp32 error of a coordinate: h, t, r are exact inputs of size
    <= 1.25 / sqrt(d) typically and <= 1.25 always, three additions round to <= 3 x 2^-24 x 1.25 = 2.3e-7, alpha and beta are sums
    of d <= 256 products of total size <= 1.5625 with an error of a few 1e-7 at most, times |r_p[j]| <= 1.25: well below 1e-6 in
    all, so 2e-6 keeps every sign;
  * from B = 4 on active and inactive examples both occur (unless the case asks for one kind alone).
Offending examples are drawn again from the same generator, and an example of the missing kind is planted, for at most MAX_DRAWS
rounds per seed and MAX_DRAWS seeds; running out is an error of the construction.  Both are counted (DRAWS / ROUNDS).  All of this
happens before any launch."""
import os

import numpy as np
import torch

from oracle import cpu_ref as O
from tests._train_step_ref import MAX_DRAWS, DRAWS, ROUNDS, _note, _rows, _d, assert_row_norms, score_tol

NE, NR = 40, 3                                   # rows collide heavily
L1_CLEAR = 2e-6
TABLES = ('E', 'R', 'Ep', 'Rp')
LD = {'E': 'lde', 'R': 'ldr', 'Ep': 'ldep', 'Rp': 'ldrp'}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'transd.npz')


def tables(c):
    return {k: _d(c[k], c['d']) for k in TABLES}


def ids(c):
    """[pos ; neg] id arrays of the launch."""
    return torch.cat([c['h'], c['nh']]), torch.cat([c['t'], c['nt']]), torch.cat([c['r'], c['nr']])


def v_of(T, h, t, r):
    he, te = T['E'][h], T['E'][t]
    al, be = (he * T['Ep'][h]).sum(1, keepdim=True), (te * T['Ep'][t]).sum(1, keepdim=True)
    return (he - te) + T['R'][r] + (al - be) * T['Rp'][r]


def score(T, h, t, r, l1):
    v = v_of(T, h, t, r)
    return v.abs().sum(1) if l1 else (v * v).sum(1)


def _state(c, margins):
    """Per example: (offending, active under every margin, inactive under every margin)."""
    T = tables(c)
    B = c['B']
    h2, t2, r2 = ids(c)
    s = score(T, h2, t2, r2, c['l1'])
    pos, neg = s[:B], s[B:]
    bad = torch.zeros(B, dtype=torch.bool)
    for m in margins:
        bad |= (pos - neg + m).abs() < 10.0 * (score_tol(pos) + score_tol(neg))
    if c['l1']:
        near = v_of(T, h2, t2, r2).abs().min(dim=1).values < L1_CLEAR
        bad |= near[:B] | near[B:]
    return bad, (pos - neg + min(margins)) > 0, (pos - neg + max(margins)) < 0


def conditions(c, margins):
    """None if the case holds no knife edge and the kinds of example it should, else what fails."""
    bad, active, inactive = _state(c, margins)
    if bool(bad.any()):
        return 'a hinge argument within ten score tolerances of 0, or an L1 coordinate within %g of 0' % L1_CLEAR
    if c['only'] == 'inactive' and not bool(inactive.all()):
        return 'an active example in an all-inactive case'
    if c['only'] == 'active' and not bool(active.all()):
        return 'an inactive example in an all-active case'
    if c['only'] is None and c['B'] >= 4 and not (bool(active.any()) and bool(inactive.any())):
        return 'no active or no inactive example'
    return None


def _draw_entities(c, idx, gen):
    """(Re-)draw the entities of the examples `idx`: one triple in eight has h == t; a twin keeps its head or its tail and takes a
    uniform entity at the other end (which may be an entity of a positive triple, or make the twin the triple itself)."""
    n, ne = idx.numel(), c['ne']
    h, t = torch.randint(0, ne, (n,), generator=gen), torch.randint(0, ne, (n,), generator=gen)
    t = torch.where(torch.rand(n, generator=gen) < 0.125, h, t)
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


def case(d, B, l1, seed, margins=(1.0,), pitch=(0, 0, 0, 0), ne=NE, n_rel=NR, stray=(), only=None, zero_proj=False, family='transd'):
    """A TransD step case: fp32 tables E, Ep (ne rows) and R, Rp (n_rel rows) of pitch d + pitch[k] whose gaps hold junk, uniform
    relation ids, the twin's relation equal to its triple's except for the examples `stray`, which name the next relation.
    only: 'inactive' / 'active' -- every example must be of that kind (needs a margin the caller picked for it)."""
    for draw in range(MAX_DRAWS):
        gen = torch.Generator().manual_seed(1000003 * seed + draw)
        c = {'d': d, 'B': B, 'n_rel': n_rel, 'l1': bool(l1), 'ne': ne, 'only': only,
             'lde': d + pitch[0], 'ldr': d + pitch[1], 'ldep': d + pitch[2], 'ldrp': d + pitch[3]}
        c['E'], c['R'] = _rows(ne, d, c['lde'], gen), _rows(n_rel, d, c['ldr'], gen, 1)
        c['Ep'], c['Rp'] = _rows(ne, d, c['ldep'], gen, 1), _rows(n_rel, d, c['ldrp'], gen)
        if zero_proj:
            c['Ep'][:, :d] = 0.0
            c['Rp'][:, :d] = 0.0
        c['r'] = torch.randint(0, n_rel, (B,), generator=gen)
        c['nr'] = c['r'].clone()
        for k in stray:
            c['nr'][k] = (c['r'][k] + 1) % n_rel
        for k in ('h', 't', 'nh', 'nt'):
            c[k] = torch.zeros(B, dtype=torch.int64)
        _draw_entities(c, torch.arange(B), gen)
        done = False
        for rounds in range(MAX_DRAWS + 1):
            bad, active, inactive = _state(c, margins)
            lacks = []
            if only == 'inactive':
                bad = bad | ~inactive
            elif only == 'active':
                bad = bad | ~active
            elif B >= 4:
                lacks = [(0, False)] * (not bool(inactive.any())) + [(1, True)] * (not bool(active.any()))
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
    raise AssertionError('no admissible TransD case in %d draws: the construction is wrong' % MAX_DRAWS)


def loss_terms(c, T, margin, regs):
    """The loss slots 0, 2, 3 as graph nodes (None where `regs` switches one off)."""
    B = c['B']
    h2, t2, r2 = ids(c)
    s = score(T, h2, t2, r2, c['l1'])
    terms = [O.margin_loss(s[:B], s[B:], margin), None, None, None]
    if regs & 2:
        terms[2] = O.norm_loss(T['E'][torch.cat([c['h'], c['t'], c['nh'], c['nt']])])
    if regs & 4:
        terms[3] = O.norm_loss(T['R'][r2])
    return terms


def touched_rows(c, margin, regs):
    """{'E', 'R', 'Ep', 'Rp'}: bool per table row -- does the step add anything to that row of the gradient?  A row is touched by a
    triple of an ACTIVE example (fp64 hinge argument > 0: the entity rows of both ends in gE and gEp, the relation's row in gR and
    gRp) and, in gE / gR, by its regulariser where `regs` has it on and |row|^2 > 1.  Everything else keeps its content bit for bit.
    (Touched is not "the reference's row is non-zero": the halves of an example whose twin is the triple itself add +x and -x.)"""
    T = tables(c)
    B = c['B']
    h2, t2, r2 = ids(c)
    s = score(T, h2, t2, r2, c['l1'])
    act = (s[:B] - s[B:] + margin) > 0
    act2 = torch.cat([act, act])
    out = {k: torch.zeros(c['ne'] if k in ('E', 'Ep') else c['n_rel'], dtype=torch.bool) for k in TABLES}
    for k in ('E', 'Ep'):
        out[k][h2[act2]] = True
        out[k][t2[act2]] = True
    for k in ('R', 'Rp'):
        out[k][r2[act2]] = True
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
    """What ONE ktup_train_transd_step adds: ([4 loss slots, unscaled], {'E', 'R', 'Ep', 'Rp'}: gradients x gscale)."""
    T = {k: v.clone().requires_grad_(True) for k, v in tables(c).items()}
    terms = loss_terms(c, T, margin, regs)
    (gscale * sum(t for t in terms if t is not None)).backward()
    return [0.0 if t is None else float(t.detach()) for t in terms], \
        {k: (torch.zeros_like(v) if v.grad is None else v.grad) for k, v in T.items()}


_MEMO = {}


def reference_of(key, c, margin, gscale, regs):
    """reference() and touched_rows() of a shared case, computed once per (key, margin, gscale, regs) and never modified."""
    k = (key, margin, gscale, regs)
    if k not in _MEMO:
        _MEMO[k] = reference(c, margin, gscale, regs) + (touched_rows(c, margin, regs),)
    return _MEMO[k]


# ---------------------------------------------------------------------------------------------------- the reference's goldens
GOLDEN_NAMES = {'E': 'ent_embeddings.weight', 'R': 'rel_embeddings.weight', 'Ep': 'ent_proj_embeddings.weight', 'Rp': 'rel_proj_embeddings.weight'}


def golden_case(d, l1):
    """The step of tests/golden/transd.npz at width d as a case (contiguous tables, the twin's relation is the triple's; margin 1,
    regs 6, gscale 1) and its recorded results: ({'pos', 'neg', 'loss', 'grad': {table: array}})."""
    g = np.load(GOLDEN)
    pre = 'score.d%d.' % d
    tag = pre + ('L1.' if l1 else 'L2.')
    c = {'d': d, 'l1': bool(l1), 'only': None, 'lde': d, 'ldr': d, 'ldep': d, 'ldrp': d}
    for k, name in GOLDEN_NAMES.items():
        c[k] = torch.from_numpy(g[pre + name]).clone()
    for k, name in (('h', 'ph'), ('t', 'pt'), ('r', 'pr'), ('nh', 'nh'), ('nt', 'nt'), ('nr', 'pr')):
        c[k] = torch.from_numpy(g[pre + name]).clone()
    c['B'], c['ne'], c['n_rel'] = c['h'].numel(), c['E'].shape[0], c['R'].shape[0]
    want = {'pos': g[tag + 'pos'], 'neg': g[tag + 'neg'], 'loss': float(g[tag + 'loss'][0]),
            'grad': {k: g[tag + 'grad.' + name] for k, name in GOLDEN_NAMES.items()}}
    return c, want


# ---------------------------------------------------------------------------------------------------- the cases of the GPU test
WIDTHS = (4, 60, 64, 68, 100, 128, 132, 252, 256)
PITCHES = ((4, 4, 4, 4), (8, 4, 12, 4), (4, 8, 4, 12))
REGS = (6, 0, 2, 4)
GSCALES = (1.0, 0.5)
GRID_CAP = 1024                                  # launch_transd: at most 1024 workgroups, the rest by the grid-stride loop


def group_lanes(d):
    """Lanes per example, as the launch chooses them from d / 4."""
    return 16 if d <= 64 else 32 if d <= 128 else 64


def per_workgroup(d):
    return 256 // group_lanes(d)


def grid_specs():
    """d x l1 x B in full with B at the edges of the workgroup (G examples); regs, gscale and the pitches rotate at strides chosen so
    that every value of each meets every d and both distances.  Then one B beyond the grid cap at the widest group (d = 132, 256)."""
    out = []
    idx = 0
    for d in WIDTHS:
        G = per_workgroup(d)
        for l1 in (0, 1):
            for B in (1, G - 1, G, G + 1, 67):
                out.append(dict(d=d, l1=l1, B=B, pitch=PITCHES[idx % 3], regs=REGS[idx % 4], gscale=GSCALES[(idx // 2) % 2], seed=idx + 1))
                idx += 1
    for d in (132, 256):
        for l1 in (0, 1):
            out.append(dict(d=d, l1=l1, B=GRID_CAP * per_workgroup(d) + 3, pitch=PITCHES[idx % 3], regs=6, gscale=GSCALES[idx % 2], seed=idx + 1))
            idx += 1
    return out


def spec_id(s):
    return 'd%d-%s-B%d-p%d.%d.%d.%d-regs%d-g%s' % ((s['d'], 'L1' if s['l1'] else 'L2', s['B']) + tuple(s['pitch']) + (s['regs'], s['gscale']))


_CACHE = {}


def spec_case(s):
    """The (cached: built once, shared, never modified) case of a spec."""
    key = spec_id(s)
    if key not in _CACHE:
        _CACHE[key] = case(s['d'], s['B'], s['l1'], s['seed'], pitch=s['pitch'])
    return _CACHE[key]


INACTIVE_MARGIN, ACTIVE_MARGIN = -1.0e4, 1.0e4   # beyond every s+ - s- the small tables can produce


def inactive_case(d, l1, seed=83):
    return case(d, 20, l1, seed, margins=(INACTIVE_MARGIN,), pitch=(4, 4, 4, 4), only='inactive', family='transd_inactive')


def active_case(d, l1, seed=89):
    return case(d, 20, l1, seed, margins=(ACTIVE_MARGIN,), pitch=(4, 4, 4, 4), only='active', family='transd_active')


def stray_case(d, l1, seed=71):
    """B = 40 with six examples whose twin names another relation."""
    return case(d, 40, l1, seed, pitch=(4, 4, 4, 4), stray=(0, 3, 17, 18, 31, 39), family='transd_stray')


def zero_proj_case(d, l1, seed=97):
    """Zero Ep and Rp: TransD is TransE."""
    return case(d, 40, l1, seed, pitch=(4, 4, 4, 4), zero_proj=True, family='transd_zero')
