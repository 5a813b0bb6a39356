"""TransD on the GPU, through the C ABI (jTransUP.hip.ops / lib): the reference's recorded outputs (tests/golden/transd.npz, written
by tests/golden/make_transd_goldens.py), both evaluation routes against each other, seeded shapes against an fp64 restatement of the
formulas, the KG stepper against the autograd route, and the command line.

Tolerances.  Against the goldens: scores rtol 1e-4 / atol 1e-5 and gradients atol 3e-5 (the RT, AT, GAT of tests/test_hip_score.py),
loss rtol 1e-4, evaluation matrices rtol 1e-4 / atol 1e-5 (what tests/test_hip_eval.py applies to TransH's), ranks exact.  Against
fp64 on seeded shapes the same bars, with the floor test_hip_score.py gives to gradients that are fp32 sums over a batch
(atol = max(3e-5, 2e-6 x the largest gradient entry): a row listed thousands of times accumulates thousands of roundings of 6e-8
relative each, in an order the atomics choose)."""
import copy
import json
import logging
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.synth import make_dataset

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'joint-kg-recommender_amd')
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
RT, AT, GAT = 1e-4, 1e-5, 3e-5
NAMES = ('ent_embeddings.weight', 'rel_embeddings.weight', 'ent_proj_embeddings.weight', 'rel_proj_embeddings.weight')


def ops():
    from jTransUP.hip import ops as o
    return o


def close(got, want, rtol=RT, atol=AT, what=''):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    want = want.detach().cpu().numpy() if torch.is_tensor(want) else np.asarray(want)
    err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max()) if got.size else 0.0
    print('%-60s max|diff| %.3e  (max|want| %.3e)' % (what, err, float(np.abs(want).max()) if want.size else 0.0))
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol, err_msg=what)


class eval_mc(object):
    """The library's `eval_mc` option for the span of a `with`: 0 forces the pair route."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        from jTransUP.hip import lib as L
        self.old = L.set_option('eval_mc', self.value)

    def __exit__(self, *exc):
        from jTransUP.hip import lib as L
        L.set_option('eval_mc', self.old)


# ------------------------------------------------------------------------------------------------ fp64 restatement (from the formulas)
def ref_score(E, R, Ep, Rp, h, t, r, l1):
    he, te = E[h], E[t]
    hp = he + (he * Ep[h]).sum(1, keepdim=True) * Rp[r]
    tp = te + (te * Ep[t]).sum(1, keepdim=True) * Rp[r]
    v = hp + R[r] - tp
    return v.abs().sum(1) if l1 else (v * v).sum(1)


def ref_eval(E, R, Ep, Rp, q, r, l1, head, C=None):
    C = E if C is None else C
    a, b = Ep[q], Rp[r]
    qp = E[q] + (E[q] * a).sum(1, keepdim=True) * b
    c = qp - R[r] if head else qp + R[r]
    z = c[:, None, :] - C[None, :, :] - (C @ a.t()).t()[:, :, None] * b[:, None, :]
    return z.abs().sum(2) if l1 else (z * z).sum(2)


def seeded_tables(ne, nr, d, seed, pitch=None, zero_proj=False):
    """fp32 tables on the device (row norms ~ 0.5 .. 1.5) -> (E, R, Ep, Rp); pitch > d: rows of a wider buffer (non-contiguous rows)."""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for k, rows in enumerate((ne, nr, ne, nr)):
        w = torch.randn(rows, d, generator=gen)
        w = w / w.norm(dim=1, keepdim=True) * (0.5 + torch.rand(rows, 1, generator=gen))
        if zero_proj and k >= 2:
            w.zero_()
        if pitch:
            buf = torch.zeros(rows, pitch[k % len(pitch)], device=DEV)
            buf[:, :d] = w.to(DEV)
            out.append(buf[:, :d])
        else:
            out.append(w.to(DEV))
    return out[0], out[1], out[2], out[3]


# ------------------------------------------------------------------------------------------------ goldens
@pytest.mark.parametrize('d', [36, 50, 64, 100])
@pytest.mark.parametrize('l1', [True, False])
def test_scores_loss_and_gradients_match_the_reference(d, l1):
    from jTransUP.utils import loss
    g = np.load(os.path.join(GOLDEN, 'transd.npz'))
    pre = 'score.d%d.' % d
    tag = pre + ('L1.' if l1 else 'L2.')
    W = [torch.from_numpy(g[pre + n]).to(DEV).requires_grad_(True) for n in NAMES]
    E, R, Ep, Rp = W
    ids = lambda n: torch.from_numpy(g[pre + n]).to(DEV)
    ph, pt, pr, nh, nt = ids('ph'), ids('pt'), ids('pr'), ids('nh'), ids('nt')
    pos, neg = ops().score_transd(E, R, Ep, Rp, ph, pt, pr, l1), ops().score_transd(E, R, Ep, Rp, nh, nt, pr, l1)
    close(pos, g[tag + 'pos'], what=tag + 'pos'); close(neg, g[tag + 'neg'], what=tag + 'neg')
    total = loss.marginLoss()(pos, neg, 1.0) + loss.normLoss(E, ids=torch.cat([ph, pt, nh, nt])) + loss.normLoss(R, ids=torch.cat([pr, pr]))
    close(total, g[tag + 'loss'], rtol=1e-4, atol=0, what=tag + 'loss')
    total.backward()
    for w, n in zip(W, NAMES):
        close(w.grad, g[tag + 'grad.' + n], atol=GAT, what=tag + 'grad.' + n)


@pytest.mark.parametrize('d', [36, 50, 64, 100])
@pytest.mark.parametrize('l1', [True, False])
def test_evaluation_matrices_match_the_reference_on_both_routes(d, l1):
    g = np.load(os.path.join(GOLDEN, 'transd.npz'))
    pre = 'score.d%d.' % d
    tag = pre + ('L1.' if l1 else 'L2.')
    E, R, Ep, Rp = (torch.from_numpy(g[pre + n]).to(DEV) for n in NAMES)
    q, r = torch.from_numpy(g[pre + 'q']).to(DEV), torch.from_numpy(g[pre + 'qr']).to(DEV)
    for head in (True, False):
        want = g[tag + ('eval_head' if head else 'eval_tail')]
        got = ops().eval_transd(E, R, Ep, Rp, q, r, l1, head)
        close(got, want, what=tag + ('head' if head else 'tail') + ' default route')
        with eval_mc(0):
            pair = ops().eval_transd(E, R, Ep, Rp, q, r, l1, head)
        close(pair, want, what=tag + ('head' if head else 'tail') + ' pair route')
        close(got, pair, what=tag + ('head' if head else 'tail') + ' default vs pair route')


def _rank_case(S):
    keys = [(int(e), int(r)) for e, r in S['keys']]
    gold = {(int(e), int(r)): sorted(v) for e, r, v in S['eval']}
    filt = {}
    for k in ('train', 'valid'):
        for e, r, v in S[k]:
            filt.setdefault((int(e), int(r)), set()).update(v)
    want = {(int(e), int(r), int(gid)): int(rank) for e, r, gid, rank, hit in S['rows']}
    g_off, g_ids, f_off, f_ids, expect = [0], [], [0], [], []
    for k in keys:
        g_ids += gold[k]; g_off.append(len(g_ids))
        f_ids += sorted(filt.get(k, ())); f_off.append(len(f_ids))
        expect += [want[k + (gid,)] for gid in gold[k]]
    dv = lambda a, dt: torch.tensor(a, dtype=dt, device=DEV)
    return (dv([k[0] for k in keys], torch.int64), dv([k[1] for k in keys], torch.int64), dv(g_off, torch.int64), dv(g_ids, torch.int32),
            dv(f_off, torch.int64), dv(f_ids, torch.int32), expect, S['mean'])


@pytest.mark.parametrize('l1', [True, False])
@pytest.mark.parametrize('side', ['head', 'tail'])
def test_rank_pass_reproduces_the_reference_pass_on_every_route(l1, side):
    """Every filtered rank of the pass equals the reference's integer (near-ties were removed from the fixture's input, see the
    generator): matrix-core route (squared L2), pair route, a chunk size that does not divide the keys, the model's rank_entities."""
    from jTransUP.models import transD
    g = np.load(os.path.join(GOLDEN, 'transd.npz'))
    J = json.load(open(os.path.join(GOLDEN, 'transd.json')))['rank']
    case = J['cases']['%s.%s' % ('L1' if l1 else 'L2', side)]
    assert case['dropped_near_ties'] <= 0.05 * case['candidate_keys']
    E, R, Ep, Rp = (torch.from_numpy(g['rank.' + n]).to(DEV) for n in NAMES)
    q, r, g_off, g_ids, f_off, f_ids, expect, mean = _rank_case(case)
    head = side == 'head'
    runs = {}
    runs['default chunk 16'] = ops().eval_kg_ranks_transd(E, R, Ep, Rp, q, r, l1, head, False, g_off, g_ids, f_off, f_ids, chunk=16)
    runs['default chunk 50'] = ops().eval_kg_ranks_transd(E, R, Ep, Rp, q, r, l1, head, False, g_off, g_ids, f_off, f_ids, chunk=50)
    runs['default one chunk'] = ops().eval_kg_ranks_transd(E, R, Ep, Rp, q, r, l1, head, False, g_off, g_ids, f_off, f_ids)
    with eval_mc(0):
        runs['pair route chunk 16'] = ops().eval_kg_ranks_transd(E, R, Ep, Rp, q, r, l1, head, False, g_off, g_ids, f_off, f_ids, chunk=16)
    m = transD.TransDModel(l1, E.shape[1], E.shape[0], R.shape[0])
    m.load_state_dict({n: w for n, w in zip(NAMES, (E, R, Ep, Rp))})
    runs['rank_entities'] = m.rank_entities(q, r, head, False, g_off, g_ids, f_off, f_ids)
    for name, ranks in runs.items():
        got = ranks.cpu().numpy()[:len(expect)].astype(np.int64)
        wrong = int((got != np.asarray(expect)).sum())
        print('%s %s %-20s %d of %d ranks differ' % ('L1' if l1 else 'L2', side, name, wrong, len(expect)))
        assert got.tolist() == expect, name
        np.testing.assert_allclose([float((got < 10).mean()), float(got.mean())], mean, rtol=1e-12)


# ------------------------------------------------------------------------------------------------ seeded shapes against fp64
def _draw_triples(E, R, Ep, Rp, ne, nr, n, l1, gen, margin=1e-6):
    """n seeded triples.  The L1 gradient is sign(v), discontinuous at v = 0: a coordinate of v that fp64 puts within fp32's rounding of
    zero (|v| ~ 0.1, so ~1e-8) may come out on the other side in fp32, and that ONE sign moves gamma = g . r_p and with it four whole
    gradient rows.  Such triples are removed from the INPUT (any |v_k| < 1e-6 in fp64, ~100 x the rounding: about 0.3 % of the
    triples at d = 300), not tolerated in the output; the batch keeps exactly n triples."""
    m = n + 64 + n // 20
    h, t, r = torch.randint(0, ne, (m,), generator=gen), torch.randint(0, ne, (m,), generator=gen), torch.randint(0, nr, (m,), generator=gen)
    if l1:
        W = [w.detach().cpu().double() for w in (E, R, Ep, Rp)]
        he, te = W[0][h], W[0][t]
        v = (he + (he * W[2][h]).sum(1, keepdim=True) * W[3][r]) + W[1][r] - (te + (te * W[2][t]).sum(1, keepdim=True) * W[3][r])
        keep = v.abs().min(dim=1).values >= margin
        h, t, r = h[keep], t[keep], r[keep]
    assert h.numel() >= n
    return h[:n].contiguous(), t[:n].contiguous(), r[:n].contiguous()


@pytest.mark.parametrize('n', [1, 17, 300, 8192])
@pytest.mark.parametrize('d', [20, 36, 100, 128, 256, 300])
@pytest.mark.parametrize('l1', [True, False])
def test_score_and_gradients_on_seeded_shapes(n, d, l1):
    """Ragged batches, every width class (16 / 32 / 64 lanes per triple, one and several chunks per lane), ids drawn from few rows
    (n = 8192 on 90 entities: every row is listed ~180 times -- gradient accumulation)."""
    ne, nr = 90, 7
    E, R, Ep, Rp = (w.requires_grad_(True) for w in seeded_tables(ne, nr, d, 100 + d))
    gen = torch.Generator().manual_seed(n + d)
    h, t, r = _draw_triples(E, R, Ep, Rp, ne, nr, n, l1, gen)
    gs = torch.randn(n, generator=gen)
    s = ops().score_transd(E, R, Ep, Rp, h.to(DEV), t.to(DEV), r.to(DEV), l1)
    s.backward(gs.to(DEV))
    W64 = [w.detach().cpu().double().requires_grad_(True) for w in (E, R, Ep, Rp)]
    s64 = ref_score(*W64, h, t, r, l1)
    s64.backward(gs.double())
    tag = 'n=%d d=%d %s ' % (n, d, 'L1' if l1 else 'L2')
    close(s, s64.detach().float(), what=tag + 'score')
    for w, w64, name in zip((E, R, Ep, Rp), W64, NAMES):
        want = w64.grad.float()
        close(w.grad, want, atol=max(GAT, 2e-6 * float(want.abs().max())), what=tag + 'grad ' + name)


@pytest.mark.parametrize('d', [50, 100])
@pytest.mark.parametrize('l1', [True, False])
def test_strided_tables_and_repeated_ids(d, l1):
    """Tables that are column slices of wider buffers (row pitch > d; pitches 4 k + 1 / 4 k + 2 take the 4-byte lanes, pitch 4 k the
    16-byte ones at d = 100) and a batch that lists ONE triple 65 times among others."""
    ne, nr, n = 40, 5, 200
    for pitch in ((d + 1, d + 2), (d + 4, d + 8)):
        E, R, Ep, Rp = (w.requires_grad_(True) for w in seeded_tables(ne, nr, d, 7 + d, pitch=pitch))
        assert E.stride(0) == pitch[0] and not E.is_contiguous()
        gen = torch.Generator().manual_seed(d)
        h, t, r = _draw_triples(E, R, Ep, Rp, ne, nr, n, l1, gen)
        h[:64], t[:64], r[:64] = h[70], t[70], r[70]
        gs = torch.randn(n, generator=gen)
        s = ops().score_transd(E, R, Ep, Rp, h.to(DEV), t.to(DEV), r.to(DEV), l1)
        s.backward(gs.to(DEV))
        W64 = [w.detach().cpu().double().requires_grad_(True) for w in (E, R, Ep, Rp)]
        s64 = ref_score(*W64, h, t, r, l1)
        s64.backward(gs.double())
        tag = 'pitch=%s d=%d %s ' % (pitch, d, 'L1' if l1 else 'L2')
        close(s, s64.detach().float(), what=tag + 'score')
        for w, w64, name in zip((E, R, Ep, Rp), W64, NAMES):
            want = w64.grad.float()
            assert w.grad.shape == w.shape
            close(w.grad, want, atol=max(GAT, 2e-6 * float(want.abs().max())), what=tag + 'grad ' + name)
        q, qr = torch.randint(0, ne, (9,), generator=gen), torch.randint(0, nr, (9,), generator=gen)
        for head in (True, False):
            got = ops().eval_transd(E.detach(), R.detach(), Ep.detach(), Rp.detach(), q.to(DEV), qr.to(DEV), l1, head)
            want = ref_eval(*[w.detach() for w in W64], q, qr, l1, head).float()
            close(got, want, what=tag + 'eval head=%s' % head)


@pytest.mark.parametrize('d', [36, 100])
@pytest.mark.parametrize('l1', [True, False])
def test_zero_projection_tables_make_transd_transe(d, l1):
    """The reference's initial state: with Ep = Rp = 0 every projection is the identity."""
    ne, nr, n = 60, 6, 300
    E, R, Ep, Rp = seeded_tables(ne, nr, d, 3, zero_proj=True)
    gen = torch.Generator().manual_seed(5)
    h, t, r = (torch.randint(0, hi, (n,), generator=gen).to(DEV) for hi in (ne, ne, nr))
    close(ops().score_transd(E, R, Ep, Rp, h, t, r, l1), ops().score_transe(E, R, h, t, r, l1), what='score vs TransE')
    for head in (True, False):
        close(ops().eval_transd(E, R, Ep, Rp, h[:40], r[:40], l1, head), ops().eval_transe(E, R, h[:40], r[:40], l1, head),
              what='eval vs TransE head=%s' % head)


@pytest.mark.parametrize('d', [20, 36, 64, 100, 128, 256, 300])
@pytest.mark.parametrize('l1', [True, False])
def test_evaluation_on_seeded_shapes_and_a_candidate_slice(d, l1):
    """Key counts and candidate counts that are not multiples of the tiles (64 x 64), every matrix-core width and the widths that
    only the pair route serves, both routes, and a candidate slice E[lo:hi] (sharded-candidate evaluation)."""
    ne, nr, nq = 333, 6, 71
    E, R, Ep, Rp = seeded_tables(ne, nr, d, 40 + d)
    gen = torch.Generator().manual_seed(d)
    q, r = torch.randint(0, ne, (nq,), generator=gen), torch.randint(0, nr, (nq,), generator=gen)
    W64 = [w.cpu().double() for w in (E, R, Ep, Rp)]
    for head in (True, False):
        want = ref_eval(*W64, q, r, l1, head).float()
        tag = 'd=%d %s head=%s ' % (d, 'L1' if l1 else 'L2', head)
        got = ops().eval_transd(E, R, Ep, Rp, q.to(DEV), r.to(DEV), l1, head)
        close(got, want, what=tag + 'default route')
        with eval_mc(0):
            pair = ops().eval_transd(E, R, Ep, Rp, q.to(DEV), r.to(DEV), l1, head)
        close(pair, want, what=tag + 'pair route')
        close(got, pair, what=tag + 'default vs pair')
        lo, hi = 70, 201
        part = ops().eval_transd(E, R, Ep, Rp, q.to(DEV), r.to(DEV), l1, head, candidates=E[lo:hi])
        assert tuple(part.shape) == (nq, hi - lo)
        close(part, want[:, lo:hi], what=tag + 'candidate slice')


@pytest.mark.parametrize('l1', [True, False])
def test_ml1m_size_matrix(l1):
    """512 keys x 14,709 entities at d = 100 (one chunk of the ml1m link-prediction pass)."""
    ne, nr, nq, d = 14709, 20, 512, 100
    E, R, Ep, Rp = seeded_tables(ne, nr, d, 77)
    gen = torch.Generator().manual_seed(78)
    q, r = torch.randint(0, ne, (nq,), generator=gen), torch.randint(0, nr, (nq,), generator=gen)
    got = ops().eval_transd(E, R, Ep, Rp, q.to(DEV), r.to(DEV), l1, True)
    W64 = [w.double() for w in (E, R, Ep, Rp)]                     # (fp64 torch on the device: the restatement, not the code under test)
    want = torch.cat([ref_eval(*W64, q[s:s + 64].to(DEV), r[s:s + 64].to(DEV), l1, True) for s in range(0, nq, 64)]).float()
    close(got, want, what='ml1m-size %s' % ('L1' if l1 else 'L2'))
    if not l1:
        with eval_mc(0):
            pair = ops().eval_transd(E, R, Ep, Rp, q.to(DEV), r.to(DEV), l1, True)
        close(pair, want, what='ml1m-size L2 pair route')


def test_kg_shard_fn_serves_transd():
    """-shard_eval_candidates: the slice scores of models/_shard_eval.kg_shard_fn are the columns of the whole matrix."""
    from jTransUP.models import transD
    from jTransUP.models._shard_eval import kg_shard_fn
    E, R, Ep, Rp = seeded_tables(150, 5, 36, 21)
    m = transD.TransDModel(True, 36, 150, 5)
    m.load_state_dict({n: w for n, w in zip(NAMES, (E, R, Ep, Rp))})
    q, r = torch.arange(0, 40, device=DEV), torch.arange(0, 40, device=DEV) % 5
    for head in (True, False):
        n_cand, f = kg_shard_fn(m, head)
        assert n_cand == 150
        whole = m.evaluateHead(q, r) if head else m.evaluateTail(q, r)
        assert torch.equal(torch.cat([f(q, r, 0, 70), f(q, r, 70, 150)], dim=1), whole)


# ------------------------------------------------------------------------------------------------ the stepper
def _trainer_for(tmp_path, model, optimizer):
    from jTransUP.models.base import get_flags
    from jTransUP.utils.flags import FLAGS
    from jTransUP.utils.trainer import ModelTrainer
    get_flags(); FLAGS.reset()
    FLAGS(['prog', '-model_type', 'transd', '-log_path', str(tmp_path), '-experiment_name', 'st', '-optimizer_type', optimizer,
           '-learning_rate', '0.05'])
    FLAGS.ckpt_path = str(tmp_path)
    return FLAGS, ModelTrainer(model, logging.getLogger('st'), 10, FLAGS)


@pytest.mark.parametrize('graphs', [False, True])
@pytest.mark.parametrize('D,l1', [(36, False), (100, True)])
def test_kg_stepper_matches_the_autograd_route(tmp_path, D, l1, graphs):
    """20 steps of KGStepper on a TransD model equal 20 steps of the autograd route on a copy (tests/test_fast_train.py's criterion for
    TransR), launched one by one and replayed from a captured graph.  The projection tables start non-zero: at the reference's
    zero initialisation their gradients vanish identically and the comparison would not see them."""
    from jTransUP.models import transD
    from jTransUP.utils import loss
    from jTransUP.utils.fast_train import KGStepper
    STRAY_CAP = 2.1 * 0.05
    NE, NR, B = 70, 6, 64
    torch.manual_seed(4)
    m1 = transD.TransDModel(l1, D, NE, NR)
    with torch.no_grad():
        m1.ent_proj_embeddings.weight.copy_(torch.randn(NE, D) * 0.2)
        m1.rel_proj_embeddings.weight.copy_(torch.randn(NR, D) * 0.2)
    m2 = transD.TransDModel(l1, D, NE, NR)
    m2.load_state_dict(copy.deepcopy(m1.state_dict()))
    FLAGS, tr1 = _trainer_for(tmp_path, m1, 'SGD')
    _, tr2 = _trainer_for(tmp_path, m2, 'SGD')
    fast = KGStepper(m2, tr2, FLAGS, B, use_graphs=graphs)
    assert fast.transd and not fast.transh and not fast.transr
    gen = torch.Generator().manual_seed(9)
    rnd = lambda hi: torch.randint(0, hi, (B,), generator=gen).to(DEV)
    start = copy.deepcopy(m1.state_dict())
    for step in range(20):
        ph, pt, pr, nh, nt = rnd(NE), rnd(NE), rnd(NR), rnd(NE), rnd(NE)
        tr1.optimizer_zero_grad()
        losses = loss.marginLoss()(m1(ph, pt, pr), m1(nh, nt, pr), FLAGS.margin)
        rel_ids = torch.cat([pr, pr])
        losses = losses + loss.normLoss(m1.ent_embeddings.weight, ids=torch.cat([ph, pt, nh, nt])) \
            + loss.normLoss(m1.rel_embeddings.weight, ids=rel_ids)
        losses.backward()
        tr1.clip_and_step(FLAGS.clipping_max_value)
        fast_loss = fast.kg_step(ph, pt, pr, nh, nt, pr)
        torch.testing.assert_close(fast_loss, losses.detach(), rtol=1e-5, atol=1e-6)
        for (k, a), (_, b) in zip(m1.state_dict().items(), m2.state_dict().items()):
            err = (b - a).abs()
            bad = err > 2e-6 + 2e-5 * a.abs()
            assert float(bad.float().mean()) <= 2e-3 and float(err.max()) <= STRAY_CAP, \
                '%s after step %d: %d elements off, max %.3g' % (k, step, int(bad.sum()), float(err.max()))
    assert fast.fused_step is False
    assert bool(fast._graphs) == graphs
    for k, a in m1.state_dict().items():                         # every table trained, the projection tables included
        assert float((a - start[k]).abs().max()) > 1e-4, k


# ------------------------------------------------------------------------------------------------ the command line
def run_cli(tmp, name, extra, env=None):
    data = str(tmp)
    logs = os.path.join(data, 'log')
    os.makedirs(logs, exist_ok=True)
    cmd = [sys.executable, os.path.join(PKG, 'run_knowledge_representation.py'), '-data_path', data, '-log_path', logs, '-dataset', 'ml1m',
           '-experiment_name', name, '-nohas_visualization', '-batch_size', '32', '-embedding_size', '20', '-seed', '3',
           '-eval_interval_steps', '10', '-training_steps', '25', '-early_stopping_steps_to_wait', '0', '-learning_rate', '0.05',
           '-topn', '10', '-model_type', 'transd'] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return open(os.path.join(logs, name + '.log')).read(), logs


@pytest.fixture(scope='module')
def dataset(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('ds')
    make_dataset(str(tmp))
    return tmp


METRIC = r'avg hit:(\d\.\d+), avg mean rank:(\d+\.\d+), topn:10'


def test_cli_trains_evaluates_and_reloads(dataset):
    log, logs = run_cli(dataset, 'kg-transd', ['-kg_test_files', 'valid.dat:test.dat'])
    rows = re.findall(METRIC, log)
    assert len(rows) >= 6                                               # 3 evaluations x 2 files
    assert 'GPU-resident training step enabled' in log and 'device-resident' in log
    assert 'train loss:' in log and os.path.isfile(os.path.join(logs, 'kg-transd.ckpt_final'))
    # the checkpoint the run wrote last, evaluated alone, reproduces the numbers of the evaluation that wrote it
    ckpt = os.path.join(logs, 'kg-transd.ckpt')
    assert os.path.isfile(ckpt)
    sd = torch.load(ckpt, map_location='cpu', weights_only=False)
    best_step = int(sd['step'])
    log2, _ = run_cli(dataset, 'kg-transd-eval', ['-kg_test_files', 'valid.dat:test.dat', '-eval_only_mode', '-load_experiment_name', ckpt])
    assert 'Found checkpoint, restoring.' in log2
    rows2 = re.findall(METRIC, log2)
    assert len(rows2) == 2
    # the evaluations run at steps 0, 10, 20: rows 2 k, 2 k + 1 belong to step 10 k
    k = best_step // 10
    assert rows[2 * k:2 * k + 2] == rows2, (best_step, rows, rows2)


@pytest.mark.parametrize('mode', ['host_sampling', 'autograd', 'l1'])
def test_cli_training_routes(dataset, mode):
    extra, env = ['-kg_test_files', 'valid.dat'], None
    if mode == 'host_sampling':
        extra.append('-nodevice_sampling')
    elif mode == 'autograd':
        env = {'KTUP_FAST_TRAIN': '0'}
    else:
        extra.append('-L1_flag')
    log, logs = run_cli(dataset, 'kg-transd-' + mode, extra, env)
    assert len(re.findall(METRIC, log)) >= 3
    assert ('GPU-resident training step enabled' in log) == (mode != 'autograd')
    assert ('device-resident' in log) == (mode == 'l1')
    assert os.path.isfile(os.path.join(logs, 'kg-transd-%s.ckpt_final' % mode))
