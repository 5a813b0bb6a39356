#!/usr/bin/env python3
"""Generate tests/golden/transd.npz and transd.json by IMPORTING THE REFERENCE (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_transd_goldens.py --ref <checkout of the reference> [--out DIR]

Data only: seeded tables and index batches, and what the reference's transD.py (class TransHModel there) computes from them.

  * score cases (d in 36, 50, 64, 100; L1 and squared L2) on the toy world of make_goldens.py (53 entities, 7 relations, B = 48),
    all four tables seeded non-zero with row norms spread around 1: pos / neg scores, the KG driver's loss line
    (marginLoss + normLoss(entity rows) + normLoss(relation rows), knowledge_representation.py:189-204) and the four gradients;
  * evaluateHead matrices from the reference.  evaluateTail of the reference raises NameError (transD.py:127 names
    `t_proj_expand`, which it never defines) -- asserted below and recorded in the JSON; the tail matrices come from the
    reference's own projection_transD_pytorch_samesize applied with the h_proj_expand that function builds and never uses;
  * a rank pass at d = 100 on 230 entities, head and tail, L1 and L2, filter lists and up to 3 golds per key, ranked by the
    reference's evalKGProcess (stable argsort, as make_goldens.py pins the tie rule).  NEAR-TIES ARE REMOVED FROM THE INPUT: each
    candidate key's row is evaluated in fp64 and the key is dropped when any gold's score lies within TIE_MARGIN x (the row's largest
    |score|) of another candidate's -- the reference's fp32 direct form errs by ~3e-7 x row maximum against fp64, the margin is
    ~15 x that.  The generator fails if more than 5 % of the keys are dropped; the dropped count is recorded;
  * the module surface of the reference's transD.py, read with ast.

The .npz is written with fixed zip timestamps, so that regenerating reproduces the committed bytes.
"""
import argparse
import ast
import io
import json
import os
import sys
import zipfile

import numpy as np

sys.dont_write_bytecode = True

ap = argparse.ArgumentParser()
ap.add_argument('--ref', required=True)
ap.add_argument('--out', default=os.path.dirname(os.path.abspath(__file__)))
args = ap.parse_args()
sys.path.insert(0, args.ref)

import warnings
warnings.filterwarnings('ignore')
import torch
from torch.autograd import Variable as V

from jTransUP.models import transD                      # the REFERENCE
from jTransUP.utils import loss as rloss
from jTransUP.utils import misc as rmisc

torch.set_num_threads(1)

NE, NR, B = 53, 7, 48                                   # make_goldens.py's toy world
TIE_MARGIN = 5e-6
MAX_DROP = 0.05


def npy(t):
    return t.detach().cpu().numpy().copy()


def save_npz(path, arrs):
    """np.savez_compressed with fixed member timestamps (numpy stamps the members with the clock)."""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrs):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrs[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def set_weights(model, gen):
    """Every table seeded non-zero (the reference zero-initialises the two projection tables: with zeros TransD is TransE), rows
    scaled to norms spread over 0.6 .. 1.4."""
    sd = {}
    for name, p in model.named_parameters():
        w = torch.randn(p.shape, generator=gen)
        w = w / w.norm(dim=1, keepdim=True) * (0.6 + 0.8 * torch.rand(p.shape[0], 1, generator=gen))
        p.data.copy_(w)
        sd[name] = npy(p.data)
    return sd


def tail_matrix(m, h, r):
    """evaluateTail as transD.py:107-134 evidently means it: its own lines with h_proj_expand where line 127 names t_proj_expand."""
    n = len(h)
    h_e, r_e = m.ent_embeddings(h), m.rel_embeddings(r)
    h_proj, r_proj = m.ent_proj_embeddings(h), m.rel_proj_embeddings(r)
    c_t_e = rmisc.projection_transD_pytorch_samesize(h_e, h_proj, r_proj) + r_e
    c_t_expand = c_t_e.expand(m.ent_total, n, m.embedding_size).permute(1, 0, 2)
    h_proj_expand = h_proj.expand(m.ent_total, n, m.embedding_size).permute(1, 0, 2)
    r_proj_expand = r_proj.expand(m.ent_total, n, m.embedding_size).permute(1, 0, 2)
    ent_expand = m.ent_embeddings.weight.expand(n, m.ent_total, m.embedding_size)
    proj_ent_expand = rmisc.projection_transD_pytorch_samesize(ent_expand, h_proj_expand, r_proj_expand)
    if m.L1_flag:
        return torch.sum(torch.abs(c_t_expand - proj_ent_expand), 2)
    return torch.sum((c_t_expand - proj_ent_expand) ** 2, 2)


def tail_raises_name_error():
    m = transD.TransHModel(False, 8, 5, 3)
    try:
        m.evaluateTail(V(torch.LongTensor([0, 1])), V(torch.LongTensor([0, 1])))
    except NameError:
        return True
    return False


def rows_fp64(sd, q, r, head, l1):
    """The score rows of keys (q, r) in fp64, direct form."""
    E, R = sd['ent_embeddings.weight'].astype(np.float64), sd['rel_embeddings.weight'].astype(np.float64)
    Ep, Rp = sd['ent_proj_embeddings.weight'].astype(np.float64), sd['rel_proj_embeddings.weight'].astype(np.float64)
    out = np.empty((len(q), E.shape[0]))
    for i, (qi, ri) in enumerate(zip(q, r)):
        a, b = Ep[qi], Rp[ri]
        c = E[qi] + E[qi].dot(a) * b + (-R[ri] if head else R[ri])
        z = c[None, :] - E - E.dot(a)[:, None] * b[None, :]
        out[i] = np.abs(z).sum(1) if l1 else (z * z).sum(1)
    return out


def score_cases(out, meta):
    rng = np.random.RandomState(211)
    gen = torch.Generator().manual_seed(223)
    for d in (36, 50, 64, 100):
        ph, pt, nh, nt = (torch.from_numpy(rng.randint(0, NE, B)).long() for _ in range(4))
        pr = torch.from_numpy(rng.randint(0, NR, B)).long()
        q = torch.from_numpy(rng.randint(0, NE, 16)).long()
        qr = torch.from_numpy(rng.randint(0, NR, 16)).long()
        pre = 'score.d%d.' % d
        out.update({pre + 'ph': npy(ph), pre + 'pt': npy(pt), pre + 'pr': npy(pr), pre + 'nh': npy(nh), pre + 'nt': npy(nt),
                    pre + 'q': npy(q), pre + 'qr': npy(qr)})
        keep = None
        for l1 in (True, False):
            m = transD.TransHModel(l1, d, NE, NR)
            if keep is None:
                sd = set_weights(m, gen)
                out.update({pre + k: v for k, v in sd.items()})
                keep = {k: p.data.clone() for k, p in m.named_parameters()}
            else:
                for k, p in m.named_parameters():
                    p.data.copy_(keep[k])
            tag = pre + ('L1.' if l1 else 'L2.')
            pos, neg = m(V(ph), V(pt), V(pr)), m(V(nh), V(nt), V(pr))
            loss = rloss.marginLoss()(pos, neg, 1.0)
            ent = m.ent_embeddings(V(torch.cat([ph, pt, nh, nt])))
            rel = m.rel_embeddings(V(torch.cat([pr, pr])))
            loss = loss + rloss.normLoss(ent) + rloss.normLoss(rel)        # no orthogonalLoss: TransH's only
            for p in m.parameters():
                p.grad = None
            loss.backward()
            out.update({tag + 'pos': npy(pos), tag + 'neg': npy(neg), tag + 'loss': npy(loss)})
            out.update({tag + 'grad.' + n: npy(p.grad) for n, p in m.named_parameters()})
            out[tag + 'eval_head'] = npy(m.evaluateHead(V(q), V(qr)))
            out[tag + 'eval_tail'] = npy(tail_matrix(m, V(q), V(qr)))
    meta['score'] = {'dims': [36, 50, 64, 100], 'margin': 1.0, 'n_ent': NE, 'n_rel': NR, 'batch': B}


def rank_cases(out, meta):
    rng = np.random.RandomState(227)
    gen = torch.Generator().manual_seed(229)
    NEk, d, NKEY = 230, 100, 160
    real_argsort = np.argsort
    np.argsort = lambda a, *aa, **kw: real_argsort(a, *aa, **dict(kw, kind='stable'))
    meta['rank'] = {'n_ent': NEk, 'd': d, 'tie_margin': TIE_MARGIN, 'cases': {}}
    try:
        keep = None
        for l1 in (True, False):
            m = transD.TransHModel(l1, d, NEk, NR)
            if keep is None:
                sd = set_weights(m, gen)
                out.update({'rank.' + k: v for k, v in sd.items()})
                keep = {k: p.data.clone() for k, p in m.named_parameters()}
            else:
                for k, p in m.named_parameters():
                    p.data.copy_(keep[k])
            for side in ('head', 'tail'):                               # head prediction: keys (t, r), golds are heads
                cand = []
                while len(cand) < NKEY:
                    k = (int(rng.randint(NEk)), int(rng.randint(NR)))
                    if k not in cand:
                        cand.append(k)
                eval_dict, train_dict, valid_dict = {}, {}, {}
                for k in cand:
                    perm = rng.permutation(NEk)
                    ng, nt, nv = rng.randint(1, 4), rng.randint(0, 12), rng.randint(0, 4)
                    eval_dict[k] = set(int(x) for x in perm[:ng])
                    if nt:
                        train_dict[k] = set(int(x) for x in perm[ng:ng + nt])
                    if nv:
                        valid_dict[k] = set(int(x) for x in perm[ng + nt:ng + nt + nv])
                # near-ties leave the input
                rows = rows_fp64(sd, [k[0] for k in cand], [k[1] for k in cand], side == 'head', l1)
                keys = []
                for k, row in zip(cand, rows):
                    tol = TIE_MARGIN * np.abs(row).max()
                    close = False
                    for g in eval_dict[k]:
                        gap = np.abs(row - row[g])
                        gap[g] = np.inf
                        close = close or bool(gap.min() <= tol)
                    if not close:
                        keys.append(k)
                dropped = len(cand) - len(keys)
                assert dropped <= MAX_DROP * len(cand), 'near-tie rule drops %d of %d keys (> 5 %%)' % (dropped, len(cand))
                for dct in (eval_dict, train_dict, valid_dict):
                    for k in list(dct):
                        if k not in keys:
                            del dct[k]
                results = []
                for b0 in range(0, len(keys), 16):                      # the eval iterator's batches
                    batch = keys[b0:b0 + 16]
                    e = V(torch.LongTensor([k[0] for k in batch]))
                    r = V(torch.LongTensor([k[1] for k in batch]))
                    scores = m.evaluateHead(e, r) if side == 'head' else tail_matrix(m, e, r)
                    preds = zip(batch, scores.data.cpu().numpy())
                    results.extend(rmisc.evalKGProcess(list(preds), eval_dict, all_dicts=[train_dict, valid_dict], descending=False,
                                                       num_processes=2, topn=10, queue_limit=10))
                results = sorted((tuple(int(x) for x in r[2]), int(r[3]), int(r[1]), int(r[0])) for r in results)   # worker order is arbitrary
                perf = np.array([[r[3], r[2]] for r in results], dtype=np.float64)
                ser = lambda dct: [[k[0], k[1], sorted(v)] for k, v in sorted(dct.items())]
                meta['rank']['cases']['%s.%s' % ('L1' if l1 else 'L2', side)] = {
                    'keys': [list(k) for k in keys], 'eval': ser(eval_dict), 'train': ser(train_dict), 'valid': ser(valid_dict),
                    'rows': [[r[0][0], r[0][1], r[1], r[2], r[3]] for r in results],       # entity, relation, gold id, filtered rank, hit
                    'mean': [float(x) for x in perf.mean(axis=0)],
                    'candidate_keys': len(cand), 'dropped_near_ties': dropped}
    finally:
        np.argsort = real_argsort


def surface(path):
    """Top-level functions and the classes' public methods (+ __init__) with their argument names; nothing is executed."""
    tree = ast.parse(open(path).read())
    names = lambda fn: [a.arg for a in fn.args.args]
    funcs, classes = {}, {}
    for node in tree.body:
        if isinstance(node, ast.FunctionDef):
            funcs[node.name] = names(node)
        elif isinstance(node, ast.ClassDef):
            classes[node.name] = {f.name: names(f) for f in node.body
                                  if isinstance(f, ast.FunctionDef) and (not f.name.startswith('_') or f.name == '__init__')}
    return {'functions': funcs, 'classes': classes}


def main():
    out, meta = {}, {}
    assert tail_raises_name_error(), "the reference's transD.evaluateTail no longer raises NameError: regenerate from its own matrices"
    meta['reference_evaluateTail_raises_NameError'] = True
    score_cases(out, meta)
    rank_cases(out, meta)
    meta['surface'] = surface(os.path.join(args.ref, 'jTransUP', 'models', 'transD.py'))
    path = os.path.join(args.out, 'transd.npz')
    save_npz(path, out)
    with open(os.path.join(args.out, 'transd.json'), 'w') as f:
        json.dump(meta, f, indent=0, sort_keys=True)
    print('transd.npz %.1f KB (%d arrays), transd.json %.1f KB' % (os.path.getsize(path) / 1024, len(out),
                                                                 os.path.getsize(os.path.join(args.out, 'transd.json')) / 1024))
    for k, c in sorted(meta['rank']['cases'].items()):
        print('rank %-8s keys %d dropped %d' % (k, len(c['keys']), c['dropped_near_ties']))


if __name__ == '__main__':
    main()
