"""Recorded reference integers for TransR's link-prediction pass (tests/test_hip_transr_pass.py).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_transr_pass_goldens.py --ref <checkout of the reference> [--out DIR] [--tie-margin M]

Data only: seeded tables and evaluation dictionaries, and what the reference computes from them -- its TransRModel.evaluateHead /
evaluateTail (transR.py:80-128) per batch of 16 keys and its own filtered rank walk (utils/misc.py:61-146 evalKGProcess, stable
argsort as make_goldens.py pins the tie rule).  230 entities, 5 relations, d = 64 (no tail MFMA on the matrix-core route) and d = 100
(the b32 tail), L1 and squared L2, head and tail, filter lists (train + valid) and up to 3 golds per key.

NEAR-TIES ARE REMOVED FROM THE INPUT by make_transd_goldens.py's rule: each candidate key's row is evaluated in fp64 (direct form) and
the key is dropped when any gold's score lies within TIE_MARGIN x (the row's largest |score|) of another candidate's; at most 5 % of
the candidate keys may go (asserted here).  The margin starts from TransD's 5e-6 and is validated against the CHUNKED route
(ops.eval_kg_ranks_transr(fused=False)) only; the json records the margin and the dropped counts."""
import argparse
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
ap.add_argument('--tie-margin', type=float, default=5e-6)
args = ap.parse_args()
sys.path.insert(0, args.ref)

import warnings
warnings.filterwarnings('ignore')
import torch
from torch.autograd import Variable as V

from jTransUP.models import transR                      # the REFERENCE
from jTransUP.utils import misc as rmisc

torch.set_num_threads(1)

NE, NR, NKEY = 230, 5, 120
TIE_MARGIN = args.tie_margin
MAX_DROP = 0.05
NAMES = ('ent_embeddings.weight', 'rel_embeddings.weight', 'proj_embeddings.weight')


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


def set_weights(model, d, gen):
    """Entity and relation rows with norms spread over 0.6 .. 1.4; projection matrices N(0, 1/d) so that |M e| stays O(|e|)."""
    sd = {}
    for name, p in model.named_parameters():
        w = torch.randn(p.shape, generator=gen)
        if name.startswith('proj'):
            w = w / float(np.sqrt(d))
        else:
            w = w / w.norm(dim=1, keepdim=True) * (0.6 + 0.8 * torch.rand(p.shape[0], 1, generator=gen))
        p.data.copy_(w)
        sd[name + '.weight' if not name.endswith('.weight') else name] = npy(p.data)
    return sd


def rows_fp64(sd, q, r, head, l1):
    """The score rows of keys (q, r) in fp64, direct form: dist(M_r e_q -+ r - M_r e) over every entity e."""
    E, R, M = (sd[n].astype(np.float64) for n in NAMES)
    d = E.shape[1]
    out = np.empty((len(q), E.shape[0]))
    for i, (qi, ri) in enumerate(zip(q, r)):
        Mr = M[ri].reshape(d, d)
        c = Mr.dot(E[qi]) + (-R[ri] if head else R[ri])
        z = c[None, :] - E.dot(Mr.T)
        out[i] = np.abs(z).sum(1) if l1 else (z * z).sum(1)
    return out


def rank_cases(out, meta):
    rng = np.random.RandomState(331)
    gen = torch.Generator().manual_seed(337)
    real_argsort = np.argsort
    np.argsort = lambda a, *aa, **kw: real_argsort(a, *aa, **dict(kw, kind='stable'))
    meta.update({'n_ent': NE, 'n_rel': NR, 'dims': [64, 100], 'tie_margin': TIE_MARGIN, 'max_dropped_share': MAX_DROP, 'cases': {}})
    try:
        for d in (64, 100):
            keep = None
            for l1 in (True, False):
                m = transR.TransRModel(l1, d, NE, NR)
                if keep is None:
                    sd = set_weights(m, d, gen)
                    out.update({'d%d.%s' % (d, k): v for k, v in sd.items()})
                    keep = {k: p.data.clone() for k, p in m.named_parameters()}
                else:
                    for k, p in m.named_parameters():
                        p.data.copy_(keep[k])
                for side in ('head', 'tail'):                           # head prediction: keys (t, r), golds are heads
                    cand = []
                    while len(cand) < NKEY:
                        k = (int(rng.randint(NE)), int(rng.randint(NR)))
                        if k not in cand:
                            cand.append(k)
                    eval_dict, train_dict, valid_dict = {}, {}, {}
                    for k in cand:
                        perm = rng.permutation(NE)
                        ng, nt, nv = rng.randint(1, 4), rng.randint(0, 12), rng.randint(0, 4)
                        eval_dict[k] = set(int(x) for x in perm[:ng])
                        if nt:
                            train_dict[k] = set(int(x) for x in perm[ng:ng + nt])
                        if nv:
                            valid_dict[k] = set(int(x) for x in perm[ng + nt:ng + nt + nv])
                    rows = rows_fp64(sd, [k[0] for k in cand], [k[1] for k in cand], side == 'head', l1)
                    keys = []
                    for k, row in zip(cand, rows):                      # near-ties leave the input
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
                    for b0 in range(0, len(keys), 16):                  # the eval iterator's batches
                        batch = keys[b0:b0 + 16]
                        e = V(torch.LongTensor([k[0] for k in batch]))
                        r = V(torch.LongTensor([k[1] for k in batch]))
                        scores = m.evaluateHead(e, r) if side == 'head' else m.evaluateTail(e, r)
                        preds = zip(batch, scores.data.cpu().numpy())
                        results.extend(rmisc.evalKGProcess(list(preds), eval_dict, all_dicts=[train_dict, valid_dict], descending=False,
                                                           num_processes=2, topn=10, queue_limit=10))
                    results = sorted((tuple(int(x) for x in r[2]), int(r[3]), int(r[1]), int(r[0])) for r in results)   # worker order is arbitrary
                    perf = np.array([[r[3], r[2]] for r in results], dtype=np.float64)
                    ser = lambda dct: [[k[0], k[1], sorted(v)] for k, v in sorted(dct.items())]
                    meta['cases']['d%d.%s.%s' % (d, 'L1' if l1 else 'L2', side)] = {
                        'keys': [list(k) for k in keys], 'eval': ser(eval_dict), 'train': ser(train_dict), 'valid': ser(valid_dict),
                        'rows': [[r[0][0], r[0][1], r[1], r[2], r[3]] for r in results],       # entity, relation, gold id, filtered rank, hit
                        'mean': [float(x) for x in perf.mean(axis=0)],
                        'candidate_keys': len(cand), 'dropped_near_ties': dropped}
    finally:
        np.argsort = real_argsort


def main():
    out, meta = {}, {}
    rank_cases(out, meta)
    path = os.path.join(args.out, 'transr_pass.npz')
    save_npz(path, out)
    with open(os.path.join(args.out, 'transr_pass.json'), 'w') as f:
        json.dump(meta, f, indent=0, sort_keys=True)
    print('transr_pass.npz %.1f KB (%d arrays), transr_pass.json %.1f KB' % (os.path.getsize(path) / 1024, len(out),
                                                                           os.path.getsize(os.path.join(args.out, 'transr_pass.json')) / 1024))
    for k, c in sorted(meta['cases'].items()):
        print('rank %-14s keys %d dropped %d' % (k, len(c['keys']), c['dropped_near_ties']))


if __name__ == '__main__':
    main()
