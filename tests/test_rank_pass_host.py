"""Host side of the rec rank pass (no GPU): rec_rank_metrics against brute-force pair counting, RankIndex.n_neg, and the driver hook
(models/_driver.py rec_rank_pass) on a stub model -- unset: no call and no line; KTUP_REC_RANKS=1 with a model whose rank_items
declines: the batch walk, logged as route `walk`."""
import logging
import types

import numpy as np
import pytest
import torch

from jTransUP.utils.ranking import RankIndex, rec_rank_metrics


def _host_gold_ranks(scores, descending, g_off, g_ids, f_off=None, f_ids=None):
    """ops.gold_ranks on the host: candidates ordered before the gold (descending score, ties -> lower id) that are neither filtered nor
    gold; -1 for a gold that is filtered or outside the catalogue."""
    s = scores.cpu().numpy().astype(np.float64)
    s = -s if descending else s
    g_off, g_ids = g_off.cpu().numpy(), g_ids.cpu().numpy()
    out = np.full(len(g_ids), -7, dtype=np.int32)
    n = s.shape[1]
    for b in range(s.shape[0]):
        filt = set() if f_off is None else set(f_ids.cpu().numpy()[int(f_off[b]):int(f_off[b + 1])].tolist())
        gold = set(g_ids[g_off[b]:g_off[b + 1]].tolist())
        for e in range(g_off[b], g_off[b + 1]):
            g = int(g_ids[e])
            if g in filt or not 0 <= g < n:
                out[e] = -1
                continue
            out[e] = sum(1 for j in range(n) if j not in filt and j not in gold and (s[b, j] < s[b, g] or (s[b, j] == s[b, g] and j < g)))
    return torch.from_numpy(out[:int(g_off[-1])])


def _world(seed, nq=23, n=31):
    rng = np.random.RandomState(seed)
    scores = rng.randint(0, 12, size=(nq, n)).astype(np.float32)          # many ties
    gold = {b: set(rng.choice(n, size=rng.randint(1, 6), replace=False).tolist()) for b in range(nq) if b % 5}
    train = {b: set(rng.choice(n, size=rng.randint(0, 9), replace=False).tolist()) for b in range(nq)}
    train[1] = set(range(n))                                               # user 1: every gold is filtered -> only -1 entries
    train[2] = set(range(n)) - gold[2]                                     # user 2: nothing but golds left -> n_neg = 0
    return scores, gold, train


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_rank_metrics_are_brute_force_pair_counts(seed):
    scores, gold, train = _world(seed)
    nq, n = scores.shape
    keys = list(range(nq))
    index = RankIndex(keys, gold, [train], torch.device('cpu'))
    ranks = _host_gold_ranks(torch.from_numpy(scores), True, index.g_off, index.g_ids, index.f_off, index.f_ids).numpy()
    n_neg = index.n_neg(n)
    rr, all_ranks, aucs = [], [], []
    for b in range(nq):
        shown = [g for g in sorted(gold.get(b, ())) if g not in train[b]]
        others = [j for j in range(n) if j not in train[b] and j not in gold.get(b, ())]
        assert n_neg[b] == len(others)
        if not shown:
            continue
        before = lambda j, g: scores[b, j] > scores[b, g] or (scores[b, j] == scores[b, g] and j < g)
        mine = [sum(1 for j in others if before(j, g)) for g in shown]
        all_ranks += mine
        rr.append(1.0 / (1 + min(mine)))
        if others:
            aucs.append(sum(1 for g in shown for j in others if not before(j, g)) / float(len(shown) * len(others)))
    assert (ranks[index.g_off_h[1]:index.g_off_h[2]] == -1).all() and n_neg[2] == 0 and len(aucs) < len(rr)
    mrr, mean_rank, auc = rec_rank_metrics(ranks, index.g_off_h, n_neg)
    assert mrr == pytest.approx(np.mean(rr), rel=1e-12)
    assert mean_rank == pytest.approx(np.mean(all_ranks), rel=1e-12)
    assert auc == pytest.approx(np.mean(aucs), rel=1e-12)


def test_rank_metrics_with_nothing_ranked():
    assert rec_rank_metrics(np.array([-1, -1]), np.array([0, 1, 2]), np.array([3, 0])) == (0.0, 0.0, 0.0)
    assert rec_rank_metrics(np.zeros(0, np.int32), np.array([0, 0]), np.array([5])) == (0.0, 0.0, 0.0)


class _Log(logging.Handler):
    def __init__(self):
        super(_Log, self).__init__()
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def _stub(monkeypatch):
    from jTransUP.hip import ops
    from jTransUP.models import _driver as D
    monkeypatch.setattr(D, 'DEV', torch.device('cpu'))
    monkeypatch.setattr(ops, 'gold_ranks', _host_gold_ranks)
    scores, gold, train = _world(7)
    nq, n = scores.shape
    batches = [list(range(0, 10)), list(range(10, nq))]
    calls = {'rank_items': 0, 'evaluate': 0}
    table = torch.from_numpy(scores)

    def rank_items(u, items, go, gi, fo, fi):
        calls['rank_items'] += 1
        return None                                                        # the sweep declines

    def evaluate(u):
        calls['evaluate'] += 1
        return table[u]
    model = types.SimpleNamespace(rank_items=rank_items, evaluate=evaluate, item_total=n, topk_descending=True)
    log = logging.getLogger('rank-pass-host')
    log.setLevel(logging.INFO)
    log.propagate = False
    handler = _Log()
    log.handlers = [handler]
    FL = types.SimpleNamespace(topn=10, shard_eval_candidates=False)
    run = lambda **kw: D.rec_rank_pass(FL, model.evaluate, batches, gold, [train], True, n, log,
                                       rank_fn=lambda u, go, gi, fo, fi: model.rank_items(u, None, go, gi, fo, fi), pass_descending=True, **kw)
    return D, run, calls, handler, (scores, gold, train, batches)


@pytest.mark.parametrize('value', [None, '0', ''])
def test_hook_unset_computes_and_logs_nothing(monkeypatch, value):
    D, run, calls, handler, _ = _stub(monkeypatch)
    if value is None:
        monkeypatch.delenv('KTUP_REC_RANKS', raising=False)
    else:
        monkeypatch.setenv('KTUP_REC_RANKS', value)
    assert run() is None
    assert calls == {'rank_items': 0, 'evaluate': 0} and handler.lines == []


def test_hook_takes_the_walk_where_the_model_declines(monkeypatch):
    D, run, calls, handler, (scores, gold, train, batches) = _stub(monkeypatch)
    monkeypatch.setenv('KTUP_REC_RANKS', '1')
    monkeypatch.delenv('KTUP_EVAL_PASS', raising=False)
    got = run()
    assert calls == {'rank_items': 1, 'evaluate': len(batches)}
    index = D.rank_index(batches, gold, [train])
    ranks = _host_gold_ranks(torch.from_numpy(scores), True, index.g_off, index.g_ids, index.f_off, index.f_ids).numpy()
    want = rec_rank_metrics(ranks, index.g_off_h, index.n_neg(scores.shape[1]))
    assert got == want
    assert handler.lines == ['mrr:{:.4f}, mean rank:{:.4f}, auc:{:.4f} (walk).'.format(*want)]
    handler.lines[:] = []
    assert run(sharded=True) is None                                       # sharded candidates: skipped, one line says so
    assert len(handler.lines) == 1 and handler.lines[0].startswith('rec rank pass skipped')
    assert calls == {'rank_items': 1, 'evaluate': len(batches)}
