"""Host side of the TUP / KTUP rank pass (no GPU): the header declares the three entry points and the binding table carries them
with matching arity; the entry point's refusals by name (no launch is made); both model classes have rank_items; and the driver hook
(models/_driver.py rec_rank_pass) on stub models -- a rank_items that answers is logged as route `sweep` with ASCENDING scores, one
that answers None falls to the batch walk."""
import ctypes
import inspect
import logging
import os
import re
import types

import numpy as np
import pytest
import torch

from jTransUP.utils.ranking import rec_rank_metrics
from tests.test_rank_pass_host import _Log, _host_gold_ranks, _world

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'ktup_hip.h')
NAMES = ['ktup_eval_pref_ranks_supported', 'ktup_eval_pref_ranks_workspace_bytes', 'ktup_eval_pref_ranks']
ERR_INVALID, ERR_UNSUPPORTED = -1, -3


@pytest.fixture(scope='module')
def lib():
    from jTransUP.hip import lib as L
    if not os.path.exists(L.LIB_PATH):
        import importlib.util
        spec = importlib.util.spec_from_file_location('build_hip', os.path.join(ROOT, 'joint-kg-recommender_amd', 'build_hip.py'))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mod.build(verbose=False)
    return L


def test_header_and_binding_table_carry_the_entry_points(lib):
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    loaded = lib.load()
    for name in NAMES:
        ret, args = re.search(r'\b(\w+)[\s*]+%s\s*\(([^)]*)\)' % name, text).groups()
        assert name in lib.SIGNATURES, name
        assert len(args.split(',')) == len(lib.SIGNATURES[name]), name
        assert hasattr(loaded, name)
        assert (ret == 'size_t') == (lib._RESTYPE.get(name) is ctypes.c_size_t), name
    # the table / pref_ws / u_ids head of ktup_eval_pref_topk, then ktup_eval_dot_ranks' filter / gold / ... / stream tail
    topk, dot, mine = (lib.SIGNATURES[n] for n in ('ktup_eval_pref_topk', 'ktup_eval_dot_ranks', 'ktup_eval_pref_ranks'))
    assert mine[:16] == topk[:16] and mine[14:] == dot[10:]
    assert re.search(r'#define\s+KTUP_PREF_RANK_BLOCK_GOLDS\s+KTUP_RANK_BLOCK_GOLDS\b', text) and re.search(r'#define\s+KTUP_RANK_BLOCK_GOLDS\s+3072\b', text)


def test_the_entry_points_refuse_by_name_before_any_launch(lib):
    L = lib.load()
    cap = 3072
    assert L.ktup_eval_pref_ranks_supported(100, 20, 0, 3240, 1100) == 1
    assert L.ktup_eval_pref_ranks_supported(64, 1, 0, 5, 0) == 1 and L.ktup_eval_pref_ranks_supported(128, 32, 0, 5, cap) == 1
    for d, P, l1, n, bg in ((100, 20, 1, 3240, 10), (36, 20, 0, 3240, 10), (256, 20, 0, 3240, 10), (100, 33, 0, 3240, 10), (100, 20, 0, 1 << 31, 10),
                            (100, 20, 0, 3240, cap + 1)):
        assert L.ktup_eval_pref_ranks_supported(d, P, l1, n, bg) == 0, (d, P, l1, n, bg)
        assert L.ktup_eval_pref_ranks_workspace_bytes(d, P, l1, 64, n, cap + 10, bg) == 0, (d, P, l1, n, bg)
    old = lib.set_option('eval_mc', 0)
    try:
        assert L.ktup_eval_pref_ranks_supported(100, 20, 0, 3240, 10) == 0
        assert L.ktup_eval_pref_ranks_workspace_bytes(100, 20, 0, 64, 3240, 100, 10) == 0
    finally:
        lib.set_option('eval_mc', old)
    # the workspace: keys, permutation, filter bits and the list pass's operand tables (QGeom<25, 5>: 272 + 4 floats a user, 164 an item)
    nq, n, n_gold = 6040, 3240, 100000
    want = n_gold * 8 + n_gold * 4 + nq * ((n + 31) // 32) * 4 + (3 * 32 * 32 + 4 * 2 * 8 * 64 + nq * (272 + 4) + n * 164 + 64) * 4 + 16
    assert L.ktup_eval_pref_ranks_workspace_bytes(100, 20, 0, nq, n, n_gold, 1100) == want
    # argument errors and declines of the call itself, host side only (the pointers are never read)
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    base = dict(U=p, ldu=100, I=p, ldi=100, E=None, lde=0, i2e=None, pws=p, P=20, d=100, u=p, nq=4, n=10, l1=0, fo=None, fi=None, go=p, gi=p,
                n_gold=3, bg=3, nsplit=0, ranks=p, ws=p, st=None)

    def status(**kw):
        a = dict(base, **kw)
        try:
            lib.call('ktup_eval_pref_ranks', *[a[k] for k in base])
        except lib.KtupError as e:
            return e.code, str(e)
        return 0, ''
    for kw, word in ((dict(ranks=None), 'null ranks'), (dict(gi=None), 'gold_ids'), (dict(go=None), 'gold_off'), (dict(fo=p), 'filt_off and filt_ids'),
                     (dict(bg=4), 'block_golds'), (dict(E=p), 'E and item2ent'), (dict(ldu=64), 'pitch'), (dict(U=None), 'table')):
        code, text = status(**kw)
        assert code == ERR_INVALID and word in text, (kw, code, text)
    for kw, word in ((dict(l1=1), 'L1'), (dict(d=36, ldu=36, ldi=36), '36'), (dict(d=256, ldu=256, ldi=256), '256'), (dict(P=33), '33'),
                     (dict(n=1 << 31), '32-bit'), (dict(n_gold=cap + 5, bg=cap + 1), 'gold entries')):
        code, text = status(**kw)
        assert code == ERR_UNSUPPORTED and word in text, (kw, code, text)
    assert status(nq=0) == (0, '') and status(n_gold=0, bg=0) == (0, '')          # nothing to do: KTUP_OK without a launch
    for kw, word in ((dict(ws=None), 'workspace'), (dict(ws=p + 8 if p % 16 == 0 else p + (16 - p % 16) + 8), '16-byte')):
        code, text = status(**kw)
        assert code == ERR_INVALID and word in text, (kw, code, text)


def test_both_model_classes_have_rank_items():
    from jTransUP.models.CFKG import CFKG
    from jTransUP.models.jTransUP import jTransUPModel
    from jTransUP.models.transUP import TransUPModel
    want = list(inspect.signature(CFKG.rank_items).parameters)
    assert want == ['self', 'u_ids', 'items', 'gold_off', 'gold_ids', 'filt_off', 'filt_ids']
    for cls in (TransUPModel, jTransUPModel):
        sig = inspect.signature(cls.rank_items)
        assert list(sig.parameters) == want, cls
        assert sig.parameters['filt_off'].default is None and sig.parameters['filt_ids'].default is None
    # under the ST-Gumbel gate the models answer None before they touch a table
    for cls in (TransUPModel, jTransUPModel):
        stub = types.SimpleNamespace(use_st_gumbel=True)
        assert cls.rank_items(stub, None, None, None, None) is None


def _stub(monkeypatch, answers):
    """A TUP-like stub (ascending distances, no topk_descending attribute) through the driver hook, wired as the drivers wire it."""
    from jTransUP.hip import ops
    from jTransUP.models import _driver as D
    monkeypatch.setattr(D, 'DEV', torch.device('cpu'))
    monkeypatch.setattr(ops, 'gold_ranks', _host_gold_ranks)
    scores, gold, train = _world(9)
    nq, n = scores.shape
    batches = [list(range(0, 10)), list(range(10, nq))]
    calls = {'rank_items': 0, 'evaluate': 0}
    table = torch.from_numpy(scores)

    def rank_items(u, items, go, gi, fo, fi):
        calls['rank_items'] += 1
        assert items is None and u.tolist() == list(range(nq))
        return _host_gold_ranks(table[u], False, go, gi, fo, fi) if answers else None

    def evaluate(u):
        calls['evaluate'] += 1
        return table[u]
    model = types.SimpleNamespace(rank_items=rank_items, evaluate=evaluate, item_total=n)
    log = logging.getLogger('pref-ranks-host')
    log.setLevel(logging.INFO)
    log.propagate = False
    handler = _Log()
    log.handlers = [handler]
    FL = types.SimpleNamespace(topn=10, shard_eval_candidates=False)
    rank_fn = (lambda u, go, gi, fo, fi: model.rank_items(u, None, go, gi, fo, fi)) if hasattr(model, 'rank_items') else None
    run = lambda: D.rec_rank_pass(FL, model.evaluate, batches, gold, [train], False, n, log, rank_fn=rank_fn,
                                  pass_descending=getattr(model, 'topk_descending', False))
    index = D.rank_index(batches, gold, [train])
    ranks = _host_gold_ranks(table, False, index.g_off, index.g_ids, index.f_off, index.f_ids).numpy()
    want = rec_rank_metrics(ranks, index.g_off_h, index.n_neg(n))
    return run, calls, handler, want, len(batches)


def test_hook_logs_the_sweep_for_ascending_scores(monkeypatch):
    run, calls, handler, want, nb = _stub(monkeypatch, True)
    monkeypatch.setenv('KTUP_REC_RANKS', '1')
    monkeypatch.delenv('KTUP_EVAL_PASS', raising=False)
    assert run() == want
    assert calls == {'rank_items': 1, 'evaluate': 0}
    assert handler.lines == ['mrr:{:.4f}, mean rank:{:.4f}, auc:{:.4f} (sweep).'.format(*want)]
    monkeypatch.delenv('KTUP_REC_RANKS')                                   # opt-in: nothing is computed or logged without the switch
    handler.lines[:] = []
    assert run() is None and handler.lines == [] and calls == {'rank_items': 1, 'evaluate': 0}


def test_hook_falls_to_the_walk_where_rank_items_answers_none(monkeypatch):
    run, calls, handler, want, nb = _stub(monkeypatch, False)
    monkeypatch.setenv('KTUP_REC_RANKS', '1')
    monkeypatch.delenv('KTUP_EVAL_PASS', raising=False)
    assert run() == want
    assert calls == {'rank_items': 1, 'evaluate': nb}
    assert handler.lines == ['mrr:{:.4f}, mean rank:{:.4f}, auc:{:.4f} (walk).'.format(*want)]
