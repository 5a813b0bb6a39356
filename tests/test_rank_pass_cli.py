"""KTUP_REC_RANKS=1 on the command lines (synthetic datasets of tests/synth.py): one extra line per periodic rec evaluation -- MRR,
mean rank and AUC with the route that made the ranks -- and nothing else changes; for BPRMF the sweep's figures are those of the
matrix route's ranks (the walk: model.evaluate per batch + ops.gold_ranks, forced with KTUP_EVAL_PASS=0)."""
import os
import re
import subprocess
import sys

import pytest

from tests.synth import make_dataset

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'joint-kg-recommender_amd')
METRIC = r'f1:\d\.\d+, p:\d\.\d+, r:\d\.\d+, hit:\d\.\d+, ndcg:\d\.\d+, topn:10\.'
RANKS = r'mrr:(\d\.\d+), mean rank:(\d+\.\d+), auc:(\d\.\d+) \((\w+)\)\.'
JOINT = ['-kg_test_files', 'valid.dat', '-joint_ratio', '0.5']


@pytest.fixture(scope='module')
def dataset(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('ds')
    make_dataset(str(tmp))
    return str(tmp)


def _messages(script, data, name, extra, env):
    """The log's messages from the first evaluation on, without the time stamps."""
    logs = os.path.join(data, 'log')
    os.makedirs(logs, exist_ok=True)
    cmd = [sys.executable, os.path.join(PKG, script), '-data_path', data, '-log_path', logs, '-dataset', 'ml1m', '-experiment_name', name,
           '-nohas_visualization', '-batch_size', '32', '-embedding_size', '36', '-seed', '3', '-eval_interval_steps', '6',
           '-training_steps', '12', '-early_stopping_steps_to_wait', '0', '-learning_rate', '0.05', '-topn', '10',
           '-rec_test_files', 'valid.dat'] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = open(os.path.join(logs, name + '.log')).read().splitlines()
    msgs = [ln.split(' - ', 3)[3] for ln in lines if ln.count(' - ') >= 3]
    return [m for m in msgs if re.fullmatch(METRIC, m) or re.fullmatch(RANKS, m) or m.startswith('rec rank pass skipped')]


@pytest.mark.parametrize('script,model,extra,route', [
    ('run_item_recommendation.py', 'bprmf', [], 'sweep'),
    ('run_knowledgable_recommendation.py', 'cfkg', JOINT, 'sweep'),
    ('run_knowledgable_recommendation.py', 'jtransup', JOINT, 'walk')])
def test_switch_adds_one_line_per_evaluation_and_changes_nothing_else(dataset, script, model, extra, route):
    args = ['-model_type', model] + extra
    env = {k: v for k, v in os.environ.items() if k not in ('KTUP_REC_RANKS', 'KTUP_EVAL_PASS')}
    plain = _messages(script, dataset, 'ranks-' + model + '-plain', args, env)
    ranks = _messages(script, dataset, 'ranks-' + model + '-on', args, dict(env, KTUP_REC_RANKS='1'))
    assert len(plain) >= 2 and all(re.fullmatch(METRIC, m) for m in plain)
    assert [m for m in ranks if not re.fullmatch(RANKS, m)] == plain       # the extra line removed: the plain run's metric lines
    extra_lines = [re.fullmatch(RANKS, m) for m in ranks if re.fullmatch(RANKS, m)]
    assert len(extra_lines) == len(plain)
    for i, m in enumerate(ranks):                                          # each one right after a metric line
        if re.fullmatch(RANKS, m):
            assert i > 0 and re.fullmatch(METRIC, ranks[i - 1])
    assert {m.group(4) for m in extra_lines} == {route}
    for m in extra_lines:
        assert 0.0 < float(m.group(1)) <= 1.0 and 0.0 <= float(m.group(3)) <= 1.0 and float(m.group(2)) >= 0.0
    if model == 'bprmf':                                                   # the matrix route's ranks through rec_rank_metrics: the walk
        walk = _messages(script, dataset, 'ranks-bprmf-walk', args, dict(env, KTUP_REC_RANKS='1', KTUP_EVAL_PASS='0'))
        walk_lines = [re.fullmatch(RANKS, m) for m in walk if re.fullmatch(RANKS, m)]
        assert {m.group(4) for m in walk_lines} == {'walk'}
        assert [m.groups()[:3] for m in walk_lines] == [m.groups()[:3] for m in extra_lines]
