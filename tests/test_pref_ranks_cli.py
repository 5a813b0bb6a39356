"""KTUP_REC_RANKS=1 on the command lines for TUP and KTUP (synthetic datasets of tests/synth.py, -embedding_size 64: a width of the
preference-space pass): one extra line per periodic rec evaluation, logged with route `sweep` (model.rank_items), and nothing else
changes; KTUP with -L1_flag keeps the batch walk.  (The width 36 of tests/test_rank_pass_cli.py is declined and stays `walk` there.)"""
import os
import re
import subprocess
import sys

import pytest

from tests.synth import make_dataset
from tests.test_rank_pass_cli import JOINT, METRIC, PKG, RANKS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dataset(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('ds')
    make_dataset(str(tmp))
    return str(tmp)


def _messages(script, data, name, extra, env):
    """The log's messages from the first evaluation on, without the time stamps (the flags of tests/test_rank_pass_cli.py at width 64)."""
    logs = os.path.join(data, 'log')
    os.makedirs(logs, exist_ok=True)
    cmd = [sys.executable, os.path.join(PKG, script), '-data_path', data, '-log_path', logs, '-dataset', 'ml1m', '-experiment_name', name,
           '-nohas_visualization', '-batch_size', '32', '-embedding_size', '64', '-seed', '3', '-eval_interval_steps', '6',
           '-training_steps', '12', '-early_stopping_steps_to_wait', '0', '-learning_rate', '0.05', '-topn', '10',
           '-rec_test_files', 'valid.dat'] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = open(os.path.join(logs, name + '.log')).read().splitlines()
    msgs = [ln.split(' - ', 3)[3] for ln in lines if ln.count(' - ') >= 3]
    return [m for m in msgs if re.fullmatch(METRIC, m) or re.fullmatch(RANKS, m) or m.startswith('rec rank pass skipped')]


@pytest.mark.parametrize('script,model,extra,route', [
    ('run_item_recommendation.py', 'transup', [], 'sweep'),
    ('run_knowledgable_recommendation.py', 'jtransup', JOINT, 'sweep'),
    ('run_knowledgable_recommendation.py', 'jtransup', JOINT + ['-L1_flag'], 'walk')])
def test_switch_logs_the_sweep_and_changes_nothing_else(dataset, script, model, extra, route):
    args = ['-model_type', model] + extra
    tag = model + ('-l1' if '-L1_flag' in extra else '')
    env = {k: v for k, v in os.environ.items() if k not in ('KTUP_REC_RANKS', 'KTUP_EVAL_PASS')}
    ranks = _messages(script, dataset, 'pref-ranks-' + tag + '-on', args, dict(env, KTUP_REC_RANKS='1'))
    metric = [m for m in ranks if re.fullmatch(METRIC, m)]
    extra_lines = [re.fullmatch(RANKS, m) for m in ranks if re.fullmatch(RANKS, m)]
    assert len(metric) >= 2 and len(extra_lines) == len(metric) and len(ranks) == 2 * len(metric)
    for i, m in enumerate(ranks):                                          # each one right after a metric line
        if re.fullmatch(RANKS, m):
            assert i > 0 and re.fullmatch(METRIC, ranks[i - 1])
    assert {m.group(4) for m in extra_lines} == {route}
    for m in extra_lines:
        assert 0.0 < float(m.group(1)) <= 1.0 and 0.0 <= float(m.group(3)) <= 1.0 and float(m.group(2)) >= 0.0
    if route == 'sweep':                                                   # the metric lines are those of the plain run
        plain = _messages(script, dataset, 'pref-ranks-' + tag + '-plain', args, env)
        assert all(re.fullmatch(METRIC, m) for m in plain) and plain == metric
