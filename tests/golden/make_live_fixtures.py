#!/usr/bin/env python3
"""Record what the drop-in tests compare against, from a checkout of the reference (names, values and outputs only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_live_fixtures.py --ref <checkout of the reference>

reference_surface.json    the flags of its jTransUP/models/base.py (name, kind, default, enum choices), the argument vectors of
                          the `python run_*.py ...` lines of its shell scripts, and the argument names of the top-level functions
                          and public methods of its in-scope modules (tests/test_cli_dropin_live.py)
reference_host.json       what tests/golden/live_host.py prints when run against its package (tests/test_cli_dropin_live.py)
reference_samplers.json   the draws of its host samplers in tests/test_oracle_live_reference.py's scenario
reference_worlds_<s>_<w>_<p>.npz  the outputs of its modules on live_check.py's random worlds, seeds 0 and 1, each world in one
                          or more parts (tests/golden/live_check.py --record; replayed against the oracle by tests/test_oracle_live_reference.py)"""
import argparse
import importlib.util
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'joint-kg-recommender_amd'))

ap = argparse.ArgumentParser()
ap.add_argument('--ref', required=True, help='a checkout of the reference (the directory holding its jTransUP package)')
args = ap.parse_args()
REF = os.path.abspath(args.ref)

from tests import test_cli_dropin_live as T                           # noqa: E402
from tests import test_oracle_live_reference as S                     # noqa: E402


def dump(name, doc):
    path = os.path.join(HERE, name)
    with open(path, 'w') as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write('\n')
    print('%-26s %7.1f KB' % (name, os.path.getsize(path) / 1024))


modules = {}
for mod in T.IN_SCOPE:
    funcs, classes = T._surface(os.path.join(REF, 'jTransUP', mod + '.py'))
    modules[mod] = {'functions': funcs, 'classes': classes}
dump('reference_surface.json', {'flags': T._reference_flags(REF), 'command_lines': list(T._script_command_lines(REF)), 'modules': modules})

env = dict(os.environ, PYTHONDONTWRITEBYTECODE='1')
env.pop('PYTHONPATH', None)
out = subprocess.run([sys.executable, os.path.join(HERE, 'live_host.py'), '--pkg', REF], capture_output=True, text=True, timeout=120,
                     env=env, cwd=ROOT, check=True)
dump('reference_host.json', {'stdout': out.stdout.strip().splitlines()})

spec = importlib.util.spec_from_file_location('ktup_reference_utils_data', os.path.join(REF, 'jTransUP', 'utils', 'data.py'))
ref_data = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref_data)
dump('reference_samplers.json', {'draws': S.plain_draws(S.sampler_draws(ref_data))})

for seed in S.WORLD_SEEDS:
    subprocess.run([sys.executable, os.path.join(HERE, 'live_check.py'), '--worlds', str(S.WORLDS), '--seed', str(seed), '--ref', REF,
                    '--record', os.path.join(HERE, 'reference_worlds_%d.npz' % seed)], env=env, cwd=ROOT, check=True)
