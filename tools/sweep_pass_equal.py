"""Are the lists of the one-sweep passes (ktup_eval_cfkg_topk, ktup_eval_dot_topk) of two builds of the library the same bits?

    python tools/sweep_pass_equal.py --other /path/to/another/libktup_hip.so [-o profiles/sweep_pass_equal.txt]

The tests referee the CFKG pass against fp64 scores only, so a change that is meant to move no bit (a refactor of the sweep) needs
this comparison.  Neither pass has a float atomic (the only atomic is the filter bitmap's atomicOr), so equal means every id and
every score bit.  Two child processes, one per library (KTUP_HIP_LIB; the ABI has to be the same), each under its own time limit,
run the seeded case generators of tests/test_hip_cfkg_pass.py and tests/test_hip_dot_pass.py:
  CFKG  SHAPES x {L1, squared L2} x {cand_ids None, a subset} x nsplit {0, 1, 3, 32} x {filter, none} x {with scores, ids only}
  dot   (SHAPES + MANY_SPLITS) x {terms, none} x {filter, none} x nsplit {0, 1, 3, 32}, with scores
and dump ids and score bits, which are compared with numpy.array_equal."""
import argparse
import importlib
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'joint-kg-recommender_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)
CHILD_LIMIT_S = 300
NSPLITS = (0, 1, 3, 32)


def dump(path):
    import numpy as np
    from jTransUP.hip import ops
    C = importlib.import_module('tests.test_hip_cfkg_pass')
    Dt = importlib.import_module('tests.test_hip_dot_pass')
    out = {}

    def keep(name, got, with_scores=True):
        ids, sc = got if with_scores else (got, None)
        out[name + ' ids'] = ids.cpu().numpy()
        if sc is not None:
            out[name + ' score bits'] = sc.cpu().numpy().view(np.uint32)
    for shape in C.SHAPES:
        topn = shape[5]
        for l1 in (True, False):
            c = C.case(shape, l1)
            for which in ('all', 'sub'):
                f_off, f_ids, _ = c['filt'][which]
                for nsplit in NSPLITS:
                    for filt in (True, False):
                        for ws in (True, False):
                            got = ops.eval_cfkg_topk(c['U'], c['R'], C.NR - 1, c['E'], c['u'], topn, l1, cand_ids=None if which == 'all' else c['cand'],
                                                     filt_off=f_off if filt else None, filt_ids=f_ids if filt else None, with_scores=ws, nsplit=nsplit)
                            keep('cfkg %s %s %s nsplit=%d filter=%d scores=%d' % (shape, 'L1' if l1 else 'L2', which, nsplit, filt, ws), got, ws)
    for shape in Dt.SHAPES + Dt.MANY_SPLITS:
        U, I, u, ua, ia, f_off, f_ids, _ = Dt.case(shape)
        for terms in (True, False):
            for filt in (True, False):
                for nsplit in NSPLITS:
                    got = ops.eval_dot_topk(U, I, u, shape[4], f_off if filt else None, f_ids if filt else None, ua if terms else None,
                                            ia if terms else None, with_scores=True, nsplit=nsplit)
                    keep('dot %s terms=%d filter=%d nsplit=%d' % (shape, terms, filt, nsplit), got)
    np.savez(path, **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--other', help='the library to compare the tree\'s build with')
    ap.add_argument('--dump', help='(child) run the cases with the library of KTUP_HIP_LIB and write them here')
    ap.add_argument('-o', '--output', default=os.path.join(ROOT, 'profiles', 'sweep_pass_equal.txt'))
    a = ap.parse_args()
    if a.dump:
        return dump(a.dump)
    import numpy as np
    mine = os.path.join(ROOT, 'joint-kg-recommender_amd', 'libktup_hip.so')
    other = os.path.abspath(a.other)
    assert os.path.exists(mine) and os.path.exists(other) and not os.path.samefile(mine, other)
    with tempfile.TemporaryDirectory(prefix='sweep_equal_') as tmp:
        got = []
        for i, lib in enumerate((mine, other)):                           # a GPU process each; a child that fails ends the run
            path = os.path.join(tmp, '%d.npz' % i)
            r = subprocess.run(['timeout', '-k', '10', str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__), '--dump', path],
                               env=dict(os.environ, KTUP_HIP_LIB=lib), capture_output=True, text=True)
            if r.returncode != 0:
                sys.stderr.write(r.stdout[-3000:] + r.stderr[-3000:] + '\nthe child of %s ended with status %d: nothing further is started\n' % (lib, r.returncode))
                return r.returncode
            got.append(dict(np.load(path)))
    a_, b_ = got
    assert sorted(a_) == sorted(b_)
    bad = [k for k in sorted(a_) if not np.array_equal(a_[k], b_[k])]
    calls = {p: sum(1 for k in a_ if k.startswith(p) and k.endswith(' ids')) for p in ('cfkg', 'dot')}
    out = ['# tools/sweep_pass_equal.py: the tree\'s build against another build of the library, ids and score bits of every call',
           'cfkg pass: %d calls, dot pass: %d calls, %d arrays compared' % (calls['cfkg'], calls['dot'], len(a_)),
           'unequal arrays: %d%s' % (len(bad), ''.join('\n  ' + k for k in bad)),
           'result: %s' % ('EQUAL, every id and every score bit' if not bad else 'NOT equal')]
    text = '\n'.join(out) + '\n'
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.output)), exist_ok=True)
    open(a.output, 'w').write(text)
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
