"""csrc/ktup_split_plan.h -- the slot plan of the packed split stage 2 (ktup_score_pref_mc.hip) -- compiled on its own with the host
compiler: the header holds constexpr tables only, and its static_asserts are the test (every product class of every logit group exactly
once, no slot pairing two groups, unused slots zero on both sides, at most three planes), for three, four and five logits per lane.
The small program also evaluates the same predicates at run time and names the plan that fails."""
import importlib.util
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'joint-kg-recommender_amd', 'csrc')

MAIN = r'''
#include <cstdio>
#include "ktup_split_plan.h"
int main() {
  using namespace ktup::split_plan;
  int bad = 0;
  for (int ns = 3; ns <= 5; ++ns) {
    const Plan& p = plan_for(ns);
    if (p.ns != ns || !valid(p)) { std::printf("plan for %d logits per lane is not valid\n", ns); ++bad; }
    int used = 0;
    for (int m = 0; m < p.nmfma; ++m)
      for (int k = 0; k < 8; ++k) used += product_class(a_term(p, m, k), p.mfma[m].b[k]) >= 0;
    std::printf("NS %d: %d planes, %d MFMAs, %d of %d slots used\n", ns, p.nplanes, p.nmfma, used, 8 * p.nmfma);
    if (used != 6 * ns) ++bad;
  }
  return bad;
}
'''


def _host_compiler():
    for cxx in (os.environ.get('CXX'), 'c++', 'g++', 'clang++'):
        if cxx and shutil.which(cxx):
            return [shutil.which(cxx)]
    spec = importlib.util.spec_from_file_location('ktup_build_hip', os.path.join(ROOT, 'joint-kg-recommender_amd', 'build_hip.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return [mod.HIPCC, '-x', 'c++']                       # the device compiler's host side: still no device code in the header


def test_split_plan_header_compiles_alone_and_its_plans_hold(tmp_path):
    src, exe = tmp_path / 'plan_check.cpp', tmp_path / 'plan_check'
    src.write_text(MAIN)
    r = subprocess.run(_host_compiler() + ['-std=c++17', '-Wall', '-Werror', '-I', CSRC, str(src), '-o', str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'NS 5: 3 planes, 4 MFMAs, 30 of 32 slots used' in r.stdout and 'NS 4: 2 planes, 3 MFMAs, 24 of 24 slots used' in r.stdout
