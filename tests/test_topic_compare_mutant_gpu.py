"""
NEGATIVE CONTROL of tests/test_topic_compare_gpu.py, after the pattern of tests/test_kmeans_mutant_gpu.py (whose stamp logic it reuses through
tests/test_neighbors_mutant_gpu.py): the library with tmvb_topic_compare.hip recompiled under -DTMVB_MUTANT_TD_DROP_TAIL=1 (tools/build_mutants.sh:
mut_topicdiv_drop_tail).  Its pair kernel leaves out the last, partial run of terms -- what a run loop bounded by V / TMVB_TD_RUN loses.  Every exact
total-variation case with V % 256 != 0 whose tail carries mass (the restatement without the tail gives another matrix) must FAIL on it with an
assertion of that test; the cases with V % 256 == 0 must pass.  All pass on the shipped library.  A wrong-answer library, not a faulting one: a loop
bound differs.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import test_neighbors_mutant_gpu as nm
import topic_compare_restatement as tr
from test_topic_compare_gpu import CASES, exact_case

pytestmark = pytest.mark.gpu
ROOT, PKG = nm.ROOT, nm.PKG
NAME, UNIT, FLAG = "mut_topicdiv_drop_tail", "tmvb_topic_compare.hip", "-DTMVB_MUTANT_TD_DROP_TAIL=1"
TEST = "tests/test_topic_compare_gpu.py::test_exact_total_variation"


def _shows(case):
    """does the sum without the last, partial run differ on this case?"""
    a, b, want = exact_case(*case[:3])
    return not np.array_equal(tr.divergence(tr.TV, a, b, drop_tail=True)[0], want)


SHOWING = [c for c in CASES if c[2] % tr.RUN != 0 and _shows(c)]
CONTROL = [c for c in CASES if c[2] % tr.RUN == 0]


@pytest.fixture(scope="module")
def mutant():
    """the mutant library, built here if the tree does not carry a current one (tools/build_variant.sh links it from the shipped objects)"""
    lib = os.path.join(PKG, f"libtmvb_hip_{NAME}.so")
    stamp = os.path.join(PKG, f"libtmvb_hip_{NAME}.stamp")
    if not (os.path.exists(lib) and os.path.exists(stamp) and open(stamp).read().split() == [nm._source_hash(), UNIT, FLAG]):
        if not os.path.exists(os.path.join(PKG, "build", UNIT + ".o")):
            import tmvb_amd
            tmvb_amd.pkg.build(force=True)
        subprocess.run([os.path.join(ROOT, "tools", "build_variant.sh"), NAME, UNIT, FLAG], check=True, timeout=1500, capture_output=True)
    return NAME


def _run(cases, variant):
    """the given cases of the exact test in one child process"""
    env = dict(os.environ, TMVB_LIB_VARIANT=variant)
    env.pop("TMVB_TOPICDIV_RECORD", None)
    ids = [f"{TEST}[{'-'.join(str(v) for v in c)}]" for c in cases]
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider"] + ids, capture_output=True, text=True, env=env, cwd=ROOT,
                       timeout=600)
    return r, len(ids)


def test_cases_with_mass_in_the_tail_fail_on_the_mutant(mutant):
    assert len(SHOWING) >= 5
    r, k = _run(SHOWING, mutant)
    out = r.stdout[-6000:]
    assert r.returncode == 1, f"the cases did NOT fail on {mutant} (rc {r.returncode}):\n{out}\n{r.stderr[-1500:]}"
    assert "AssertionError" in out or "assert " in out, out        # a comparison failed -- not a loader error or a crash
    assert f"{k} failed" in out and "passed" not in out.splitlines()[-1] and "error" not in out.splitlines()[-1], out


def test_whole_run_cases_pass_on_the_mutant_and_all_on_the_shipped_library(mutant):
    assert len(CONTROL) >= 3
    r, k = _run(CONTROL, mutant)
    assert r.returncode == 0 and f"{k} passed" in r.stdout, (r.stdout[-2000:], r.stderr[-1000:])
    r, k = _run(SHOWING, "")                                       # the control of the control
    assert r.returncode == 0 and f"{k} passed" in r.stdout, (r.stdout[-2000:], r.stderr[-1000:])
