"""
NEGATIVE CONTROL of tests/test_kmeans_gpu.py, after the pattern of tests/test_neighbors_mutant_gpu.py (whose stamp logic it reuses): the library
with tmvb_kmeans.hip recompiled under -DTMVB_MUTANT_KM_NO_BIAS=1 (tools/build_mutants.sh: mut_kmeans_no_bias).  The epilogue of its assignment
kernel compares the dot products without b_c = -n_c / 2.  Every exact-assignment case whose centroids differ in norm so that the restatement
without the bias selects other labels must FAIL on it with an assertion of that test; the control set, whose centroids are permutations of one
integer vector (equal norms), must pass.  All pass on the shipped library.  A wrong-answer library, not a faulting one: two added constants differ.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import kmeans_restatement as kr
import test_neighbors_mutant_gpu as nm
from test_kmeans_gpu import CASES, CONTROL, exact_inputs

pytestmark = pytest.mark.gpu
ROOT, PKG = nm.ROOT, nm.PKG
NAME, UNIT, FLAG = "mut_kmeans_no_bias", "tmvb_kmeans.hip", "-DTMVB_MUTANT_KM_NO_BIAS=1"
TEST = "tests/test_kmeans_gpu.py::test_exact_assignment"


def _shows(case):
    """does the arg-max of the dot product alone select other labels on this case?"""
    x, init = exact_inputs(*case)
    F, Cf = kr.features32(x, kr.EUCLID), kr.features32(init, kr.EUCLID)
    return not np.array_equal(kr.assign32(F, Cf)[0], kr.assign32(F, Cf, no_bias=True)[0])


SHOWING = [c for c in CASES if c[1] > 1 and c[2] <= 130 and _shows(c)]         # K = 1024 left out: the restated chain would slow the collection


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


def _run(test, cases, variant):
    """the given cases of one test in one child process"""
    env = dict(os.environ, TMVB_LIB_VARIANT=variant)
    env.pop("TMVB_KMEANS_RECORD", None)
    ids = [f"{test}[{'-'.join(str(v) for v in c)}]" for c in cases]
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider"] + ids, capture_output=True, text=True, env=env, cwd=ROOT,
                       timeout=600)
    return r, len(ids)


def test_cases_with_unequal_norms_fail_on_the_mutant(mutant):
    assert len(SHOWING) >= 5
    r, k = _run(TEST, SHOWING, mutant)
    out = r.stdout[-6000:]
    assert r.returncode == 1, f"the cases did NOT fail on {mutant} (rc {r.returncode}):\n{out}\n{r.stderr[-1500:]}"
    assert "AssertionError" in out or "assert " in out, out        # a comparison failed -- not a loader error or a crash
    assert f"{k} failed" in out and "passed" not in out.splitlines()[-1] and "error" not in out.splitlines()[-1], out


def test_the_equal_norm_control_passes_on_the_mutant_and_all_on_the_shipped_library(mutant):
    r, k = _run(TEST + "_equal_norms", CONTROL, mutant)
    assert r.returncode == 0 and f"{k} passed" in r.stdout, (r.stdout[-2000:], r.stderr[-1000:])
    r, k = _run(TEST, SHOWING, "")                                 # the control of the control
    assert r.returncode == 0 and f"{k} passed" in r.stdout, (r.stdout[-2000:], r.stderr[-1000:])
