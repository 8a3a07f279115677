"""
NEGATIVE CONTROL of tests/test_svi_gpu.py, after the pattern of tests/test_coherence_mutant_gpu.py: the library with tmvb_lda_svi.hip recompiled under
-DTMVB_MUTANT_SVI_KEEP_BATCH_STATS=1 (tools/build_mutants.sh: mut_svi_keep_stats).  Its fused global update does not clear the batch's statistics, so
the next E-step accumulates on top of them.  The teacher-forced test forces the whole model state before every step, but not that buffer: on the mutant
its first step must pass -- the buffer is still zero -- and the steps behind it, the doubled batch at the end among them, must fail with an assertion
of that test.
"""
import hashlib
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "topicmodelsvb.jl_amd")
NAME, UNIT, FLAG = "mut_svi_keep_stats", "tmvb_lda_svi.hip", "-DTMVB_MUTANT_SVI_KEEP_BATCH_STATS=1"
TEST = "tests/test_svi_gpu.py::test_teacher_forced_steps"
CASES = ("7-even5", "50-ragged5")
DOUBLED = 6                     # index of the second visit in a row of batch 2 in STEPS = [0, 1, 2, 3, 4, 2, 2]


def _source_hash():
    h = hashlib.sha256()
    d = os.path.join(PKG, "csrc")
    for f in sorted(os.listdir(d)):                       # the order of the shell's `cat csrc/*` in tools/build_variant.sh
        h.update(open(os.path.join(d, f), "rb").read())
    h.update(open(os.path.join(ROOT, "include", "tmvb.h"), "rb").read())
    return h.hexdigest()[:16]


@pytest.fixture(scope="module")
def mutant():
    """the mutant library, built here if the tree does not carry a current one (tools/build_variant.sh links it from the shipped objects)"""
    lib = os.path.join(PKG, f"libtmvb_hip_{NAME}.so")
    stamp = os.path.join(PKG, f"libtmvb_hip_{NAME}.stamp")
    if not (os.path.exists(lib) and os.path.exists(stamp) and open(stamp).read().split() == [_source_hash(), UNIT, FLAG]):
        if not os.path.exists(os.path.join(PKG, "build", UNIT + ".o")):
            import tmvb_amd
            tmvb_amd.pkg.build(force=True)
        subprocess.run([os.path.join(ROOT, "tools", "build_variant.sh"), NAME, UNIT, FLAG], check=True, timeout=1500, capture_output=True)
    return NAME


def _run(case, variant):
    env = dict(os.environ, TMVB_LIB_VARIANT=variant)
    env.pop("TMVB_TOL_RECORD", None)
    return subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider", f"{TEST}[{case}]"], capture_output=True, text=True,
                          env=env, cwd=ROOT, timeout=600)


@pytest.mark.parametrize("case", CASES)
def test_the_doubled_batch_fails_on_the_mutant_and_the_first_step_passes(mutant, case):
    r = _run(case, mutant)
    out = r.stdout[-8000:]
    assert r.returncode == 1, f"{case} did NOT fail on {mutant} (rc {r.returncode}):\n{out}\n{r.stderr[-1500:]}"
    assert "1 failed" in out and "passed" not in out.splitlines()[-1] and "error" not in out.splitlines()[-1], out
    m = re.search(r"svi teacher-forced: failed steps \[([0-9, ]+)\] of 7", out)
    assert m, out                                                    # a comparison of the test failed -- not a loader error or a crash
    failed = [int(x) for x in m.group(1).split(",")]
    assert DOUBLED in failed and 0 not in failed, failed


def test_the_same_cases_pass_on_the_shipped_library(mutant):
    for case in CASES:                                               # the control of the control
        r = _run(case, "")
        assert r.returncode == 0 and "1 passed" in r.stdout, (case, r.stdout[-2000:], r.stderr[-1000:])
