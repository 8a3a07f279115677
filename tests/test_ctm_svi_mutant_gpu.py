"""
NEGATIVE CONTROL of tests/test_ctm_svi_gpu.py, after the pattern of tests/test_svi_mutant_gpu.py: the library with tmvb_ctm_svi.hip recompiled under
-DTMVB_MUTANT_CTM_SVI_NO_RECENTRE=1 (tools/build_mutants.sh: mut_ctm_svi_no_recentre).  Its tail kernel blends the running scatter matrix as it stands,
about m_ref, without moving it to the current mu first.  On the mutant the test of a forced move of mu and the teacher-forced steps after mu has moved
(MOVED_STEPS below) must fail with an assertion of the test; step 0 from the default state -- m_ref = mu_0 -- must pass.
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
NAME, UNIT, FLAG = "mut_ctm_svi_no_recentre", "tmvb_ctm_svi.hip", "-DTMVB_MUTANT_CTM_SVI_NO_RECENTRE=1"
FORCED = "tests/test_ctm_svi_gpu.py::test_teacher_forced_steps"
MOVED = "tests/test_ctm_svi_gpu.py::test_a_move_of_mu_between_visits_is_recentred"
CASES = ((FORCED, "7-even5"), (FORCED, "70-ragged5"), (MOVED, "7"), (MOVED, "130"))
# the teacher-forced steps in front of which mu has moved away from m_ref.  even5: every step but the first.  ragged5: step 1 visits the batch that holds only
# the empty document, whose lambda settles on mu itself (no tokens: the gradient is invsigma (mu - lambda)), so l_b = mu and the blend leaves mu where it
# was -- step 2 starts with m_ref = mu, there is nothing to recentre, and the mutant is right there by construction.
MOVED_STEPS = {"7-even5": [1, 2, 3, 4, 5, 6], "70-ragged5": [1, 3, 4, 5, 6]}


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


def _run(test, case, variant):
    env = dict(os.environ, TMVB_LIB_VARIANT=variant)
    env.pop("TMVB_TOL_RECORD", None)
    return subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider", f"{test}[{case}]"], capture_output=True, text=True,
                          env=env, cwd=ROOT, timeout=600)


@pytest.mark.parametrize("test,case", CASES)
def test_a_moved_mu_fails_on_the_mutant_and_the_first_step_passes(mutant, test, case):
    r = _run(test, case, mutant)
    out = r.stdout[-8000:]
    assert r.returncode == 1, f"{case} did NOT fail on {mutant} (rc {r.returncode}):\n{out}\n{r.stderr[-1500:]}"
    assert "1 failed" in out and "passed" not in out.splitlines()[-1] and "error" not in out.splitlines()[-1], out
    if test == FORCED:
        m = re.search(r"ctm svi teacher-forced: failed steps \[([0-9, ]+)\] of 7", out)
        assert m, out                                                # a comparison of the test failed -- not a loader error or a crash
        failed = [int(x) for x in m.group(1).split(",")]
        assert failed == MOVED_STEPS[case], failed                   # every step after mu has moved, and not step 0
    else:
        assert re.search(r"AssertionError: (ctmsvi\.cbar_rel|ctm\.sigma_rel|ctm\.invsigma_rel)", out), out


def test_the_same_cases_pass_on_the_shipped_library(mutant):
    for test, case in CASES:                                         # the control of the control
        r = _run(test, case, "")
        assert r.returncode == 0 and "1 passed" in r.stdout, (case, r.stdout[-2000:], r.stderr[-1000:])
