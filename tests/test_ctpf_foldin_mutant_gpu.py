"""
NEGATIVE CONTROL of tests/test_ctpf_foldin_gpu.py, after the pattern of tests/test_rectopn_mutant_gpu.py: the library with tmvb_ctpf_foldin.hip
recompiled under -DTMVB_MUTANT_FOLDIN_DROP_ZAYIN=1 (tools/build_mutants.sh: mut_foldin_drop_zayin).  Its table kernel leaves the zayin term out of
W: the users are folded in against gimel alone.  Every case of "users against the restatement" (case 1) and of "one sweep is the oracle's
statistic" (case 3) must FAIL on it with an assertion of that test; the empty-library check of case 4 (no W row is read) and predict_ctpf (case 5:
the existing E-step, not this unit) must pass on it, and everything passes on the shipped library.
"""
import hashlib
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "topicmodelsvb.jl_amd")
NAME, UNIT, FLAG = "mut_foldin_drop_zayin", "tmvb_ctpf_foldin.hip", "-DTMVB_MUTANT_FOLDIN_DROP_ZAYIN=1"
FILE = "tests/test_ctpf_foldin_gpu.py"
FAILING = {"test_users_against_the_restatement": 10, "test_one_sweep_is_the_oracles_statistic": 2}       # test: its cases
PASSING = {"test_empty_library_is_e_exactly": 1, "test_predict_ctpf_against_the_oracle": 6}


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


def _run(test, variant):
    """every case of one test in one child process"""
    env = dict(os.environ, TMVB_LIB_VARIANT=variant)
    env.pop("TMVB_TOL_RECORD", None)                      # a recording run never fails a comparison
    return subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider", f"{FILE}::{test}"], capture_output=True, text=True,
                          env=env, cwd=ROOT, timeout=600)


@pytest.mark.parametrize("test", sorted(FAILING))
def test_every_case_that_reads_w_fails_on_the_mutant(mutant, test):
    r = _run(test, mutant)
    k = FAILING[test]
    out = r.stdout[-6000:]
    assert r.returncode == 1, f"{test} did NOT fail on {mutant} (rc {r.returncode}):\n{out}\n{r.stderr[-1500:]}"
    assert "AssertionError" in out or "assert " in out, out        # a comparison failed -- not a loader error or a crash
    assert f"{k} failed" in out and "passed" not in out.splitlines()[-1] and "error" not in out.splitlines()[-1], out


def test_the_cases_without_w_pass_on_the_mutant_and_all_on_the_shipped_library(mutant):
    for test, k in sorted(PASSING.items()):
        r = _run(test, mutant)
        assert r.returncode == 0 and f"{k} passed" in r.stdout, (test, r.stdout[-2000:], r.stderr[-1000:])
    for test, k in sorted(FAILING.items()):                        # the control of the control
        r = _run(test, "")
        assert r.returncode == 0 and f"{k} passed" in r.stdout, (test, r.stdout[-2000:], r.stderr[-1000:])
