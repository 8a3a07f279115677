"""
NEGATIVE CONTROL of tests/test_heldout_gpu.py, after the pattern of tests/test_mutants_gpu.py: the library with tmvb_heldout.hip recompiled
under -DTMVB_MUTANT_HELDOUT_DROP_TAIL=1 (tools/build_mutants.sh: mut_heldout_tail).  Its scoring kernel drops the last, partial 16-byte chunk
of a beta row -- the topics past the last multiple of four, what a careless vectorisation of the dot product loses.  The K = 50 and K = 70
cases of the log-likelihood test must FAIL on it with an assertion of that test, and the K = 64 case (no partial chunk) must pass.
"""
import hashlib
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "topicmodelsvb.jl_amd")
NAME, UNIT, FLAG = "mut_heldout_tail", "tmvb_heldout.hip", "-DTMVB_MUTANT_HELDOUT_DROP_TAIL=1"
TEST = "tests/test_heldout_gpu.py::test_loglik_against_numpy_fp64"


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


def _run(test_id, variant):
    env = dict(os.environ, TMVB_LIB_VARIANT=variant)
    return subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", test_id], capture_output=True, text=True,
                          env=env, cwd=ROOT, timeout=600)


@pytest.mark.parametrize("case", ["50-60-0-0.0", "70-60-0-0.0"])
def test_a_partial_chunk_case_fails_on_the_mutant(mutant, case):
    r = _run(f"{TEST}[{case}]", mutant)
    out = r.stdout[-3000:]
    assert r.returncode == 1, f"{case} did NOT fail on {mutant} (rc {r.returncode}):\n{out}\n{r.stderr[-1500:]}"
    assert "AssertionError" in out or "assert " in out, out        # a comparison failed -- not a loader error or a crash
    assert "1 failed" in out and "error" not in out.splitlines()[-1], out


def test_the_whole_chunk_case_passes_on_the_mutant_and_all_on_the_shipped_library(mutant):
    r = _run(f"{TEST}[64-60-0-0.0]", mutant)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-1000:])
    for case in ("50-60-0-0.0", "70-60-0-0.0"):                    # the control of the control
        r = _run(f"{TEST}[{case}]", "")
        assert r.returncode == 0, (case, r.stdout[-2000:], r.stderr[-1000:])
