"""
NEGATIVE CONTROL of tests/test_coherence_gpu.py, after the pattern of tests/test_heldout_mutant_gpu.py: the library with tmvb_coherence.hip
recompiled under -DTMVB_MUTANT_CODF_DROP_TAIL=1 (tools/build_mutants.sh: mut_coherence_tail).  Its pair kernel skips the last, partial
64-document word of the bit matrix -- what a word loop bounded by M / 64 loses.  The M = 65 and M = 130 cases of the count test must FAIL on
it with an assertion of that test, and the M = 64 cases (no partial word) must pass.
"""
import hashlib
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "topicmodelsvb.jl_amd")
NAME, UNIT, FLAG = "mut_coherence_tail", "tmvb_coherence.hip", "-DTMVB_MUTANT_CODF_DROP_TAIL=1"
TEST = "tests/test_coherence_gpu.py::test_counts_against_numpy"
KN = ("1-2", "3-10", "7-64")


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


def _run(M, variant):
    """the three (K, N) cases of one M in one child process"""
    env = dict(os.environ, TMVB_LIB_VARIANT=variant)
    ids = [f"{TEST}[{M}-{kn}]" for kn in KN]
    return subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider"] + ids, capture_output=True, text=True, env=env, cwd=ROOT,
                          timeout=600)


@pytest.mark.parametrize("M", [65, 130])
def test_a_partial_word_case_fails_on_the_mutant(mutant, M):
    r = _run(M, mutant)
    out = r.stdout[-6000:]
    assert r.returncode == 1, f"M = {M} did NOT fail on {mutant} (rc {r.returncode}):\n{out}\n{r.stderr[-1500:]}"
    assert "AssertionError" in out or "assert " in out, out        # a comparison failed -- not a loader error or a crash
    assert "3 failed" in out and "passed" not in out.splitlines()[-1] and "error" not in out.splitlines()[-1], out


def test_the_whole_word_case_passes_on_the_mutant_and_all_on_the_shipped_library(mutant):
    r = _run(64, mutant)
    assert r.returncode == 0 and "3 passed" in r.stdout, (r.stdout[-2000:], r.stderr[-1000:])
    for M in (65, 130):                                            # the control of the control
        r = _run(M, "")
        assert r.returncode == 0 and "3 passed" in r.stdout, (M, r.stdout[-2000:], r.stderr[-1000:])
