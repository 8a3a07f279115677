"""
NEGATIVE CONTROL of tests/test_token_topics_gpu.py, after the pattern of tests/test_heldout_mutant_gpu.py: the library with
tmvb_token_topics.hip recompiled under -DTMVB_MUTANT_TT_TIE_LAST=1 (tools/build_mutants.sh: mut_tt_tie_last).  In its top-t selection the
merge across the lanes of an entry lets the HIGHER topic id win an exact tie of the r bits.  The exact-selection case at K = 50 (four lanes per
entry, integer factors, ties everywhere) must FAIL on it with an assertion of that test; the floating case at K = 50 has no ties and must pass.
Both pass on the shipped library.  A wrong-answer library, not a faulting one: only a comparison of two registers differs.
"""
import hashlib
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "topicmodelsvb.jl_amd")
NAME, UNIT, FLAG = "mut_tt_tie_last", "tmvb_token_topics.hip", "-DTMVB_MUTANT_TT_TIE_LAST=1"
EXACT = "tests/test_token_topics_gpu.py::test_exact_selection_with_ties[50]"
FLOATING = "tests/test_token_topics_gpu.py::test_floating_factors[50]"


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
    env.pop("TMVB_TT_RECORD", None)
    return subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", test_id], capture_output=True, text=True,
                          env=env, cwd=ROOT, timeout=600)


def test_the_tie_case_fails_on_the_mutant(mutant):
    r = _run(EXACT, mutant)
    out = r.stdout[-3000:]
    assert r.returncode == 1, f"{EXACT} did NOT fail on {mutant} (rc {r.returncode}):\n{out}\n{r.stderr[-1500:]}"
    assert "AssertionError" in out or "assert " in out, out        # a comparison failed -- not a loader error or a crash
    assert "1 failed" in out and "error" not in out.splitlines()[-1], out


def test_the_floating_case_passes_on_the_mutant_and_both_on_the_shipped_library(mutant):
    r = _run(FLOATING, mutant)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-1000:])
    for case in (EXACT, FLOATING):                                 # the control of the control
        r = _run(case, "")
        assert r.returncode == 0, (case, r.stdout[-2000:], r.stderr[-1000:])
