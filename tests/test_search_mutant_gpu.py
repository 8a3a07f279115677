"""
NEGATIVE CONTROL of tests/test_search_gpu.py, after the pattern of tests/test_neighbors_mutant_gpu.py: the library with tmvb_search.hip
recompiled under -DTMVB_MUTANT_SEARCH_DROP_LAST_ENTRY=1 (tools/build_mutants.sh: mut_search_drop_last_entry).  Its scan kernel stops the walk
over a query's column segment one entry early: a query of one entry scores 0 everywhere and returns the first n indices, a longer one loses
its last word.  Every floating case of query length 1 and of length 5 must FAIL on it with an assertion of that test, and the same cases
pass on the shipped library.  A wrong-answer library, not a faulting one: the walk reads less, never more.

The mutant library is built here when the tree does not carry a current one, as the other mutant tests do; without a compiler the module
skips.
"""
import hashlib
import os
import subprocess
import sys

import pytest

from test_search_gpu import CASES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "topicmodelsvb.jl_amd")
NAME, UNIT, FLAG = "mut_search_drop_last_entry", "tmvb_search.hip", "-DTMVB_MUTANT_SEARCH_DROP_LAST_ENTRY=1"
TEST = "tests/test_search_gpu.py::test_floating_scores"


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
        if not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")):
            pytest.skip(f"libtmvb_hip_{NAME}.so is not built and there is no hipcc to build it (tools/build_mutants.sh)")
        if not os.path.exists(os.path.join(PKG, "build", UNIT + ".o")):
            import tmvb_amd
            tmvb_amd.pkg.build(force=True)
        subprocess.run([os.path.join(ROOT, "tools", "build_variant.sh"), NAME, UNIT, FLAG], check=True, timeout=1500, capture_output=True)
    return NAME


def _ids(L):
    ids = [f"{TEST}[{'-'.join(str(v) for v in c)}]" for c in CASES if c[1] == L]
    assert len(ids) >= 5                                  # the cover pairs every length with every K
    return ids


def _run(L, variant):
    """every floating case of one query length in one child process"""
    env = dict(os.environ, TMVB_LIB_VARIANT=variant)
    env.pop("TMVB_SEARCH_RECORD", None)
    ids = _ids(L)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider"] + ids, capture_output=True, text=True, env=env, cwd=ROOT,
                       timeout=600)
    return r, len(ids)


@pytest.mark.parametrize("L", [1, 5])
def test_a_query_length_fails_on_the_mutant(mutant, L):
    r, k = _run(L, mutant)
    out = r.stdout[-6000:]
    assert r.returncode == 1, f"L = {L} did NOT fail on {mutant} (rc {r.returncode}):\n{out}\n{r.stderr[-1500:]}"
    assert "AssertionError" in out or "assert " in out, out        # a comparison failed -- not a loader error or a crash
    assert f"{k} failed" in out and "passed" not in out.splitlines()[-1] and "error" not in out.splitlines()[-1], out


def test_the_same_cases_pass_on_the_shipped_library(mutant):
    for L in (1, 5):                                               # the control of the control
        r, k = _run(L, "")
        assert r.returncode == 0 and f"{k} passed" in r.stdout, (L, r.stdout[-2000:], r.stderr[-1000:])
