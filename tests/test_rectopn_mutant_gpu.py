"""
NEGATIVE CONTROL of tests/test_rectopn_gpu.py, after the pattern of tests/test_recranks_mutant_gpu.py: the library with tmvb_rectopn.hip
recompiled under -DTMVB_MUTANT_TOPN_MISS_LAST_EXCL=1 (tools/build_mutants.sh: mut_rectopn_last_excl).  The binary search of its scan kernel
never finds the last id of an exclusion list -- a search off by one at its upper end.  Every exact case with exclusions "random" (query 0
always lists the planted best row, the last id there is) and "all-but-three" (every query does) must FAIL on it with an assertion of that
test, and the cases without exclusions must pass.
"""
import hashlib
import os
import subprocess
import sys

import pytest

from test_rectopn_gpu import CASES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "topicmodelsvb.jl_amd")
NAME, UNIT, FLAG = "mut_rectopn_last_excl", "tmvb_rectopn.hip", "-DTMVB_MUTANT_TOPN_MISS_LAST_EXCL=1"
TEST = "tests/test_rectopn_gpu.py::test_exact_topn"


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


def _ids(mode):
    ids = [f"{TEST}[{'-'.join(str(v) for v in c)}]" for c in CASES if c[4] == mode]
    assert len(ids) >= 8                                  # the cover pairs every exclusion mode with every Md
    return ids


def _run(mode, variant):
    """every exact case of one exclusion mode in one child process"""
    env = dict(os.environ, TMVB_LIB_VARIANT=variant)
    ids = _ids(mode)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider"] + ids, capture_output=True, text=True, env=env, cwd=ROOT,
                       timeout=600)
    return r, len(ids)


@pytest.mark.parametrize("mode", ["random", "all-but-three"])
def test_every_case_with_exclusions_fails_on_the_mutant(mutant, mode):
    r, k = _run(mode, mutant)
    out = r.stdout[-6000:]
    assert r.returncode == 1, f"{mode} did NOT fail on {mutant} (rc {r.returncode}):\n{out}\n{r.stderr[-1500:]}"
    assert "AssertionError" in out or "assert " in out, out        # a comparison failed -- not a loader error or a crash
    assert f"{k} failed" in out and "passed" not in out.splitlines()[-1] and "error" not in out.splitlines()[-1], out


def test_the_cases_without_exclusions_pass_on_the_mutant_and_all_on_the_shipped_library(mutant):
    r, k = _run("none", mutant)
    assert r.returncode == 0 and f"{k} passed" in r.stdout, (r.stdout[-2000:], r.stderr[-1000:])
    for mode in ("random", "all-but-three"):                       # the control of the control
        r, k = _run(mode, "")
        assert r.returncode == 0 and f"{k} passed" in r.stdout, (mode, r.stdout[-2000:], r.stderr[-1000:])
