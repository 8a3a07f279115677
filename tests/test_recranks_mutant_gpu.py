"""
NEGATIVE CONTROL of tests/test_recranks_gpu.py, after the pattern of tests/test_neighbors_mutant_gpu.py: the library with tmvb_recranks.hip
recompiled under -DTMVB_MUTANT_RK_DROP_TAIL=1 (tools/build_mutants.sh: mut_recranks_tail).  Its scan kernel skips the last, partial database
tile -- what a tile loop bounded by Md / TMVB_NB_TILE_DB loses.  Every exact-rank case with Md = T + 1 and Md = 2 T + 2 must FAIL on it with an
assertion of that test (the last database row comes before every target there), and the cases with Md = T (no partial tile) must pass.
"""
import hashlib
import os
import subprocess
import sys

import pytest

from test_recranks_gpu import CASES, T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "topicmodelsvb.jl_amd")
NAME, UNIT, FLAG = "mut_recranks_tail", "tmvb_recranks.hip", "-DTMVB_MUTANT_RK_DROP_TAIL=1"
TEST = "tests/test_recranks_gpu.py::test_exact_ranks"


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


def _ids(Md):
    ids = [f"{TEST}[{'-'.join(str(v) for v in c)}]" for c in CASES if c[0] == Md]
    assert len(ids) >= 5                                  # the cover pairs every Md with every K
    return ids


def _run(Md, variant):
    """every exact-rank case of one Md in one child process"""
    env = dict(os.environ, TMVB_LIB_VARIANT=variant)
    ids = _ids(Md)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider"] + ids, capture_output=True, text=True, env=env, cwd=ROOT,
                       timeout=600)
    return r, len(ids)


@pytest.mark.parametrize("Md", [T + 1, 2 * T + 2])
def test_a_partial_tile_case_fails_on_the_mutant(mutant, Md):
    r, k = _run(Md, mutant)
    out = r.stdout[-6000:]
    assert r.returncode == 1, f"Md = {Md} did NOT fail on {mutant} (rc {r.returncode}):\n{out}\n{r.stderr[-1500:]}"
    assert "AssertionError" in out or "assert " in out, out        # a comparison failed -- not a loader error or a crash
    assert f"{k} failed" in out and "passed" not in out.splitlines()[-1] and "error" not in out.splitlines()[-1], out


def test_the_whole_tile_case_passes_on_the_mutant_and_all_on_the_shipped_library(mutant):
    r, k = _run(T, mutant)
    assert r.returncode == 0 and f"{k} passed" in r.stdout, (r.stdout[-2000:], r.stderr[-1000:])
    for Md in (T + 1, 2 * T + 2):                                  # the control of the control
        r, k = _run(Md, "")
        assert r.returncode == 0 and f"{k} passed" in r.stdout, (Md, r.stdout[-2000:], r.stderr[-1000:])
