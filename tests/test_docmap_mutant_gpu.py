"""
NEGATIVE CONTROL of tests/test_docmap_gpu.py, after the pattern of tests/test_kmeans_mutant_gpu.py (whose stamp logic it reuses): the library with
tmvb_docmap.hip recompiled under -DTMVB_MUTANT_MAP_Z_SELF=1 (tools/build_mutants.sh: mut_docmap_z_with_self).  Its normaliser keeps the M self terms:
Z = the blocked sum of zrow, without - M.  The Z and grad assertions of the teacher-forced cases must FAIL on it with an assertion of that test; the
rep / zrow / att assertions and the affinity tests must pass.  Everything passes on the shipped library.  A wrong-answer library, not a faulting one:
one subtraction is missing.
"""
import os
import subprocess
import sys

import pytest

import test_neighbors_mutant_gpu as nm
from test_docmap_gpu import AFF_MS, AFF_NS, FORCE_MS, SCALES, SPLITS

pytestmark = pytest.mark.gpu
ROOT, PKG = nm.ROOT, nm.PKG
NAME, UNIT, FLAG = "mut_docmap_z_with_self", "tmvb_docmap.hip", "-DTMVB_MUTANT_MAP_Z_SELF=1"
FILE = "tests/test_docmap_gpu.py::"
FORCE = [(M, s, j) for M in FORCE_MS for s in SCALES for j in SPLITS]
AFFINITY = [(M, n) for M in AFF_MS for n in AFF_NS]


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
    env.pop("TMVB_DOCMAP_RECORD", None)
    ids = [f"{FILE}{test}[{'-'.join(str(v) for v in c)}]" for c in cases]
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider"] + ids, capture_output=True, text=True, env=env, cwd=ROOT,
                       timeout=600)
    return r, len(ids)


def test_z_and_gradient_fail_on_the_mutant(mutant):
    r, k = _run("test_force_z_and_gradient", FORCE, mutant)
    out = r.stdout[-6000:]
    assert r.returncode == 1, f"the cases did NOT fail on {mutant} (rc {r.returncode}):\n{out}\n{r.stderr[-1500:]}"
    assert "AssertionError" in out or "assert " in out, out        # a comparison failed -- not a loader error or a crash
    assert f"{k} failed" in out and "passed" not in out.splitlines()[-1] and "error" not in out.splitlines()[-1], out


def test_pieces_and_affinity_pass_on_the_mutant_and_all_on_the_shipped_library(mutant):
    r, k = _run("test_force_pieces", FORCE, mutant)
    assert r.returncode == 0 and f"{k} passed" in r.stdout, (r.stdout[-2000:], r.stderr[-1000:])
    r, k = _run("test_affinity", AFFINITY, mutant)
    assert r.returncode == 0 and f"{k} passed" in r.stdout, (r.stdout[-2000:], r.stderr[-1000:])
    r, k = _run("test_force_z_and_gradient", FORCE, "")           # the control of the control
    assert r.returncode == 0 and f"{k} passed" in r.stdout, (r.stdout[-2000:], r.stderr[-1000:])
