"""
NEGATIVE CONTROL of tests/test_group_topics_gpu.py, after the pattern of tests/test_topic_compare_mutant_gpu.py (whose stamp logic it reuses through
tests/test_neighbors_mutant_gpu.py): the library with tmvb_group_topics.hip recompiled under -DTMVB_MUTANT_GT_SEG_CUT=1 (tools/build_mutants.sh:
mut_gt_seg_cut).  Its combine kernel leaves out the last segment of a run of more than one segment -- what a segment loop bounded by nseg - 1 loses.
Every exact case with a run longer than TMVB_GT_SEG ("long") must FAIL on it with an assertion of that test (the restatement with cut_mutant=True
gives another S there); the cases whose runs stop at TMVB_GT_SEG ("short") must pass.  All pass on the shipped library.  A wrong-answer library, not
a faulting one: a loop bound differs.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import group_topics_restatement as gr
import test_neighbors_mutant_gpu as nm
from test_group_topics_gpu import CASES, V, exact_corpus

pytestmark = pytest.mark.gpu
ROOT, PKG = nm.ROOT, nm.PKG
NAME, UNIT, FLAG = "mut_gt_seg_cut", "tmvb_group_topics.hip", "-DTMVB_MUTANT_GT_SEG_CUT=1"
TEST = "tests/test_group_topics_gpu.py::test_exact"


def _shows(case):
    """does the sum without the last segment of the long runs differ on this case?  (responsibilities of any positive kind do: ones)"""
    import tmvb_amd
    pc, group = exact_corpus(tmvb_amd.pkg, case[1], case[2])
    ones = np.ones((len(pc.terms), 1), dtype=np.float32)
    a = gr.stats(ones, pc.doc_ptr, pc.terms, pc.counts, group, case[1], V)["S"]
    return not np.array_equal(a, gr.stats(ones, pc.doc_ptr, pc.terms, pc.counts, group, case[1], V, cut_mutant=True)["S"])


SHOWING = [c for c in CASES if c[2] == "long" and _shows(c)]
CONTROL = [c for c in CASES if c[2] == "short" and not _shows(c)]


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


def _run(cases, variant):
    """the given cases of the exact test in one child process"""
    env = dict(os.environ, TMVB_LIB_VARIANT=variant)
    env.pop("TMVB_GT_RECORD", None)
    ids = [f"{TEST}[{'-'.join(str(v) for v in c)}]" for c in cases]
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider"] + ids, capture_output=True, text=True, env=env, cwd=ROOT,
                       timeout=600)
    return r, len(ids)


def test_cases_with_a_run_longer_than_a_segment_fail_on_the_mutant(mutant):
    assert len(SHOWING) >= 12
    r, k = _run(SHOWING, mutant)
    out = r.stdout[-6000:]
    assert r.returncode == 1, f"the cases did NOT fail on {mutant} (rc {r.returncode}):\n{out}\n{r.stderr[-1500:]}"
    assert "AssertionError" in out or "assert " in out, out        # a comparison failed -- not a loader error or a crash
    assert f"{k} failed" in out and "passed" not in out.splitlines()[-1] and "error" not in out.splitlines()[-1], out


def test_short_run_cases_pass_on_the_mutant_and_all_on_the_shipped_library(mutant):
    assert len(CONTROL) >= 4
    r, k = _run(CONTROL, mutant)
    assert r.returncode == 0 and f"{k} passed" in r.stdout, (r.stdout[-2000:], r.stderr[-1000:])
    r, k = _run(SHOWING, "")                                       # the control of the control
    assert r.returncode == 0 and f"{k} passed" in r.stdout, (r.stdout[-2000:], r.stderr[-1000:])
