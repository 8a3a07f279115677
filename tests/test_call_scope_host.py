"""
CPU tests of csrc/tmvb_call.h, the owner of the device scratch of one call of a stateless entry point.

tests/host/call_scope_main.cpp is a stand-alone program (its own main, its own stub HIP runtime, no HIP library, no device) built with
AddressSanitizer / UBSan: it runs a representative call once clean and once per HIP call of the sequence with that call failing, and checks
the release order the header promises -- wait for the stream, then device memory and events (each once), then host staging and the result
struct.  The second test keeps the converted translation units from growing a pool, a cleanup lambda or an error macro of their own again.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "topicmodelsvb.jl_amd", "csrc")
UNITS = ["tmvb_heldout.hip", "tmvb_gencorp.hip", "tmvb_coherence.hip", "tmvb_neighbors.hip", "tmvb_topics.hip", "tmvb_ctpf_recs.hip"]


def test_call_scope_release_order(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on this machine")
    rocm = os.path.dirname(os.path.dirname(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")))
    exe = str(tmp_path / "call_scope")
    cmd = [gxx, "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "host", "call_scope_main.cpp")]
    # the sanitizer runtimes inside the program where the toolchain has them as archives: a shared runtime refuses to start when the environment
    # preloads any other library in front of it
    res = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if res.returncode != 0:
        res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, (res.stdout + res.stderr)[-3000:]
    assert "call scope ok: 13 injected failures and the success path" in res.stdout


@pytest.mark.parametrize("unit", UNITS)
def test_units_own_no_device_scratch(unit):
    src = open(os.path.join(CSRC, unit)).read()
    assert '#include "tmvb_call.h"' in src
    for pat in (r"hipMalloc\(", r"hipFree\(", r"hipEventCreate\(", r"hipEventDestroy\(", r"struct \w*_pool", r"auto cleanup", r"#define [A-Z]+_(HIP|TRY)"):
        assert not re.search(pat, src), f"{unit}: {pat} -- device memory and events of a call come from tmvb_call (csrc/tmvb_call.h)"
