"""
CPU tests of csrc/tmvb_handle.h, the owner of what a model handle keeps on the device for its lifetime.

tests/host/handle_owner_main.cpp is a stand-alone program (its own main, its own stub HIP runtime, no HIP library, no device) built with
AddressSanitizer / UBSan: it runs a representative handle life once clean and once per creating call of the sequence with that call failing, and
checks what the header promises -- the stream waits in front of the first free, everything the handle made released exactly once, nothing it only
used ever released, a second release a no-op.  The source checks keep the converted translation units from growing a hand-kept list of frees, or a
copy of a shared entry point, again.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "topicmodelsvb.jl_amd", "csrc")
# the seven converted units and the translation unit each lives in (fCTM shares CTM's)
UNITS = {"lda": "tmvb_lda.hip", "flda": "tmvb_flda.hip", "ctm": "tmvb_ctm.hip", "fctm": "tmvb_ctm.hip", "ctpf": "tmvb_ctpf.hip",
         "lda_svi": "tmvb_lda_svi.hip", "ctm_svi": "tmvb_ctm_svi.hip"}
FAMILIES = ["lda", "flda", "ctm", "fctm", "ctpf"]


def test_handle_owner_release_rules(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on this machine")
    rocm = os.path.dirname(os.path.dirname(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")))
    exe = str(tmp_path / "handle_owner")
    cmd = [gxx, "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "host", "handle_owner_main.cpp")]
    # the sanitizer runtimes inside the program where the toolchain has them as archives: a shared runtime refuses to start when the environment
    # preloads any other library in front of it
    res = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if res.returncode != 0:
        res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, (res.stdout + res.stderr)[-3000:]
    assert "handle owner ok: 29 injected failures and the success path" in res.stdout


@pytest.mark.parametrize("unit", sorted(UNITS))
def test_units_keep_no_release_list(unit):
    src = open(os.path.join(CSRC, UNITS[unit])).read()
    assert '#include "tmvb_handle.h"' in src
    for pat in (r"hipMalloc\(", r"hipFree\(", r"hipEventCreate", r"hipEventDestroy\(", r"dmalloc\("):
        assert not re.search(pat, src), f"{UNITS[unit]}: {pat} -- device memory and events of a handle come from its tmvb_owned (csrc/tmvb_handle.h)"


def _body(src, name):
    """the text between the braces of the definition of the C function `name`; None: the unit does not define it"""
    m = re.search(r'extern "C" int ' + name + r"\([^)]*\)\s*\{", src)
    if m is None:
        return None
    depth, i = 1, m.end()
    while depth:
        depth += {"{": 1, "}": -1}.get(src[i], 0)
        i += 1
    return src[m.end():i - 1]


@pytest.mark.parametrize("family", FAMILIES)
def test_shared_getters_are_written_once(family):
    src = open(os.path.join(CSRC, UNITS[family])).read()
    found = 0
    for what in ("elbo_form", "doc_sweeps", "last_estep_ms"):
        body = _body(src, f"tmvb_{family}_{what}")
        if body is None:
            assert (family, what) == ("fctm", "last_estep_ms"), f"tmvb_{family}_{what} is not defined in {UNITS[family]}"     # (not in include/tmvb.h either)
            continue
        found += 1
        for call in ("hipMemcpyAsync", "hipEventElapsedTime"):
            assert call not in body, f"tmvb_{family}_{what} calls {call} itself: the shared form is in csrc/tmvb_model.h"
    assert found >= 2
