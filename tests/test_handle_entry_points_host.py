"""
The entry points the five model families share (csrc/tmvb_model.h: the ELBO-form getter, the sweep counts and their histogram, the last E-step's
time, tmvb_*_bind_stats) answer a NULL handle and a NULL out-argument as they always did: same return code, same tmvb_last_error text, byte for
byte.  These checks return before any HIP call, so the library is loaded here without a device.

EXPECTED was recorded by running CALLS against a library built from the commit before the shared functions existed (five hand-written copies).
"""
import ctypes as C

import pytest

EINVAL, ESHAPE = 1, 2
HANDLE = "handle"        # a zeroed block of memory standing in for a handle (K = V = 0, no E-step timed): only passed where a check refuses before any HIP call
OUT = "out"              # a valid out-argument

# (function, arguments)
CALLS = [
    ("tmvb_lda_elbo_form", (None, OUT)), ("tmvb_lda_elbo_form", (HANDLE, None)),
    ("tmvb_lda_doc_sweeps", (None, OUT)), ("tmvb_lda_doc_sweeps", (None, None)),
    ("tmvb_lda_sweep_hist", (None, OUT, 4)), ("tmvb_lda_sweep_hist", (HANDLE, None, 4)), ("tmvb_lda_sweep_hist", (HANDLE, OUT, 0)),
    ("tmvb_lda_last_estep_ms", (None, OUT)), ("tmvb_lda_last_estep_ms", (HANDLE, None)), ("tmvb_lda_last_estep_ms", (HANDLE, OUT)),
    ("tmvb_lda_bind_stats", (None, OUT, 8)), ("tmvb_lda_bind_stats", (HANDLE, None, 8)), ("tmvb_lda_bind_stats", (HANDLE, OUT, -1)),
    ("tmvb_flda_elbo_form", (None, OUT)), ("tmvb_flda_elbo_form", (HANDLE, None)),
    ("tmvb_flda_doc_sweeps", (None, OUT)), ("tmvb_flda_doc_sweeps", (None, None)),
    ("tmvb_flda_last_estep_ms", (None, OUT)), ("tmvb_flda_last_estep_ms", (HANDLE, None)), ("tmvb_flda_last_estep_ms", (HANDLE, OUT)),
    ("tmvb_ctm_elbo_form", (None, OUT)), ("tmvb_ctm_elbo_form", (HANDLE, None)),
    ("tmvb_ctm_doc_sweeps", (None, OUT)), ("tmvb_ctm_doc_sweeps", (None, None)),
    ("tmvb_ctm_sweep_hist", (None, OUT, 4, OUT)), ("tmvb_ctm_sweep_hist", (HANDLE, None, 4, OUT)), ("tmvb_ctm_sweep_hist", (HANDLE, OUT, 0, None)),
    ("tmvb_ctm_last_estep_ms", (None, OUT)), ("tmvb_ctm_last_estep_ms", (HANDLE, None)), ("tmvb_ctm_last_estep_ms", (HANDLE, OUT)),
    ("tmvb_ctm_bind_stats", (None, OUT, 8)), ("tmvb_ctm_bind_stats", (HANDLE, None, 8)), ("tmvb_ctm_bind_stats", (HANDLE, OUT, -1)),
    ("tmvb_fctm_elbo_form", (None, OUT)), ("tmvb_fctm_elbo_form", (HANDLE, None)),
    ("tmvb_fctm_doc_sweeps", (None, OUT)), ("tmvb_fctm_doc_sweeps", (None, None)),
    ("tmvb_fctm_sweep_hist", (None, OUT, 4, OUT)), ("tmvb_fctm_sweep_hist", (None, None, 4, None)),
    ("tmvb_ctpf_elbo_form", (None, OUT)), ("tmvb_ctpf_elbo_form", (HANDLE, None)),
    ("tmvb_ctpf_doc_sweeps", (None, OUT)), ("tmvb_ctpf_doc_sweeps", (None, None)),
    ("tmvb_ctpf_sweep_hist", (None, OUT, 4)), ("tmvb_ctpf_sweep_hist", (HANDLE, None, 4)), ("tmvb_ctpf_sweep_hist", (HANDLE, OUT, 0)),
    ("tmvb_ctpf_last_estep_ms", (None, OUT)), ("tmvb_ctpf_last_estep_ms", (HANDLE, None)), ("tmvb_ctpf_last_estep_ms", (HANDLE, OUT)),
    ("tmvb_ctpf_bind_stats", (None, OUT, 8)), ("tmvb_ctpf_bind_stats", (HANDLE, None, 8)), ("tmvb_ctpf_bind_stats", (HANDLE, OUT, -1)),
]

EXPECTED = [
    (1, 'tmvb_lda_elbo_form: NULL argument'),
    (1, 'tmvb_lda_elbo_form: NULL argument'),
    (1, 'tmvb_lda_doc_sweeps: NULL argument'),
    (1, 'tmvb_lda_doc_sweeps: NULL argument'),
    (1, 'tmvb_lda_sweep_hist: bad argument'),
    (1, 'tmvb_lda_sweep_hist: bad argument'),
    (1, 'tmvb_lda_sweep_hist: bad argument'),
    (1, 'tmvb_lda_last_estep_ms: NULL argument'),
    (1, 'tmvb_lda_last_estep_ms: NULL argument'),
    (1, 'tmvb_lda_last_estep_ms: E-step timing is off (set TMVB_ESTEP_TIMING=1 before creating the model)'),
    (1, 'tmvb_lda_bind_stats: NULL argument'),
    (1, 'tmvb_lda_bind_stats: NULL argument'),
    (2, 'tmvb_lda_bind_stats: buffer holds -1 floats, need 0'),
    (1, 'tmvb_flda_elbo_form: NULL argument'),
    (1, 'tmvb_flda_elbo_form: NULL argument'),
    (1, 'tmvb_flda_doc_sweeps: NULL argument'),
    (1, 'tmvb_flda_doc_sweeps: NULL argument'),
    (1, 'tmvb_flda_last_estep_ms: NULL argument'),
    (1, 'tmvb_flda_last_estep_ms: NULL argument'),
    (1, 'tmvb_flda_last_estep_ms: no E-step has run'),
    (1, 'tmvb_ctm_elbo_form: NULL argument'),
    (1, 'tmvb_ctm_elbo_form: NULL argument'),
    (1, 'tmvb_ctm_doc_sweeps: NULL argument'),
    (1, 'tmvb_ctm_doc_sweeps: NULL argument'),
    (1, 'tmvb_ctm_sweep_hist: bad argument'),
    (1, 'tmvb_ctm_sweep_hist: bad argument'),
    (1, 'tmvb_ctm_sweep_hist: bad argument'),
    (1, 'tmvb_ctm_last_estep_ms: NULL argument'),
    (1, 'tmvb_ctm_last_estep_ms: NULL argument'),
    (1, 'tmvb_ctm_last_estep_ms: no E-step has run'),
    (1, 'tmvb_ctm_bind_stats: NULL argument'),
    (1, 'tmvb_ctm_bind_stats: NULL argument'),
    (2, 'tmvb_ctm_bind_stats: buffer holds -1 floats, need 0'),
    (1, 'tmvb_fctm_elbo_form: NULL argument'),
    (1, 'tmvb_fctm_elbo_form: NULL argument'),
    (1, 'tmvb_fctm_doc_sweeps: handle is NULL'),
    (1, 'tmvb_fctm_doc_sweeps: handle is NULL'),
    (1, 'tmvb_fctm_sweep_hist: handle is NULL'),
    (1, 'tmvb_fctm_sweep_hist: handle is NULL'),
    (1, 'tmvb_ctpf_elbo_form: NULL argument'),
    (1, 'tmvb_ctpf_elbo_form: NULL argument'),
    (1, 'tmvb_ctpf_doc_sweeps: NULL argument'),
    (1, 'tmvb_ctpf_doc_sweeps: NULL argument'),
    (1, 'tmvb_ctpf_sweep_hist: bad argument'),
    (1, 'tmvb_ctpf_sweep_hist: bad argument'),
    (1, 'tmvb_ctpf_sweep_hist: bad argument'),
    (1, 'tmvb_ctpf_last_estep_ms: NULL argument'),
    (1, 'tmvb_ctpf_last_estep_ms: NULL argument'),
    (1, 'tmvb_ctpf_last_estep_ms: E-step timing is off (set TMVB_ESTEP_TIMING=1 before creating the model)'),
    (1, 'tmvb_ctpf_bind_stats: NULL argument'),
    (1, 'tmvb_ctpf_bind_stats: NULL argument'),
    (2, 'tmvb_ctpf_bind_stats: buffer holds -1 floats, need 0'),
]


def run_call(L, fn, args):
    """-> (return code, tmvb_last_error text) of one call of CALLS against the loaded library L"""
    handle, out = C.create_string_buffer(1 << 16), C.create_string_buffer(256)
    cargs = []
    for a in args:
        if a is None:
            cargs.append(C.c_void_p(None))
        elif a == HANDLE:
            cargs.append(C.cast(handle, C.c_void_p))
        elif a == OUT:
            cargs.append(C.cast(out, C.c_void_p))
        else:
            cargs.append(C.c_int64(a) if fn.endswith("_bind_stats") else C.c_int32(a))
    f = getattr(L, fn)
    f.restype, f.argtypes = C.c_int, None
    L.tmvb_last_error.restype = C.c_char_p
    rc = f(*cargs)
    return rc, L.tmvb_last_error().decode()


def test_the_table_covers_every_call():
    assert len(EXPECTED) == len(CALLS)
    for fam in ("lda", "flda", "ctm", "fctm", "ctpf"):
        assert any(fn.startswith(f"tmvb_{fam}_") for fn, _ in CALLS)


@pytest.mark.parametrize("i", range(len(CALLS)), ids=[f"{fn}-{k}" for k, (fn, _) in enumerate(CALLS)])
def test_null_arguments_answer_as_before(tmvb, i):
    tmvb.build()
    L = C.CDLL(tmvb.LIB_PATH)
    fn, args = CALLS[i]
    rc, msg = run_call(L, fn, args)
    assert (rc, msg) == EXPECTED[i]
    assert rc in (EINVAL, ESHAPE) and msg.startswith(fn + ": ")
