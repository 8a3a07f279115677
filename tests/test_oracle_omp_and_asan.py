"""
CPU tests of the oracle's own plumbing (test infrastructure): the OpenMP document-parallel E-steps (what bench.py's
cpu_baseline times) must agree with the sequential restatement on condensed corpora, and the oracle must run clean under
AddressSanitizer / UBSan (`make -C oracle asan`) on one golden case per model.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def _nsf(tmvb, M=120, V=500, seed=5):
    pc = tmvb.syn_nsf(M=M, V=V, seed=seed)
    return pc


def test_omp_estep_matches_sequential_lda_ctm(tmvb, oracle):
    pc = _nsf(tmvb)
    K = 6
    beta0 = tmvb.dirichlet_rows(K, pc.V, seed=3)
    csr = oracle.CSR(pc.doc_ptr, pc.terms, pc.counts, pc.V)
    a, b = oracle.LDA(csr, K, beta0), oracle.LDA(csr, K, beta0)
    for _ in range(2):
        sa = a.estep(); a.update_beta(); a.update_alpha()
        sb = b.estep(omp_threads=3); b.update_beta(); b.update_alpha()
        assert np.array_equal(sa, sb)                       # per-document sweep counts (the full-size parity checks use them)
    np.testing.assert_allclose(a.gamma, b.gamma, rtol=1e-12)
    np.testing.assert_allclose(a.beta, b.beta, rtol=1e-11, atol=1e-300)
    a, b = oracle.CTM(csr, K, beta0), oracle.CTM(csr, K, beta0)
    for _ in range(2):
        sa = a.estep(); a.update_beta(); a.update_sigma_mu()
        sb = b.estep(omp_threads=3); b.update_beta(); b.update_sigma_mu()
        assert np.array_equal(sa, sb) and a.newton_steps == b.newton_steps == int(b.newton_per_doc.sum())
    np.testing.assert_allclose(a.lam, b.lam, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(a.beta, b.beta, rtol=1e-9, atol=1e-300)


def test_omp_estep_matches_sequential_filtered(tmvb, oracle):
    pc = _nsf(tmvb, M=80, V=300, seed=8)
    K = 5
    beta0 = tmvb.dirichlet_rows(K, pc.V, seed=3); kappa0 = tmvb.dirichlet_rows(1, pc.V, seed=9)[0]
    csr = oracle.CSR(pc.doc_ptr, pc.terms, pc.counts, pc.V)
    a, b = oracle.fLDA(csr, K, beta0, kappa0), oracle.fLDA(csr, K, beta0, kappa0)
    for _ in range(2):
        a.estep(); a.mstep()
        b.estep(omp_threads=3); b.mstep()
    np.testing.assert_allclose(a.tau, b.tau, rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(a.beta, b.beta, rtol=1e-10, atol=1e-300)
    np.testing.assert_allclose(a.kappa, b.kappa, rtol=1e-10, atol=1e-300)
    assert abs(a.eta - b.eta) <= 1e-13
    a, b = oracle.fCTM(csr, K, beta0, kappa0), oracle.fCTM(csr, K, beta0, kappa0)
    for _ in range(2):
        a.estep(); a.mstep()
        b.estep(omp_threads=3); b.mstep()
    np.testing.assert_allclose(a.tau, b.tau, rtol=1e-9, atol=1e-13)
    np.testing.assert_allclose(a.lam, b.lam, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(a.kappa, b.kappa, rtol=1e-9, atol=1e-300)


def _plain_omp(m, kind, threads=3):
    """the OpenMP entry point without per-document outputs (orc_flda_estep_omp / orc_fctm_estep_omp), as cpu_baseline calls it"""
    from oracle import oracle as oc
    C = oc.C
    a = (*m._corp_args(), oc.c_i64(0), oc.c_i64(m.M), oc.c_dbl(m.eta))
    if kind == "flda":
        vt = 1.0 / m.K ** 2
        oc.lib().orc_flda_estep_omp(*a, oc._pd(m.alpha), oc._pd(m.kappa), oc._pd(m.beta), oc._pd(m.beta_temp), oc._pd(m.kappa_temp),
                                    oc._pd(m.gamma), oc._pd(m.Elogtheta), oc._pd(m.Elogtheta_old), oc._pd(m.tau), oc._pd(m.tau_old),
                                    C.c_int(10), oc.c_dbl(vt), C.c_int(threads))
    else:
        vt = 1.0 / m.K ** 2
        oc.lib().orc_fctm_estep_omp(*a, oc._pd(m.kappa), oc._pd(m.mu), oc._pd(m.invsigma), oc._pd(m.beta), oc._pd(m.beta_temp),
                                    oc._pd(m.kappa_temp), oc._pd(m.lam), oc._pd(m.lam_old), oc._pd(m.vsq), oc._pd(m.logzeta), oc._pd(m.tau),
                                    oc._pd(m.tau_old), C.c_int(1000), oc.c_dbl(vt), C.c_int(10), oc.c_dbl(vt), C.c_int(threads))


@pytest.mark.parametrize("kind", ["flda", "fctm"])
def test_omp_sw_sweep_counts_filtered(tmvb, oracle, kind):
    """orc_flda/fctm_estep_omp_sw (what oracle/parity.py's fix-up runs on): the per-document sweep counts are the sequential E-step's,
    the state is the plain OpenMP entry point's, and re-running every document with its own reported sweep count and vtol = 0 -- the
    fix-up, applied to all of them -- reproduces that state and its statistics"""
    pc = _nsf(tmvb, M=80, V=300, seed=8)
    K = 5
    beta0 = tmvb.dirichlet_rows(K, pc.V, seed=3); kappa0 = tmvb.dirichlet_rows(1, pc.V, seed=9)[0]
    csr = oracle.CSR(pc.doc_ptr, pc.terms, pc.counts, pc.V)
    cls = oracle.fLDA if kind == "flda" else oracle.fCTM
    docf = ("gamma", "Elogtheta") if kind == "flda" else ("lam", "vsq", "logzeta")
    seq, sw_m, plain, pinned = (cls(csr, K, beta0, kappa0) for _ in range(4))
    for it in range(2):                                             # the cold start and the state one iteration later
        s_seq = seq.estep()
        s_sw = sw_m.estep(omp_threads=3)
        _plain_omp(plain, kind)
        assert np.array_equal(s_seq, s_sw) and s_sw.dtype == np.int32 and len(s_sw) == pc.M, kind
        assert len(np.unique(s_sw)) >= 2, np.unique(s_sw)           # the default rule left documents at different sweeps
        if kind == "fctm":
            assert sw_m.newton_steps == seq.newton_steps and len(sw_m.newton_per_doc) == pc.M
        for n in docf + ("tau", "tau_old"):
            assert np.array_equal(getattr(sw_m, n), getattr(plain, n)), (kind, n)          # documents are independent: bit for bit
        for n in docf + ("tau", "tau_old", "beta_temp", "kappa_temp"):
            # (the statistics' summation order follows the dynamic schedule: not bit for bit between two OpenMP runs)
            np.testing.assert_allclose(getattr(sw_m, n), getattr(plain, n), rtol=1e-12, atol=1e-300, err_msg=f"{kind} {n}")
            np.testing.assert_allclose(getattr(sw_m, n), getattr(seq, n), rtol=1e-10, atol=1e-13, err_msg=f"{kind} {n}")
        for d in range(pc.M):                                       # document by document, each with its own sweep count, through _sw
            s1 = pinned.estep(viter=int(s_sw[d]), vtol=0.0, d0=d, d1=d + 1, omp_threads=2)
            assert s1.tolist() == [s_sw[d]]
        for n in docf + ("tau", "tau_old"):
            assert np.array_equal(getattr(pinned, n), getattr(plain, n)), (kind, n)
        np.testing.assert_allclose(pinned.beta_temp, plain.beta_temp, rtol=1e-12, atol=1e-300)
        np.testing.assert_allclose(pinned.kappa_temp, plain.kappa_temp, rtol=1e-12, atol=1e-300)
        seq.mstep()
        from oracle import parity
        for m in (sw_m, plain, pinned):                             # all four from the same state again (the statistics' order moves the last bits)
            for n in (parity.FLDA_FIELDS if kind == "flda" else parity.FCTM_FIELDS) + ("beta_temp", "kappa_temp"):
                v = getattr(seq, n)
                setattr(m, n, np.array(v, copy=True, order="F") if isinstance(v, np.ndarray) else v)


ASAN_SCRIPT = r'''
import ctypes as C, os, sys, numpy as np
sys.path.insert(0, sys.argv[1])
from oracle import oracle as oc
oc._LIB_PATH = os.path.join(sys.argv[1], "oracle", "libtmvb_oracle_asan.so")
oc._lib = None
G = os.path.join(sys.argv[1], "tests", "golden")
def load(n):
    z = np.load(os.path.join(G, n + ".npz")); return {k: z[k] for k in z.files}
g = load("lda_m30_v50_k70_empty")
m = oc.LDA(oc.CSR(g["doc_ptr"], g["terms"], g["counts"], int(g["V"])), int(g["K"]), g["beta0"])
t = m.train(iter=3, tol=0.0, checkelbo=1); assert np.all(np.isfinite(t))
m.estep(omp_threads=2); m.update_beta()
g = load("ctm_m40_v60_k5")
m = oc.CTM(oc.CSR(g["doc_ptr"], g["terms"], g["counts"], int(g["V"])), int(g["K"]), g["beta0"])
t = m.train(iter=2, tol=0.0, checkelbo=1); assert np.all(np.isfinite(t))
m.estep(omp_threads=2)
g = load("ctpf_m30_v40_u12_k6_r1")
m = oc.CTPF(oc.CSR(g["doc_ptr"], g["terms"], g["counts"], int(g["V"]), g["rdr_ptr"], g["readers"], g["ratings"], int(g["U"])), int(g["K"]), g["alef0"])
t = m.train(iter=2, tol=0.0, checkelbo=1); assert np.all(np.isfinite(t))
m.estep(omp_threads=2)
g = load("flda_m30_v50_k9_empty")
m = oc.fLDA(oc.CSR(g["doc_ptr"], g["terms"], g["counts"], int(g["V"])), int(g["K"]), g["beta0"], g["kappa0"])
t = m.train(iter=2, tol=0.0, checkelbo=1); assert np.all(np.isfinite(t))
m.estep(omp_threads=2)
sw = m.estep(omp_threads=2); assert len(sw) == m.M and sw.min() >= 1
m.estep(viter=int(sw[3]), vtol=0.0, d0=3, d1=4, omp_threads=2)
g = load("fctm_m30_v50_k4")
m = oc.fCTM(oc.CSR(g["doc_ptr"], g["terms"], g["counts"], int(g["V"])), int(g["K"]), g["beta0"], g["kappa0"])
t = m.train(iter=2, tol=0.0, checkelbo=1); assert np.all(np.isfinite(t))
m.estep(omp_threads=2)
sw = m.estep(omp_threads=2); assert len(sw) == m.M and sw.min() >= 1 and len(m.newton_per_doc) == m.M
m.estep(viter=int(sw[3]), vtol=0.0, d0=3, d1=4, omp_threads=2)
print("asan-ok")
'''


def _libasan():
    try:
        out = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:
        return None
    return out if os.path.isabs(out) and os.path.exists(out) else None


def test_oracle_runs_clean_under_asan_ubsan(tmp_path):
    """`make -C oracle asan` builds the oracle with -fsanitize=address,undefined; one golden case per model (train! +
    the OpenMP E-step) must finish without a sanitizer report."""
    asan = _libasan()
    if asan is None:
        pytest.skip("gcc has no libasan.so in this image")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-s", "asan"])
    script = tmp_path / "run_asan.py"
    script.write_text(ASAN_SCRIPT)
    env = dict(os.environ, LD_PRELOAD=asan, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1",
               OMP_NUM_THREADS="2")
    res = subprocess.run([sys.executable, str(script), ROOT], capture_output=True, text=True, env=env, timeout=600)
    assert res.returncode == 0 and "asan-ok" in res.stdout, (res.stdout[-2000:], res.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr[-4000:]
