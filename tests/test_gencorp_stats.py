"""
gendoc / gencorp (src/modelutils.jl:594-649): the statistical helpers of tests/test_gencorp_gpu.py, proof that they have power, and the
parts of the feature that need no GPU (argument errors, "no device", exports, the Philox known answers).

Every statistical assertion of the two files has the form p >= P_MIN = 1e-6 (two-sided for z) and goes through `accept`, which counts them:
at most 200 in the whole suite (24 here, the rest in the GPU file), so a correct sampler fails on an unlucky seed with probability <= 2e-4.
Seeds are fixed below and in the GPU file and are not tuned.  A pooled chi-square cell may hide an error, so `chi2_pooled` also asserts that
the pooled cell holds at most 5 % of the expected mass.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
from scipy import stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P_MIN = 1e-6
MAX_POOLED_SHARE = 0.05
N_ASSERTIONS = {"n": 0}


def accept(p, what):
    """The one form of statistical assertion: p >= 1e-6."""
    N_ASSERTIONS["n"] += 1
    assert N_ASSERTIONS["n"] <= 200, "more than 200 statistical assertions in one run"
    assert p >= P_MIN, f"{what}: p = {p:.3e} < {P_MIN}"


def chi2_pooled(observed, expected):
    """Pearson chi-square of counts against expected counts; every cell of expected count < 5 is pooled into ONE cell.
    Returns (p, pooled share of the expected mass, number of cells)."""
    observed = np.asarray(observed, dtype=np.float64).ravel()
    expected = np.asarray(expected, dtype=np.float64).ravel()
    assert observed.shape == expected.shape and abs(observed.sum() - expected.sum()) <= 1e-6 * max(expected.sum(), 1.0)
    small = expected < 5.0
    o, e = observed[~small], expected[~small]
    share = 0.0
    if small.any():
        share = expected[small].sum() / expected.sum()
        if expected[small].sum() > 0:
            o, e = np.append(o, observed[small].sum()), np.append(e, expected[small].sum())
        else:
            assert observed[small].sum() == 0, "counts in cells of zero expectation"
    assert len(e) >= 2
    x2 = ((o - e) ** 2 / e).sum()
    return float(stats.chi2.sf(x2, len(e) - 1)), float(share), len(e)


def assert_chi2(observed, expected, what):
    p, share, cells = chi2_pooled(observed, expected)
    print(f"{what}: p = {p:.4g}, pooled share = {share:.4f}, cells = {cells}")
    assert share <= MAX_POOLED_SHARE, f"{what}: the pooled cell holds {share:.3f} of the expected mass (> {MAX_POOLED_SHARE})"
    accept(p, what)
    return p


def z_pvalue(value, mean, variance):
    """Two-sided p of a normal z-test with the stated variance."""
    z = (value - mean) / np.sqrt(variance)
    return float(2.0 * stats.norm.sf(abs(z)))


def assert_z(value, mean, variance, what):
    p = z_pvalue(value, mean, variance)
    print(f"{what}: value = {value:.6g}, expected = {mean:.6g}, sd = {np.sqrt(variance):.3g}, p = {p:.4g}")
    accept(p, what)
    return p


def zipf_gamma_beta(K, V, seed, conc=0.05, zipf_s=1.05):
    """beta rows = Gamma(conc) x shuffled Zipf(zipf_s), normalised (the shape of the SYN-NSF generating topics)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    base = 1.0 / np.arange(1, V + 1, dtype=np.float64) ** zipf_s
    rng.shuffle(base)
    b = rng.gamma(conc, size=(K, V)) * base[None, :]
    return b / b.sum(axis=1, keepdims=True)


def smoothed(beta, a):
    """(beta[i,:] + a) / (1 + a V), src/modelutils.jl:601"""
    return (beta + a) / (1.0 + a * beta.shape[1])


# ------------------------------------------------------------------------------------------------ the helpers have power
K_SMALL, V_SMALL, M_SMALL, MEAN_C_SMALL = 8, 2000, 20000, 120.0
SMOOTHINGS = (0.0, 1e-5, 1e-3)


@pytest.mark.parametrize("a", SMOOTHINGS)
def test_chi2_accepts_numpy_samples_and_rejects_the_controls(a):
    """K = 8, V = 2000, about 300 k tokens per topic (M = 20 000 documents of mean length 120 over 8 topics): NumPy multinomial samples of
    the smoothed rows pass; the same counts with term ids shifted by one, and the right counts against the WRONG smoothing, are rejected."""
    beta = zipf_gamma_beta(K_SMALL, V_SMALL, seed=20261016)
    rng = np.random.Generator(np.random.PCG64(99 + int(a * 1e6)))
    n_k = int(M_SMALL * MEAN_C_SMALL / K_SMALL)
    bt = smoothed(beta, a)
    wrong = smoothed(beta, {0.0: 1e-5, 1e-5: 1e-3, 1e-3: 1e-5}[a])
    for k in range(K_SMALL):
        obs = rng.multinomial(n_k, bt[k])
        assert_chi2(obs, n_k * bt[k], f"numpy sample, a = {a}, topic {k}")
        # controls (these are rejections, not acceptances: they do not count towards the 200)
        shifted = np.roll(obs, 1)
        assert chi2_pooled(shifted, n_k * bt[k])[0] < P_MIN
        assert chi2_pooled(obs, n_k * wrong[k])[0] < P_MIN


def test_z_test_has_power():
    rng = np.random.Generator(np.random.PCG64(5))
    x = rng.normal(1.0, 2.0, size=100000)
    assert z_pvalue(x.mean(), 1.0, 4.0 / len(x)) > 1e-3            # not counted: a property of the helper, not of the sampler
    assert z_pvalue(x.mean(), 1.05, 4.0 / len(x)) < P_MIN
    assert chi2_pooled([50, 50], [50, 50])[0] == 1.0


def test_pooled_share_is_reported():
    p, share, cells = chi2_pooled([100, 3, 2], [95, 5, 5])
    assert cells == 3 and share == 0.0
    p, share, cells = chi2_pooled([100, 3, 2], [97, 4, 4])
    assert cells == 2 and abs(share - 8 / 105) < 1e-12
    with pytest.raises(AssertionError):
        assert_chi2([100, 3, 2], [97, 4, 4], "pooled cell above 5 %")


# ------------------------------------------------------------------------------------------------ the generator's random bits
def test_philox_known_answers(tmvb):
    """Philox4x32-10 known-answer vectors of the Random123 distribution (kat_vectors), through the header the kernels compile."""
    L = tmvb.lib()
    for ctr, key, want in (([0] * 4, [0] * 2, [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
                           ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
                           ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1])):
        out = (C.c_uint32 * 4)()
        assert L.tmvb_philox4x32_10((C.c_uint32 * 4)(*ctr), (C.c_uint32 * 2)(*key), out) == 0
        assert list(out) == want


# ------------------------------------------------------------------------------------------------ interface without a GPU
def _host_lda(tmvb, K=3):
    pc = tmvb.PackedCorpus([0, 2, 3], [0, 1, 2], [2, 1, 4], 6)
    return tmvb.LDA(pc, K)


def test_python_argument_errors(tmvb):
    m = _host_lda(tmvb)
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match="corp_size parameter must be a positive integer."):
            tmvb.gencorp(m, bad)
    with pytest.raises(ValueError, match="laplace_smooth parameter must be nonnegative."):
        tmvb.gencorp(m, 5, laplace_smooth=-1e-9)
    with pytest.raises(ValueError, match="laplace_smooth parameter must be nonnegative."):
        tmvb.gendoc(m, laplace_smooth=-1.0)
    with pytest.raises(ValueError, match="laplace_smooth parameter must be nonnegative."):
        tmvb.gendoc(m, laplace_smooth=float("nan"))
    pf = tmvb.PackedCorpus([0, 2], [0, 1], [1, 1], 3, [0, 1], [0], [1], 2)
    with pytest.raises(TypeError, match="CTPF"):
        tmvb.gencorp(tmvb.CTPF(pf, 2), 5)
    with pytest.raises(TypeError):
        tmvb.gencorp(object(), 5)


def test_no_device_is_an_engine_error(tmvb):
    """No silent CPU path: the Python mirror raises EngineError, the ABI answers TMVB_ENODEVICE (after judging the arguments)."""
    if tmvb.lib().tmvb_device_count() > 0:
        return                                  # covered on the GPU by tests/test_gencorp_gpu.py
    m = _host_lda(tmvb)
    with pytest.raises(tmvb.EngineError):
        tmvb.gencorp(m, 5)
    with pytest.raises(tmvb.EngineError):
        tmvb.gendoc(tmvb.CTM(m.corp, 3))
    beta = np.full((3, 6), 1.0 / 6)
    rc, res = tmvb.gencorp_raw(None, 3, 6, beta, 5, 2.0, alpha=np.ones(3))
    assert rc == 7 and "no HIP device" in res["error"]
    rc, res = tmvb.gencorp_raw(None, 3, 6, beta, 5, 2.0, mu=np.zeros(3), sigma=np.eye(3))
    assert rc == 7 and "no HIP device" in res["error"]


EINVAL, ESHAPE = 1, 2


def abi_error_cases():
    """(name, keyword changes, status, message part): one case for each EINVAL / ESHAPE cause of include/tmvb.h.  The arguments are judged
    before the device, so the same table runs here with a NULL context and on the GPU with a live one."""
    K, V = 3, 6
    beta = np.full((K, V), 1.0 / V)
    base = dict(K=K, V=V, beta=beta, M=5, mean_C=4.0, alpha=np.ones(K))
    ctm = dict(K=K, V=V, beta=beta, M=5, mean_C=4.0, mu=np.zeros(K), sigma=np.eye(K))
    bad_beta = beta.copy(); bad_beta[1, 2] += 0.01
    neg_beta = beta.copy(); neg_beta[0, 0] = -0.1; neg_beta[0, 1] += 0.1 + 1.0 / V
    indef = np.eye(K); indef[0, 1] = indef[1, 0] = 2.0
    return [
        ("M zero", base, dict(M=0), EINVAL, "corp_size parameter must be a positive integer."),
        ("M negative", base, dict(M=-4), EINVAL, "corp_size parameter must be a positive integer."),
        ("M above the per-call limit", base, dict(M=2 ** 26), EINVAL, "documents per call"),
        ("laplace_smooth negative", base, dict(laplace_smooth=-1e-3), EINVAL, "laplace_smooth parameter must be nonnegative."),
        ("mean_C zero", base, dict(mean_C=0.0), EINVAL, "mean_C"),
        ("mean_C negative", base, dict(mean_C=-2.0), EINVAL, "mean_C"),
        ("mean_C infinite", base, dict(mean_C=float("inf")), EINVAL, "mean_C"),
        ("mean_C nan", base, dict(mean_C=float("nan")), EINVAL, "mean_C"),
        ("LDA K above 1024", dict(base, K=1025, beta=np.full((1025, V), 1.0 / V), alpha=np.ones(1025)), {}, EINVAL, "K = 1025"),
        ("CTM K above 256", dict(ctm, K=257, beta=np.full((257, V), 1.0 / V), mu=np.zeros(257), sigma=np.eye(257)), {}, EINVAL, "K = 257"),
        ("CTM M zero", ctm, dict(M=0), EINVAL, "corp_size"),
        ("beta row does not sum to one", base, dict(beta=bad_beta), ESHAPE, "beta must be a right stochastic matrix."),
        ("beta negative entry", base, dict(beta=neg_beta), ESHAPE, "beta must be a right stochastic matrix."),
        ("CTM beta not stochastic", ctm, dict(beta=bad_beta), ESHAPE, "beta must be a right stochastic matrix."),
        ("alpha zero", base, dict(alpha=np.array([1.0, 0.0, 1.0])), ESHAPE, "alpha must be positive."),
        ("alpha negative", base, dict(alpha=np.array([1.0, 2.0, -0.5])), ESHAPE, "alpha must be positive."),
        ("sigma indefinite", ctm, dict(sigma=indef), ESHAPE, "sigma must be positive-definite."),
        ("sigma negative definite", ctm, dict(sigma=-np.eye(K)), ESHAPE, "sigma must be positive-definite."),
    ]


@pytest.mark.parametrize("case", abi_error_cases(), ids=lambda c: c[0].replace(" ", "_"))
def test_abi_argument_errors_without_a_context(tmvb, case):
    _, base, change, status, msg = case
    kw = dict(base, **change)
    rc, res = tmvb.gencorp_raw(None, kw.pop("K"), kw.pop("V"), kw.pop("beta"), kw.pop("M"), kw.pop("mean_C"), **kw)
    assert rc == status and msg in res["error"], (rc, res)


def test_exports_and_header(tmvb):
    syms = tmvb.exported_symbols()
    L = C.CDLL(tmvb.LIB_PATH)
    for s in ("tmvb_lda_gencorp", "tmvb_ctm_gencorp", "tmvb_gencorp_free", "tmvb_philox4x32_10"):
        assert s in syms and hasattr(L, s)
    assert tmvb.lib().tmvb_abi_version() == 2
    for name in ("gencorp", "gendoc"):
        assert name in tmvb.__all__ and callable(getattr(tmvb, name))
    hdr = open(os.path.join(ROOT, "include", "tmvb.h")).read()
    body = hdr[hdr.index("gendoc / gencorp"):]
    assert "src/modelutils.jl:594-649" in body
    # the Python structure mirrors the header's field order
    fields = re.search(r"typedef struct \{([^}]*)\} tmvb_gencorp_t;", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)).group(1)
    names = re.findall(r"\b(\w+)\s*[;,]", fields)
    import sys
    mod = sys.modules[tmvb.__name__ + ".gencorp"]          # the attribute `gencorp` of the package is the function
    assert names == [f[0] for f in mod.GenCorpResult._fields_]
    assert "tmvb_gencorp.hip" in tmvb._lib.SOURCES


def test_julia_shim_binds_gencorp():
    src = open(os.path.join(ROOT, "topicmodelsvb.jl_amd", "julia", "TMVBHip.jl")).read()
    for s in (":tmvb_lda_gencorp", ":tmvb_ctm_gencorp", ":tmvb_gencorp_free", "function gencorp(", "function gendoc("):
        assert s in src, s
