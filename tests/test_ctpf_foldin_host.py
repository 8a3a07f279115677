"""
CTPF fold-in (include/tmvb.h, "CTPF fold-in"), the part that needs no GPU:
  (a) the direct form of tests/ctpf_foldin_restatement.py (2K-row softmax per entry) equals the W form the device uses, rel 1e-12, equal sweeps;
  (b) the pin to the oracle: one sweep from he is what orc_ctpf_estep(viter = 1) leaves in he_temp;
  (c) host-side behaviour of foldin_users: argument validation, id sorting, 1-based -> 0-based, duplicate rejection -- no device call is made;
  plus the straddle count of the GPU test's K (the users whose fp64 exit norm lies within 0.2 % of vtol), the ABI declaration, the bindings and
  the error paths that are judged before the device is touched.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ctpf_foldin_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (4, 12, 50, 64, 77, 128, 150, 256, 300, 512)                         # tests/test_ctpf_foldin_gpu.py, case 1


def foldin_wform(digamma, st, lib_ptr, lib_docs, lib_ratings, he0=None, viter=10, vtol=None):
    """the operator as include/tmvb.h writes it: W once, then sweeps"""
    K = st.K
    vtol = 1.0 / K ** 2 if vtol is None else vtol
    W = (np.exp(digamma(st.gimel)) / st.dalet[:, None] + np.exp(digamma(st.zayin)) / st.het[:, None]) / st.vav[:, None]
    Un = len(lib_ptr) - 1
    he = np.empty((K, Un), order="F"); sw = np.zeros(Un, dtype=np.int32)
    for u in range(Un):
        docs = lib_docs[lib_ptr[u]:lib_ptr[u + 1]]; r = lib_ratings[lib_ptr[u]:lib_ptr[u + 1]].astype(np.float64)
        h = np.ones(K) if he0 is None else he0[:, u].copy()
        for _ in range(viter):
            p = np.exp(digamma(h))[:, None] * W[:, docs]
            hn = st.e + (p / p.sum(axis=0, keepdims=True)) @ r
            nrm = np.linalg.norm(hn - h); h = hn; sw[u] += 1
            if nrm < vtol:
                break
        he[:, u] = h
    return he, sw


@pytest.mark.parametrize("K", [4, 12, 50, 130])
def test_direct_form_equals_w_form(tmvb, oracle, K):
    om, g, libs = R.trained_oracle(tmvb, oracle, K)
    st = R.state_of(om)
    a, sa = R.foldin_direct(oracle.digamma, st, *libs)
    b, sb = foldin_wform(oracle.digamma, st, *libs)
    assert np.array_equal(sa, sb)
    assert np.abs(a - b).max() <= 1e-12 * np.abs(a).max() and (np.abs(a - b) / np.abs(a)).max() <= 1e-12
    he0 = om.he.copy()
    a, sa = R.foldin_direct(oracle.digamma, st, *libs, he0=he0, viter=3, vtol=0.0)
    b, sb = foldin_wform(oracle.digamma, st, *libs, he0=he0, viter=3, vtol=0.0)
    assert np.all(sa == 3) and np.all(sb == 3) and (np.abs(a - b) / np.abs(a)).max() <= 1e-12


@pytest.mark.parametrize("K", [12, 50])
def test_one_sweep_is_the_oracles_he_temp(tmvb, oracle, K):
    """(b): state after 3 iterations, he_temp = e; after estep(viter = 1, vtol = 0) he_temp equals one sweep from he0 = he over the transposed reader lists"""
    om0, g, libs = R.trained_oracle(tmvb, oracle, K, iters=3)
    om = oracle.CTPF(om0.corp, K, g["alef0"])
    for n in ("alef", "he", "bet", "vav", "dalet", "het", "gimel", "zayin"):
        setattr(om, n, np.array(getattr(om0, n), copy=True, order="F"))
    st = R.state_of(om)                                                   # gimel / zayin BEFORE the sweep: update_xi! runs first (src/CTPF.jl:355)
    om.he_temp[:] = 0.1
    om.estep(viter=1, vtol=0.0)
    he, sw = R.foldin_direct(oracle.digamma, st, *libs, he0=om.he, viter=1, vtol=0.0)
    assert np.all(sw == 1)
    assert (np.abs(he - om.he_temp) / np.abs(om.he_temp)).max() <= 1e-12


def test_exit_rule_edge_cases(oracle):
    rng = np.random.default_rng(0)
    K, M = 6, 9
    st = R.State(rng.gamma(0.3, size=(K, M)) + 0.1, rng.gamma(0.3, size=(K, M)) + 0.1, *(rng.uniform(0.5, 2, size=K) for _ in range(3)))
    ptr = np.array([0, 0, 3], dtype=np.int64); docs = np.array([1, 4, 8], dtype=np.int32); r = np.array([1, 2, 5], dtype=np.int32)
    he, sw = R.foldin_direct(oracle.digamma, st, ptr, docs, r)
    assert np.all(he[:, 0] == 0.1) and sw[0] == 2                          # an empty library: e exactly, two sweeps under the defaults
    assert np.isclose(he[:, 1].sum(), 0.1 * K + r.sum(), rtol=1e-13)       # the ratings are shared out among the topics
    h0 = rng.uniform(0.5, 2, size=(K, 2))
    he, sw = R.foldin_direct(oracle.digamma, st, ptr, docs, r, he0=h0, viter=0)
    assert np.array_equal(he, h0) and np.all(sw == 0)
    he, sw = R.foldin_direct(oracle.digamma, st, ptr, docs, r, sweeps=[3, 7])
    assert list(sw) == [3, 7]


@pytest.mark.parametrize("K", KS)
def test_straddle_count_of_the_gpu_cases(tmvb, oracle, K):
    """At most 1 of the 60 users of GPU case 1 may have an fp64 exit norm within 0.2 % of vtol (the stand-in for fp32 rounding under the 3-of-60
    condition of that test); no K needed another seed of synth_case."""
    om, g, libs = R.trained_oracle(tmvb, oracle, K)
    norms = []
    R.foldin_direct(oracle.digamma, R.state_of(om), *libs, norms=norms)
    assert len(R.straddlers(norms, 1.0 / K ** 2)) <= 1


# ------------------------------------------------------------------------------------------------ (c) host-side behaviour
def test_foldin_libraries_sorts_converts_and_rejects(tmvb):
    ptr, docs, rat = tmvb.foldin_libraries([[5, 2, 9], [], [1]], [[3, 1, 2], [], [4]], 9)
    assert list(ptr) == [0, 3, 3, 4] and list(docs) == [1, 4, 8, 0] and list(rat) == [1, 3, 2, 4]         # each rating moves with its id
    assert ptr.dtype == np.int64 and docs.dtype == np.int32 and rat.dtype == np.int32
    p2, d2, r2 = tmvb.foldin_libraries((np.array([0, 3, 3, 4]), np.array([5, 2, 9, 1])), None, 9)          # a CSR pair, 1-based as well
    assert list(p2) == [0, 3, 3, 4] and list(d2) == [1, 4, 8, 0] and list(r2) == [1, 1, 1, 1]
    assert tmvb.foldin_libraries([], None, 5)[0].tolist() == [0]
    for bad in ([[1, 1]], [[2, 3, 2]]):
        with pytest.raises(tmvb.CorpusError):
            tmvb.foldin_libraries(bad, None, 9)                            # duplicates
    for bad in ([[0]], [[10]], [[-1, 2]]):
        with pytest.raises(tmvb.CorpusError):
            tmvb.foldin_libraries(bad, None, 9)                            # outside [1, M]
    with pytest.raises(tmvb.CorpusError):
        tmvb.foldin_libraries([[1, 2]], [[1]], 9)
    with pytest.raises(tmvb.CorpusError):
        tmvb.foldin_libraries([[1, 2]], [[1, 0]], 9)
    with pytest.raises(tmvb.CorpusError):
        tmvb.foldin_libraries((np.array([0, 3]), np.array([1, 2])), None, 9)


def test_foldin_users_validates_before_any_device_call(tmvb):
    """every one of these raises on the host; the machine of this test has no device, so a device call would raise EngineError instead"""
    pc = tmvb.syn_citeu(M=20, V=50, U=10, seed=1)
    m = tmvb.CTPF(pc, 4)
    with pytest.raises(ValueError):
        tmvb.foldin_users(m, [[1]], viter=-1)
    with pytest.raises(ValueError):
        tmvb.foldin_users(m, [[1]], vtol=-1.0)
    with pytest.raises(ValueError):
        tmvb.foldin_users(m, [[1]], vtol=float("nan"))
    with pytest.raises(tmvb.CorpusError):
        tmvb.foldin_users(m, [[1, 1]])
    with pytest.raises(tmvb.CorpusError):
        tmvb.foldin_users(m, [[21]])
    with pytest.raises(tmvb.TopicModelError):
        tmvb.foldin_users(m, [[1]], he0=np.ones((4, 2)))
    with pytest.raises(tmvb.TopicModelError):
        tmvb.foldin_users(m, [[1]], he0=np.zeros((4, 1)))
    with pytest.raises(tmvb.TopicModelError):
        tmvb.foldin_users(tmvb.LDA(pc, 4), [[1]])
    with pytest.raises(ValueError):
        tmvb.recommend_new_users(m, [[1]], topn=0)
    with pytest.raises(tmvb.CorpusError):
        tmvb.predict_ctpf(tmvb.syn_citeu(M=5, V=51, U=10, seed=2), m)
    with pytest.raises(tmvb.CorpusError):
        tmvb.predict_ctpf(tmvb.syn_citeu(M=5, V=50, U=11, seed=2), m)
    assert tmvb.foldin_reg_capacity(256) == tmvb.FOLDIN_REG_CAPACITY == 32 and tmvb.foldin_reg_capacity(257) == tmvb.FOLDIN_REG_CAPACITY_BIGK == 16


# ------------------------------------------------------------------------------------------------ the ABI: errors judged before the device
def _args(K=3, M=4, Un=2):
    rng = np.random.default_rng(1)
    return dict(K=K, M=M, gimel=rng.uniform(0.5, 2, (K, M)), zayin=rng.uniform(0.5, 2, (K, M)), dalet=np.ones(K), het=np.ones(K), vav=np.ones(K), e=0.1,
                lib_ptr=np.array([0, 2, 3], dtype=np.int64)[:Un + 1], lib_docs=np.array([0, 3, 1], dtype=np.int32), lib_ratings=np.array([1, 2, 1], dtype=np.int32))


EINVAL_CASES = {
    "K=0": dict(K=0), "K=513": dict(K=513), "M=0": dict(M=0), "Un=-1": dict(Un=-1), "viter=-1": dict(viter=-1), "vtol=-1": dict(vtol=-1.0),
    "vtol=nan": dict(vtol=float("nan")), "vtol=inf": dict(vtol=float("inf")), "e=0": dict(e=0.0), "gimel=NULL": dict(gimel=None), "vav=NULL": dict(vav=None),
    "lib_ptr=NULL": dict(lib_ptr=None, Un=2), "lib_docs=NULL": dict(lib_docs=None), "lib_ratings=NULL": dict(lib_ratings=None),
}
ESHAPE_CASES = {
    "ptr start": dict(lib_ptr=np.array([1, 2, 3], dtype=np.int64)), "ptr decreases": dict(lib_ptr=np.array([0, 3, 2], dtype=np.int64)),
    "id = M": dict(lib_docs=np.array([0, 4, 1], dtype=np.int32)), "id < 0": dict(lib_docs=np.array([-1, 3, 1], dtype=np.int32)),
    "not ascending": dict(lib_docs=np.array([3, 0, 1], dtype=np.int32)), "repeated id": dict(lib_docs=np.array([3, 3, 1], dtype=np.int32)),
    "rating 0": dict(lib_ratings=np.array([1, 0, 1], dtype=np.int32)), "gimel 0": "gimel", "zayin nan": "zayin", "dalet < 0": "dalet", "het inf": "het", "vav 0": "vav",
    "he0 0": "he0",
}


def foldin_error_case(tmvb, ctx, name):
    """(status, message, expected status) of one EINVAL / ESHAPE case of include/tmvb.h on the stateless form; shared with the GPU test"""
    a = _args()
    if name in EINVAL_CASES:
        a.update(EINVAL_CASES[name]); want = 1
    else:
        ch = ESHAPE_CASES[name]; want = 2
        if isinstance(ch, dict):
            a.update(ch)
        elif ch == "he0":
            a["he0"] = np.ones((3, 2)); a["he0"][1, 1] = 0.0
        else:
            bad = {"gimel 0": 0.0, "zayin nan": np.nan, "dalet < 0": -1.0, "het inf": np.inf, "vav 0": 0.0}[name]
            a[ch] = np.array(a[ch], copy=True); a[ch].flat[1] = bad
    rc, msg = tmvb.foldin_users_raw(ctx, **a)
    return rc, msg, want


@pytest.mark.parametrize("name", sorted(EINVAL_CASES) + sorted(ESHAPE_CASES))
def test_errors_are_judged_before_the_device(tmvb, name):
    rc, msg, want = foldin_error_case(tmvb, None, name)
    assert rc == want and isinstance(msg, str) and msg.startswith("tmvb_ctpf_foldin_users:"), (rc, msg)
    assert tmvb.lib().tmvb_last_error().decode() == msg
    if name == "K=0":
        rc = tmvb.lib().tmvb_ctpf_foldin_users_on(None, 0, None, None, None, None, 1, 0.0, None, None, None)
        assert rc == 1 and "handle is NULL" in tmvb.lib().tmvb_last_error().decode()


def test_header_binding_and_julia_agree(tmvb):
    hdr = open(os.path.join(ROOT, "include", "tmvb.h")).read()
    fields = re.search(r"typedef struct \{([^}]*)\} tmvb_foldin_info_t;", hdr).group(1)
    names = re.findall(r"\b(\w+)\s*[;,]", fields)
    from tmvb_amd import pkg
    import importlib
    L = importlib.import_module(pkg.__name__ + "._lib")
    assert names == [n for n, _ in L.FoldinInfo._fields_] and C.sizeof(L.FoldinInfo) == 32
    for fn, n in (("tmvb_ctpf_foldin_users", 19), ("tmvb_ctpf_foldin_users_on", 11)):
        args = re.search(r"int %s\(([^;]*)\);" % fn, hdr).group(1)
        assert len(args.split(",")) == len(getattr(tmvb.lib(), fn).argtypes) == n
        assert fn in tmvb.exported_symbols()
        assert fn in open(os.path.join(ROOT, "topicmodelsvb.jl_amd", "csrc", "tmvb_call.h")).read().split("#pragma once")[0]
        assert ":" + fn in open(os.path.join(ROOT, "topicmodelsvb.jl_amd", "julia", "TMVBHip.jl")).read()
    assert int(re.search(r"#define TMVB_FOLDIN_REG_CAP (\d+)", hdr).group(1)) == tmvb.FOLDIN_REG_CAPACITY
    assert int(re.search(r"#define TMVB_FOLDIN_REG_CAP_BIGK (\d+)", hdr).group(1)) == tmvb.FOLDIN_REG_CAPACITY_BIGK
    assert "tmvb_ctpf_foldin.hip" in L.SOURCES and "tmvb_ctpf_foldin.hip" in open(os.path.join(ROOT, "tools", "build_mutants.sh")).read()
