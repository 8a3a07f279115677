"""
CTPF fold-in on the device (include/tmvb.h, "CTPF fold-in") against its fp64 restatement in the direct form
(tests/ctpf_foldin_restatement.py: the 2K-row softmax per library entry; the device sweeps over the table W) and against the oracle.

  1. users against the restatement: K in {4 .. 512}, the oracle's state after 5 iterations of synth_case (tests/test_ctpf_gpu.py), libraries = the
     transposed reader lists (lengths 1 .. 46), default viter / vtol; sweep counts by the convention of test_teacher_forced_step.
  2. library lengths around every boundary of the two user kernels (0 .. 65, C - 1, C, C + 1, 4 C + 3, 3000), pinned sweeps.
  3. one sweep from he is the oracle's he_temp after estep(viter = 1).
  4. exactness and reproducibility: an empty library, permutations, slices, single users, repeated calls, the handle form, viter = 0.
  5. predict_ctpf against the oracle, with and without readers.
  6. recommend_new_users / recommend_new_docs are plumbing: exactly rec_topn_raw on the hand-built features of the same fold-in.
  7. every EINVAL / ESHAPE case of the header leaves tmvb_last_error set.

Tolerances: FI_T below, (frozen, measured on MI355X against the fp64 restatement / oracle), frozen at <= 10 x the measurement
(profiles/ctpf_foldin_tolerances_measured.json).  TMVB_TOL_RECORD=1 records instead of failing, like tests/tol.py; with
TMVB_CTPF_FOLDIN_TOL_OUT=<file> the worst values seen are written there as JSON.
"""
import json
import os

import numpy as np
import pytest

import ctpf_foldin_restatement as R
import tol
from test_ctpf_foldin_host import EINVAL_CASES, ESHAPE_CASES, foldin_error_case

pytestmark = pytest.mark.gpu

KS = (4, 12, 50, 64, 77, 128, 150, 256, 300, 512)

# key: (frozen, worst measured on MI355X -- profiles/ctpf_foldin_tolerances_measured.json)
FI_T = {
    # he of folded-in users, max relative deviation over every entry, K <= 256.  Frozen at 1.2 x, not 3 - 10 x: on this data zayin stays within 1e-3 of g, and W
    # without its zayin term (mutant mut_foldin_drop_zayin) moves case 3 by only 1.7e-4 (K = 12) / 2.4e-4 (K = 150) and case 1 at K = 4 by 2.3e-4 (fp64 NumPy,
    # both forms of W): a looser bound would have no teeth there.  The worst case, K = 77 after ten sweeps short of the fixed point, is bit-reproducible.
    "foldin.he_rel":              (0.00015, 0.000129),
    "foldin.he_rel_bigk":         (0.0001, 2.23e-05),      # K > 256
    "foldin.doc_shape_rel":       (0.0002, 3.87e-05),      # gimel, zayin of predict_ctpf, K <= 256; may not exceed ctpf.shape_rel
    "foldin.doc_shape_rel_bigk":  (0.0001, 2.05e-05),      # K > 256; may not exceed ctpf.shape_rel_bigk
}
SEEN = {}


def fi_within(key, value, detail=None):
    v = float(np.max(value)) if np.size(value) else 0.0
    if not (v <= SEEN.get(key, -1.0)):
        SEEN[key] = v
    print(f"{key}: {v:.3g}  [{detail}]")
    if tol.RECORD:
        return True
    assert np.isfinite(v) and v <= FI_T[key][0], f"{key}: {v:.3g} > {FI_T[key][0]:.3g}" + (f"  [{detail}]" if detail is not None else "")
    return True


@pytest.fixture(scope="module", autouse=True)
def _dump_measured():
    yield
    path = os.environ.get("TMVB_CTPF_FOLDIN_TOL_OUT", "")
    if SEEN and path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        old = json.load(open(path)) if os.path.exists(path) else {}
        for k, v in SEEN.items():
            old[k] = max(v, old.get(k, 0.0))
        json.dump(old, open(path, "w"), indent=1, sort_keys=True)


def test_new_keys_are_frozen_within_ten_times_the_measurement():
    for k, (frozen, measured) in FI_T.items():
        assert frozen is not None and measured is not None and 0 < measured <= frozen <= 10 * measured, (k, frozen, measured)
    assert FI_T["foldin.doc_shape_rel"][0] <= tol.TOL["ctpf.shape_rel"] and FI_T["foldin.doc_shape_rel_bigk"][0] <= tol.TOL["ctpf.shape_rel_bigk"]


@pytest.fixture(scope="module")
def ctx(tmvb):
    c = tmvb.DeviceContext(0)
    yield c
    c.close()


def he_key(K):
    return "foldin.he_rel" if K <= 256 else "foldin.he_rel_bigk"


def raw(tmvb, ctx, st, libs, **kw):
    rc, out = tmvb.foldin_users_raw(ctx, st.K, st.M, st.gimel, st.zayin, st.dalet, st.het, st.vav, st.e, *libs, **kw)
    assert rc == 0, out
    return out


def sub(libs, sel):
    """the libraries of the users `sel` (any order) as a CSR of their own"""
    ptr, docs, rat = libs
    lens = ptr[np.asarray(sel) + 1] - ptr[np.asarray(sel)]
    take = np.concatenate([np.arange(ptr[u], ptr[u + 1]) for u in sel]).astype(np.int64) if len(sel) else np.zeros(0, dtype=np.int64)
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), docs[take], rat[take]


_REF = {}


def reference(tmvb, oracle, K):
    """restatement of case 1, once per K"""
    if K not in _REF:
        om, g, libs = R.trained_oracle(tmvb, oracle, K)
        st = R.state_of(om)
        _REF[K] = (st, libs) + R.foldin_direct(oracle.digamma, st, *libs)
    return _REF[K]


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("K", KS)
def test_users_against_the_restatement(tmvb, oracle, ctx, K):
    st, libs, he_ref, sw_ref = reference(tmvb, oracle, K)
    assert np.diff(libs[0]).min() >= 1 and np.diff(libs[0]).max() == 46
    out = raw(tmvb, ctx, st, libs)
    sw = out["sweeps"]
    same = sw == sw_ref
    # a user whose exit norm straddles vtol in fp32 leaves one sweep earlier or later than in fp64: at most 3 of the 60 (a condition, not a measurement),
    # and the restatement is run with the DEVICE's count for them, so that every user is compared
    assert (~same).sum() <= 0.05 * len(sw), (K, int((~same).sum()))
    assert np.all(np.abs(sw[~same].astype(int) - sw_ref[~same]) <= 1)
    ref = he_ref.copy()
    if (~same).any():
        ref[:, ~same] = R.foldin_direct(oracle.digamma, st, *libs, sweeps=sw)[0][:, ~same]
    assert out["n_reg"] + out["n_long"] == 60 and out["n_long"] == int((np.diff(libs[0]) > tmvb.foldin_reg_capacity(K)).sum())
    assert out["kp"] == (K + 3) // 4 * 4 and out["capacity"] == tmvb.foldin_reg_capacity(K)
    fi_within(he_key(K), tol.rel(out["he"], ref), (K, "users", int((~same).sum())))


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("K", [50, 300])
def test_library_lengths(tmvb, oracle, ctx, K):
    rng = np.random.default_rng(K)
    M = 3000
    st = R.State(rng.gamma(0.3, size=(K, M)) + 0.1, rng.gamma(0.3, size=(K, M)) + 0.1, *(rng.uniform(0.5, 2.0, size=K) for _ in range(3)))
    cap = tmvb.foldin_reg_capacity(K)
    lengths = [0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, cap - 1, cap, cap + 1, 4 * cap + 3, 3000]
    docs = [np.sort(rng.choice(M, size=n, replace=False)).astype(np.int32) for n in lengths]
    libs = (np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64), np.concatenate(docs), rng.integers(1, 6, size=sum(lengths)).astype(np.int32))
    out = raw(tmvb, ctx, st, libs, viter=4, vtol=0.0)
    assert np.all(out["sweeps"] == 4)
    assert out["n_long"] == sum(n > cap for n in lengths) and out["n_reg"] == sum(n <= cap for n in lengths)
    ref, sw = R.foldin_direct(oracle.digamma, st, *libs, viter=4, vtol=0.0)
    assert np.all(sw == 4)
    r = tol.rel(out["he"], ref)
    fi_within(he_key(K), r, (K, "lengths", lengths[int(np.argmax(r.max(axis=0)))]))


# ------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("K", [12, 150])
def test_one_sweep_is_the_oracles_statistic(tmvb, oracle, ctx, K):
    om0, g, libs = R.trained_oracle(tmvb, oracle, K)
    om = oracle.CTPF(om0.corp, K, g["alef0"])
    for n in ("alef", "he", "bet", "vav", "dalet", "het", "gimel", "zayin"):
        setattr(om, n, np.array(getattr(om0, n), copy=True, order="F"))
    st = R.state_of(om)                                          # the state update_xi! sees: before the sweep moves gimel and zayin
    out = raw(tmvb, ctx, st, libs, he0=om.he, viter=1, vtol=0.0)
    om.he_temp[:] = 0.1
    om.estep(viter=1, vtol=0.0)
    assert np.all(out["sweeps"] == 1)
    fi_within(he_key(K), tol.rel(out["he"], om.he_temp), (K, "he_temp"))


# ------------------------------------------------------------------------------------------------ 4
def test_empty_library_is_e_exactly(tmvb, oracle, ctx):
    st, libs, _, _ = reference(tmvb, oracle, 50)
    ptr = np.array([0, 0, 2, 2], dtype=np.int64)
    out = raw(tmvb, ctx, st, (ptr, np.array([3, 7], dtype=np.int32), np.array([1, 2], dtype=np.int32)))
    e32 = np.float64(np.float32(0.1))
    assert np.all(out["he"][:, 0] == e32) and np.all(out["he"][:, 2] == e32)
    assert out["sweeps"][0] == 2 and out["sweeps"][2] == 2
    assert np.isclose(out["he"][:, 1].sum(), 50 * 0.1 + 3, rtol=1e-5)       # the user between them shares its ratings out among the topics


@pytest.mark.parametrize("K", [50, 300])
def test_reproducible_and_independent_of_the_other_users(tmvb, oracle, ctx, K):
    st, libs, _, _ = reference(tmvb, oracle, K)
    a = raw(tmvb, ctx, st, libs)
    b = raw(tmvb, ctx, st, libs)
    assert np.array_equal(a["he"], b["he"]) and np.array_equal(a["sweeps"], b["sweeps"])
    U = len(libs[0]) - 1
    perm = np.random.default_rng(1).permutation(U)
    p = raw(tmvb, ctx, st, sub(libs, perm))
    assert np.array_equal(p["he"], a["he"][:, perm]) and np.array_equal(p["sweeps"], a["sweeps"][perm])
    for sel in (np.arange(0, 17), np.arange(17, U), np.arange(5, 6)):
        s = raw(tmvb, ctx, st, sub(libs, sel))
        assert np.array_equal(s["he"], a["he"][:, sel]) and np.array_equal(s["sweeps"], a["sweeps"][sel])
    longest = int(np.argmax(np.diff(libs[0])))
    for u in (0, 1, longest, U - 1):
        s = raw(tmvb, ctx, st, sub(libs, [u]))
        assert np.array_equal(s["he"][:, 0], a["he"][:, u]) and s["sweeps"][0] == a["sweeps"][u]
    h0 = np.random.default_rng(2).uniform(0.2, 3.0, size=(K, U))
    z = raw(tmvb, ctx, st, libs, he0=h0, viter=0)
    assert np.array_equal(z["he"], h0.astype(np.float32).astype(np.float64)) and np.all(z["sweeps"] == 0)


@pytest.mark.parametrize("K", [50, 300])
def test_handle_form_equals_the_stateless_form(tmvb, oracle, ctx, K):
    om, g, libs = R.trained_oracle(tmvb, oracle, K)
    st = R.state_of(om)
    pc = tmvb.PackedCorpus(g["doc_ptr"], g["terms"], g["counts"], g["V"], g["rdr_ptr"], g["readers"], g["ratings"], g["U"])
    gm = tmvb.gpuCTPF(pc, K)
    for n in ("alef", "he", "bet", "vav", "dalet", "het", "gimel", "zayin"):
        setattr(gm, n, np.array(getattr(om, n), copy=True, order="F"))
    gm.update_buffer()
    a = raw(tmvb, ctx, st, libs)
    ids = [list(libs[1][libs[0][u]:libs[0][u + 1]][::-1] + 1) for u in range(60)]              # 1-based and unsorted: sorted on the host
    rat = [list(libs[2][libs[0][u]:libs[0][u + 1]][::-1]) for u in range(60)]
    f = tmvb.foldin_users(gm, ids, rat)
    assert np.array_equal(f.he, a["he"]) and np.array_equal(f.sweeps, a["sweeps"])
    assert np.array_equal(f.lib_docs, libs[1]) and np.array_equal(f.lib_ratings, libs[2])
    host = tmvb.CTPF(pc, K)
    for n in ("gimel", "zayin", "dalet", "het", "vav"):
        setattr(host, n, np.array(getattr(om, n), copy=True, order="F"))
    f2 = tmvb.foldin_users(host, (libs[0], libs[1] + 1), libs[2])
    assert np.array_equal(f2.he, a["he"]) and np.array_equal(f2.sweeps, a["sweeps"])
    gm.close()


# ------------------------------------------------------------------------------------------------ 5
def trained_host_model(tmvb, oracle, K):
    om, g, libs = R.trained_oracle(tmvb, oracle, K)
    pc = tmvb.PackedCorpus(g["doc_ptr"], g["terms"], g["counts"], g["V"], g["rdr_ptr"], g["readers"], g["ratings"], g["U"])
    m = tmvb.CTPF(pc, K)
    for n in ("alef", "he", "bet", "vav", "dalet", "het", "gimel", "zayin"):
        setattr(m, n, np.array(getattr(om, n), copy=True, order="F"))
    return m, om, libs


def new_corpus(tmvb, readers):
    pc = tmvb.syn_citeu(M=40, V=300, U=60, seed=11)
    if readers:
        return pc
    return tmvb.PackedCorpus(pc.doc_ptr, pc.terms, pc.counts, pc.V, np.zeros(pc.M + 1, dtype=np.int64), np.zeros(0, dtype=np.int32),
                             np.zeros(0, dtype=np.int32), pc.U)


@pytest.mark.parametrize("readers", [True, False], ids=["readers", "cold"])
@pytest.mark.parametrize("K", [12, 50, 300])
def test_predict_ctpf_against_the_oracle(tmvb, oracle, K, readers):
    m, om0, _ = trained_host_model(tmvb, oracle, K)
    before = {n: np.array(getattr(m, n), copy=True) for n in ("alef", "he", "bet", "vav", "dalet", "het", "gimel", "zayin")}
    pc = new_corpus(tmvb, readers)
    p = tmvb.predict_ctpf(pc, m)
    for n, v in before.items():
        assert np.array_equal(getattr(m, n), v), n                # the trained model is not modified

    def oracle_side():
        o = oracle.CTPF(oracle.CSR(pc.doc_ptr, pc.terms, pc.counts, pc.V, pc.rdr_ptr, pc.readers, pc.ratings, pc.U), K, om0.alef)
        for n in ("alef", "he", "bet", "vav", "dalet", "het"):
            setattr(o, n, np.array(getattr(om0, n), copy=True, order="F"))
        return o
    o = oracle_side()
    sw = np.asarray(o.estep())
    sw_g = p.doc_sweeps
    same = sw_g == sw
    assert (~same).sum() <= 0.05 * pc.M, (K, int((~same).sum()))
    assert np.all(np.abs(sw_g[~same].astype(int) - sw[~same]) <= 1)
    for d in np.nonzero(~same)[0]:                                # the oracle with the device's count for a straddling document
        o2 = oracle_side()
        o2.estep(viter=int(sw_g[d]), vtol=0.0, d0=int(d), d1=int(d) + 1)
        o.gimel[:, d] = o2.gimel[:, d]; o.zayin[:, d] = o2.zayin[:, d]
    key = "foldin.doc_shape_rel" if K <= 256 else "foldin.doc_shape_rel_bigk"
    for n in ("gimel", "zayin"):
        fi_within(key, tol.rel(getattr(p, n), getattr(o, n)), (K, readers, n))
    if not readers:
        assert np.all(p.zayin == np.float64(np.float32(0.1)))     # zayin == g exactly
    assert p.M == pc.M and p.K == K and np.array_equal(p.he, m.he) and np.array_equal(p.vav, m.vav)


def test_predict_ctpf_needs_the_trained_vocabulary_and_users(tmvb, oracle):
    m, _, _ = trained_host_model(tmvb, oracle, 12)
    with pytest.raises(tmvb.CorpusError):
        tmvb.predict_ctpf(tmvb.syn_citeu(M=10, V=301, U=60, seed=2), m)
    with pytest.raises(tmvb.CorpusError):
        tmvb.predict_ctpf(tmvb.syn_citeu(M=10, V=300, U=61, seed=2), m)


# ------------------------------------------------------------------------------------------------ 6
def same_topn(a, raw_):
    assert np.array_equal(a.idx, raw_["idx"]) and np.array_equal(a.count, raw_["count"])
    assert np.array_equal(a.score.view(np.int32), raw_["score"].view(np.int32))


@pytest.mark.parametrize("K", [50, 300])
def test_recommendations_are_plumbing(tmvb, oracle, ctx, K):
    m, om, libs = trained_host_model(tmvb, oracle, K)
    ids = [list(libs[1][libs[0][u]:libs[0][u + 1]] + 1) for u in range(60)]
    rat = [list(libs[2][libs[0][u]:libs[0][u + 1]]) for u in range(60)]
    r = tmvb.recommend_new_users(m, ids, rat, topn=15)
    fold = tmvb.foldin_users(m, ids, rat)
    assert np.array_equal(r.foldin.he, fold.he) and r.by == "user" and r.idx.shape == (60, 15)
    xd = m.gimel / m.dalet[:, None] + m.zayin / m.het[:, None]
    rc, hand = tmvb.rec_topn_raw(ctx, K, xd, fold.he / m.vav[:, None], (libs[0], libs[1]), 15)
    assert rc == 0
    same_topn(r, hand)
    for u in range(60):
        assert not set(r.idx[u, :r.count[u]]) & set(libs[1][libs[0][u]:libs[0][u + 1]])
    pc = new_corpus(tmvb, True)
    rd = tmvb.recommend_new_docs(m, pc, topn=15)
    p = rd.predicted
    xq = p.gimel / m.dalet[:, None] + p.zayin / m.het[:, None]
    rc, hand = tmvb.rec_topn_raw(ctx, K, m.he / m.vav[:, None], xq, (pc.rdr_ptr, np.asarray(pc.readers, dtype=np.int32)), 15)
    assert rc == 0 and rd.by == "doc" and rd.idx.shape == (pc.M, 15)
    same_topn(rd, hand)
    for d in range(pc.M):
        assert not set(rd.idx[d, :rd.count[d]]) & set(pc.readers[pc.rdr_ptr[d]:pc.rdr_ptr[d + 1]])


# ------------------------------------------------------------------------------------------------ 7
@pytest.mark.parametrize("name", sorted(EINVAL_CASES) + sorted(ESHAPE_CASES))
def test_errors_leave_last_error_set(tmvb, ctx, name):
    rc, msg, want = foldin_error_case(tmvb, ctx, name)
    assert rc == want and msg.startswith("tmvb_ctpf_foldin_users:") and tmvb.lib().tmvb_last_error().decode() == msg, (rc, msg)


def test_errors_of_the_handle_form(tmvb):
    gm = tmvb.gpuCTPF(tmvb.syn_citeu(M=20, V=50, U=10, seed=1), 4)
    ok = (np.array([0, 2], dtype=np.int64), np.array([0, 19], dtype=np.int32), np.array([1, 1], dtype=np.int32))
    for want, kw, libs in ((1, dict(viter=-1), ok), (1, dict(vtol=-1.0), ok), (2, {}, (ok[0], np.array([0, 20], dtype=np.int32), ok[2])),
                           (2, {}, (ok[0], np.array([5, 5], dtype=np.int32), ok[2])), (2, {}, (ok[0], ok[1], np.array([1, 0], dtype=np.int32))),
                           (2, dict(he0=np.zeros((4, 1))), ok)):
        rc, msg = tmvb.foldin_users_raw(None, 4, 20, None, None, None, None, None, 0.1, *libs, handle=gm.handle, **kw)
        assert rc == want and msg.startswith("tmvb_ctpf_foldin_users_on:") and tmvb.lib().tmvb_last_error().decode() == msg, (rc, msg)
    rc, out = tmvb.foldin_users_raw(None, 4, 20, None, None, None, None, None, 0.1, *ok, handle=gm.handle)
    assert rc == 0 and out["he"].shape == (4, 1) and np.isclose(out["he"].sum(), 0.4 + 2, rtol=1e-5)
    gm.close()
