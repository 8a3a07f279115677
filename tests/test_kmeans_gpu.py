"""
tmvb_topic_kmeans on the device (include/tmvb.h, "cluster documents in topic space") against tests/kmeans_restatement.py.

  1. exact assignment   integer features in [0, 7], EUCLID, integer init full of ties and with a duplicate centroid, max_iter = 0: label, count,
                        dist2 and inertia[0] bit for bit.  Pairwise cover of M in {1, 127, 128, 129, 257, 300} (one row, the tile edge, two tiles
                        and a row; 300 because C = 300 needs an M that holds it), C in {1, 2, 127, 128, 129, 300} (C <= M) and K in {1, 3, 50, 65, 130, 1024} (one K-chunk, the chunk edge,
                        32 chunks).  A control set whose centroids are permutations of ONE integer vector (equal norms): the mutant of
                        tests/test_kmeans_mutant_gpu.py passes it and fails the others.
  2. exact update       max_iter = 1: the centroids equal the restated fixed-order mean of the device's own label^0 -- bit for bit for EUCLID
                        and HELLINGER, within 1 fp32 ulp for COSINE --, with a cluster of exactly TMVB_KM_RUN members, one of more, an empty one.
  3. exact seeding      seeds equal the restated k-means++ for three metrics, several seeds, C in {1, 2, 5, M}; identical documents (total == 0).
  4. floating assignment  from the RETURNED centroids: s64(d, label[d]) >= max_c s64(d, c) - 2 TOL[K], |dist2 - fp64| <= 2 TOL[K], inertia[iters]
                        = the fixed-order sum of the returned dist2 bits.
  5. free-running       on the admissible inputs (tests/test_kmeans_host.py shows them admissible from the restatement alone): label, iters and
                        seeds equal the fp64 Lloyd loop, stop = 1; centroids within 2^-23, inertia[t] within 2 M TOL[K].
  6. stops              max_iter, tol at a known iteration, max_iter = 0.
  7. purity             identical bytes over two calls; assign-only slices equal the whole.
  8. cross-check        COSINE labels = idx[:, 0] of tmvb_topic_neighbors (DOT, database = the returned centroids, queries = the features)
                        wherever that call's best and second-best score differ by more than 2 ulp.
  9. models             cluster_docs on the trained golden LDA, CTM and CTPF corpora, .assign(predict(...)).

TOL[K] bounds |s - s64| (s64: the NumPy fp64 score of the fp64 features against the returned centroids).  The device does not return s, so
the measuring mode (TMVB_KMEANS_RECORD=<file>) records per K the worst of the two quantities the assertions of 4. bound, each halved:
(max_c s64(d, c) - s64(d, label[d])) / 2 and |dist2 - fp64| / 2.  Each literal is within [1, 10] x that record
(profiles/kmeans_tolerances_measured.json) and never above cap(K) = (1.5 K + 4) 2^-24 (tests/test_kmeans_host.py asserts both).
"""
import itertools
import json
import os

import numpy as np
import pytest

import kmeans_restatement as kr
from kmeans_restatement import COSINE, EUCLID, HELLINGER, RUN, cap

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MS = [1, 127, 128, 129, 257, 300]          # 300: the one M that admits C = 300 (C <= M)
CS = [1, 2, 127, 128, 129, 300]
KS = [1, 3, 50, 65, 130, 1024]
FLOAT_KS = [1, 3, 50, 65, 130, 1024]
# about 4 x the worst deviation per K over every floating and free-running case of this module on one MI355X (1.2e-7, 3.4e-7, 3.6e-7, 5.8e-7,
# 1.2e-6); K = 1: every feature, centroid and score is exact
TOL = {1: 0.0, 3: 4.7e-7, 50: 1.4e-6, 65: 1.5e-6, 130: 2.4e-6, 1024: 5.0e-6}
WORST = {K: 0.0 for K in FLOAT_KS}
# (K, M, C, planted groups, generator seed): pinned from 40 generator seeds by the restatement alone (tests/test_kmeans_host.py)
FREE = [(3, 257, 4, 3, 2), (50, 700, 7, 5, 28), (65, 300, 6, 4, 34), (130, 260, 5, 3, 11)]


def pairwise_cover(axes, ok):
    """greedy: the admissible grid in its natural order, each time the point that covers most value pairs not covered yet"""
    grid = [p for p in itertools.product(*axes) if ok(p)]
    pairs = lambda p: {(i, p[i], j, p[j]) for i in range(len(p)) for j in range(i + 1, len(p))}
    todo = set().union(*(pairs(p) for p in grid))
    out = []
    while todo:
        best = max(grid, key=lambda p: len(pairs(p) & todo))
        out.append(best)
        todo -= pairs(best)
    return out


CASES = pairwise_cover([MS, CS, KS], lambda p: p[1] <= p[0])
assert all({c[i] for c in CASES} == set(ax) for i, ax in enumerate([MS, CS, KS])) and len(CASES) < 60
CONTROL = [(129, 2, 3), (257, 129, 50), (128, 127, 65), (257, 257, 130)]


@pytest.fixture(scope="module")
def ctx(tmvb):
    c = tmvb.DeviceContext(0)
    yield c
    c.close()
    out = os.environ.get("TMVB_KMEANS_RECORD", "")
    if not out:
        return
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump({"kmeans.score_abs": {"measured": {str(K): WORST[K] for K in FLOAT_KS}, "tolerance": {str(K): TOL[K] for K in FLOAT_KS},
                                        "cap": {str(K): cap(K) for K in FLOAT_KS},
                                        "what": "per K, max over documents of (max_c s64(d, c) - s64(d, label[d])) / 2 and |dist2 - fp64| / 2 against the "
                                                "returned centroids, every case of test_floating_assignment and test_free_running of tests/test_kmeans_gpu.py"}},
                  f, indent=1)


def run(tmvb, ctx, K, metric, x, C, init=None, seed=0, max_iter=100, tol=0.0):
    rc, res = tmvb.kmeans_raw(ctx, K, metric, x, C, init, seed, max_iter, tol)
    assert rc == 0, res
    return res


def exact_inputs(M, C, K, control=False):
    """integer documents and centroids; the last centroid repeats the first (C >= 2): it stays empty"""
    x = kr.integer_cols(K, M, seed=1000 * M + K)
    if control:                                                       # permutations of one vector: equal norms, b_c cannot change the order
        rng = np.random.Generator(np.random.PCG64(7 * C + K))
        base = np.resize(np.array([0.0, 1.0, 2.0, 7.0, 1.0]), K)
        init = np.stack([rng.permutation(base) for _ in range(C)], axis=1)
    else:
        init = kr.integer_cols(K, C, seed=77 * C + K, levels=(0, 1, 2, 3, 7))
    if C >= 2:
        init[:, C - 1] = init[:, 0]
    return x, init


def assert_exact_assignment(tmvb, ctx, M, C, K, control):
    x, init = exact_inputs(M, C, K, control)
    F, Cf = kr.features32(x, EUCLID), kr.features32(init, EUCLID)
    label, dist2, count, J, s = kr.assign32(F, Cf)
    assert s.max() < 2 ** 24 and np.array_equal(s * 2, np.rint(s * 2))               # every score is an exact half-integer
    res = run(tmvb, ctx, K, EUCLID, x, C, init, max_iter=0)
    assert res["label"].dtype == np.int32 and res["dist2"].dtype == np.float32 and res["count"].dtype == np.int64
    assert np.array_equal(res["label"], label), np.flatnonzero(res["label"] != label)[:5]
    assert np.array_equal(res["count"], count) and res["count"].sum() == M
    assert res["dist2"].tobytes() == dist2.tobytes()
    assert res["inertia"].shape == (1,) and res["inertia"][0] == J
    assert (res["iters"], res["stop"], res["n_empty"], res["kp"]) == (0, 0, int((count == 0).sum()), (K + 3) // 4 * 4)
    assert np.all(res["seeds"] == -1) and np.array_equal(res["centroid"], init)
    if C >= 2:
        assert res["count"][C - 1] == 0                               # the duplicate: the lower index wins every tie


@pytest.mark.parametrize("M,C,K", CASES, ids=lambda v: str(v))
def test_exact_assignment(tmvb, ctx, M, C, K):
    assert_exact_assignment(tmvb, ctx, M, C, K, control=False)


@pytest.mark.parametrize("M,C,K", CONTROL, ids=lambda v: str(v))
def test_exact_assignment_equal_norms(tmvb, ctx, M, C, K):
    _, init = exact_inputs(M, C, K, control=True)
    assert len(set((init * init).sum(axis=0))) == 1
    assert_exact_assignment(tmvb, ctx, M, C, K, control=True)


# ------------------------------------------------------------------------------------------------------------------ 2. exact update
SIZES = (RUN, RUN + 44, 37)


def grouped_inputs(metric, K):
    """three well separated groups of SIZES documents, interleaved; four centroids, the last a copy of the first"""
    rng = np.random.Generator(np.random.PCG64(50 + metric))
    group = rng.permutation(np.repeat(np.arange(3), SIZES))
    if metric == EUCLID:
        x = rng.integers(0, 2, size=(K, len(group))).astype(np.float64)
        x[group, np.arange(len(group))] = 7.0
        init = np.zeros((K, 4))
        init[[0, 1, 2, 0], np.arange(4)] = 7.0
        return x, init, group
    alpha = np.full((len(group), K), 0.05)
    alpha[np.arange(len(group)), group] = 200.0
    g = rng.standard_gamma(alpha) + 1e-300
    x = np.ascontiguousarray((g / g.sum(axis=1, keepdims=True)).T)
    centres = np.full((K, 4), 0.01)
    centres[[0, 1, 2, 0], np.arange(4)] = 1.0
    centres /= centres.sum(axis=0)
    return x, kr.features64(centres, metric).T, group


@pytest.mark.parametrize("metric,K", [(EUCLID, 3), (EUCLID, 50), (HELLINGER, 50), (HELLINGER, 130), (COSINE, 50)], ids=lambda v: str(v))
def test_exact_update(tmvb, ctx, metric, K):
    x, init, group = grouped_inputs(metric, K)
    F, c0 = kr.features32(x, metric), init.T.astype(np.float32)
    r0 = run(tmvb, ctx, K, metric, x, 4, init, max_iter=0)
    assert np.array_equal(r0["label"], group) and r0["count"].tolist() == list(SIZES) + [0]  # exactly RUN, more than RUN, an empty cluster
    r1 = run(tmvb, ctx, K, metric, x, 4, init, max_iter=1)
    want = kr.update32(F, r0["label"], c0, metric)
    got = r1["centroid"].T
    assert np.array_equal(got, got.astype(np.float32).astype(np.float64))            # fp32 values, widened
    assert np.array_equal(got[3], c0[3].astype(np.float64))                          # the empty cluster keeps its centroid
    if metric == COSINE:
        assert np.all(np.abs(got - want) <= np.spacing(np.abs(want)))
    else:
        assert got.astype(np.float32).tobytes() == want.tobytes()
    # K = 3, EUCLID: the documents (7, 0, 0) equal the kept duplicate centroid and move to it; everywhere else no label moves
    moved = not np.array_equal(r1["label"], r0["label"])
    assert moved == (metric == EUCLID and K == 3) and (r1["iters"], r1["stop"], r1["n_empty"]) == (1, 0 if moved else 1, 0 if moved else 1)


# ------------------------------------------------------------------------------------------------------------------ 3. exact seeding
def seeding_data(metric, K, M):
    if metric == EUCLID:
        return np.random.Generator(np.random.PCG64(5)).normal(0.0, 3.0, size=(K, M))
    return kr.dirichlet_cols(K, M, 0.5, seed=6 + metric)


@pytest.mark.parametrize("metric", [EUCLID, HELLINGER, COSINE], ids=["euclid", "hellinger", "cosine"])
def test_exact_seeding(tmvb, ctx, metric):
    K, M = 50, 300                                                    # two blocks of TMVB_KM_RUN
    x = seeding_data(metric, K, M)
    F = kr.features32(x, metric)
    for C, seeds in ((1, (0, 1, 2)), (2, (0, 3)), (5, (0, 1, 2, 11)), (M, (4,))):
        for seed in seeds:
            res = run(tmvb, ctx, K, metric, x, C, None, seed=seed, max_iter=0)
            want = kr.seeding(F, C, seed)
            assert np.array_equal(res["seeds"], want), (C, seed, np.flatnonzero(res["seeds"] != want)[:5])
            assert len(set(res["seeds"].tolist())) == C and np.array_equal(res["centroid"].T.astype(np.float32), F[want])


@pytest.mark.parametrize("metric", [EUCLID, HELLINGER, COSINE], ids=["euclid", "hellinger", "cosine"])
def test_seeding_of_identical_documents(tmvb, ctx, metric):
    K, M = 5, 260
    x = np.repeat(np.array([[0.1], [0.2], [0.3], [0.15], [0.25]]), M, axis=1)
    first = min(M - 1, int(np.floor(kr.uniforms(9, 1)[0] * M)))
    for C in (5, M):
        res = run(tmvb, ctx, K, metric, x, C, None, seed=9, max_iter=0)
        want = [first] + [d for d in range(M) if d != first][:C - 1]                 # total == 0: the lowest document not yet chosen
        assert res["seeds"].tolist() == want == kr.seeding(kr.features32(x, metric), C, 9).tolist()
        assert np.all(res["label"] == 0) and res["count"][0] == M and res["n_empty"] == C - 1 and np.all(res["dist2"] == 0)


# ------------------------------------------------------------------------------------------------------------------ 4. floating assignment
def floating_checks(res, x, metric, K, tag):
    """the assertions of 4. against the returned centroids; returns the worst deviation in units of the score"""
    F64, c = kr.features64(x, metric), res["centroid"].T
    s64 = kr.scores64(F64, c)
    lab = res["label"]
    own = s64[np.arange(len(F64)), lab]
    short = s64.max(axis=1) - own
    d64 = ((F64 - c[lab]) ** 2).sum(axis=1)
    derr = np.abs(res["dist2"].astype(np.float64) - d64)
    worst = max(float(short.max()), float(derr.max())) / 2
    print(f"kmeans {tag}: worst deviation = {worst:.3e} (tolerance {TOL[K]:.3e}, cap {cap(K):.3e})")
    WORST[K] = max(WORST[K], worst)
    assert np.all(short <= 2 * TOL[K]), (tag, short.max())
    assert np.all(derr <= 2 * TOL[K]), (tag, derr.max())
    assert res["inertia"][res["iters"]] == kr.blocked_sum(res["dist2"]) and np.all(np.isfinite(res["inertia"][:res["iters"] + 1]))
    assert np.array_equal(res["count"], np.bincount(lab, minlength=c.shape[0])) and res["n_empty"] == int((res["count"] == 0).sum())
    return worst


@pytest.mark.parametrize("alpha", [0.1, 1.0])
@pytest.mark.parametrize("metric", [HELLINGER, COSINE], ids=["hellinger", "cosine"])
@pytest.mark.parametrize("K", FLOAT_KS)
def test_floating_assignment(tmvb, ctx, K, metric, alpha):
    M, C = 2 * 128 + 2, 130                                           # two tiles of centroids, three of documents
    x = kr.dirichlet_cols(K, M, alpha, seed=31 * K + int(10 * alpha))
    res = run(tmvb, ctx, K, metric, x, C, None, seed=K, max_iter=3)
    floating_checks(res, x, metric, K, (K, metric, alpha))
    assert TOL[K] <= cap(K)


# ------------------------------------------------------------------------------------------------------------------ 5. free-running
def free_input(K, M, G, gs):
    return kr.planted_mixture(K, M, G, 1000 * K + gs)


@pytest.mark.parametrize("K,M,C,G,gs", FREE, ids=lambda v: str(v))
def test_free_running(tmvb, ctx, K, M, C, G, gs):
    x = free_input(K, M, G, gs)
    F32, F64 = kr.features32(x, HELLINGER), kr.features64(x, HELLINGER)
    seeds = kr.seeding(F32, C, gs)
    ref = kr.lloyd64(F64, F32[seeds].astype(np.float64), HELLINGER)
    res = run(tmvb, ctx, K, HELLINGER, x, C, None, seed=gs, max_iter=100)
    assert np.array_equal(res["seeds"], seeds)
    assert res["iters"] == ref["iters"] and res["stop"] == 1 and ref["stop"] == 1 and res["moved_last"] == 0
    assert np.array_equal(res["label"], ref["label"])
    assert np.all(np.abs(res["centroid"].T - ref["centroids"]) <= 2.0 ** -23)
    J = res["inertia"]
    assert J.shape == (101,) and np.all(np.isnan(J[res["iters"] + 1:]))
    assert np.all(np.abs(J[:res["iters"] + 1] - ref["inertia"]) <= 2 * M * TOL[K]), np.abs(J[:res["iters"] + 1] - ref["inertia"]).max()
    floating_checks(res, x, HELLINGER, K, ("free", K, M, C))


# ------------------------------------------------------------------------------------------------------------------ 6. stops
def test_stops(tmvb, ctx):
    K, M, C, G, gs = FREE[1]
    x = free_input(K, M, G, gs)
    F32, F64 = kr.features32(x, HELLINGER), kr.features64(x, HELLINGER)
    ref = kr.lloyd64(F64, F32[kr.seeding(F32, C, gs)].astype(np.float64), HELLINGER)
    r = run(tmvb, ctx, K, HELLINGER, x, C, None, seed=gs, max_iter=2)
    assert (r["iters"], r["stop"]) == (2, 0) and np.array_equal(r["label"], ref["labels"][2]) and r["inertia"].shape == (3,) and np.all(np.isfinite(r["inertia"]))
    assert r["moved_last"] == int((ref["labels"][2] != ref["labels"][1]).sum()) > 0
    r = run(tmvb, ctx, K, HELLINGER, x, C, None, seed=gs, max_iter=0)
    assert (r["iters"], r["stop"], r["moved_last"]) == (0, 0, M) and np.array_equal(r["label"], ref["labels"][0]) and r["inertia"].shape == (1,)
    # tol: the relative decrease of J falls from iteration to iteration; a tol between two of them stops at the later one
    J = ref["inertia"]
    rel = (J[:-1] - J[1:]) / J[:-1]
    t = next(t for t in range(2, len(rel) + 1) if rel[t - 1] < 0.25 * rel[:t - 1].min())
    tol = float(np.sqrt(rel[t - 1] * rel[:t - 1].min()))
    assert 1 < t < ref["iters"] and rel[t - 1] > 0
    r = run(tmvb, ctx, K, HELLINGER, x, C, None, seed=gs, max_iter=100, tol=tol)
    assert (r["iters"], r["stop"]) == (t, 2) and np.array_equal(r["label"], ref["labels"][t]) and np.all(np.isnan(r["inertia"][t + 1:]))


# ------------------------------------------------------------------------------------------------------------------ 7. purity
def test_purity(tmvb, ctx):
    K, M, C, G, gs = FREE[2]
    x = free_input(K, M, G, gs)
    a, b = (run(tmvb, ctx, K, HELLINGER, x, C, None, seed=gs) for _ in range(2))
    for f in ("label", "centroid", "count", "dist2", "inertia", "seeds"):
        assert a[f].tobytes() == b[f].tobytes(), f
    assert (a["iters"], a["stop"], a["n_empty"]) == (b["iters"], b["stop"], b["n_empty"])
    whole = run(tmvb, ctx, K, HELLINGER, x, C, a["centroid"], max_iter=0)
    assert np.array_equal(whole["label"], a["label"]) and whole["dist2"].tobytes() == a["dist2"].tobytes()     # the returned labels are the best of the returned centroids
    for lo, hi in ((0, C), (0, 128), (100, 300), (129, 258), (M - C, M)):
        part = run(tmvb, ctx, K, HELLINGER, x[:, lo:hi], C, a["centroid"], max_iter=0)
        assert np.array_equal(part["label"], whole["label"][lo:hi]) and part["dist2"].tobytes() == whole["dist2"][lo:hi].tobytes(), (lo, hi)


# ------------------------------------------------------------------------------------------------------------------ 8. cross-check
def test_cosine_labels_against_the_neighbours_scan(tmvb, ctx):
    K, M, C = 50, 300, 9
    x = kr.planted_mixture(K, M, 6, 77)
    res = run(tmvb, ctx, K, COSINE, x, C, None, seed=3, max_iter=100)
    F = kr.features32(x, COSINE).astype(np.float64)
    rc, nb = tmvb.neighbors_raw(ctx, K, 0, res["centroid"], F.T, 0, 2)
    assert rc == 0, nb
    clear = (nb["score"][:, 0] - nb["score"][:, 1]) > 2 * np.spacing(nb["score"][:, 0])
    assert clear.sum() > M // 2 and np.array_equal(res["label"][clear], nb["idx"][clear, 0])


# ------------------------------------------------------------------------------------------------------------------ 9. models
def load(name):
    return np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))


def check_model(tmvb, model, k, new=None):
    P = tmvb.topic_proportions(model)
    K, M = P.shape
    tolK = cap(K)
    for metric, code in (("hellinger", HELLINGER), ("cosine", COSINE), ("euclid", EUCLID)):
        r = tmvb.cluster_docs(model, k, metric=metric, seed=1)
        assert r.labels.shape == (M,) and r.counts.sum() == M and r.centroids.shape == (K, k) and r.stop == 1 and len(r.inertia) == r.iters + 1
        np.testing.assert_allclose(r.profiles.sum(axis=0), 1.0, rtol=0, atol=1e-12)
        s64 = kr.scores64(kr.features64(P, code), r.centroids.T)
        assert np.all(s64.max(axis=1) - s64[np.arange(M), r.labels] <= 2 * tolK), metric
        reps = r.representatives(3)
        assert all(len(reps[c]) == min(3, r.counts[c]) and np.all(r.labels[reps[c]] == c) for c in range(k))
        again = tmvb.cluster_docs(model, k, metric=metric, init=r)                    # from a fixed point: one assignment, nothing moves
        assert again.iters <= 1 and np.array_equal(again.labels, r.labels)
        part = r.assign(P[:, 3:17])
        assert np.array_equal(part.labels, r.labels[3:17]) and part.dist2.tobytes() == r.dist2[3:17].tobytes() and part.iters == 0
        if new is not None:
            q = r.assign(new)
            Pq = tmvb.topic_proportions(new)
            sq = kr.scores64(kr.features64(Pq, code), r.centroids.T)
            assert q.labels.shape == (Pq.shape[1],) and np.all(sq.max(axis=1) - sq[np.arange(Pq.shape[1]), q.labels] <= 2 * tolK)


def test_cluster_docs_of_a_trained_lda_and_predict(tmvb):
    g = load("lda_m40_v60_k7")
    K, V = int(g["K"]), int(g["V"])
    m = tmvb.LDA(tmvb.PackedCorpus(g["doc_ptr"], g["terms"], g["counts"], V), K)
    m.beta = np.asfortranarray(g["beta0"]); m.beta_old = m.beta.copy(order="F")
    tmvb.gpu_train(m, iter=3, tol=0.0, checkelbo=1, printelbo=False)
    check_model(tmvb, m, 4, new=tmvb.predict(tmvb.syn_nsf(M=9, V=V, seed=12), m))


def test_cluster_docs_of_a_trained_ctm(tmvb):
    g = load("ctm_m40_v60_k5")
    K, V = int(g["K"]), int(g["V"])
    m = tmvb.CTM(tmvb.PackedCorpus(g["doc_ptr"], g["terms"], g["counts"], V), K)
    m.beta = np.asfortranarray(g["beta0"]); m.beta_old = m.beta.copy(order="F")
    tmvb.gpu_train_ctm(m, iter=3, tol=0.0, checkelbo=1, printelbo=False)
    check_model(tmvb, m, 3, new=tmvb.predict_ctm(tmvb.syn_nsf(M=9, V=V, seed=13), m))


def test_cluster_docs_of_a_trained_ctpf(tmvb):
    g = load("ctpf_m40_v60_u15_k4")
    K, V, U = int(g["K"]), int(g["V"]), int(g["U"])
    m = tmvb.CTPF(tmvb.PackedCorpus(g["doc_ptr"], g["terms"], g["counts"], V, g["rdr_ptr"], g["readers"], g["ratings"], U), K)
    m.alef = np.asfortranarray(g["alef0"]); m.alef_old = m.alef.copy(order="F")
    tmvb.gpu_train_ctpf(m, iter=3, tol=0.0, checkelbo=1, printelbo=False)
    check_model(tmvb, m, 3)
