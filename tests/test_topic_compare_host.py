"""
Topic comparison without a device (tests/test_topic_compare_gpu.py holds the kernels to the restatement; this file holds the restatement, the
host-side assignment, the argument rules and the Python layer):

  1. restatement   tests/topic_compare_restatement.py's JS, Hellinger and KL sums against mpmath at 50 digits on V <= 300: within the cap
                   (min(V, RUN) + runs + 8) 2^-53 S of the GPU tests plus the conditioning of the logarithm's argument, which device and restatement
                   share; its blocked sum against math.fsum of the same addends: within 0.17 of that cap, so the cap is no empty bound and the
                   restatement alone is an admissible reference.
  2. assignment    tmvb_assignment against brute force over all injections (n <= m <= 7, integer costs: totals compared with ==; tied optima and
                   +inf entries included), against scipy.optimize.linear_sum_assignment up to 200 x 300 (totals and validity), the infeasible case.
  3. errors        every TMVB_EINVAL and TMVB_ESHAPE rule of tmvb_topic_divergence, tmvb_term_relevance and tmvb_assignment, with a NULL context:
                   they are judged before a device is touched.
  4. pcoa          points planted on a plane: pairwise distances recovered to 1e-10; the sign rule.
  5. wrappers      argument handling of the Python layer.
  6. wiring        the unit is in both source lists, the mutant in the script, and the selection is the shared segmented sort of tmvb_topics.hip.
"""
import math

import numpy as np
import pytest

import topic_compare_restatement as tr
from topic_compare_restatement import HELLINGER, JS, KL, RUN, TV

EINVAL, ESHAPE, ENODEVICE = 1, 2, 7


# ------------------------------------------------------------------------------------------------------------------ 1. restatement
def exact_sums(metric, a, b, smooth):
    """sigma[i, j] of the PREPARED fp64 operands in 50-digit arithmetic (the roots and the smoothing are part of the stated arithmetic)"""
    import mpmath as mp
    mp.mp.dps = 50
    A, B = tr.prepare(metric, a, smooth), tr.prepare(metric, b, smooth)
    out = np.zeros((A.shape[0], B.shape[0]))
    for i in range(A.shape[0]):
        for j in range(B.shape[0]):
            s = mp.mpf(0)
            for w in range(A.shape[1]):
                p, q = mp.mpf(float(A[i, w])), mp.mpf(float(B[j, w]))
                if metric == JS:
                    if p > 0:
                        s += p * mp.log(2 * p / (p + q)) / 2
                    if q > 0:
                        s += q * mp.log(2 * q / (p + q)) / 2
                elif metric == HELLINGER:
                    s += (p - q) ** 2 / 2
                elif p > 0:
                    s += p * mp.log(p / q)
            out[i, j] = float(s)
    return out


@pytest.mark.parametrize("metric,smooth", [(JS, 0.0), (HELLINGER, 0.0), (KL, 1e-3)])
@pytest.mark.parametrize("V", [1, 2, 255, 257, 300])
def test_restatement_against_mpmath(metric, smooth, V):
    pytest.importorskip("mpmath")
    a, b = tr.dirichlet_rows(4, V, 10 + V), tr.dirichlet_rows(3, V, 20 + V, shift=1)
    _, sigma, S = tr.divergence(metric, a, b, smooth)
    ref = exact_sums(metric, a, b, smooth)
    # Against the exact value the argument of a logarithm matters too, which device and restatement share bit for bit (IEEE add and divide) and
    # the cap therefore leaves out: a relative error of 2^-53 in 2 p / s, and another in s, moves p log(2 p / s) by p 2^-53 each whatever the
    # size of the logarithm.  Summed: JS 2 * 2^-53 * (sum p + sum q) / 2, KL 2^-53 * sum p'.  Hellinger has no such term.
    A, B = tr.prepare(metric, a, smooth), tr.prepare(metric, b, smooth)
    mass = {JS: A.sum(axis=1)[:, None] + B.sum(axis=1)[None, :], HELLINGER: 0.0, KL: A.sum(axis=1)[:, None] + 0.0 * B.sum(axis=1)[None, :]}[metric]
    tol = tr.cap_factor(V) * S + tr.U * mass
    err = np.abs(sigma - ref)
    print(f"metric {metric} V {V}: worst |sigma - exact| / tolerance = {float(np.max(err / np.maximum(tol, 1e-300))):.3f}")
    assert np.all(np.isfinite(ref)) and np.all(err <= tol)


@pytest.mark.parametrize("metric,smooth", [(JS, 0.0), (HELLINGER, 0.0), (KL, 0.0), (KL, 1e-3)])
@pytest.mark.parametrize("V", [2, 255, 257, 1000])
def test_blocked_sum_stays_well_inside_the_cap(metric, smooth, V):
    """the restatement's blocked sequential sum against math.fsum of the SAME fp64 addends: within 0.17 of the cap of the GPU tests, so that cap is
    not an empty bound and leaves the device 0.83 of it"""
    a, b = tr.dirichlet_rows(5, V, 30 + V), tr.dirichlet_rows(4, V, 40 + V, shift=2)
    _, sigma, S = tr.divergence(metric, a, b, smooth)
    A, B = tr.prepare(metric, a, smooth), tr.prepare(metric, b, smooth)
    worst = 0.0
    for i in range(5):
        for j in range(4):
            t = tr.terms(metric, A[i], B[j])[0]
            if not np.all(np.isfinite(t)):
                assert sigma[i, j] == np.inf
                continue
            err, cap = abs(sigma[i, j] - math.fsum(t.tolist())), tr.cap_factor(V) * S[i, j]
            assert err <= 0.17 * cap, (i, j, err, cap)
            worst = max(worst, err / cap if cap > 0 else 0.0)
    print(f"metric {metric} smooth {smooth} V {V}: worst |blocked - fsum| / cap = {worst:.3f}")


def test_restatement_sum_order_is_the_stated_one():
    rng = np.random.default_rng(3)
    t = rng.random((2, 3, 600)) * 10.0 ** rng.integers(-8, 8, size=(2, 3, 600))
    want = np.zeros((2, 3))
    for r in range(3):
        run = np.zeros((2, 3))
        for w in range(r * RUN, min((r + 1) * RUN, 600)):
            run = run + t[:, :, w]
        want = want + run
    got = np.zeros((2, 3))
    for r in range(3):
        got = got + tr.seq_sum(t[:, :, r * RUN:(r + 1) * RUN])
    assert got.tobytes() == want.tobytes()
    assert not np.array_equal(got, t.sum(axis=-1))                  # and pairwise summation is another number


def test_restatement_identities():
    a = tr.dirichlet_rows(5, 300, 1)
    b = tr.dirichlet_rows(4, 300, 2)
    for m in (JS, HELLINGER, TV, KL):
        assert np.all(np.diag(tr.divergence(m, a)[0]) == 0.0)
    for m in (JS, HELLINGER, TV):
        assert tr.divergence(m, a, b)[0].tobytes() == tr.divergence(m, b, a)[0].T.copy().tobytes()
    D = tr.divergence(KL, a, b)[0]
    assert np.isinf(D).any() and not np.isnan(D).any()               # planted zeros: q = 0 < p somewhere
    assert np.all(np.isfinite(tr.divergence(KL, a, b, 1e-3)[0]))
    assert np.all(tr.divergence(JS, a, b)[0] <= math.log(2) + 1e-12)


# ------------------------------------------------------------------------------------------------------------------ 2. assignment
def assign(tmvb, cost):
    rc, m, total = tmvb.assignment_raw(cost)
    return rc, m, total


def valid(m, shape):
    return len(m) == shape[0] and len(set(m.tolist())) == shape[0] and m.min() >= 0 and m.max() < shape[1]


@pytest.mark.parametrize("n,m", [(1, 1), (1, 4), (2, 2), (3, 5), (4, 4), (5, 7), (6, 6), (7, 7)])
def test_assignment_against_brute_force(tmvb, n, m):
    rng = np.random.default_rng(100 * n + m)
    for trial in range(6):
        hi = (3, 10, 1000)[trial % 3]                                # hi = 3: many tied optima
        cost = rng.integers(0, hi, size=(n, m)).astype(np.float64)
        if trial >= 3 and m > 1:
            cost[rng.random((n, m)) < 0.3] = np.inf
        best, arg = tr.brute_force_assignment(cost)
        rc, match, total = assign(tmvb, cost)
        if not np.isfinite(best):
            assert rc == ESHAPE and "no assignment of finite cost" in match
            continue
        assert rc == 0, match
        assert valid(match, cost.shape) and total == best and tuple(match.tolist()) in arg
        assert total == sum(cost[i, match[i]] for i in range(n))


@pytest.mark.parametrize("n,m,seed", [(50, 50, 1), (120, 300, 2), (200, 300, 3), (200, 200, 4)])
def test_assignment_against_scipy(tmvb, n, m, seed):
    opt = pytest.importorskip("scipy.optimize")
    rng = np.random.default_rng(seed)
    cost = rng.random((n, m)) if seed % 2 else rng.integers(0, 50, size=(n, m)).astype(np.float64)
    rc, match, total = assign(tmvb, cost)
    assert rc == 0 and valid(match, cost.shape)
    r, c = opt.linear_sum_assignment(cost)
    want = cost[r, c].sum()
    assert abs(total - want) <= 1e-9 * max(1.0, abs(want))
    assert abs(cost[np.arange(n), match].sum() - total) <= 1e-9 * max(1.0, abs(total))


def test_assignment_infeasible_and_bad_arguments(tmvb):
    inf = np.inf
    rc, msg, _ = assign(tmvb, np.array([[inf, 1.0, inf], [inf, 2.0, inf]]))          # two rows, one usable column
    assert rc == ESHAPE and "no assignment of finite cost" in msg
    rc, msg, _ = assign(tmvb, np.array([[inf, inf]]))
    assert rc == ESHAPE
    assert assign(tmvb, np.zeros((3, 2)))[0] == EINVAL                # n > m
    assert assign(tmvb, np.zeros((0, 2)))[0] == EINVAL
    assert assign(tmvb, np.zeros((1, tr.KMAX + 1)))[0] == EINVAL
    assert assign(tmvb, np.array([[np.nan, 1.0]]))[0] == ESHAPE
    assert assign(tmvb, np.array([[-inf, 1.0]]))[0] == ESHAPE
    assert assign(tmvb, np.zeros(3))[0] == 1
    L, P = tmvb.lib(), tmvb._lib
    c = np.zeros((2, 2)); out = np.zeros(2, dtype=np.int32)
    assert L.tmvb_assignment(2, 2, None, out.ctypes.data_as(P.P_i32), None) == EINVAL
    assert L.tmvb_assignment(2, 2, c.ctypes.data_as(P.P_dbl), None, None) == EINVAL
    assert L.tmvb_assignment(2, 2, c.ctypes.data_as(P.P_dbl), out.ctypes.data_as(P.P_i32), None) == 0 and sorted(out.tolist()) == [0, 1]


# ------------------------------------------------------------------------------------------------------------------ 3. errors
def div(tmvb, metric, a, b=None, smooth=0.0, splits=0):
    return tmvb.topic_divergence_raw(None, metric, a, b, smooth, splits)


def test_divergence_einval_rules(tmvb):
    a = tr.dirichlet_rows(3, 300, 1)
    for kw, word in ((dict(metric=4), "unknown metric"), (dict(metric=-1), "unknown metric"), (dict(splits=-1), "splits"), (dict(splits=3), "splits"),
                     (dict(smooth=-1e-3, metric=KL), "smooth"), (dict(smooth=np.inf, metric=KL), "smooth"), (dict(smooth=np.nan, metric=KL), "smooth"),
                     (dict(smooth=1e-3, metric=JS), "smooth"), (dict(smooth=1e-3, metric=TV), "smooth"), (dict(smooth=1e-3, metric=HELLINGER), "smooth")):
        args = dict(metric=JS, smooth=0.0, splits=0); args.update(kw)
        rc, msg = div(tmvb, args["metric"], a, None, args["smooth"], args["splits"])
        assert rc == EINVAL and word in msg, (kw, rc, msg)
    assert div(tmvb, JS, a, None, 0.0, 2)[0] != EINVAL                # 300 terms are two runs
    rc, msg = div(tmvb, JS, np.zeros((3, 0)))
    assert rc == EINVAL and "V must be" in msg
    rc, msg = div(tmvb, JS, np.zeros((0, 5)))
    assert rc == EINVAL and "outside [1, 4096]" in msg
    rc, msg = div(tmvb, JS, a, np.zeros((0, 300)))
    assert rc == EINVAL and "outside [1, 4096]" in msg
    big = np.broadcast_to(np.zeros(1), (tr.KMAX + 1, 2))
    assert div(tmvb, JS, big)[0] == EINVAL and div(tmvb, JS, a[:, :2] * 0 + 0.5, big)[0] == EINVAL
    L, P = tmvb.lib(), tmvb._lib
    D = np.zeros((3, 3)); af = np.asfortranarray(a)
    pa, pD = af.ctypes.data_as(P.P_dbl), D.ctypes.data_as(P.P_dbl)
    assert L.tmvb_topic_divergence(None, JS, 300, 3, None, 0, None, 0.0, 0, pD, None) == EINVAL
    assert L.tmvb_topic_divergence(None, JS, 300, 3, pa, 0, None, 0.0, 0, None, None) == EINVAL
    assert L.tmvb_topic_divergence(None, JS, 1 << 30, 2, pa, 0, None, 0.0, 0, pD, None) == EINVAL          # K V = 2^31
    assert "2^31" in L.tmvb_last_error().decode()
    assert L.tmvb_topic_divergence(None, JS, 300, 3, pa, 0, None, 0.0, 0, pD, None) in (ENODEVICE, EINVAL)  # all rules pass: no device, or "ctx is NULL"
    assert "no HIP device" in L.tmvb_last_error().decode() or "ctx is NULL" in L.tmvb_last_error().decode()


def test_divergence_eshape_rules(tmvb):
    a = tr.dirichlet_rows(3, 40, 1)
    for side in ("a", "b"):
        for v, word in ((np.nan, "non-finite"), (np.inf, "non-finite"), (-0.25, "negative")):
            x = a.copy(); x[1, 7] = v
            rc, msg = div(tmvb, JS, x) if side == "a" else div(tmvb, JS, a, x)
            assert rc == ESHAPE and word in msg and f"{side} row 1" in msg, (side, v, rc, msg)
        x = a.copy(); x[2] *= 1.0 + 3e-6
        rc, msg = div(tmvb, TV, x) if side == "a" else div(tmvb, TV, a, x)
        assert rc == ESHAPE and f"{side} row 2 does not sum to 1" in msg
    x = a.copy(); x[2] *= 1.0 + 5e-7
    assert div(tmvb, TV, x)[0] != ESHAPE                               # inside the 1e-6 rule
    rc, msg = div(tmvb, 9, a * np.nan)
    assert rc == EINVAL                                              # the order of tmvb_topic_neighbors: arguments before contents


def rel(tmvb, beta, pw, pi, lam=0.6, n=2, **kw):
    return tmvb.term_relevance_raw(None, beta, pw, pi, lam, n, **kw)


def test_relevance_einval_and_eshape_rules(tmvb):
    beta, pw, pi = tr.relevance_inputs(3, 20, 1)
    for lam in (-0.1, 1.1, np.nan, np.inf):
        rc, msg = rel(tmvb, beta, pw, pi, lam=lam)
        assert rc == EINVAL and "lambda" in msg
    for n in (0, -1, 21):
        rc, msg = rel(tmvb, beta, pw, pi, n=n)
        assert rc == EINVAL and "outside [1, V]" in msg
    assert rel(tmvb, np.zeros((0, 20)), pw, np.zeros(0))[0] == EINVAL
    assert rel(tmvb, np.zeros((3, 0)), np.zeros(0), pi)[0] == EINVAL
    assert rel(tmvb, np.zeros((tr.KMAX + 1, 2)), np.full(2, 0.5), np.zeros(tr.KMAX + 1))[0] == EINVAL
    assert rel(tmvb, beta, pw[:5], pi)[0] == 1 and rel(tmvb, beta, pw, pi[:2])[0] == 1      # the wrapper's own shape rule
    L, P = tmvb.lib(), tmvb._lib
    bf = np.asfortranarray(beta)
    idx = np.zeros((3, 2), dtype=np.int32); sc = np.zeros((3, 2)); cnt = np.zeros(3, dtype=np.int32); d = np.zeros(20); s = np.zeros(20)
    full = [bf.ctypes.data_as(P.P_dbl), pw.ctypes.data_as(P.P_dbl), pi.ctypes.data_as(P.P_dbl), 0.6, 2, idx.ctypes.data_as(P.P_i32),
            sc.ctypes.data_as(P.P_dbl), cnt.ctypes.data_as(P.P_i32), None, d.ctypes.data_as(P.P_dbl), s.ctypes.data_as(P.P_dbl), None]
    for q in (0, 1, 2, 5, 6, 7):                                     # a NULL required argument
        args = list(full); args[q] = None
        assert L.tmvb_term_relevance(None, 3, 20, *args) == EINVAL and "NULL" in L.tmvb_last_error().decode(), q
    for q in (9, 10):                                                # one of distinct / saliency without the other
        args = list(full); args[q] = None
        assert L.tmvb_term_relevance(None, 3, 20, *args) == EINVAL and "together" in L.tmvb_last_error().decode()
    assert L.tmvb_term_relevance(None, 2, 1 << 30, *full) == EINVAL and "2^31" in L.tmvb_last_error().decode()
    assert L.tmvb_term_relevance(None, 3, 20, *full) in (ENODEVICE, EINVAL)
    assert "no HIP device" in L.tmvb_last_error().decode() or "ctx is NULL" in L.tmvb_last_error().decode()
    # contents
    for v, word in ((np.nan, "non-finite"), (-0.5, "negative")):
        x = beta.copy(); x[1, 4] = v
        rc, msg = rel(tmvb, x, pw, pi)
        assert rc == ESHAPE and word in msg
    x = beta.copy(); x[0] *= 1.0 + 3e-6
    rc, msg = rel(tmvb, x, pw, pi)
    assert rc == ESHAPE and "beta row 0 does not sum to 1" in msg
    for name, q in (("pw", 1), ("pi", 2)):
        for bad in (np.nan, -0.1):
            ops = [beta, pw.copy(), pi.copy()]; ops[q][0] = bad
            rc, msg = rel(tmvb, *ops)
            assert rc == ESHAPE and name in msg, (name, bad, msg)
        ops = [beta, pw.copy(), pi.copy()]; ops[q] = ops[q] * 1.01
        rc, msg = rel(tmvb, *ops)
        assert rc == ESHAPE and f"{name} does not sum to 1" in msg


# ------------------------------------------------------------------------------------------------------------------ 4. pcoa
def test_pcoa_recovers_points_on_a_plane(tmvb):
    rng = np.random.default_rng(5)
    P2 = rng.normal(size=(12, 2)) * np.array([3.0, 1.0])
    Q, _ = np.linalg.qr(rng.normal(size=(7, 7)))
    X = P2 @ Q[:2] + rng.normal(size=7)                              # the plane, rotated into 7 dimensions and shifted
    D = np.sqrt(((X[:, None, :] - X[None, :, :]) ** 2).sum(axis=-1))
    xy = tmvb.pcoa(D)
    assert xy.shape == (12, 2)
    D2 = np.sqrt(((xy[:, None, :] - xy[None, :, :]) ** 2).sum(axis=-1))
    assert np.abs(D2 - D).max() <= 1e-10
    for c in range(2):                                               # the sign rule: the coordinate of largest magnitude is positive
        assert xy[np.argmax(np.abs(xy[:, c])), c] > 0
    assert np.abs(xy.mean(axis=0)).max() <= 1e-12 and xy[:, 0].var() >= xy[:, 1].var()
    perm = rng.permutation(12)                                       # relabelling the points moves the rows, nothing else
    np.testing.assert_allclose(tmvb.pcoa(D[np.ix_(perm, perm)]), xy[perm], rtol=0, atol=1e-9)
    assert tmvb.pcoa(np.zeros((1, 1))).tolist() == [[0.0, 0.0]]
    for bad in (np.zeros((2, 3)), np.array([[0.0, np.nan], [np.nan, 0.0]])):
        with pytest.raises(ValueError):
            tmvb.pcoa(bad)


# ------------------------------------------------------------------------------------------------------------------ 5. wrappers
def test_wrapper_arguments(tmvb):
    a = tr.dirichlet_rows(3, 30, 1)
    with pytest.raises(ValueError):
        tmvb.topic_distances(a, metric="euclid")
    with pytest.raises(ValueError):
        tmvb.compare_topics(a, metric="cosine")
    with pytest.raises(tmvb.TopicModelError):
        tmvb.topic_distances(object())
    with pytest.raises(tmvb.TopicModelError):
        tmvb.topic_distances(np.zeros(4))
    with pytest.raises(ValueError):
        tmvb.topic_stability([a])
    with pytest.raises(tmvb.TopicModelError):
        tmvb.topic_stability([a, a[:2]])                             # a run with fewer topics than the first
    with pytest.raises(tmvb.TopicModelError):
        tmvb.topic_stability([a, a[:, :20]])
    with pytest.raises(ValueError):
        tmvb.relevant_terms(a, lam=1.5)
    with pytest.raises(ValueError):
        tmvb.relevant_terms(a, topn=0)
    with pytest.raises(ValueError):
        tmvb.relevant_terms(a, topn=31)
    assert tmvb.topic_divergence_raw(None, JS, np.zeros(3))[0] == 1
    assert tmvb.topic_divergence_raw(None, JS, a, a[:, :7])[0] == 1
    assert tmvb.topic_word_matrix(a).flags.f_contiguous

    class Fake:                                                      # a CTPF-like model: expected topic weights, rows normalised
        alef = np.arange(1.0, 13.0).reshape(3, 4)
        bet = np.array([1.0, 2.0, 4.0])
    b = tmvb.topic_word_matrix(Fake())
    np.testing.assert_allclose(b.sum(axis=1), 1.0, rtol=0, atol=1e-15)
    np.testing.assert_allclose(b[1], Fake.alef[1] / Fake.alef[1].sum(), rtol=1e-15)


def test_comparison_object_on_a_given_matrix(tmvb):
    D = np.array([[0.9, 0.1, 0.5], [0.2, 0.8, 0.05]])
    c = tmvb.TopicComparison(D, "js", np.zeros((2, 1)), np.zeros((3, 1)))
    assert c.match.tolist() == [1, 2] and not c.transposed and c.match_distance.tolist() == [0.1, 0.05]
    assert c.nearest.tolist() == [1, 2] and c.unmatched.tolist() == [0]
    t = tmvb.TopicComparison(D.T.copy(), "js", np.zeros((3, 1)), np.zeros((2, 1)))
    assert t.transposed and t.match.tolist() == [1, 2] and t.unmatched.tolist() == [0] and t.match_distance.tolist() == [0.1, 0.05]
    with pytest.raises(tmvb.TopicModelError):
        c.redundant(0.5)
    with pytest.raises(tmvb.TopicModelError):
        c.jaccard()
    S = np.array([[0.0, 0.3, 0.01], [0.3, 0.0, 0.2], [0.01, 0.2, 0.0]])
    s = tmvb.TopicComparison(S, "js", np.zeros((3, 1)), None)
    assert s.redundant(0.25) == [(0, 2, 0.01), (1, 2, 0.2)] and s.redundant(0.005) == [] and s.match.tolist() == [0, 1, 2]

    class M:
        def __init__(self, topics):
            self.topics = topics
    a, b = M([np.array([1, 2, 3, 4]), np.array([5, 6, 7, 8])]), M([np.array([2, 1, 9, 9]), np.array([8, 7, 6, 5])])
    j = tmvb.TopicComparison(np.zeros((2, 2)), "js", a, b).jaccard(topn=2)
    assert j.tolist() == [[1.0, 0.0], [0.0, 0.0]]
    assert tmvb.TopicComparison(np.zeros((2, 2)), "js", a, b).jaccard(topn=4)[1, 1] == 1.0


# ------------------------------------------------------------------------------------------------------------------ 6. wiring
def test_the_unit_is_wired_in_and_shares_the_sort(tmvb):
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "topicmodelsvb.jl_amd", "csrc")
    assert "tmvb_topic_compare.hip" in tmvb._lib.SOURCES and "$(CSRC)/tmvb_topic_compare.hip" in open(os.path.join(root, "Makefile")).read()
    assert "TMVB_MUTANT_TD_DROP_TAIL" in open(os.path.join(csrc, "tmvb_internal.h")).read()
    assert "tmvb_topic_compare.hip -DTMVB_MUTANT_TD_DROP_TAIL=1" in open(os.path.join(root, "tools", "build_mutants.sh")).read()
    src = open(os.path.join(csrc, "tmvb_topic_compare.hip")).read()
    assert '#include "tmvb_call.h"' in src and "hipMalloc(" not in src and "hipFree(" not in src and "atomic" not in src.replace("atomics", "")
    # one selection: the segmented radix sort of tmvb_topic_order, not another n-best insertion list
    assert "tmvb_segmented_sort_pairs(" in src and "hipcub" not in src
    users = [f for f in os.listdir(csrc) if "DeviceSegmentedRadixSort" in open(os.path.join(csrc, f)).read()]
    assert "tmvb_topics.hip" in users and "tmvb_topic_compare.hip" not in users
    assert open(os.path.join(csrc, "tmvb_topics.hip")).read().count("tmvb_segmented_sort_pairs(") == 2      # the definition and tmvb_topic_order's call
    for name in ("tmvb_topic_divergence", "tmvb_term_relevance", "tmvb_assignment"):
        assert name in tmvb.exported_symbols()
    for name in ("topic_distances", "compare_topics", "topic_stability", "relevant_terms", "topic_map", "pcoa", "TopicComparison"):
        assert name in tmvb.__all__ and hasattr(tmvb, name)
