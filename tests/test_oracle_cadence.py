"""
The fp64 C oracle's train! at every check cadence (CPU): pins the checker of tests/test_train_loop_gpu.py before it is used there.

That module runs the oracle ONCE per case with checkelbo = 1 and masks the trajectory to k % c == 0 for the other cadences.  What licenses it, for all
five families (src/LDA.jl:161-187 and its siblings, check_elbo! src/modelutils.jl:574-585):
  * train(iter = 12, tol = 0, checkelbo = c), c in {1, 2, 5, 12, 13, Inf}: 12 entries, finite exactly where k % c == 0 and there bit-equal to the
    c = 1 trajectory; the final state bit-equal across all c (evaluating the ELBO touches nothing);
  * model.elbo afterwards is the last checked value -- for c = 13 and c = Inf the value from before the call: the baseline too is skipped when
    checkelbo > iter (src/LDA.jl:167);
  * tol = 1e30 stops at the first check: k = c, done == c;
  * two calls (4, c = 2) then (8, c = 4) on one object are the one call of 12 (the oracle holds nothing but its state).
Cases: the golden fixture lda_m40_v60_k7 and one small synthetic corpus for each other family.
"""
import math
import os

import numpy as np
import pytest

from test_train_loop_gpu import CADENCES, GOLD, ITER, STATE, checked, make_oracle, oracle_train, state_of


def _case(tmvb, fam):
    if fam == "lda":
        z = np.load(os.path.join(GOLD, "lda_m40_v60_k7.npz"))
        return dict(family="lda", K=int(z["K"]), V=int(z["V"]), U=0, doc_ptr=z["doc_ptr"], terms=z["terms"], counts=z["counts"], beta0=z["beta0"])
    if fam == "ctpf":
        pc = tmvb.syn_citeu(M=60, V=90, U=20, seed=31)
        return dict(family=fam, K=6, V=pc.V, U=pc.U, doc_ptr=pc.doc_ptr, terms=pc.terms, counts=pc.counts, rdr_ptr=pc.rdr_ptr, readers=pc.readers,
                    ratings=pc.ratings, alef0=np.exp(tmvb.dirichlet_rows(6, pc.V, seed=4) - 0.5))
    # (fLDA's ELBO is not monotone on the smallest corpora -- its eta step is no coordinate ascent -- and tol = 0 would stop it: a corpus where it rises 12 times)
    pc = tmvb.syn_nsf(M=100, V=300, seed=5) if fam == "flda" else tmvb.syn_nsf(M=50, V=80, seed=31)
    K = {"ctm": 6, "flda": 12, "fctm": 5}[fam]
    return dict(family=fam, K=K, V=pc.V, U=0, doc_ptr=pc.doc_ptr, terms=pc.terms, counts=pc.counts, beta0=tmvb.dirichlet_rows(K, pc.V, seed=3),
                kappa0=tmvb.dirichlet_rows(1, pc.V, seed=5)[0])


@pytest.fixture(scope="module")
def runs(tmvb, oracle):
    """family -> (case, {c: (trajectory, final state, elbo field)})"""
    out = {}
    for fam in STATE:
        g = _case(tmvb, fam)
        per = {}
        for c in CADENCES:
            om = make_oracle(oracle, g)
            assert om.elbo == 0.0
            t = oracle_train(om, iter=ITER, tol=0.0, checkelbo=c)
            per[c] = (t, state_of(om, fam), om.elbo)
        out[fam] = (g, per)
    return out


@pytest.mark.parametrize("fam", list(STATE))
def test_trajectory_is_the_every_iteration_one_masked(runs, fam):
    _, per = runs[fam]
    t1 = per[1][0]
    assert len(t1) == ITER and np.all(np.isfinite(t1)), t1
    for c in CADENCES:
        t, m = per[c][0], checked(c)
        assert len(t) == ITER, (fam, c, len(t))
        assert np.array_equal(np.isfinite(t), m) and np.array_equal(np.isnan(t), ~m), (fam, c, t)
        assert np.array_equal(t[m], t1[m]), (fam, c, t, t1)                    # bit-equal


@pytest.mark.parametrize("fam", list(STATE))
def test_final_state_does_not_depend_on_the_cadence(runs, fam):
    _, per = runs[fam]
    for c in CADENCES:
        for n in STATE[fam]:
            assert np.array_equal(per[c][1][n], per[1][1][n]), (fam, c, n)


@pytest.mark.parametrize("fam", list(STATE))
def test_elbo_field_is_the_last_checked_value(runs, fam):
    _, per = runs[fam]
    for c in CADENCES:
        t, _, elbo = per[c]
        m = checked(c)
        if m.any():
            assert elbo == t[m][-1] and elbo != 0.0, (fam, c, elbo, t)
        else:
            assert elbo == 0.0, (fam, c, elbo)                                  # checkelbo > iter: not even the baseline is evaluated


@pytest.mark.parametrize("fam", list(STATE))
def test_huge_tol_stops_at_the_first_check(runs, oracle, fam):
    g, per = runs[fam]
    for c in CADENCES:
        om = make_oracle(oracle, g)
        t = oracle_train(om, iter=ITER, tol=1e30, checkelbo=c)
        if checked(c).any():
            assert len(t) == c and np.array_equal(np.isfinite(t), checked(c, c)), (fam, c, t)       # done == c
            assert t[-1] == per[1][0][c - 1] == om.elbo
        else:
            assert len(t) == ITER and np.all(np.isnan(t)), (fam, c, t)


@pytest.mark.parametrize("fam", list(STATE))
def test_two_calls_are_one(runs, oracle, fam):
    g, per = runs[fam]
    om = make_oracle(oracle, g)
    a = oracle_train(om, iter=4, tol=0.0, checkelbo=2)
    b = oracle_train(om, iter=8, tol=0.0, checkelbo=4)
    t1 = per[1][0]
    assert np.array_equal(a[[1, 3]], t1[[1, 3]]) and np.array_equal(b[[3, 7]], t1[[7, 11]])
    assert np.array_equal(np.isfinite(a), checked(2, 4)) and np.array_equal(np.isfinite(b), checked(4, 8))
    s = state_of(om, fam)
    for n in STATE[fam]:
        assert np.array_equal(s[n], per[math.inf][1][n]), (fam, n)
