"""
train!'s outer loop (tmvb_train_group_loop, csrc/tmvb_train.h) as a host state machine around the kernels: check cadence, stop rule, repeated calls.

A checked iteration (k % checkelbo == 0) takes other paths than an unchecked one -- the LOGZ instantiations of the statistics kernels, the copy of
the alpha the E-step read, lda_elbo_doc_kernel on a side stream, update_beta! leaving sum S dlog beta, CTPF's msteps_after, fLDA's parts_valid, fCTM's
filt_pw_valid -- and the rest of the suite runs the loop with checkelbo = 1 or Inf almost everywhere.  Here, for all five models and every plan the
cases below reach, with iter = 12 and checkelbo in {1, 2, 5, 12, 13, Inf}:

  A  checking does not change the iteration: every field update_host returns is bit-identical across the cadences;
  B  the bookkeeping (length, NaN pattern, baseline, the host's elbo field, elbo_form) and the values against the fp64 oracle;
  C  the signed stop rule decides at a known iteration, exactly;
  D  a second train on the same handle -- through the C ABI with no set_state in between (D1), and through the host (D2);
  E  the stepwise operators behind a train! that collected parts.

The oracle is the checker: ONE run per case with checkelbo = 1, tol = 0 (cached per module); tests/test_oracle_cadence.py (CPU) proves that its
trajectory at another cadence is that trajectory masked to k % c == 0, with the same final state.  Every synthetic case's oracle ELBO rises at each of
the 12 iterations (asserted before it is relied on), so tol = 0 never stops a run early.

Measured on MI355X (shipped library):
  A   bit-identical across all six cadences in all eight cases: LDA (one pass; pipelined pieces; K = 70 with empty documents), CTM (K = 12, K = 64), fLDA,
      fCTM, CTPF.  No tolerance stands in for bit identity anywhere in this module.
  D1  the state after (4, ce = 2) + (8, ce = 4) on one handle is bit-identical to one call of 12 with ce = 0 in all eight cases.
  D2  two host-level train() calls happened to be bit-identical to the one call of 12 in all eight cases, CTPF included (printed, not asserted).
  Every comparison with the oracle stayed inside the existing keys of tests/tol.py (worst: flda.elbo_rel_free 1.8e-7 of 2e-7, ctpf.elbo_rel_step
  3.1e-7 of 5e-7 in scenario E): no trainloop.* key was needed.
"""
import contextlib
import ctypes as C
import math
import os

import numpy as np
import pytest

from tol import TOL, within

GOLD = os.path.join(os.path.dirname(__file__), "golden")
ITER = 12
CADENCES = (1, 2, 5, 12, 13, math.inf)

STATE = {
    "lda": ("alpha", "beta", "beta_old", "gamma", "Elogtheta", "Elogtheta_old"),
    "flda": ("eta", "alpha", "kappa", "kappa_old", "beta", "beta_old", "gamma", "Elogtheta", "Elogtheta_old", "tau", "tau_old"),
    "ctm": ("mu", "sigma", "invsigma", "beta", "beta_old", "lam", "lam_old", "vsq", "logzeta"),
    "fctm": ("eta", "mu", "sigma", "invsigma", "kappa", "kappa_old", "beta", "beta_old", "lam", "lam_old", "vsq", "logzeta", "tau", "tau_old"),
    "ctpf": ("alef", "alef_old", "he", "he_old", "bet", "bet_old", "vav", "vav_old", "dalet", "dalet_old", "het", "het_old", "gimel", "gimel_old",
             "zayin", "zayin_old"),
}

# name: (family, K, corpus, environment at model creation).  The smallest corpora that reach each plan; seeds and the initial beta / kappa / alef as in
# tests/test_comm_gpu.py (dirichlet_rows seed 3 / 5 / 4).
CASES = {
    "lda_k20": ("lda", 20, "nsf600", {}),                                  # one-pass plan
    "lda_k50_pieces": ("lda", 50, "nsf600", {"TMVB_LDA_PIECES": "3"}),     # pipelined pieces, shadow statistics buffer
    "ctm_k12": ("ctm", 12, "nsf300", {}),                                  # lane-per-document kernel
    "ctm_k64": ("ctm", 64, "nsf300", {}),                                  # generic CG kernel
    "flda_k20": ("flda", 20, "nsf600", {}),
    "fctm_k12": ("fctm", 12, "nsf300", {}),
    "ctpf_k10": ("ctpf", 10, "citeu400", {}),
    "lda_m30_v50_k70_empty": ("lda", 70, "golden", {}),                    # empty documents and unused terms
}
SYNTHETIC = [n for n in CASES if CASES[n][2] != "golden"]
ALL = list(CASES)


def checked(c, n=ITER):
    """mask of the iterations k = 1 .. n that check_elbo! evaluates at cadence c"""
    k = np.arange(1, n + 1)
    return np.zeros(n, dtype=bool) if c == math.inf else (k % int(c) == 0)


def case_data(tmvb, name):
    """corpus arrays and initial parameters of a case (host only: also used by tests/test_oracle_cadence.py)"""
    fam, K, corpus, env = CASES[name]
    if corpus == "golden":
        z = np.load(os.path.join(GOLD, name + ".npz"))
        g = {k: z[k] for k in z.files}
        return dict(family=fam, K=int(g["K"]), V=int(g["V"]), U=0, env=env, doc_ptr=g["doc_ptr"], terms=g["terms"], counts=g["counts"], beta0=g["beta0"])
    if corpus == "citeu400":
        pc = tmvb.syn_citeu(M=400, V=300, U=60, seed=31)
        return dict(family=fam, K=K, V=pc.V, U=pc.U, env=env, doc_ptr=pc.doc_ptr, terms=pc.terms, counts=pc.counts, rdr_ptr=pc.rdr_ptr,
                    readers=pc.readers, ratings=pc.ratings, alef0=np.exp(tmvb.dirichlet_rows(K, pc.V, seed=4) - 0.5))
    pc = tmvb.syn_nsf(M=600, V=800, seed=23) if corpus == "nsf600" else tmvb.syn_nsf(M=300, V=120, seed=31)
    return dict(family=fam, K=K, V=pc.V, U=0, env=env, doc_ptr=pc.doc_ptr, terms=pc.terms, counts=pc.counts,
                beta0=tmvb.dirichlet_rows(K, pc.V, seed=3), kappa0=tmvb.dirichlet_rows(1, pc.V, seed=5)[0])


def make_oracle(oc, g):
    fam, K = g["family"], g["K"]
    if fam == "ctpf":
        return oc.CTPF(oc.CSR(g["doc_ptr"], g["terms"], g["counts"], g["V"], g["rdr_ptr"], g["readers"], g["ratings"], g["U"]), K, g["alef0"])
    csr = oc.CSR(g["doc_ptr"], g["terms"], g["counts"], g["V"])
    if fam in ("flda", "fctm"):
        return (oc.fLDA if fam == "flda" else oc.fCTM)(csr, K, g["beta0"], g["kappa0"])
    return (oc.LDA if fam == "lda" else oc.CTM)(csr, K, g["beta0"])


def state_of(m, fam):
    return {n: np.array(getattr(m, n), copy=True) for n in STATE[fam]}


def oracle_train(om, **kw):
    return np.asarray(om.train(**kw), dtype=np.float64)


@contextlib.contextmanager
def _environment(env):
    with pytest.MonkeyPatch.context() as mp:              # the plan variables are read when the model is created
        for k, v in env.items():
            mp.setenv(k, v)
        yield


def make_device(tmvb, g):
    fam, K = g["family"], g["K"]
    with _environment(g["env"]):
        if fam == "ctpf":
            pc = tmvb.PackedCorpus(g["doc_ptr"], g["terms"], g["counts"], g["V"], g["rdr_ptr"], g["readers"], g["ratings"], g["U"])
            gm = tmvb.gpuCTPF(pc, K)
            gm.alef = np.asfortranarray(g["alef0"]); gm.alef_old = gm.alef.copy(order="F")
        else:
            pc = tmvb.PackedCorpus(g["doc_ptr"], g["terms"], g["counts"], g["V"])
            gm = {"lda": tmvb.gpuLDA, "ctm": tmvb.gpuCTM, "flda": tmvb.gpufLDA, "fctm": tmvb.gpufCTM}[fam](pc, K)
            gm.beta = np.asfortranarray(g["beta0"]); gm.beta_old = gm.beta.copy(order="F")
            if fam in ("flda", "fctm"):
                gm.kappa = np.array(g["kappa0"], dtype=np.float64); gm.kappa_old = gm.kappa.copy()
        gm.update_buffer()
    return gm


def device_train(gm, fam, **kw):
    if fam == "ctpf":
        kw["recs"] = False
    return np.asarray(gm.train(printelbo=False, **kw), dtype=np.float64)


def abi_train(tmvb, gm, fam, iters, ce, tol=0.0):
    """tmvb_<model>_train straight through the C ABI: no update_buffer (set_state) in front, no update_host behind"""
    L = tmvb.lib()
    K = gm.K
    traj = np.full(max(iters, 1), np.nan); done = C.c_int32(0); base = C.c_double(float("nan"))
    tail = (C.c_int32(ce), traj.ctypes.data_as(C.POINTER(C.c_double)), C.byref(done), C.byref(base))
    if fam == "ctpf":
        rc = L.tmvb_ctpf_train(gm.handle, C.c_int32(iters), C.c_double(tol), C.c_int32(10), C.c_double(1.0 / K ** 2), *tail)
    else:
        rc = getattr(L, f"tmvb_{fam}_train")(gm.handle, C.c_int32(iters), C.c_double(tol), C.c_int32(1000), C.c_double(1.0 / K ** 2), C.c_int32(10),
                                               C.c_double(1.0 / K ** 2), *tail)
    assert rc == 0, L.tmvb_last_error()
    return traj[:done.value], base.value


def stepwise_iteration(gm, fam):
    """one outer iteration by the stepwise operators, in train!'s order"""
    gm.estep(); gm.reduce_docs()
    if fam == "lda":
        gm.update_beta(); gm.update_alpha()
    elif fam == "ctm":
        gm.update_beta(); gm.update_sigma(); gm.update_mu()
    else:
        gm.mstep()


# --------------------------------------------------------------------------------------------------------- per-module caches
_DATA, _ORACLE, _DEVICE = {}, {}, {}


def data(tmvb, name):
    if name not in _DATA:
        _DATA[name] = case_data(tmvb, name)
    return _DATA[name]


def oracle_run(tmvb, oc, name):
    """the ONE oracle run of a case: checkelbo = 1, tol = 0 -> baseline, trajectory (12 entries), never modified afterwards"""
    if name not in _ORACLE:
        g = data(tmvb, name)
        om = make_oracle(oc, g)
        base = om.update_elbo(store=False)
        traj = oracle_train(om, iter=ITER, tol=0.0, checkelbo=1)
        assert len(traj) == ITER and np.all(np.isfinite(traj)), (name, traj)       # tol = 0 did not stop the oracle early
        if name in SYNTHETIC:
            assert np.all(np.diff(np.concatenate([[base], traj])) > 0), (name, "the oracle's ELBO must rise at every iteration", base, traj)
        traj.setflags(write=False)
        _ORACLE[name] = dict(base=base, traj=traj, emax=float(np.max(np.abs(np.concatenate([[base], traj])))))
    return _ORACLE[name]


def device_runs(tmvb, name):
    """fresh model + train(iter = 12, tol = 0, checkelbo = c) for every cadence, once per case"""
    if name not in _DEVICE:
        g = data(tmvb, name)
        fam = g["family"]
        runs = {}
        for c in CADENCES:
            gm = make_device(tmvb, g)
            elbo_before = gm.elbo
            traj = device_train(gm, fam, iter=ITER, tol=0.0, checkelbo=c)
            r = dict(traj=traj, state=state_of(gm, fam), elbo=gm.elbo, elbo_before=elbo_before, base=gm.elbo_baseline, form=gm.elbo_form())
            if c == math.inf:
                r["elbo_walk"] = gm.update_elbo(); r["form_walk"] = gm.elbo_form()
            gm.close()
            runs[c] = r
        _DEVICE[name] = runs
    return _DEVICE[name]


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)) / np.abs(b)


gpu = pytest.mark.gpu


# --------------------------------------------------------------------------------------------------------- A
@gpu
@pytest.mark.parametrize("name", ALL)
def test_a_checking_does_not_change_the_iteration(tmvb, name):
    """The collecting instantiations do the same arithmetic as the plain ones (the contract tests/test_*_elbo_parts_gpu.py state at checkelbo = 1): the
    state after 12 iterations is bit-identical whichever of them were checked, and a checked iteration's ELBO does not depend on what came before it
    beyond the form of the evaluation (the first check of a call is the one evaluated both ways)."""
    fam = CASES[name][0]
    runs = device_runs(tmvb, name)
    ref = runs[1]
    for c in CADENCES:
        for n in STATE[fam]:
            assert np.array_equal(runs[c]["state"][n], ref["state"][n]), (name, c, n, float(np.max(np.abs(runs[c]["state"][n] - ref["state"][n]))))
        t = runs[c]["traj"]
        assert len(t) == ITER
        m = np.isfinite(t)
        if m.any():
            within(fam + ".elbo_forms_rel", _rel(t[m], ref["traj"][m]), (name, c, t, ref["traj"]))


# --------------------------------------------------------------------------------------------------------- B
@gpu
@pytest.mark.parametrize("name", ALL)
def test_b_bookkeeping_and_values_against_the_oracle(tmvb, oracle, name):
    fam = CASES[name][0]
    o = oracle_run(tmvb, oracle, name)
    runs = device_runs(tmvb, name)
    for c in CADENCES:
        r = runs[c]
        t, m = r["traj"], checked(c)
        assert len(t) == ITER, (name, c, len(t))
        assert np.array_equal(np.isfinite(t), m) and np.array_equal(np.isnan(t), ~m), (name, c, t)           # the oracle's pattern: its trajectory masked
        if m.any():
            within(fam + ".elbo_rel_free", _rel(t[m], o["traj"][m]), (name, c, t, o["traj"]))
            within(fam + ".elbo_rel_step", abs(r["base"] - o["base"]) / abs(o["base"]), (name, c, "baseline", r["base"], o["base"]))
            assert r["elbo"] == t[m][-1], (name, c, r["elbo"], t)                 # the host's elbo field: the last checked value
        else:
            # checkelbo > iter: no baseline either (src/LDA.jl:167), the field keeps the value from before the call
            assert r["elbo"] == r["elbo_before"] == 0.0, (name, c, r["elbo"], r["elbo_before"])
            assert r["base"] == r["elbo_before"], (name, c, r["base"])
        if m[-1]:
            assert r["form"] == 1, (name, c, "the last iteration was checked: its evaluation took the decomposed form")
    inf = runs[math.inf]
    assert inf["form_walk"] == 0                                                  # nothing collected: update_elbo! walks the tokens
    within(fam + ".elbo_rel_free", abs(inf["elbo_walk"] - o["traj"][-1]) / abs(o["traj"][-1]), (name, "update_elbo after checkelbo = Inf"))


# --------------------------------------------------------------------------------------------------------- C
def stop_plan(o, fam, c):
    """(s, tol, margin, bound) from the ORACLE's checked increments d_1 .. d_n at cadence c (d_1 against the baseline): a stop index 1 < s < n with
    d_s < min(d_1 .. d_{s-1}), tol half way between the two; of the indices whose d_i, i <= s, all keep the margin `bound` from tol, the latest."""
    e = np.concatenate([[o["base"]], o["traj"][checked(c)]])
    d = np.diff(e)
    n = len(d)
    bound = 100.0 * TOL[fam + ".elbo_rel_free"] * o["emax"]
    best = None
    for s in range(2, n):                                   # 1-based stop index, 1 < s < n
        lo, hi = d[s - 1], d[:s - 1].min()
        if lo < hi:
            tol = 0.5 * (lo + hi)
            margin = float(np.min(np.abs(d[:s] - tol)))
            if best is None or margin >= bound:             # the LATEST stop index that keeps the margin (the first admissible one if none does)
                best = (s, tol, margin)
    assert best is not None, ("no admissible stop index", d)
    return best + (bound,)


@gpu
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("name", SYNTHETIC)
def test_c_stop_rule_stops_at_the_known_iteration(tmvb, oracle, name, c):
    """delta < tol, signed (quirk Q4, src/modelutils.jl:574-585).  tol sits between the oracle's increment at the stop index and the smallest one before
    it, every increment at least 100 x the free-running ELBO tolerance away from it (a CONDITION on the oracle, asserted): the device cannot
    legitimately decide otherwise, so it must stop at iteration s * c exactly, as the oracle does by construction of tol."""
    g = data(tmvb, name)
    fam = g["family"]
    o = oracle_run(tmvb, oracle, name)
    s, tol, margin, bound = stop_plan(o, fam, c)
    # (CTPF at c = 1: only s = 2 keeps the margin -- its key is 1e-4 -- so that case covers only the first decomposed-against-decomposed delta, the check
    #  right behind the switch of forms; c = 3 stops it at its third check)
    assert tol > 0 and margin >= bound, (name, c, s, tol, margin, bound)
    gm = make_device(tmvb, g)
    t = device_train(gm, fam, iter=ITER, tol=tol, checkelbo=c)
    gm.close()
    print(f"{name} c={c}: stop index {s}, tol {tol:.6g}, margin {margin:.4g} >= {bound:.4g}, device stopped at {len(t)}")
    assert len(t) == s * c, (name, c, "stopped at", len(t), "expected", s * c, t)
    assert np.array_equal(np.isfinite(t), checked(c, s * c))


@gpu
@pytest.mark.parametrize("c", [1, 5])
@pytest.mark.parametrize("name", ALL)
def test_c_huge_tol_stops_at_the_first_check(tmvb, name, c):
    g = data(tmvb, name)
    gm = make_device(tmvb, g)
    t = device_train(gm, g["family"], iter=ITER, tol=1e30, checkelbo=c)
    assert len(t) == c and np.array_equal(np.isfinite(t), checked(c, c)), (name, c, t)
    assert gm.elbo == t[-1]
    gm.close()


# --------------------------------------------------------------------------------------------------------- D
@gpu
@pytest.mark.parametrize("name", ALL)
def test_d1_second_train_through_the_c_abi_without_set_state(tmvb, oracle, name):
    """tmvb_<model>_train (4, ce = 2), then (8, ce = 4) on the same handle, nothing in between: the handle still holds iteration 4's parts, marked valid.
    The second call's baseline must nevertheless be the token walk (tmvb_train.h: force_walk around the baseline, `old_parts` starts false).  What
    elbo_form read between the baseline and the first iteration is not visible through the ABI (iteration 8, the last, is checked, so it reads 1 when
    the call returns), so the form is pinned through the VALUE: a twin handle runs the same four iterations unchecked (the same state bit for bit,
    scenario A), its state goes through update_host -> update_buffer (fp32 through fp64: exact; set_state drops every part, and with it LDA's
    sum S log beta left by update_beta!, which the walk would otherwise read instead of recomputing it -- the baseline of the main handle recomputes it
    too, because there update_beta! left the difference form), and update_elbo! then walks the tokens (elbo_form 0).  The baseline must equal that
    value EXACTLY, and differ from the first call's last entry, the decomposed evaluation of the same state: without force_walk the baseline would
    re-evaluate the decomposed form from the same buffers and return that entry bit for bit.  (On MI355X the two differ by 6e-9 .. 1.1e-7 relative in
    all eight cases.)  And the twelve iterations are the twelve iterations of one call: the state is bit-identical to train(12, ce = 0)."""
    g = data(tmvb, name)
    fam = g["family"]
    o = oracle_run(tmvb, oracle, name)
    one = device_runs(tmvb, name)[math.inf]["state"]
    gm = make_device(tmvb, g)
    t1, b1 = abi_train(tmvb, gm, fam, 4, 2)
    assert gm.elbo_form() == 1
    t2, b2 = abi_train(tmvb, gm, fam, 8, 4)
    assert gm.elbo_form() == 1
    gm.update_host()
    two = state_of(gm, fam)
    gm.close()
    twin = make_device(tmvb, g)
    abi_train(tmvb, twin, fam, 4, 0)
    twin.update_host(); twin.update_buffer()
    walk = twin.update_elbo()
    assert twin.elbo_form() == 0
    twin.close()
    print(f"{name}: second baseline {b2!r}, token walk of the twin {walk!r}, first call's last entry (decomposed) {t1[3]!r}")
    assert b2 == walk, (name, "the second call's baseline is not the token walk of the state the first call left", b2, walk, t1[3])
    assert b2 != t1[3], (name, "walk and decomposed form coincide bit for bit here: the comparison above cannot tell them apart", b2)
    assert len(t1) == 4 and len(t2) == 8
    assert np.array_equal(np.isfinite(t1), checked(2, 4)) and np.array_equal(np.isfinite(t2), checked(4, 8))
    for n in STATE[fam]:
        assert np.array_equal(two[n], one[n]), (name, n, float(np.max(np.abs(two[n] - one[n]))))
    within(fam + ".elbo_rel_step", abs(b1 - o["base"]) / abs(o["base"]), (name, "first baseline"))
    within(fam + ".elbo_forms_rel", abs(b2 - t1[3]) / abs(t1[3]), (name, "second baseline against the first call's last entry", b2, t1[3]))
    got = np.array([t1[1], t1[3], t2[3], t2[7]]); want = o["traj"][[1, 3, 7, 11]]
    within(fam + ".elbo_rel_free", _rel(got, want), (name, got, want))


@gpu
@pytest.mark.parametrize("name", ALL)
def test_d2_second_train_through_the_host(tmvb, oracle, name):
    """train(4, checkelbo = 2) then train(8, checkelbo = 4) by the Python method: update_host -> update_buffer between them (the fp32 state passes through
    fp64 host arrays: exact), the same two calls on ONE oracle object.  CTM K = 64 takes the oracle's single cached run masked to the checked iterations
    instead of a second nine-second run: tests/test_oracle_cadence.py proves the two bit-equal for every family.
    Bit identity with the one-shot run is not required (CTPF recomputes log(rate) on the host side of set_state: 1 ulp, tests/test_comm_gpu.py).
    Whether the state after the two calls happens to be bit-identical to one call of 12 is printed, not asserted; on MI355X it was, in all eight
    cases (CTPF included: its rates pass through the host as fp64 images of fp32 values, and log() of them landed on the same fp32 here)."""
    g = data(tmvb, name)
    fam = g["family"]
    if name == "ctm_k64":
        o = oracle_run(tmvb, oracle, name)
        o1 = np.where(checked(2, 4), o["traj"][:4], np.nan); o2 = np.where(checked(4, 8), o["traj"][4:], np.nan)
    else:
        om = make_oracle(oracle, g)
        o1 = oracle_train(om, iter=4, tol=0.0, checkelbo=2); o2 = oracle_train(om, iter=8, tol=0.0, checkelbo=4)
    gm = make_device(tmvb, g)
    t1 = device_train(gm, fam, iter=4, tol=0.0, checkelbo=2)
    t2 = device_train(gm, fam, iter=8, tol=0.0, checkelbo=4)
    b2 = gm.elbo_baseline
    two = state_of(gm, fam)
    gm.close()
    for t, ot in ((t1, o1), (t2, o2)):
        assert len(t) == len(ot) and np.array_equal(np.isfinite(t), np.isfinite(ot)), (name, t, ot)
        m = np.isfinite(ot)
        within(fam + ".elbo_rel_free", _rel(t[m], ot[m]), (name, t, ot))
    within(fam + ".elbo_forms_rel", abs(b2 - t1[3]) / abs(t1[3]), (name, "second baseline against the first call's last entry", b2, t1[3]))
    one = device_runs(tmvb, name)[math.inf]["state"]
    same = all(np.array_equal(two[n], one[n]) for n in STATE[fam])
    print(f"{name}: two host-level calls bit-identical to one call of 12: {same}")


# --------------------------------------------------------------------------------------------------------- E
@gpu
@pytest.mark.parametrize("name", ALL)
def test_e_stepwise_iteration_behind_a_collecting_train(tmvb, oracle, name):
    """train(iter = 2, checkelbo = 1) leaves iteration 2's parts behind, marked valid.  One stepwise iteration (no update_buffer in front) does not
    collect under the default *_ELBO_PARTS setting, so its E-step must invalidate them: update_elbo! then walks the tokens of the NEW state.  Evaluated
    from the stale parts it mixes two iterations -- off by at least a whole increment, where rounding is 1e-6 (the negative control mut_lda_stale_parts
    of tests/test_mutants_gpu.py does exactly that: -853280 for -402505 on lda_k20, MI355X)."""
    g = data(tmvb, name)
    fam = g["family"]
    o = oracle_run(tmvb, oracle, name)
    gm = make_device(tmvb, g)
    device_train(gm, fam, iter=2, tol=0.0, checkelbo=1)
    assert gm.elbo_form() == 1
    stepwise_iteration(gm, fam)
    e = gm.update_elbo()
    form = gm.elbo_form()
    gm.close()
    print(f"{name}: stepwise third iteration {e!r}, oracle {o['traj'][2]!r}, oracle's second {o['traj'][1]!r}")
    within(fam + ".elbo_rel_step", abs(e - o["traj"][2]) / abs(o["traj"][2]), (name, e, o["traj"][2], "oracle's previous iteration", o["traj"][1]))
    assert form == 0, (name, "a stepwise E-step does not collect and must invalidate the previous iteration's parts")
