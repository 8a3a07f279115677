"""
GPU parity tests for the filtered-CTM path (new device path; oracle src/fCTM.jl): HIP engine through the C ABI vs the fp64
oracle and the committed golden fixture.  Tolerances (fp64 -> fp32 state; fp64 Newton gradients on device): the fctm.* keys of tests/tol.py --
round 6: measured on MI355X and frozen at <= 10x (lambda in units of CTM's bound 1.5e-5 + 1.5e-5 |lambda|; round 5 they were literals up to 130x
looser); tests/test_mutants_gpu.py holds the negative control (update_vsq! in front of update_lambda!: CTM's order instead of src/fCTM.jl:239-240).
K <= 52 runs the lane-per-document kernel (FILT instantiation, CG Newton solves) and, for its documents of more than 2048 unique terms or under
TMVB_CTM_BATCH=0, the register Gauss-Jordan kernel (one wave per document); 52 < K <= 128 the generic kernel (one topic slot per lane up to
K = 64, two beyond: CG Newton solves against invsigma in LDS since round 3, K = 53 ... 60 included), K > 128 the same with four slots per lane
and invsigma read from global memory.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")

from tol import LAMBDA_ABS, LAMBDA_REL, within  # noqa: E402  (named tolerances of tests/tol.py, frozen at <= 10x their MI355X measurement)


def load(name):
    z = np.load(os.path.join(GOLD, name + ".npz"))
    return {k: z[k] for k in z.files}


def make_pair(tmvb, oracle, g):
    K, V = int(g["K"]), int(g["V"])
    gm = tmvb.gpufCTM(tmvb.PackedCorpus(g["doc_ptr"], g["terms"], g["counts"], V), K)
    gm.beta = np.asfortranarray(g["beta0"]); gm.beta_old = gm.beta.copy(order="F")
    gm.kappa = np.array(g["kappa0"], dtype=np.float64); gm.kappa_old = gm.kappa.copy()
    gm.update_buffer()
    om = oracle.fCTM(oracle.CSR(g["doc_ptr"], g["terms"], g["counts"], V), K, g["beta0"], g["kappa0"])
    return gm, om


def force(gm, om):
    for n in ("eta", "mu", "sigma", "invsigma", "kappa", "kappa_old", "beta", "beta_old", "lam", "lam_old", "vsq", "logzeta", "tau", "tau_old"):
        v = getattr(om, n)
        setattr(gm, n, np.array(v, copy=True, order="F") if isinstance(v, np.ndarray) else v)
    gm.update_buffer()


def step(m, **kw):
    m.estep(**kw)
    if hasattr(m, "reduce_docs"):
        m.reduce_docs()
    m.mstep()


def synth_case(tmvb, K, M=60, V=300, seed=3):
    pc = tmvb.syn_nsf(M=M, V=V, seed=seed)
    return dict(K=K, V=V, doc_ptr=pc.doc_ptr, terms=pc.terms, counts=pc.counts, beta0=tmvb.dirichlet_rows(K, V, seed=5),
                kappa0=tmvb.dirichlet_rows(1, V, seed=9)[0])


def compare(gm, om, it, tag=""):
    within("fctm.lambda_err" + tag, np.abs(gm.lam - om.lam) / (LAMBDA_ABS + LAMBDA_REL * np.abs(om.lam)), (it, "lambda", np.abs(gm.lam - om.lam).max()))
    within("fctm.vsq_rel" + tag, np.abs(gm.vsq - om.vsq) / om.vsq, (it, "vsq"))
    within("fctm.logzeta_abs" + tag, np.abs(gm.logzeta - om.logzeta).max(), (it, "logzeta"))
    within("fctm.tau_abs" + tag, np.abs(gm.tau - om.tau).max(initial=0.0), (it, "tau"))
    within("fctm.tau_abs" + tag, np.abs(gm.tau_old - om.tau_old).max(initial=0.0), (it, "tau_old"))
    big = om.beta > 1e-6
    within("fctm.beta_rel" + tag, (np.abs(gm.beta[big] - om.beta[big]) / om.beta[big]).max(), (it, "beta"))
    bk = om.kappa > 1e-8
    within("fctm.kappa_rel" + tag, (np.abs(gm.kappa[bk] - om.kappa[bk]) / om.kappa[bk]).max(), (it, "kappa"))
    within("fctm.mu_abs" + tag, np.abs(gm.mu - om.mu).max(), (it, "mu"))
    within("fctm.sigma_rel" + tag, np.abs(gm.sigma - om.sigma).max() / np.abs(om.sigma).max(), (it, "sigma"))
    np.testing.assert_allclose(gm.beta.sum(axis=1), 1.0, rtol=1e-5)
    np.testing.assert_allclose(gm.kappa.sum(), 1.0, rtol=1e-5)
    assert np.all(gm.vsq > 0) and np.all((gm.tau >= 0) & (gm.tau <= 1))
    np.linalg.cholesky(gm.sigma)


@pytest.mark.parametrize("case", ["golden_k4", "syn_k3", "syn_k12", "syn_k25", "syn_k41", "syn_k50", "syn_k57", "syn_k64", "syn_k100", "syn_k150", "syn_k256"])
def test_teacher_forced_step(tmvb, oracle, case):
    g = load("fctm_m30_v50_k4") if case == "golden_k4" else synth_case(tmvb, int(case.split("_k")[1]))
    gm, om = make_pair(tmvb, oracle, g)
    for it in range(3):
        force(gm, om)
        step(gm); sw_o = om.estep(); om.mstep()
        e_g = gm.update_elbo(); e_o = om.update_elbo()
        gm.update_host()
        same = gm.doc_sweeps() == np.asarray(sw_o)
        assert same.mean() >= 0.9, (it, same.mean())
        big = "" if int(case.split("_k")[1]) <= 128 else ".bigk"      # K > 128: invsigma read from global memory, eight topic slots per lane
        if same.all():
            compare(gm, om, it, big)
            within("fctm.elbo_rel_step" + big, abs(e_g - e_o) / abs(e_o), (case, it, e_g, e_o))
        else:                               # a document at the vtol boundary took one sweep more or less: compare the rest
            within("fctm.lambda_err" + big, np.abs(gm.lam[:, same] - om.lam[:, same]) / (LAMBDA_ABS + LAMBDA_REL * np.abs(om.lam[:, same])), (case, it))
            assert abs(e_g - e_o) <= 2e-4 * abs(e_o), (it, e_g, e_o)      # (two ELBOs of states that differ by a sweep of one document: a sanity bound, not a parity tolerance; no flip occurs on MI355X today)


@pytest.mark.parametrize("K", [5, 30, 70])
def test_teacher_forced_fixed_sweeps(tmvb, oracle, K):
    """vtol = 0 pins every document to exactly `viter` sweeps on both sides."""
    g = synth_case(tmvb, K, M=40, V=200, seed=11)
    gm, om = make_pair(tmvb, oracle, g)
    for it in range(2):
        force(gm, om)
        step(gm, viter=3, vtol=0.0); step(om, viter=3, vtol=0.0)
        e_g = gm.update_elbo(); e_o = om.update_elbo()
        gm.update_host()
        assert np.all(gm.doc_sweeps() == 3)
        compare(gm, om, it)
        within("fctm.elbo_rel_step", abs(e_g - e_o) / abs(e_o), (K, it, e_g, e_o))


def test_free_running_train_vs_golden(tmvb):
    g = load("fctm_m30_v50_k4")
    K, V = int(g["K"]), int(g["V"])
    m = tmvb.fCTM(tmvb.PackedCorpus(g["doc_ptr"], g["terms"], g["counts"], V), K)
    m.beta = np.asfortranarray(g["beta0"]); m.beta_old = m.beta.copy(order="F")
    m.kappa = np.array(g["kappa0"], dtype=np.float64); m.kappa_old = m.kappa.copy()
    traj = tmvb.gpu_train_fctm(m, iter=int(g["iters"]), tol=0.0, checkelbo=1, printelbo=False)
    tmvb.check_model_fctm(m)
    gold = g["elbo_traj"]
    assert len(traj) == len(gold)
    within("fctm.elbo_rel_free", np.abs(traj - gold) / np.abs(gold), (traj, gold))
    assert m.eta == 0.5                                                     # update_eta! is not part of train! (src/fCTM.jl:253)
    within("fctm.mu_abs_free", np.abs(m.mu - g["mu"]).max())
    within("fctm.beta_abs_free", np.abs(m.beta - g["beta"]).max())
    within("fctm.kappa_abs_free", np.abs(m.kappa - g["kappa"]).max())
    within("fctm.tau_abs_free", np.abs(m.tau - g["tau"]).max())


def test_long_documents_stream_chunks(tmvb, oracle):
    """Documents longer than the LDS window stream their token rows in chunks (tau round-trips through memory)."""
    rng = np.random.default_rng(3)
    V, K, M = 3000, 20, 12
    docs = []
    for d in range(M):
        n = int(rng.integers(300, 900)) if d % 2 == 0 else int(rng.integers(5, 60))
        t = np.sort(rng.choice(V, size=n, replace=False)); c = rng.integers(1, 4, size=n)
        docs.append((t, c))
    doc_ptr = np.concatenate([[0], np.cumsum([len(t) for t, _ in docs])]).astype(np.int64)
    terms = np.concatenate([t for t, _ in docs]).astype(np.int32); counts = np.concatenate([c for _, c in docs]).astype(np.int32)
    g = dict(K=K, V=V, doc_ptr=doc_ptr, terms=terms, counts=counts, beta0=tmvb.dirichlet_rows(K, V, seed=5), kappa0=tmvb.dirichlet_rows(1, V, seed=9)[0])
    gm, om = make_pair(tmvb, oracle, g)
    for it in range(2):
        force(gm, om)
        step(gm, viter=3, vtol=0.0); step(om, viter=3, vtol=0.0)
        gm.update_host()
        compare(gm, om, it)


@pytest.mark.parametrize("K", [4, 28, 44])
def test_wave_per_document_kernel_matches_lane_kernel(tmvb, monkeypatch, K):
    """fCTM's twin of test_lane_per_document_kernel_matches_wave_per_document_kernel (tests/test_ctm_gpu.py): TMVB_CTM_BATCH=0 sends every document
    to ctm_estep_kernel<KP, true> (direct Newton solves in registers), which otherwise only documents of more than 2048 unique terms reach; the
    default handle runs ctm_estep_batch_kernel<KP, false, true> (CG).  Same corpus (130 documents and an empty one: not a multiple of 64) and
    state in, two outer iterations, the wave handle's state carried into the lane handle between them.  Bounds: the CTM twin's literals and
    fctm.tau_abs.  Measured on MI355X before the launch layer was rewritten (profiles/ctm_launch_refactor_ab.json), worst of K = 4 / 28 / 44:
    lambda 2.7e-5, vsq 4.4e-6 of its max, mu 1.7e-6, sigma 1.2e-6 of its max, ELBO 5.3e-9 relative, tau 1.0e-6, no document's sweep count differs."""
    pc = tmvb.syn_nsf(M=130, V=300, seed=3)
    pc = tmvb.PackedCorpus(np.concatenate([pc.doc_ptr[:41], pc.doc_ptr[40:]]), pc.terms, pc.counts, pc.V)     # document 40: empty
    pair = []
    for flag in ("0", "1"):
        monkeypatch.setenv("TMVB_CTM_BATCH", flag)
        g = tmvb.gpufCTM(pc, K)
        g.beta = np.asfortranarray(tmvb.dirichlet_rows(K, pc.V, seed=5)); g.beta_old = g.beta.copy(order="F")
        g.kappa = np.array(tmvb.dirichlet_rows(1, pc.V, seed=9)[0], dtype=np.float64); g.kappa_old = g.kappa.copy()
        g.update_buffer()
        pair.append(g)
    gw, gb = pair
    for it in range(2):
        for g in (gw, gb):
            step(g)
        # (gpufCTM has no solver_stats of its own: gpuCTM's method, called on the fCTM handle, reaches tmvb_fctm_solver_stats through the handle's _ABI)
        solver_stats = tmvb.gpuCTM.solver_stats
        assert solver_stats(gw)["waves"] == 0 and solver_stats(gb)["waves"] == (pc.M + 63) // 64
        for g in (gw, gb):
            g.update_host()
        assert np.array_equal(gw.doc_sweeps() > 0, gb.doc_sweeps() > 0)
        assert (gw.doc_sweeps() != gb.doc_sweeps()).mean() <= 0.02
        assert np.abs(gw.lam - gb.lam).max() <= 1e-3, (it, np.abs(gw.lam - gb.lam).max())
        assert np.abs(gw.vsq - gb.vsq).max() <= 1e-3 * gw.vsq.max()
        assert np.abs(gw.mu - gb.mu).max() <= 1e-4 and np.abs(gw.sigma - gb.sigma).max() <= 1e-4 * np.abs(gw.sigma).max()
        ew, eb = gw.update_elbo(), gb.update_elbo()
        assert abs(ew - eb) <= 1e-6 * abs(ew), (it, ew, eb)
        within("fctm.tau_abs", np.abs(gw.tau - gb.tau).max(initial=0.0), (it, "tau"))
        # carry ONE state forward so that differences do not compound into different trajectories
        for n, _ in gw._STATE:
            v = getattr(gw, n); setattr(gb, n, np.array(v, copy=True, order="F") if isinstance(v, np.ndarray) else v)
        gb.update_buffer()


def test_errors_and_invariants(tmvb):
    pc = tmvb.syn_nsf(M=200, V=800, seed=2)
    with pytest.raises(ValueError):
        tmvb.gpufCTM(pc, 0)
    with pytest.raises(ValueError):
        tmvb.gpufCTM(pc, 257)
    gm = tmvb.gpufCTM(pc, 16)
    with pytest.raises(ValueError):
        gm.train(niter=-1, printelbo=False)
    gm.tau = np.full(pc.nnz, 1.5)
    with pytest.raises(tmvb.TopicModelError):
        gm.train(iter=1, printelbo=False)
    gm.tau = np.full(pc.nnz, 0.5)
    traj = gm.train(iter=4, tol=0.0, printelbo=False)
    assert len(traj) == 4 and np.all(np.isfinite(traj)) and np.all(np.diff(traj) > 0)
    assert np.isfinite(gm.elbo_baseline)
