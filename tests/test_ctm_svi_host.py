"""
Host side of stochastic CTM training (topicmodelsvb.jl_amd/ctm_svi.py, tests/ctm_svi_restatement.py), no device: every argument error of
gpu_train_ctm_stochastic (messages and types of the LDA stochastic path), the tmvb_ctm_svi_* names in include/tmvb.h and in the built library, and the
restatement itself -- its recentred scatter matrix against the directly summed weighted scatter, and its step at B = 1, tau0 = 0 against one oracle
iteration on the golden corpus.
"""
import os
import re

import numpy as np
import pytest

import ctm_svi_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("create", "destroy", "set_state", "get_state", "set_schedule", "run", "final_pass", "info", "doc_sweeps", "last_run_ms")


def _model(tmvb):
    doc_ptr, terms, counts = tmvb.synthetic_lda_corpus(12, 30, seed=3, Kstar=3, len_mu=2.5, len_min=3, len_max=20)
    return tmvb.CTM(tmvb.PackedCorpus(doc_ptr, terms, counts, 30), 3)


@pytest.mark.parametrize("kw,msg", [
    (dict(kappa=0.5), "kappa parameter must be in (0.5, 1]."), (dict(kappa=0.2), "kappa parameter must be in (0.5, 1]."),
    (dict(kappa=1.01), "kappa parameter must be in (0.5, 1]."), (dict(kappa=float("nan")), "kappa parameter must be in (0.5, 1]."),
    (dict(tau0=-1e-9), "tau0 parameter must be nonnegative."), (dict(tau0=float("inf")), "tau0 parameter must be nonnegative."),
    (dict(batch=0), "batch parameter must be a positive integer."), (dict(batch=-4), "batch parameter must be a positive integer."),
    (dict(batch=2.5), "batch parameter must be a positive integer."),
    (dict(epochs=-1), "epochs parameter must be a nonnegative integer."), (dict(epochs=1.5), "epochs parameter must be a nonnegative integer."),
    (dict(vtol=-1.0), "tolerance parameters must be nonnegative."), (dict(ntol=-1.0), "tolerance parameters must be nonnegative."),
    (dict(viter=-1), "iteration parameters must be nonnegative."), (dict(niter=-1), "iteration parameters must be nonnegative."),
])
def test_every_rejected_argument_raises_before_the_device(tmvb, kw, msg):
    with pytest.raises(ValueError) as e:
        tmvb.gpu_train_ctm_stochastic(_model(tmvb), **kw)
    assert str(e.value) == msg


def test_a_model_of_another_kind_is_rejected(tmvb):
    with pytest.raises(ValueError) as e:
        tmvb.gpu_train_ctm_stochastic(object())
    assert "only applies to" in str(e.value)
    doc_ptr, terms, counts = tmvb.synthetic_lda_corpus(12, 30, seed=3, Kstar=3, len_mu=2.5, len_min=3, len_max=20)
    with pytest.raises(ValueError):
        tmvb.gpu_train_ctm_stochastic(tmvb.LDA(tmvb.PackedCorpus(doc_ptr, terms, counts, 30), 3))


def test_the_names_are_exported(tmvb):
    for n in ("gpuCTMStochastic", "gpu_train_ctm_stochastic"):
        assert n in tmvb.__all__ and callable(getattr(tmvb, n))
    for m in ("set_schedule", "run", "final_pass", "update_host", "update_buffer", "info", "close", "doc_sweeps", "last_run_ms"):
        assert callable(getattr(tmvb.gpuCTMStochastic, m))
    assert "tmvb_ctm_svi.hip" in tmvb._lib.SOURCES


def test_every_entry_point_is_in_the_header_and_in_the_library(tmvb):
    header = open(os.path.join(ROOT, "include", "tmvb.h")).read()
    declared = set(re.findall(r"\bint (tmvb_ctm_svi_\w+)\(", header))
    assert declared == {"tmvb_ctm_svi_" + n for n in NAMES}
    exported = set(tmvb.exported_symbols())
    assert declared <= exported, declared - exported
    assert not [s for s in exported if re.match(r"tmvb_ctm_(share_globals|globals_view_of|set_cur|sigma_mu_from_tail)$", s)]     # the hooks stay internal


@pytest.mark.parametrize("K,n,seed", [(3, 17, 0), (8, 200, 1), (20, 50, 2)])
def test_the_recentred_scatter_is_the_weighted_scatter_about_mu(K, n, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(K, n)) * rng.uniform(0.5, 3.0, size=(K, 1)) + rng.normal(size=(K, 1))
    w = rng.uniform(0.1, 2.0, size=n)
    M = w.sum()
    mref, mu = rng.normal(size=K), rng.normal(size=K) + 1.0
    scatter = lambda m: ((x - m[:, None]) * w) @ (x - m[:, None]).T
    lbar = (x * w).sum(axis=1)
    got, want = R.recentre(scatter(mref), lbar, mref, mu, M), scatter(mu)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    assert np.array_equal(R.recentre(scatter(mref), lbar, mref, mref, M), scatter(mref))           # no move: nothing is added


def test_coefficients_are_rounded_once():
    rho, c0, c1 = R.coefficients(3, 1.0, 0.7, 320, 64)
    assert rho == 4.0 ** -0.7 and c0 == float(np.float32(1.0 - rho)) and c1 == float(np.float32(rho * 320 / 64))
    assert R.coefficients(1, 0.0, 0.7, 40, 40) == (1.0, 0.0, 1.0)


def test_one_batch_without_delay_is_one_oracle_iteration(oracle):
    z = np.load(os.path.join(ROOT, "tests", "golden", "ctm_m40_v60_k5.npz"))
    K, V = int(z["K"]), int(z["V"])
    mk = lambda: oracle.CTM(oracle.CSR(z["doc_ptr"], z["terms"], z["counts"], V), K, z["beta0"])
    r = R.Restatement(oracle, z["doc_ptr"], z["terms"], z["counts"], V, K, [0, 40], z["beta0"], 0.0, 0.7)
    om = mk()
    close = lambda a, b: np.abs(a - b).max() <= 1e-12 * np.abs(b).max()
    for it in range(3):                                  # the later steps start from a moved mu: the recentring takes part
        r.t = 0                                          # rho = 1 again
        sw, rho, c0, c1 = r.step(0, 10, 1.0 / K ** 2)
        assert (rho, c0, c1) == (1.0, 0.0, 1.0)
        sw_o = om.estep(); om.update_beta(); om.update_sigma_mu()
        assert np.array_equal(sw, sw_o)
        for n in ("lam", "vsq", "logzeta", "beta", "beta_old", "mu", "sigma", "invsigma"):
            assert close(getattr(r.om, n), getattr(om, n)), (it, n)
