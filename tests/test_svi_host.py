"""
Host side of stochastic LDA training (topicmodelsvb.jl_amd/lda_svi.py), no device: the step-size schedule svi_rho, the equal cuts svi_cuts, the visiting
order, every argument error of gpu_train_stochastic, and the exported names.  (That include/tmvb.h, the library and the Julia shim agree on the new entry
points is checked by tests/test_capi_loads.py and tests/test_julia_shim_static.py as they stand.)
"""
import numpy as np
import pytest


def test_rho_is_one_at_the_first_step_without_delay(tmvb):
    assert tmvb.svi_rho(1, 0.0, 0.7) == 1.0
    assert tmvb.svi_rho(1, 0.0, 1.0) == 1.0 and tmvb.svi_rho(1, 0.0, 0.51) == 1.0


@pytest.mark.parametrize("tau0,kappa", [(0.0, 0.51), (1.0, 0.7), (64.0, 1.0)])
def test_rho_is_strictly_decreasing(tmvb, tau0, kappa):
    r = np.array([tmvb.svi_rho(t, tau0, kappa) for t in range(1, 2000)])
    assert np.all(np.diff(r) < 0) and np.all(r > 0) and np.all(r <= 1)


def test_rho_is_the_fp64_power(tmvb):
    for t in range(1, 6):
        assert tmvb.svi_rho(t, 1.0, 0.7) == (1.0 + t) ** -0.7
    assert isinstance(tmvb.svi_rho(3), float) and tmvb.svi_rho(3) == 4.0 ** -0.7           # the defaults: tau0 = 1, kappa = 0.7


@pytest.mark.parametrize("M,batch,B", [(4096, 1024, 4), (1025, 1024, 2), (320, 4096, 1), (7, 1, 7), (10, 3, 4)])
def test_cuts_cover_the_corpus_without_overlap(tmvb, M, batch, B):
    cuts = tmvb.svi_cuts(M, batch)
    assert cuts.dtype == np.int64 and len(cuts) == B + 1 and cuts[0] == 0 and cuts[-1] == M
    n = np.diff(cuts)
    assert np.all(n >= 1) and np.all(n[:-1] == batch) and 1 <= n[-1] <= batch
    assert np.array_equal(np.concatenate([np.arange(cuts[b], cuts[b + 1]) for b in range(B)]), np.arange(M))


def test_order_is_the_identity_per_epoch_or_a_seeded_permutation(tmvb):
    assert np.array_equal(tmvb.svi_order(3, 2), [0, 1, 2, 0, 1, 2]) and len(tmvb.svi_order(3, 0)) == 0 and len(tmvb.svi_order(3, 0, 5)) == 0
    a, b = tmvb.svi_order(17, 3, shuffle_seed=4), tmvb.svi_order(17, 3, shuffle_seed=4)
    assert np.array_equal(a, b) and a.dtype == np.int32
    for e in range(3):
        assert np.array_equal(np.sort(a[17 * e:17 * (e + 1)]), np.arange(17))
    assert not np.array_equal(a[:17], np.arange(17)) and not np.array_equal(a, tmvb.svi_order(17, 3, shuffle_seed=5))


def _model(tmvb):
    doc_ptr, terms, counts = tmvb.synthetic_lda_corpus(12, 30, seed=3, Kstar=3, len_mu=2.5, len_min=3, len_max=20)
    return tmvb.LDA(tmvb.PackedCorpus(doc_ptr, terms, counts, 30), 3)


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
        tmvb.gpu_train_stochastic(_model(tmvb), **kw)
    assert str(e.value) == msg


def test_helpers_reject_what_the_driver_rejects(tmvb):
    for bad in (dict(kappa=0.5), dict(kappa=1.5), dict(tau0=-1.0)):
        with pytest.raises(ValueError):
            tmvb.svi_rho(1, **bad)
    for t in (0, -3, 1.5):
        with pytest.raises(ValueError):
            tmvb.svi_rho(t)
    for M, batch in ((0, 4), (10, 0), (10, -1), (10, 2.0)):
        with pytest.raises(ValueError):
            tmvb.svi_cuts(M, batch)
    with pytest.raises(ValueError) as e:
        tmvb.gpu_train_stochastic(object())
    assert "only applies to" in str(e.value)


def test_the_names_are_exported(tmvb):
    for n in ("gpuLDAStochastic", "gpu_train_stochastic", "svi_rho", "svi_cuts", "svi_order"):
        assert n in tmvb.__all__ and callable(getattr(tmvb, n))
    for m in ("set_schedule", "run", "final_pass", "update_host", "update_buffer", "info", "close", "doc_sweeps", "last_run_ms"):
        assert callable(getattr(tmvb.gpuLDAStochastic, m))
    assert "tmvb_lda_svi.hip" in tmvb._lib.SOURCES
