"""
Host-side mirror of the reference's fLDA interface above the C ABI (filtered LDA, src/fLDA.jl).

    fLDA(corp, K)                      src/fLDA.jl:6-60     host fp64 state
    gpufLDA(corp, K)                   NEW: the reference has no device model for the filtered models (`@gpu train!` on an
                                       fLDA is a no-op, src/macros.jl:274-278); this one follows the gpuLDA pattern
      .update_buffer() / .update_host()
      .estep(viter, vtol)              update_phi!/update_tau!/update_gamma!/update_Elogtheta! sweeps + update_beta!(d) +
                                       update_kappa!(d), src/fLDA.jl:222-236
      .update_beta() .update_alpha() .update_eta() .update_elbo()      :152/:138, :128, :122, :108
      .train(iter=150, tol=1.0, niter=1000, ntol=1/K^2, viter=10, vtol=1/K^2, checkelbo=1, printelbo=True)   :213-247
    gpu_train_flda(model, **kwargs)    `@gpu train!(model::fLDA; kwargs...)`

tau / tau_old are flat [nnz] arrays in CSR token order (the reference's tau[d][n]).  No CPU fallback.
"""
from __future__ import annotations

import functools

import numpy as np

from ._lib import CorpusError, TopicModelError
from ._model import DeviceContext, DeviceModel, EstepTimer, _op
from .corpus import dirichlet_rows
from .lda import LDA, _packed, check_model


class fLDA(LDA):
    """Host (fp64) fLDA state with the reference's field names, src/fLDA.jl:6-60."""

    def __init__(self, corp, K: int, seed: int = 7):
        super().__init__(corp, K, seed)
        self.eta = 0.5                                                              # :38
        self.kappa = dirichlet_rows(1, self.V, seed + 1)[0].copy() if self.V else np.zeros(0)   # :40 (Julia RNG in the reference)
        self.kappa_old = self.kappa.copy()
        self.kappa_temp = np.zeros(self.V)
        self.tau = np.full(self.corp.nnz, self.eta)                                 # :49
        self.tau_old = self.tau.copy()


def check_model_flda(model, rtol: float = 1.5e-8):
    """check_model(::fLDA)  src/modelutils.jl:69-107 (array form)."""
    check_model(model, rtol=rtol)
    if not (0.0 <= model.eta <= 1.0):
        raise TopicModelError("eta must belong to the interval [0,1].")
    for name in ("kappa", "kappa_old"):
        k = getattr(model, name)
        if k.shape != (model.V,):
            raise TopicModelError(f"{name} must be of length V.")
        if model.V and not (np.all(k >= 0) and np.isclose(k.sum(), 1.0, rtol=rtol, atol=0)):
            raise TopicModelError(f"{name} must be a probability vector.")
    if model.tau.shape != (model.corp.nnz,):
        raise TopicModelError("tau must contain vectors of lengths N.")
    if not np.all((model.tau >= 0) & (model.tau <= 1)):
        raise TopicModelError("tau must belong to the interval [0,1].")


class gpufLDA(EstepTimer, DeviceModel):
    """Device-backed filtered LDA model on libtmvb_hip.so."""

    _ABI, _HOST, _check = "flda", fLDA, staticmethod(functools.partial(check_model_flda, rtol=3.5e-4))
    _STATE = (("eta", ""), ("alpha", "K"), ("kappa", "V"), ("kappa_old", "V"), ("beta", "KV"), ("beta_old", "KV"), ("gamma", "KM"),
              ("Elogtheta", "KM"), ("Elogtheta_old", "KM"), ("tau", "N"), ("tau_old", "N"))

    def __init__(self, corp, K: int, seed: int = 7, ctx: DeviceContext | None = None, device_id: int = 0, _from: fLDA | None = None):
        if not (isinstance(K, (int, np.integer)) and K > 0):
            raise ValueError("number of topics must be a positive integer.")
        super().__init__(corp, K, seed, ctx, device_id, _from=_from)

    def estep(self, viter: int = 10, vtol: float | None = None):
        self._call("estep", viter, self._default_tol(vtol))

    reduce_docs, update_eta = _op("reduce_docs"), _op("update_eta")
    update_beta = _op("update_beta")                    # beta and kappa (src/fLDA.jl:237-238)

    def update_alpha(self, niter: int = 1000, ntol: float | None = None):
        self._call("update_alpha", niter, self._default_tol(ntol))

    def mstep(self, niter: int = 1000, ntol: float | None = None):
        self.update_beta(); self.update_alpha(niter, ntol); self.update_eta()

    def set_comm(self, comm, M_total: int, C_total: int):
        self._set_comm(comm, M_total, C_total)

    def train(self, iter: int = 150, tol: float = 1.0, niter: int = 1000, ntol: float | None = None, viter: int = 10,
              vtol: float | None = None, checkelbo=1, printelbo: bool = True):
        """train!(model::fLDA; ...) src/fLDA.jl:213-247 on the device.  Returns the ELBO trajectory."""
        return self._train(iter, tol, (niter, self._default_tol(ntol), viter, self._default_tol(vtol)), checkelbo, printelbo)


def gpu_train_flda(model: fLDA, device_id: int = 0, **kwargs):
    """`@gpu train!(model::fLDA; kwargs...)`: in the reference this branch does nothing (src/macros.jl:274-275); here the
    model trains on the device and comes back like the LDA branch does (beta / kappa re-normalised in fp64, *_old synced)."""
    if not isinstance(model, fLDA):
        raise ValueError("gpu_train_flda needs an fLDA model.")
    g = gpufLDA(model.corp, model.K, device_id=device_id, _from=model)
    traj = g.train(**kwargs)
    for n in ("topics", "eta", "alpha", "gamma", "Elogtheta", "tau", "elbo"):
        setattr(model, n, getattr(g, n))
    model.beta = g.beta / g.beta.sum(axis=1, keepdims=True); model.beta_old = model.beta.copy(order="F")
    model.kappa = g.kappa / g.kappa.sum(); model.kappa_old = model.kappa.copy()
    model.Elogtheta_old = model.Elogtheta.copy(order="F"); model.tau_old = model.tau.copy()
    g.close()
    return traj


def predict_flda(corp, train_model, iter: int = 10, tol: float | None = None, device_id: int = 0, seed: int = 7) -> fLDA:
    """predict(corp, train_model::fLDA; iter=10, tol=1/K^2)  src/modelutils.jl:858-883 on the device: one pass of the fused
    filtered E-step (phi, tau, gamma, Elogtheta sweeps), no M-step.  As in the reference only alpha, beta and topics come
    from the trained model (:866-868): kappa and eta are those of the fresh fLDA(corp, K) (`seed` stands in for Julia's
    RNG).  The reference's loop tests `vtol`, a name that function never defines (:877); `tol` is used here."""
    K = train_model.K
    tol = 1.0 / K ** 2 if tol is None else tol
    pc = _packed(corp)
    if pc.V != train_model.V:
        raise CorpusError("predict corpus and train_model corpus must have identical vocabularies.")
    if tol < 0:
        raise ValueError("tolerance parameter must be nonnegative.")
    if iter < 0:
        raise ValueError("iteration parameter must be nonnegative.")
    host = fLDA(pc, K, seed)
    host.alpha = np.array(train_model.alpha, dtype=np.float64)
    host.beta = np.asfortranarray(train_model.beta); host.beta_old = host.beta.copy(order="F")
    host.topics = train_model.topics
    g = gpufLDA(None, K, device_id=device_id, _from=host)
    g.estep(iter, tol)
    g.update_host()
    for n in ("gamma", "Elogtheta", "Elogtheta_old", "tau", "tau_old"):
        setattr(host, n, getattr(g, n))
    g.close()
    return host
