"""
Host-side mirror of the reference's CTM / gpuCTM interface above the C ABI.

    CTM(corp, K)                      src/CTM.jl:6-53      host fp64 state
    gpuCTM(corp, K)                   src/gpuCTM.jl:6-99   device-backed model
      .update_buffer() / .update_host()      src/modelutils.jl:400-435 / :519-537
      .estep(niter, ntol, viter, vtol)       update_phi!/update_logzeta!/update_vsq!/update_lambda! sweeps +
                                             update_beta!(d), CPU-path semantics src/CTM.jl:194-205
      .update_beta() .update_sigma() .update_mu() .update_elbo()
      .train(iter=150, tol=1.0, niter=1000, ntol=1/K^2, viter=10, vtol=1/K^2, checkelbo=1, printelbo=True)
                                             src/gpuCTM.jl:487-519
    gpu_train_ctm(model, **kwargs)    `@gpu train!(model::CTM; kwargs...)`  src/macros.jl:152-195
"""
from __future__ import annotations

import ctypes as C
import functools
import math

import numpy as np

from ._lib import CorpusError, TopicModelError, P_i64
from ._model import DeviceModel, EstepTimer, PackedStats, _op
from .corpus import dirichlet_rows
from .lda import _packed


class CTM:
    """Host (fp64) CTM state with the reference's field names, src/CTM.jl:6-53."""

    def __init__(self, corp, K: int, seed: int = 7):
        if not (isinstance(K, (int, np.integer)) and K > 0):
            raise ValueError("number of topics must be a positive integer.")
        self.corp = _packed(corp)
        self.K, self.M, self.V = int(K), self.corp.M, self.corp.V
        self.N, self.C = self.corp.N, self.corp.C
        K, M, V = self.K, self.M, self.V
        self.topics = [np.arange(1, V + 1) for _ in range(K)]
        self.mu = np.zeros(K)
        self.sigma = np.asfortranarray(np.eye(K))
        self.invsigma = np.asfortranarray(np.eye(K))
        self.beta = dirichlet_rows(K, V, seed)
        self.beta_old = self.beta.copy(order="F")
        self.beta_temp = np.zeros((K, V), order="F")
        self.lam = np.zeros((K, M), order="F")               # `lambda` is a Python keyword
        self.lam_old = np.zeros((K, M), order="F")
        self.vsq = np.ones((K, M), order="F")
        self.logzeta = np.full(M, 0.5)
        self.elbo = 0.0


def check_model_ctm(model, rtol: float = 1.5e-8):
    """check_model(::CTM) src/modelutils.jl:108-138 (array form)."""
    K, M, V = model.K, model.M, model.V
    if not np.all(np.isfinite(model.mu)):
        raise TopicModelError("mu must be finite.")
    for name in ("sigma", "invsigma"):
        a = getattr(model, name)
        if a.shape != (K, K):
            raise TopicModelError(f"{name} must be of size (K, K).")
        try:
            np.linalg.cholesky(0.5 * (a + a.T))
        except np.linalg.LinAlgError:
            raise TopicModelError(f"{name} must be positive-definite.")
    if model.beta.shape != (K, V):
        raise TopicModelError("beta must be of size (K, V).")
    if V and not (np.all(model.beta >= 0) and np.allclose(model.beta.sum(axis=1), 1.0, rtol=rtol, atol=0)):
        raise TopicModelError("beta must be a right stochastic matrix.")
    if model.lam.shape != (K, M) or not np.all(np.isfinite(model.lam)):
        raise TopicModelError("lambda must be finite.")
    if model.vsq.shape != (K, M) or not np.all(np.isfinite(model.vsq)):
        raise TopicModelError("vsq must be finite.")
    if not np.all(model.vsq > 0):
        raise TopicModelError("vsq must be positive.")
    if model.logzeta.shape != (M,) or not np.all(np.isfinite(model.logzeta)):
        raise TopicModelError("logzeta must be finite.")
    if not math.isfinite(model.elbo):
        raise TopicModelError("elbo must be finite.")


class gpuCTM(PackedStats, EstepTimer, DeviceModel):
    """GPU accelerated correlated topic model (src/gpuCTM.jl:6-99) on libtmvb_hip.so."""

    _ABI, _HOST, _check = "ctm", CTM, staticmethod(functools.partial(check_model_ctm, rtol=3.5e-4))
    _STATE = (("mu", "K"), ("sigma", "KK"), ("invsigma", "KK"), ("beta", "KV"), ("beta_old", "KV"), ("lam", "KM"), ("lam_old", "KM"),
              ("vsq", "KM"), ("logzeta", "M"))

    def estep(self, niter: int = 1000, ntol: float | None = None, viter: int = 10, vtol: float | None = None):
        self._call("estep", niter, self._default_tol(ntol), viter, self._default_tol(vtol))

    reduce_docs, update_beta, update_sigma, update_mu = _op("reduce_docs"), _op("update_beta"), _op("update_sigma"), _op("update_mu")

    def set_distributed(self, M_total: int, distributed: bool = True):
        self.M_total = int(M_total)
        self._call("set_distributed", M_total, 1 if distributed else 0)

    def sweep_hist(self, nbins: int = 11):
        h = np.zeros(nbins, dtype=np.int64)
        ns = C.c_int64(0)
        self._call("sweep_hist", h.ctypes.data_as(P_i64), nbins, C.byref(ns))
        return h, ns.value

    def solver_stats(self):
        """Lane-per-document kernel diagnostics of the last E-step (tmvb_ctm_solver_stats)."""
        out = np.zeros(12, dtype=np.int64)
        self._call("solver_stats", out.ctypes.data_as(P_i64))
        names = ("cg_trips", "newton_trips", "waves", "cyc_token", "cyc_logzeta", "cyc_vsq", "cyc_gradient", "cyc_cg", "cyc_gradmv",
                 "cyc_update", "cyc_spare", "cyc_kernel")
        return dict(zip(names, out.tolist()))

    def set_comm(self, comm, M_total: int):
        """Attach a communicator (comm.py): document-sharded train!, every rank calls train() with the same arguments."""
        self.M_total = int(M_total) if comm is not None else self.M
        self._set_comm(comm, self.M_total)

    def train(self, iter: int = 150, tol: float = 1.0, niter: int = 1000, ntol: float | None = None, viter: int = 10,
              vtol: float | None = None, checkelbo=1, printelbo: bool = True):
        """train!(model::gpuCTM; ...) src/gpuCTM.jl:487-519."""
        return self._train(iter, tol, (niter, self._default_tol(ntol), viter, self._default_tol(vtol)), checkelbo, printelbo)


def gpu_train_ctm(model: CTM, device_id: int = 0, **kwargs):
    """`@gpu train!(model::CTM; kwargs...)` (src/macros.jl:152-195)."""
    g = gpuCTM(None, model.K, device_id=device_id, _from=model)
    traj = g.train(**kwargs)
    model.topics, model.mu, model.sigma, model.invsigma = g.topics, g.mu, g.sigma, g.invsigma
    model.beta = g.beta / g.beta.sum(axis=1, keepdims=True)         # src/macros.jl:190
    model.beta_old = model.beta.copy(order="F")
    model.lam = g.lam; model.lam_old = g.lam.copy(order="F")        # :183
    model.vsq, model.logzeta, model.elbo = g.vsq, g.logzeta, g.elbo
    g.close()
    return traj


def predict_ctm(corp, train_model, iter: int = 10, tol: float | None = None, niter: int = 1000, ntol: float | None = None,
                device_id: int = 0) -> CTM:
    """predict(corp, train_model::Union{CTM, gpuCTM}; iter, tol, niter, ntol)  src/modelutils.jl:886-913: one pass of the
    fused CTM E-step with the trained mu / sigma / beta frozen."""
    K = train_model.K
    tol = 1.0 / K ** 2 if tol is None else tol
    ntol = 1.0 / K ** 2 if ntol is None else ntol
    pc = _packed(corp)
    if pc.V != train_model.V:
        raise CorpusError("predict corpus and train_model corpus must have identical vocabularies.")
    if tol < 0 or ntol < 0:
        raise ValueError("tolerance parameters must be nonnegative.")
    if iter < 0 or niter < 0:
        raise ValueError("iteration parameters must be nonnegative.")
    host = CTM(pc, K)
    host.mu, host.sigma, host.invsigma = np.array(train_model.mu), np.asfortranarray(train_model.sigma), np.asfortranarray(train_model.invsigma)
    host.beta = np.asfortranarray(train_model.beta); host.beta_old = host.beta.copy(order="F")
    g = gpuCTM(None, K, device_id=device_id, _from=host)
    g.estep(niter, ntol, iter, tol)
    g.update_host()
    for n in ("lam", "lam_old", "vsq", "logzeta"):
        setattr(host, n, getattr(g, n))
    host.topics = train_model.topics
    g.close()
    return host


def topicdist_ctm(model, d):
    """topicdist(model::Union{CTM, gpuCTM}, d)  src/modelutils.jl:953-958: additive_logistic(lambda + vsq/2)."""
    if not isinstance(d, (int, np.integer)):
        return [topicdist_ctm(model, int(x)) for x in d]
    if not (1 <= d <= model.M):
        raise CorpusError("document index outside corpus range.")
    x = model.lam[:, d - 1] + 0.5 * model.vsq[:, d - 1]
    x = np.exp(x - x.max())
    return x / x.sum()
