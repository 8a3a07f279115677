"""
Host-side mirror of the reference's fCTM interface above the C ABI (filtered CTM, src/fCTM.jl).

    fCTM(corp, K)                      src/fCTM.jl:6-65     host fp64 state
    gpufCTM(corp, K)                   NEW: the reference has no device model for the filtered models (`@gpu train!` on an
                                       fCTM is a no-op, src/macros.jl:274-278); this one follows the gpuCTM pattern
      .update_buffer() / .update_host()
      .estep(niter, ntol, viter, vtol) update_phi!/update_tau!/update_logzeta!/update_lambda!/update_vsq! sweeps +
                                       update_beta!(d) + update_kappa!(d), src/fCTM.jl:233-248
      .update_beta() .update_sigma() .update_mu() .update_elbo()       :148/:134, :128, :122, :105
      .train(iter=150, tol=1.0, niter=1000, ntol=1/K^2, viter=10, vtol=1/K^2, checkelbo=1, printelbo=True)   :226-262
    gpu_train_fctm(model, **kwargs)    `@gpu train!(model::fCTM; kwargs...)`

tau / tau_old are flat [nnz] arrays in CSR token order (the reference's tau[d][n]).  eta is a fixed parameter: update_eta!
is commented out of the reference's train! (src/fCTM.jl:253).  No CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from ._lib import CorpusError, TopicModelError, P_i64
from ._model import DeviceContext, DeviceModel, _op
from .corpus import dirichlet_rows
from .ctm import CTM, check_model_ctm
from .lda import _packed


class fCTM(CTM):
    """Host (fp64) fCTM state with the reference's field names, src/fCTM.jl:6-65."""

    def __init__(self, corp, K: int, seed: int = 7):
        super().__init__(corp, K, seed)
        self.eta = 0.5                                                              # :37
        self.kappa = dirichlet_rows(1, self.V, seed + 1)[0].copy() if self.V else np.zeros(0)   # :44 (Julia RNG in the reference)
        self.kappa_old = self.kappa.copy()
        self.kappa_temp = np.zeros(self.V)
        self.tau = np.full(self.corp.nnz, self.eta)                                 # :54
        self.tau_old = self.tau.copy()


def check_model_fctm(model, rtol: float = 1.5e-8):
    """check_model(::fCTM)  src/modelutils.jl:139-178 (array form)."""
    check_model_ctm(model, rtol=rtol)
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


class gpufCTM(DeviceModel):
    """Device-backed filtered CTM model on libtmvb_hip.so."""

    _ABI, _HOST, _check = "fctm", fCTM, staticmethod(functools.partial(check_model_fctm, rtol=3.5e-4))
    _STATE = (("eta", ""), ("mu", "K"), ("sigma", "KK"), ("invsigma", "KK"), ("kappa", "V"), ("kappa_old", "V"), ("beta", "KV"),
              ("beta_old", "KV"), ("lam", "KM"), ("lam_old", "KM"), ("vsq", "KM"), ("logzeta", "M"), ("tau", "N"), ("tau_old", "N"))

    def __init__(self, corp, K: int, seed: int = 7, ctx: DeviceContext | None = None, device_id: int = 0, _from: fCTM | None = None):
        if not (isinstance(K, (int, np.integer)) and K > 0):
            raise ValueError("number of topics must be a positive integer.")
        super().__init__(corp, K, seed, ctx, device_id, _from=_from)

    def estep(self, niter: int = 1000, ntol: float | None = None, viter: int = 10, vtol: float | None = None):
        self._call("estep", niter, self._default_tol(ntol), viter, self._default_tol(vtol))

    reduce_docs, update_sigma, update_mu = _op("reduce_docs"), _op("update_sigma"), _op("update_mu")
    update_beta = _op("update_beta")                    # beta and kappa (src/fCTM.jl:249-250)

    def mstep(self):
        self.update_beta(); self.update_sigma(); self.update_mu()

    def sweep_hist(self, nbins: int = 11):
        h = np.zeros(nbins, dtype=np.int64)
        ns = C.c_int64(0)
        self._call("sweep_hist", h.ctypes.data_as(P_i64), nbins, C.byref(ns))
        return h, ns.value

    def set_comm(self, comm, M_total: int):
        self.M_total = int(M_total) if comm is not None else self.M
        self._set_comm(comm, self.M_total)

    def train(self, iter: int = 150, tol: float = 1.0, niter: int = 1000, ntol: float | None = None, viter: int = 10,
              vtol: float | None = None, checkelbo=1, printelbo: bool = True):
        """train!(model::fCTM; ...) src/fCTM.jl:226-262 on the device.  Returns the ELBO trajectory."""
        return self._train(iter, tol, (niter, self._default_tol(ntol), viter, self._default_tol(vtol)), checkelbo, printelbo)


def gpu_train_fctm(model: fCTM, device_id: int = 0, **kwargs):
    """`@gpu train!(model::fCTM; kwargs...)`: a no-op in the reference (src/macros.jl:274-275); here the model trains on the
    device and comes back like the CTM branch does (beta / kappa re-normalised in fp64, *_old synced)."""
    if not isinstance(model, fCTM):
        raise ValueError("gpu_train_fctm needs an fCTM model.")
    g = gpufCTM(model.corp, model.K, device_id=device_id, _from=model)
    traj = g.train(**kwargs)
    for n in ("topics", "eta", "mu", "sigma", "invsigma", "lam", "vsq", "logzeta", "tau", "elbo"):
        setattr(model, n, getattr(g, n))
    model.beta = g.beta / g.beta.sum(axis=1, keepdims=True); model.beta_old = model.beta.copy(order="F")
    model.kappa = g.kappa / g.kappa.sum(); model.kappa_old = model.kappa.copy()
    model.lam_old = model.lam.copy(order="F"); model.tau_old = model.tau.copy()
    g.close()
    return traj


def predict_fctm(corp, train_model, iter: int = 10, tol: float | None = None, niter: int = 1000, ntol: float | None = None,
                 device_id: int = 0, seed: int = 7) -> fCTM:
    """predict(corp, train_model::fCTM; iter, tol, niter, ntol)  src/modelutils.jl:916-943 on the device: one pass of the
    fused filtered CTM E-step (phi, tau, logzeta, lambda, vsq sweeps) with mu / sigma / invsigma / beta frozen (:924-928);
    kappa and eta are those of the fresh fCTM(corp, K), as in the reference.  `tol` stands for the reference's undefined
    `vtol` (:937)."""
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
    host = fCTM(pc, K, seed)
    host.mu, host.sigma, host.invsigma = np.array(train_model.mu), np.asfortranarray(train_model.sigma), np.asfortranarray(train_model.invsigma)
    host.beta = np.asfortranarray(train_model.beta); host.beta_old = host.beta.copy(order="F")
    host.topics = train_model.topics
    g = gpufCTM(None, K, device_id=device_id, _from=host)
    g.estep(niter, ntol, iter, tol)
    g.update_host()
    for n in ("lam", "lam_old", "vsq", "logzeta", "tau", "tau_old"):
        setattr(host, n, getattr(g, n))
    g.close()
    return host
