"""
Host-side mirror of the reference's LDA / gpuLDA interface above the C ABI.

    LDA(corp, K)                       src/LDA.jl:6-47     host fp64 state (what @gpu reads/writes)
    gpuLDA(corp, K)                    src/gpuLDA.jl:6-85  device-backed model
      .update_buffer() / .update_host()   src/modelutils.jl:370-397 / :501-516
      .estep(viter, vtol)                 update_phi!/update_gamma!/update_Elogtheta! sweeps + update_beta!(d),
                                          CPU-path semantics src/LDA.jl:170-180
      .update_beta() .update_alpha(niter, ntol) .update_elbo()   src/gpuLDA.jl:201, :132, :120
      .train(iter=150, tol=1.0, niter=1000, ntol=1/K^2, viter=10, vtol=1/K^2, checkelbo=1, printelbo=True)
                                          src/gpuLDA.jl:347-376
    gpu_train(model, **kwargs)         `@gpu train!(model; kwargs...)`  src/macros.jl:106-150

All compute goes through libtmvb_hip.so; there is no CPU fallback in this module.
"""
from __future__ import annotations

import ctypes as C
import functools
import math

import numpy as np

from ._lib import CorpusError, TopicModelError, P_i64
from ._model import (DeviceContext, DeviceCorpus, DeviceModel, EstepTimer, PackedStats, TimingEvent, call_context, _F, _op, _pd,  # noqa: F401
                     _print_delbo, _topic_orders, _validate_train_args)             # (re-exported: the other modules and the tests import them from here)
from .corpus import Corpus, PackedCorpus, check_corp, dirichlet_rows  # noqa: F401

EPSILON = 2.0 ** -99          # src/utils.jl:3
EULERGAMMA = 0.5772156649015329


def _digamma_int(k: int) -> float:
    # psi(k) for a positive integer: -eulergamma + H_{k-1}
    return -EULERGAMMA + sum(1.0 / j for j in range(1, k))


def _packed(corp):
    if isinstance(corp, PackedCorpus):
        return corp
    check_corp(corp)
    return PackedCorpus.from_corpus(corp)


class LDA:
    """Host (fp64) LDA state with the reference's field names, src/LDA.jl:6-47."""

    def __init__(self, corp, K: int, seed: int = 7):
        if not (isinstance(K, (int, np.integer)) and K > 0):
            raise ValueError("number of topics must be a positive integer.")
        self.corp = _packed(corp)
        self.K, self.M, self.V = int(K), self.corp.M, self.corp.V
        self.N = self.corp.N
        self.C = self.corp.C
        K, M, V = self.K, self.M, self.V
        self.topics = [np.arange(1, V + 1) for _ in range(K)]
        self.alpha = np.ones(K)
        self.beta = dirichlet_rows(K, V, seed)                       # :35 (Julia RNG in the reference)
        self.beta_old = self.beta.copy(order="F")
        self.beta_temp = np.zeros((K, V), order="F")
        e0 = -EULERGAMMA - _digamma_int(K)                           # :38
        self.Elogtheta = np.full((K, M), e0, order="F")
        self.Elogtheta_old = self.Elogtheta.copy(order="F")
        self.gamma = np.ones((K, M), order="F")
        self.elbo = 0.0


def check_model(model, rtol: float = 1.5e-8):
    """check_model(::LDA) / (::gpuLDA)  src/modelutils.jl:39-67, :255-279 (array form).
    rtol mirrors isapprox's default sqrt(eps(T)): 1.5e-8 for Float64 fields, 3.5e-4 for the
    Float32-derived fields of a gpu model."""
    K, M, V = model.K, model.M, model.V
    if model.alpha.shape != (K,):
        raise TopicModelError("alpha must be of length K.")
    if not np.all(np.isfinite(model.alpha)):
        raise TopicModelError("alpha must be finite.")
    if not np.all(model.alpha > 0):
        raise TopicModelError("alpha must be positive.")
    if model.beta.shape != (K, V):
        raise TopicModelError("beta must be of size (K, V).")
    if V and not (np.all(model.beta >= 0) and np.allclose(model.beta.sum(axis=1), 1.0, rtol=rtol, atol=0)):
        raise TopicModelError("beta must be a right stochastic matrix.")
    for name in ("Elogtheta", "gamma"):
        a = getattr(model, name)
        if a.shape != (K, M):
            raise TopicModelError(f"{name} must contain vectors of length K.")
        if not np.all(np.isfinite(a)):
            raise TopicModelError(f"{name} must be finite.")
    if not np.all(model.Elogtheta <= 0):
        raise TopicModelError("Elogtheta must be nonpositive.")
    if not np.all(model.gamma > 0):
        raise TopicModelError("gamma must be positive.")
    if not math.isfinite(model.elbo):
        raise TopicModelError("elbo must be finite.")


class gpuLDA(PackedStats, EstepTimer, DeviceModel):
    """GPU accelerated latent Dirichlet allocation model (src/gpuLDA.jl:6-85) on libtmvb_hip.so."""

    _ABI, _HOST, _check = "lda", LDA, staticmethod(functools.partial(check_model, rtol=3.5e-4))
    _STATE = (("alpha", "K"), ("beta", "KV"), ("beta_old", "KV"), ("gamma", "KM"), ("Elogtheta", "KM"), ("Elogtheta_old", "KM"))

    def __init__(self, corp, K: int, seed: int = 7, ctx: DeviceContext | None = None, device_id: int = 0, stream=None,
                 _from: LDA | None = None):
        if not (isinstance(K, (int, np.integer)) and K > 0):
            raise ValueError("number of topics must be a positive integer.")
        super().__init__(corp, K, seed, ctx, device_id, stream, _from)

    # ---- device operators
    def estep(self, viter: int = 10, vtol: float | None = None):
        self._call("estep", viter, self._default_tol(vtol))

    def estep_allreduce(self, viter: int = 10, vtol: float | None = None):
        """estep + reduce_docs + the statistics all-reduce over the attached communicator, the collective issued in vocabulary
        slabs under the last statistics pass (tmvb_lda_estep_allreduce, include/tmvb.h)."""
        self._call("estep_allreduce", viter, self._default_tol(vtol))

    reduce_docs, update_beta = _op("reduce_docs"), _op("update_beta")

    def update_alpha(self, niter: int = 1000, ntol: float | None = None):
        self._call("update_alpha", niter, self._default_tol(ntol))

    def set_distributed(self, M_total: int, distributed: bool = True):
        self.M_total = int(M_total)
        self._call("set_distributed", M_total, 1 if distributed else 0)

    def sweep_hist(self, nbins: int = 11):
        h = np.zeros(nbins, dtype=np.int64)
        self._call("sweep_hist", h.ctypes.data_as(P_i64), nbins)
        return h

    def estep_launches(self) -> int:
        return self._get("estep_launches", C.c_int32)

    def estep_pieces(self) -> int:
        """Document pieces of the E-step's statistics passes, fixed at construction (1: one pass)."""
        return self._get("estep_pieces", C.c_int32)

    def set_comm(self, comm, M_total: int):
        """Attach a communicator (comm.py): this model's corpus is one document shard of M_total documents and
        train() becomes the sharded train! -- every rank calls it with the same arguments."""
        self.M_total = int(M_total) if comm is not None else self.M
        self._set_comm(comm, self.M_total)

    def train(self, iter: int = 150, tol: float = 1.0, niter: int = 1000, ntol: float | None = None, viter: int = 10,
              vtol: float | None = None, checkelbo=1, printelbo: bool = True):
        """train!(model::gpuLDA; ...) src/gpuLDA.jl:347-376.  Returns the ELBO trajectory."""
        return self._train(iter, tol, (niter, self._default_tol(ntol), viter, self._default_tol(vtol)), checkelbo, printelbo)


def gpu_train(model: LDA, device_id: int = 0, **kwargs):
    """`@gpu train!(model; kwargs...)` for LDA (src/macros.jl:113-150): copy the host model onto the
    device, train there, copy back, renormalise beta in fp64."""
    if not isinstance(model, LDA):
        raise ValueError("GPU acceleration only applies to LDA / CTM / CTPF models.")
    g = gpuLDA(None, model.K, device_id=device_id, _from=model)
    traj = g.train(**kwargs)
    model.topics = g.topics
    model.alpha = g.alpha
    model.beta = g.beta / g.beta.sum(axis=1, keepdims=True)          # src/macros.jl:147
    model.beta_old = model.beta.copy(order="F")                      # :148
    model.Elogtheta = g.Elogtheta
    model.Elogtheta_old = g.Elogtheta.copy(order="F")                # :142
    model.gamma = g.gamma
    model.elbo = g.elbo
    g.close()
    return traj


def predict(corp, train_model, iter: int = 10, tol: float | None = None, device_id: int = 0) -> LDA:
    """predict(corp, train_model::Union{LDA, gpuLDA}; iter=10, tol=1/K^2)  src/modelutils.jl:831-855:
    topic distributions of unseen documents with the trained alpha / beta frozen -- one pass of the fused
    E-step kernel (<= iter sweeps per document, same exit rule), no M-step."""
    K = train_model.K
    tol = 1.0 / K ** 2 if tol is None else tol
    pc = _packed(corp)
    if pc.V != train_model.V:
        raise CorpusError("predict corpus and train_model corpus must have identical vocabularies.")
    if tol < 0:
        raise ValueError("tolerance parameter must be nonnegative.")
    if iter < 0:
        raise ValueError("iteration parameter must be nonnegative.")
    g = gpuLDA(pc, K, device_id=device_id)
    g.alpha = np.array(train_model.alpha, dtype=np.float64)
    g.beta = np.asfortranarray(train_model.beta); g.beta_old = g.beta.copy(order="F")
    g.update_buffer()
    g.estep(iter, tol)
    g.update_host()
    out = LDA(pc, K)
    for n in ("alpha", "beta", "beta_old", "gamma", "Elogtheta", "Elogtheta_old"):
        setattr(out, n, getattr(g, n))
    out.topics = train_model.topics
    g.close()
    return out


def topicdist(model, d):
    """topicdist(model::Union{LDA, gpuLDA}, d)  src/modelutils.jl:946-951 (d is 1-based like the reference;
    a list / range of indices returns a list)."""
    if not isinstance(d, (int, np.integer)):
        return [topicdist(model, int(x)) for x in d]
    if not (1 <= d <= model.M):
        raise CorpusError("document index outside corpus range.")
    g = model.gamma[:, d - 1]
    return g / g.sum()
