"""
Host-side mirror of the reference's CTPF / gpuCTPF interface above the C ABI.

    CTPF(corp, K)                     src/CTPF.jl:6-108     host fp64 state (Hebrew-letter field names kept)
    gpuCTPF(corp, K)                  src/gpuCTPF.jl:6-153  device-backed model
      .update_buffer() / .update_host()     src/modelutils.jl:438-494 / :539-570
      .estep(viter, vtol)                   update_xi!/update_phi!/update_zayin!/update_gimel! sweeps + update_he!(d),
                                            update_alef!(d); CPU-path semantics src/CTPF.jl:353-365
      .mstep()                              update_he!/alef!/dalet!/het!/bet!/vav! in that order, src/CTPF.jl:366-371
      .train(iter=150, tol=1.0, viter=10, vtol=1/K^2, checkelbo=Inf, printelbo=True)   src/gpuCTPF.jl:677-705
      .recommend(scores=True)               scores / drecs / urecs of the end of train!, src/CTPF.jl:379-399 (device GEMM +
                                            segmented sort; the reference does it on the host, src/gpuCTPF.jl:711-731)
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from ._lib import CorpusError, TopicModelError, P_i32, P_i64
from ._model import DeviceModel, EstepTimer, PackedStats, _F, _op, _pd
from .corpus import dirichlet_rows
from .lda import _packed


class CTPF:
    """Host (fp64) CTPF state, src/CTPF.jl:6-108.  scores / drecs / urecs are filled by train! (1-based ids, like topics)."""

    def __init__(self, corp, K: int, seed: int = 7):
        if not (isinstance(K, (int, np.integer)) and K > 0):
            raise ValueError("number of topics must be a positive integer.")
        self.corp = _packed(corp)
        self.K, self.M, self.V, self.U = int(K), self.corp.M, self.corp.V, self.corp.U
        self.N, self.C, self.R = self.corp.N, self.corp.C, np.diff(self.corp.rdr_ptr)
        K, M, V, U = self.K, self.M, self.V, self.U
        self.topics = [np.arange(1, V + 1) for _ in range(K)]
        self.a = self.b = self.c = self.d = self.e = self.f = self.g = self.h = 0.1                # :81
        self.alef = np.asfortranarray(np.exp(dirichlet_rows(K, V, seed) - 0.5))                    # :83
        self.alef_old = self.alef.copy(order="F")
        self.he = np.ones((K, U), order="F"); self.he_old = self.he.copy(order="F")
        for n in ("bet", "vav", "dalet", "het"):
            setattr(self, n, np.ones(K)); setattr(self, n + "_old", np.ones(K))
        for n in ("gimel", "zayin"):
            setattr(self, n, np.ones((K, M), order="F")); setattr(self, n + "_old", np.ones((K, M), order="F"))
        self.elbo = 0.0
        # libs[u] = documents user u has read (src/CTPF.jl:62-65), 1-based; recommendations start unranked (:67-79)
        self.libs = [[] for _ in range(U)]
        for d in range(M):
            for u in self.corp.readers[self.corp.rdr_ptr[d]:self.corp.rdr_ptr[d + 1]]:
                self.libs[int(u)].append(d + 1)
        self.scores = None
        self.drecs = None
        self.urecs = None

    def hyper(self):
        return np.array([self.a, self.b, self.c, self.d, self.e, self.f, self.g, self.h], dtype=np.float64)


def check_model_ctpf(model):
    """check_model(::CTPF) src/modelutils.jl:181-253 (array form)."""
    for n in "abcdefgh":
        if not getattr(model, n) > 0:
            raise TopicModelError(f"{n} must be positive.")
    for n in ("alef", "he", "bet", "vav", "dalet", "het", "gimel", "zayin"):
        a = getattr(model, n)
        if not np.all(np.isfinite(a)):
            raise TopicModelError(f"{n} must be finite.")
        if not np.all(a > 0):
            raise TopicModelError(f"{n} must be positive.")
    if not math.isfinite(model.elbo):
        raise TopicModelError("elbo must be finite.")


class gpuCTPF(PackedStats, EstepTimer, DeviceModel):
    """GPU accelerated collaborative topic Poisson factorization model (src/gpuCTPF.jl:6-153) on libtmvb_hip.so."""

    _ABI, _HOST, _check = "ctpf", CTPF, staticmethod(check_model_ctpf)
    _RATES = ("bet", "vav", "dalet", "het")
    _ARRAYS = ("alef", "he") + _RATES + ("gimel", "zayin")
    _ATTRS = (("corp", "K", "M", "V", "U", "N", "C", "R", "topics", "a", "b", "c", "d", "e", "f", "g", "h", "libs", "scores", "drecs", "urecs")
              + _ARRAYS + tuple(n + "_old" for n in _ARRAYS))

    hyper = CTPF.hyper

    # tmvb_ctpf_set_state takes the hyper-parameters and the current fields, _set_state_old the *_old ones, and _get_state packs the eight
    # rate vectors into one array: the copies are written out here, not driven by _STATE
    def update_buffer(self):
        K, M, V, U = self.K, self.M, self.V, self.U

        def arrays(old):                 # the eight fields as tmvb_ctpf_set_state (old = "") and _set_state_old (old = "_old") take them
            f = lambda n: getattr(self, n + old)
            return [_F(f("alef"), (K, V)), _F(f("he"), (K, U)), *[np.ascontiguousarray(f(n), dtype=np.float64) for n in self._RATES],
                    _F(f("gimel"), (K, M)), _F(f("zayin"), (K, M))]
        hy, cur, old = self.hyper(), arrays(""), arrays("_old")
        self._call("set_state", _pd(hy), *map(_pd, cur), C.byref(C.c_double(float(self.elbo))))
        # the *_old fields feed update_elbo! (src/CTPF.jl:239-240) and are part of update_buffer! (src/modelutils.jl:474-493)
        self._call("set_state_old", *map(_pd, old))

    def update_host(self):
        K, M, V, U = self.K, self.M, self.V, self.U
        self.alef = np.empty((K, V), order="F"); self.alef_old = np.empty((K, V), order="F")
        self.he = np.empty((K, U), order="F"); self.he_old = np.empty((K, U), order="F")
        rates = np.empty(8 * K)
        self.gimel = np.empty((K, M), order="F"); self.gimel_old = np.empty((K, M), order="F")
        self.zayin = np.empty((K, M), order="F"); self.zayin_old = np.empty((K, M), order="F")
        elbo = C.c_double(0.0)
        self._call("get_state", _pd(self.alef), _pd(self.alef_old), _pd(self.he), _pd(self.he_old), _pd(rates), _pd(self.gimel),
                   _pd(self.gimel_old), _pd(self.zayin), _pd(self.zayin_old), C.byref(elbo))
        for q, n in enumerate(self._RATES + tuple(n + "_old" for n in self._RATES)):
            setattr(self, n, rates[q * K:(q + 1) * K].copy())
        self.elbo = elbo.value

    def estep(self, viter: int = 10, vtol: float | None = None):
        self._call("estep", viter, self._default_tol(vtol))

    reduce_docs, mstep = _op("reduce_docs"), _op("mstep")

    def update_elbo_parts(self):
        """(per-document part summed over this context's documents, global (beta, eta) part) for document-sharded hosts."""
        a, b = C.c_double(0.0), C.c_double(0.0)
        self._call("update_elbo_parts", C.byref(a), C.byref(b))
        return a.value, b.value

    def set_distributed(self, distributed: bool = True):
        self._call("set_distributed", 1 if distributed else 0)

    def set_comm(self, comm):
        """Attach a communicator (comm.py): document-sharded train!, every rank calls train() with the same arguments."""
        self._set_comm(comm)

    def sweep_hist(self, nbins: int = 11):
        h = np.zeros(nbins, dtype=np.int64)
        self._call("sweep_hist", h.ctypes.data_as(P_i64), nbins)
        return h

    def recommend(self, scores: bool = True):
        """scores (M x U fp64), drecs[d], urecs[u] from the device-resident state (src/CTPF.jl:379-399).  Ids are 1-based.
        Returns (ms_scores, ms_rank): device time of the score pass and of the two segmented sorts."""
        M, U = self.M, self.U
        if M == 0 or U == 0:
            self.scores = np.zeros((M, U), order="F"); self.drecs = [np.arange(1, U + 1) for _ in range(M)]
            self.urecs = [np.arange(1, M + 1) for _ in range(U)]
            return 0.0, 0.0
        sc = np.empty((M, U), order="F") if scores else None
        dr = np.empty((M, U), dtype=np.int32); dc = np.empty(M, dtype=np.int32)
        ur = np.empty((U, M), dtype=np.int32); uc = np.empty(U, dtype=np.int32)
        ms0, ms1 = C.c_float(0.0), C.c_float(0.0)
        p32 = lambda a: a.ctypes.data_as(P_i32)
        self._call("recommend", _pd(sc) if scores else None, p32(dr), p32(dc), p32(ur), p32(uc), C.byref(ms0), C.byref(ms1))
        if scores:
            self.scores = sc
        self.drecs = [dr[d, :dc[d]] + 1 for d in range(M)]
        self.urecs = [ur[u, :uc[u]] + 1 for u in range(U)]
        return ms0.value, ms1.value

    def recommend_topn(self, topn: int = 15, by: str = "user", ids=None, splits: int = 0):
        """The `topn` best entries of urecs[u] (by="user") or drecs[d] (by="doc") for the 1-based `ids` (default all) from the
        device-resident state, without the M x U rankings of recommend(): recs_topn.recommend_topn on this handle's context."""
        from .recs_topn import recommend_topn
        self.update_host()
        return recommend_topn(self, topn, by, ids, splits)

    def _topic_weights(self):
        return self.alef / self.bet[:, None]                                                      # src/gpuCTPF.jl:707-708

    def train(self, iter: int = 150, tol: float = 1.0, viter: int = 10, vtol: float | None = None, checkelbo=1,
              printelbo: bool = True, recs: bool = True):
        """train!(model::gpuCTPF; ...) src/gpuCTPF.jl:677-705.  recs=False skips the M x U recommendation tail (:711-731)."""
        traj = self._train(iter, tol, (viter, self._default_tol(vtol)), checkelbo, printelbo)
        if recs:
            self.recommend()                                                                      # :711-731
        return traj


def gpu_train_ctpf(model: CTPF, device_id: int = 0, **kwargs):
    """`@gpu train!(model::CTPF; kwargs...)` (src/macros.jl:197-272)."""
    g = gpuCTPF(None, model.K, device_id=device_id, _from=model)
    traj = g.train(**kwargs)
    for n in ("topics", "alef", "he", "bet", "vav", "dalet", "het", "gimel", "zayin", "elbo", "scores", "drecs", "urecs"):
        setattr(model, n, getattr(g, n))
    for n in ("alef", "he", "bet", "vav", "dalet", "het", "gimel", "zayin"):
        setattr(model, n + "_old", np.array(getattr(g, n), copy=True, order="F"))
    g.close()
    return traj


def topicdist_ctpf(model, d):
    """topicdist(model::Union{CTPF, gpuCTPF}, d)  src/modelutils.jl:960-965: gimel[d] / sum(gimel[d]) (d is 1-based like the
    reference; a list / range of indices returns a list, :972-983)."""
    if not isinstance(d, (int, np.integer)):
        return [topicdist_ctpf(model, int(x)) for x in d]
    if not (1 <= d <= model.M):
        raise CorpusError("document index outside corpus range.")
    g = model.gimel[:, d - 1]
    return g / g.sum()
