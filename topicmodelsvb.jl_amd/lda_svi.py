"""
Stochastic (minibatch) training for LDA above the C ABI: stepwise EM on the device (include/tmvb.h, "stochastic (minibatch) training").

    gpuLDAStochastic(corp, K, cuts)       device-backed model over document batches [cuts[b], cuts[b + 1]); the host fields of gpuLDA plus the
                                          running statistic `sbar` (K x V), its tail `ebar` (K) and the step counter `t`
      .set_schedule(tau0, kappa)          rho_t = (tau0 + t)^(-kappa)
      .run(batches, niter, ntol, viter, vtol)   one step of train!'s loop body (src/LDA.jl:170-182) per listed batch id, repeats allowed
      .final_pass(viter, vtol)            the E-step of every batch under the final alpha, beta
      .update_buffer() / .update_host() / .info() / .doc_sweeps() / .last_run_ms() / .close()
    gpu_train_stochastic(model, ...)      the `@gpu train!` shape of gpu_train (src/macros.jl:113-150) with minibatch steps
    svi_rho(t, tau0, kappa), svi_cuts(M, batch)     the schedule and the equal cuts, on the host

All compute goes through libtmvb_hip.so; there is no CPU fallback in this module and no random number in the library: the host decides the
order of the visits.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._abi import SviInfo  # noqa: F401 (re-exported)
from ._lib import TopicModelError, check, lib, P_i32, P_i64, VP
from .lda import LDA, DeviceContext, _F, _packed, _pd, _topic_orders, check_model


def _validate_schedule(tau0, kappa):
    if not (np.isfinite(tau0) and tau0 >= 0):
        raise ValueError("tau0 parameter must be nonnegative.")
    if not (0.5 < kappa <= 1.0):
        raise ValueError("kappa parameter must be in (0.5, 1].")


def svi_rho(t: int, tau0: float = 1.0, kappa: float = 0.7) -> float:
    """The step size of step t = 1, 2, ...: (tau0 + t)^(-kappa), fp64."""
    _validate_schedule(tau0, kappa)
    if not (isinstance(t, (int, np.integer)) and t >= 1):
        raise ValueError("step parameter must be a positive integer.")
    return float((float(tau0) + float(t)) ** -float(kappa))


def svi_cuts(M: int, batch: int) -> np.ndarray:
    """Equal cuts of `batch` documents with a ragged last one: 0 = c_0 < ... < c_B = M."""
    if not (isinstance(M, (int, np.integer)) and M >= 1):
        raise ValueError("corpus size must be a positive integer.")
    if not (isinstance(batch, (int, np.integer)) and batch >= 1):
        raise ValueError("batch parameter must be a positive integer.")
    cuts = list(range(0, int(M), int(batch))) + [int(M)]
    return np.asarray(cuts, dtype=np.int64)


def _validate_svi_args(tols, iters, batch, epochs, tau0, kappa):
    if not all(t >= 0 for t in tols):
        raise ValueError("tolerance parameters must be nonnegative.")
    if not all(i >= 0 for i in iters):
        raise ValueError("iteration parameters must be nonnegative.")
    if not (isinstance(batch, (int, np.integer)) and batch >= 1):
        raise ValueError("batch parameter must be a positive integer.")
    if not (isinstance(epochs, (int, np.integer)) and epochs >= 0):
        raise ValueError("epochs parameter must be a nonnegative integer.")
    _validate_schedule(tau0, kappa)


class gpuLDAStochastic:
    """LDA trained in minibatches on libtmvb_hip.so (tmvb_lda_svi_*)."""

    def __init__(self, corp, K: int, cuts=None, batch: int = 4096, seed: int = 7, ctx: DeviceContext | None = None, device_id: int = 0,
                 _from: LDA | None = None):
        if not (isinstance(K, (int, np.integer)) and K > 0):
            raise ValueError("number of topics must be a positive integer.")
        host = _from if _from is not None else LDA(corp, K, seed)
        for k in ("corp", "K", "M", "V", "N", "C", "topics", "alpha", "beta", "beta_old", "Elogtheta", "Elogtheta_old", "gamma", "elbo"):
            setattr(self, k, getattr(host, k))
        self.cuts = svi_cuts(self.M, batch) if cuts is None else np.ascontiguousarray(cuts, dtype=np.int64)
        if self.cuts.ndim != 1 or len(self.cuts) < 2:
            raise ValueError("batch cuts must hold at least two entries.")
        self.B = len(self.cuts) - 1
        self.sbar, self.ebar, self.t = None, None, 0
        self._own_ctx = ctx is None
        self.ctx = ctx or DeviceContext(device_id)
        self.handle = VP()
        c = self.corp
        check(lib().tmvb_lda_svi_create(self.ctx.handle, c.M, c.V, c.doc_ptr.ctypes.data_as(P_i64),
                                        c.terms.ctypes.data_as(P_i32), c.counts.ctypes.data_as(P_i32), self.K,
                                        self.cuts.ctypes.data_as(P_i64), self.B, C.byref(self.handle)))
        self.update_buffer()

    # ---- marshalling
    def update_buffer(self):
        """Host fields -> device.  `sbar` / `ebar` None: left as they are on the device (the initial statistic is formed when there is none yet)."""
        K, M, V = self.K, self.M, self.V
        a = np.ascontiguousarray(self.alpha, dtype=np.float64)
        if a.shape != (K,):
            raise TopicModelError("alpha must be of length K.")
        b, bo = _F(self.beta, (K, V)), _F(self.beta_old, (K, V))
        g, e = _F(self.gamma, (K, M)), _F(self.Elogtheta, (K, M))
        s = _F(self.sbar, (K, V)) if self.sbar is not None else None
        eb = np.ascontiguousarray(self.ebar, dtype=np.float64) if self.ebar is not None else None
        if eb is not None and eb.shape != (K,):
            raise TopicModelError("ebar must be of length K.")
        t = C.c_int64(int(self.t))
        check(lib().tmvb_lda_svi_set_state(self.handle, _pd(a), _pd(b), _pd(bo), _pd(g), _pd(e), _pd(s) if s is not None else None,
                                           _pd(eb) if eb is not None else None, C.byref(t)))

    def update_host(self):
        """Device -> host fields (waits for the enqueued steps)."""
        K, M, V = self.K, self.M, self.V
        self.alpha = np.empty(K)
        self.beta = np.empty((K, V), order="F"); self.beta_old = np.empty((K, V), order="F")
        self.gamma = np.empty((K, M), order="F"); self.Elogtheta = np.empty((K, M), order="F")
        self.sbar = np.empty((K, V), order="F"); self.ebar = np.empty(K)
        t = C.c_int64(0)
        check(lib().tmvb_lda_svi_get_state(self.handle, _pd(self.alpha), _pd(self.beta), _pd(self.beta_old), _pd(self.gamma), _pd(self.Elogtheta),
                                           _pd(self.sbar), _pd(self.ebar), C.byref(t)))
        self.Elogtheta_old = self.Elogtheta.copy(order="F")
        self.t = int(t.value)

    # ---- operators
    def set_schedule(self, tau0: float = 1.0, kappa: float = 0.7):
        _validate_schedule(tau0, kappa)
        check(lib().tmvb_lda_svi_set_schedule(self.handle, tau0, kappa))

    def run(self, batches, niter: int = 1000, ntol: float | None = None, viter: int = 10, vtol: float | None = None):
        """One step per entry of `batches` (ids in [0, B), repeats allowed); asynchronous."""
        ntol = 1.0 / self.K ** 2 if ntol is None else ntol
        vtol = 1.0 / self.K ** 2 if vtol is None else vtol
        _validate_svi_args([ntol, vtol], [niter, viter], 1, 0, 0.0, 1.0)
        b = np.ascontiguousarray(batches, dtype=np.int64).ravel()
        if b.size and (b.min() < 0 or b.max() >= self.B):
            raise ValueError(f"batch ids must lie in [0, {self.B}).")
        b = b.astype(np.int32)
        check(lib().tmvb_lda_svi_run(self.handle, b.ctypes.data_as(P_i32), b.size, niter, ntol, viter, vtol))

    def final_pass(self, viter: int = 10, vtol: float | None = None):
        vtol = 1.0 / self.K ** 2 if vtol is None else vtol
        _validate_svi_args([vtol], [viter], 1, 0, 0.0, 1.0)
        check(lib().tmvb_lda_svi_final_pass(self.handle, viter, vtol))

    def info(self) -> dict:
        out = SviInfo()
        check(lib().tmvb_lda_svi_info(self.handle, C.byref(out)))
        return {n: getattr(out, n) for n, _ in out._fields_}

    def doc_sweeps(self):
        """Sweeps each document ran in the last E-step of its batch (uint8 per document, corpus order)."""
        out = np.zeros(self.M, dtype=np.uint8)
        check(lib().tmvb_lda_svi_doc_sweeps(self.handle, out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def last_run_ms(self) -> dict:
        """Device time of the last run() by part, summed over its steps (TMVB_ESTEP_TIMING=1 when the model was made)."""
        e, u, a, n = C.c_float(0.0), C.c_float(0.0), C.c_float(0.0), C.c_int64(0)
        check(lib().tmvb_lda_svi_last_run_ms(self.handle, C.byref(e), C.byref(u), C.byref(a), C.byref(n)))
        return {"estep_ms": e.value, "update_ms": u.value, "alpha_ms": a.value, "steps": int(n.value)}

    def synchronize(self):
        self.ctx.synchronize()

    def close(self):
        if getattr(self, "handle", None):
            lib().tmvb_lda_svi_destroy(self.handle)
            self.handle = VP()
        if getattr(self, "_own_ctx", False) and getattr(self, "ctx", None) is not None:
            self.ctx.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def svi_order(B: int, epochs: int, shuffle_seed=None) -> np.ndarray:
    """The visiting order of `epochs` epochs over B batches: the identity per epoch, or with a seed one NumPy Philox permutation per epoch."""
    if shuffle_seed is None:
        return np.tile(np.arange(B, dtype=np.int32), epochs)
    rng = np.random.Generator(np.random.Philox(int(shuffle_seed)))
    return np.concatenate([rng.permutation(B).astype(np.int32) for _ in range(epochs)]) if epochs else np.zeros(0, dtype=np.int32)


def gpu_train_stochastic(model: LDA, batch: int = 4096, epochs: int = 2, tau0: float = 1.0, kappa: float = 0.7, shuffle_seed=None,
                         final_pass: bool = True, niter: int = 1000, ntol: float | None = None, viter: int = 10, vtol: float | None = None,
                         device_id: int = 0):
    """`@gpu train!` in minibatches (the shape of gpu_train, src/macros.jl:113-150): copy the host model up, take epochs * B steps, copy
    back, renormalise beta in fp64, fill `topics`.  Returns the list of visited batch ids."""
    if not isinstance(model, LDA):
        raise ValueError("GPU acceleration only applies to LDA / CTM / CTPF models.")
    ntol = 1.0 / model.K ** 2 if ntol is None else ntol
    vtol = 1.0 / model.K ** 2 if vtol is None else vtol
    _validate_svi_args([ntol, vtol], [niter, viter], batch, epochs, tau0, kappa)
    check_model(model)
    g = gpuLDAStochastic(model.corp, model.K, batch=batch, device_id=device_id, _from=model)
    try:
        g.set_schedule(tau0, kappa)
        order = svi_order(g.B, epochs, shuffle_seed)
        g.run(order, niter=niter, ntol=ntol, viter=viter, vtol=vtol)
        if final_pass:
            g.final_pass(viter=viter, vtol=vtol)
        g.update_host()
        model.topics = _topic_orders(g.ctx, g.beta)
        model.alpha = g.alpha
        model.beta = g.beta / g.beta.sum(axis=1, keepdims=True)          # src/macros.jl:147
        model.beta_old = model.beta.copy(order="F")                      # :148
        model.Elogtheta = g.Elogtheta
        model.Elogtheta_old = g.Elogtheta.copy(order="F")                # :142
        model.gamma = g.gamma
        model.sbar, model.ebar, model.t = g.sbar, g.ebar, g.t
    finally:
        g.close()
    return order
