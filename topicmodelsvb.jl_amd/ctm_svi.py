"""
Stochastic (minibatch) training for CTM above the C ABI: stepwise EM on the device (include/tmvb.h, "stochastic (minibatch) training for CTM").

    gpuCTMStochastic(corp, K, cuts)       device-backed model over document batches [cuts[b], cuts[b + 1]); the host fields of gpuCTM plus the
                                          running statistic `sbar` (K x V), its tail `lbar`, `vbar` (K), `cbar` (K x K) about `mref` (K), and the
                                          step counter `t`
      .set_schedule(tau0, kappa)          rho_t = (tau0 + t)^(-kappa)
      .run(batches, niter, ntol, viter, vtol)   one step of train!'s loop body (src/CTM.jl:194-208) per listed batch id, repeats allowed
      .final_pass(niter, ntol, viter, vtol)     the E-step of every batch under the final mu, sigma, beta
      .update_buffer() / .update_host() / .info() / .doc_sweeps() / .last_run_ms() / .close()
    gpu_train_ctm_stochastic(model, ...)  the `@gpu train!` shape of gpu_train_ctm (src/macros.jl:152-195) with minibatch steps

The schedule, the equal cuts and the visiting order are those of LDA's stochastic path (svi_rho, svi_cuts, svi_order).  All compute goes through
libtmvb_hip.so; there is no CPU fallback in this module and no random number in the library: the host decides the order of the visits.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import TopicModelError, check, lib, P_i32, P_i64, VP
from .ctm import CTM, check_model_ctm
from .lda import DeviceContext, _F, _pd, _topic_orders
from .lda_svi import SviInfo, _validate_schedule, _validate_svi_args, svi_cuts, svi_order


class gpuCTMStochastic:
    """CTM trained in minibatches on libtmvb_hip.so (tmvb_ctm_svi_*)."""

    _TAIL = ("lbar", "vbar", "cbar", "mref")

    def __init__(self, corp, K: int, cuts=None, batch: int = 4096, seed: int = 7, ctx: DeviceContext | None = None, device_id: int = 0,
                 _from: CTM | None = None):
        if not (isinstance(K, (int, np.integer)) and K > 0):
            raise ValueError("number of topics must be a positive integer.")
        host = _from if _from is not None else CTM(corp, K, seed)
        for k in ("corp", "K", "M", "V", "N", "C", "topics", "mu", "sigma", "invsigma", "beta", "beta_old", "lam", "lam_old", "vsq", "logzeta", "elbo"):
            setattr(self, k, getattr(host, k))
        self.cuts = svi_cuts(self.M, batch) if cuts is None else np.ascontiguousarray(cuts, dtype=np.int64)
        if self.cuts.ndim != 1 or len(self.cuts) < 2:
            raise ValueError("batch cuts must hold at least two entries.")
        self.B = len(self.cuts) - 1
        self.sbar, self.lbar, self.vbar, self.cbar, self.mref, self.t = None, None, None, None, None, 0
        self._own_ctx = ctx is None
        self.ctx = ctx or DeviceContext(device_id)
        self.handle = VP()
        c = self.corp
        check(lib().tmvb_ctm_svi_create(self.ctx.handle, c.M, c.V, c.doc_ptr.ctypes.data_as(P_i64),
                                        c.terms.ctypes.data_as(P_i32), c.counts.ctypes.data_as(P_i32), self.K,
                                        self.cuts.ctypes.data_as(P_i64), self.B, C.byref(self.handle)))
        self.update_buffer()

    # ---- marshalling
    def update_buffer(self):
        """Host fields -> device.  `sbar` None, or the tail (`lbar`, `vbar`, `cbar`, `mref`) None: left as they are on the device (the initial
        statistic is formed when there is none yet).  The tail is set as a whole."""
        K, M, V = self.K, self.M, self.V
        mu = np.ascontiguousarray(self.mu, dtype=np.float64)
        if mu.shape != (K,):
            raise TopicModelError("mu must be of length K.")
        lz = np.ascontiguousarray(self.logzeta, dtype=np.float64)
        if lz.shape != (M,):
            raise TopicModelError("logzeta must be of length M.")
        s = _F(self.sbar, (K, V)) if self.sbar is not None else None
        given = [getattr(self, n) is not None for n in self._TAIL]
        if any(given) and not all(given):
            raise TopicModelError("the running tail (lbar, vbar, cbar, mref) is set as a whole.")
        tail = [None] * 4
        if all(given):
            tail = [np.ascontiguousarray(self.lbar, dtype=np.float64), np.ascontiguousarray(self.vbar, dtype=np.float64), _F(self.cbar, (K, K)),
                    np.ascontiguousarray(self.mref, dtype=np.float64)]
            if any(a.shape != (K,) for a in (tail[0], tail[1], tail[3])):
                raise TopicModelError("lbar, vbar and mref must be of length K.")
        opt = lambda a: _pd(a) if a is not None else None
        t = C.c_int64(int(self.t))
        check(lib().tmvb_ctm_svi_set_state(self.handle, _pd(mu), _pd(_F(self.sigma, (K, K))), _pd(_F(self.invsigma, (K, K))), _pd(_F(self.beta, (K, V))),
                                           _pd(_F(self.beta_old, (K, V))), _pd(_F(self.lam, (K, M))), _pd(_F(self.vsq, (K, M))), _pd(lz), opt(s),
                                           opt(tail[0]), opt(tail[1]), opt(tail[2]), opt(tail[3]), C.byref(t)))

    def update_host(self):
        """Device -> host fields (waits for the enqueued steps)."""
        K, M, V = self.K, self.M, self.V
        self.mu = np.empty(K)
        self.sigma = np.empty((K, K), order="F"); self.invsigma = np.empty((K, K), order="F")
        self.beta = np.empty((K, V), order="F"); self.beta_old = np.empty((K, V), order="F")
        self.lam = np.empty((K, M), order="F"); self.vsq = np.empty((K, M), order="F"); self.logzeta = np.empty(M)
        self.sbar = np.empty((K, V), order="F"); self.lbar = np.empty(K); self.vbar = np.empty(K)
        self.cbar = np.empty((K, K), order="F"); self.mref = np.empty(K)
        t = C.c_int64(0)
        check(lib().tmvb_ctm_svi_get_state(self.handle, _pd(self.mu), _pd(self.sigma), _pd(self.invsigma), _pd(self.beta), _pd(self.beta_old),
                                           _pd(self.lam), _pd(self.vsq), _pd(self.logzeta), _pd(self.sbar), _pd(self.lbar), _pd(self.vbar),
                                           _pd(self.cbar), _pd(self.mref), C.byref(t)))
        self.lam_old = self.lam.copy(order="F")
        self.t = int(t.value)

    # ---- operators
    def set_schedule(self, tau0: float = 1.0, kappa: float = 0.7):
        _validate_schedule(tau0, kappa)
        check(lib().tmvb_ctm_svi_set_schedule(self.handle, tau0, kappa))

    def _tols(self, ntol, vtol):
        return (1.0 / self.K ** 2 if ntol is None else ntol), (1.0 / self.K ** 2 if vtol is None else vtol)

    def run(self, batches, niter: int = 1000, ntol: float | None = None, viter: int = 10, vtol: float | None = None):
        """One step per entry of `batches` (ids in [0, B), repeats allowed); asynchronous."""
        ntol, vtol = self._tols(ntol, vtol)
        _validate_svi_args([ntol, vtol], [niter, viter], 1, 0, 0.0, 1.0)
        b = np.ascontiguousarray(batches, dtype=np.int64).ravel()
        if b.size and (b.min() < 0 or b.max() >= self.B):
            raise ValueError(f"batch ids must lie in [0, {self.B}).")
        b = b.astype(np.int32)
        check(lib().tmvb_ctm_svi_run(self.handle, b.ctypes.data_as(P_i32), b.size, niter, ntol, viter, vtol))

    def final_pass(self, niter: int = 1000, ntol: float | None = None, viter: int = 10, vtol: float | None = None):
        ntol, vtol = self._tols(ntol, vtol)
        _validate_svi_args([ntol, vtol], [niter, viter], 1, 0, 0.0, 1.0)
        check(lib().tmvb_ctm_svi_final_pass(self.handle, niter, ntol, viter, vtol))

    def info(self) -> dict:
        out = SviInfo()
        check(lib().tmvb_ctm_svi_info(self.handle, C.byref(out)))
        return {n: getattr(out, n) for n, _ in out._fields_}

    def doc_sweeps(self):
        """Sweeps each document ran in the last E-step of its batch (uint8 per document, corpus order)."""
        out = np.zeros(self.M, dtype=np.uint8)
        check(lib().tmvb_ctm_svi_doc_sweeps(self.handle, out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def last_run_ms(self) -> dict:
        """Device time of the last run() by part, summed over its steps (TMVB_ESTEP_TIMING=1 when the model was made)."""
        e, u, a, n = C.c_float(0.0), C.c_float(0.0), C.c_float(0.0), C.c_int64(0)
        check(lib().tmvb_ctm_svi_last_run_ms(self.handle, C.byref(e), C.byref(u), C.byref(a), C.byref(n)))
        return {"estep_ms": e.value, "update_ms": u.value, "sigma_mu_ms": a.value, "steps": int(n.value)}

    def synchronize(self):
        self.ctx.synchronize()

    def close(self):
        if getattr(self, "handle", None):
            lib().tmvb_ctm_svi_destroy(self.handle)
            self.handle = VP()
        if getattr(self, "_own_ctx", False) and getattr(self, "ctx", None) is not None:
            self.ctx.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def gpu_train_ctm_stochastic(model: CTM, batch: int = 4096, epochs: int = 2, tau0: float = 1.0, kappa: float = 0.7, shuffle_seed=None,
                             final_pass: bool = True, niter: int = 1000, ntol: float | None = None, viter: int = 10, vtol: float | None = None,
                             device_id: int = 0):
    """`@gpu train!` in minibatches (the shape of gpu_train_ctm, src/macros.jl:152-195): copy the host model up, take epochs * B steps, copy
    back, renormalise beta in fp64, fill `topics`.  Returns the list of visited batch ids."""
    if not isinstance(model, CTM):
        raise ValueError("GPU acceleration only applies to LDA / CTM / CTPF models.")
    ntol = 1.0 / model.K ** 2 if ntol is None else ntol
    vtol = 1.0 / model.K ** 2 if vtol is None else vtol
    _validate_svi_args([ntol, vtol], [niter, viter], batch, epochs, tau0, kappa)
    check_model_ctm(model, rtol=3.5e-4)
    g = gpuCTMStochastic(model.corp, model.K, batch=batch, device_id=device_id, _from=model)
    try:
        g.set_schedule(tau0, kappa)
        order = svi_order(g.B, epochs, shuffle_seed)
        g.run(order, niter=niter, ntol=ntol, viter=viter, vtol=vtol)
        if final_pass:
            g.final_pass(niter=niter, ntol=ntol, viter=viter, vtol=vtol)
        g.update_host()
        model.topics = _topic_orders(g.ctx, g.beta)
        model.mu, model.sigma, model.invsigma = g.mu, g.sigma, g.invsigma
        model.beta = g.beta / g.beta.sum(axis=1, keepdims=True)          # src/macros.jl:190
        model.beta_old = model.beta.copy(order="F")
        model.lam = g.lam; model.lam_old = g.lam.copy(order="F")         # :183
        model.vsq, model.logzeta = g.vsq, g.logzeta
        model.sbar, model.lbar, model.vbar, model.cbar, model.mref, model.t = g.sbar, g.lbar, g.vbar, g.cbar, g.mref, g.t
    finally:
        g.close()
    return order
