"""
What the five device models (gpuLDA, gpufLDA, gpuCTM, gpufCTM, gpuCTPF) share above the C ABI: the device context and corpus, the
handle's life cycle, the operators that only pass the handle, the state copies driven by a per-model field list, and the body of train!.

A model names its ABI prefix (`_ABI`, the <m> of tmvb_<m>_*), its host class (`_HOST`), its check_model (`_check`) and its state
fields (`_STATE`, in the argument order of tmvb_<m>_set_state / _get_state); what differs between the models -- estep's arguments,
set_comm / set_distributed, sweep_hist, the recommendation calls -- stays in the model's own file.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math

import numpy as np

from ._lib import CorpusInfo, TopicModelError, check, lib, P_dbl, P_i32, P_i64, VP
from .corpus import PackedCorpus


def _pd(a):
    return a.ctypes.data_as(P_dbl)


def _F(a, shape):
    a = np.asfortranarray(np.asarray(a, dtype=np.float64))
    if a.shape != tuple(shape):
        raise TopicModelError(f"expected an array of size {tuple(shape)}, got {a.shape}.")
    return a


class DeviceContext:
    """One GPU + one stream (replaces cl.create_compute_context(), src/gpuLDA.jl:64)."""

    def __init__(self, device_id: int = 0, stream=None):
        self.handle = VP()
        check(lib().tmvb_ctx_create(device_id, stream if stream else None, C.byref(self.handle)))
        self.device_id = device_id

    def synchronize(self):
        check(lib().tmvb_ctx_synchronize(self.handle))

    def timing_event(self):
        """A HIP timing event on this context's stream without the system-scope fence of a default event (tmvb_event_create)."""
        return TimingEvent(self)

    def close(self):
        if self.handle:
            lib().tmvb_ctx_destroy(self.handle)
            self.handle = VP()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


@contextlib.contextmanager
def call_context(device_id: int = 0, ctx=None):
    """A DeviceContext for the length of one call of a stateless entry point, closed on the way out; a model's own `ctx` is handed
    through and stays open."""
    own = ctx is None
    if own:
        ctx = DeviceContext(device_id)
    try:
        yield ctx
    finally:
        if own:
            ctx.close()


class TimingEvent:
    """tmvb_event_*: record() on the context's stream; a.elapsed_ms(b) waits for b."""

    def __init__(self, ctx):
        self.handle = VP()
        check(lib().tmvb_event_create(ctx.handle, C.byref(self.handle)))

    def record(self):
        check(lib().tmvb_event_record(self.handle))

    def elapsed_ms(self, stop) -> float:
        ms = C.c_float(0.0)
        check(lib().tmvb_event_elapsed_ms(self.handle, stop.handle, C.byref(ms)))
        return float(ms.value)

    def close(self):
        if self.handle:
            lib().tmvb_event_destroy(self.handle)
            self.handle = VP()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceCorpus:
    """Corpus half of update_buffer! (src/modelutils.jl:370-388)."""

    def __init__(self, ctx: DeviceContext, corp: PackedCorpus):
        self.ctx, self.corp = ctx, corp
        self.handle = VP()
        has_r = corp.U > 0
        check(lib().tmvb_corpus_create(ctx.handle, corp.M, corp.V, corp.U,
                                       corp.doc_ptr.ctypes.data_as(P_i64), corp.terms.ctypes.data_as(P_i32),
                                       corp.counts.ctypes.data_as(P_i32),
                                       corp.rdr_ptr.ctypes.data_as(P_i64) if has_r else None,
                                       corp.readers.ctypes.data_as(P_i32) if has_r else None,
                                       corp.ratings.ctypes.data_as(P_i32) if has_r else None,
                                       C.byref(self.handle)))

    def info(self):
        out = CorpusInfo()
        check(lib().tmvb_corpus_info(self.handle, C.byref(out)))
        return {n: getattr(out, n) for n, _ in out._fields_}

    def close(self):
        if self.handle:
            lib().tmvb_corpus_destroy(self.handle)
            self.handle = VP()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _validate_train_args(tols, iters, checkelbo):
    # src/gpuLDA.jl:349-351
    if not all(t >= 0 for t in tols):
        raise ValueError("tolerance parameters must be nonnegative.")
    if not all(i >= 0 for i in iters):
        raise ValueError("iteration parameters must be nonnegative.")
    if not ((isinstance(checkelbo, (int, np.integer)) and checkelbo > 0) or checkelbo == math.inf):
        raise ValueError("checkelbo parameter must be a positive integer or Inf.")


def _topic_orders(ctx, B):
    """model.topics = [reverse(sortperm(vec(B[i,:]))) for i in 1:K]  (src/gpuLDA.jl:374 and its siblings), 1-based: tmvb_topic_order, one
    segmented sort on the device (K numpy sorts one after the other were 65 ms of a 209 ms train!(iter=150) call at K = 50, V = 25 319)."""
    B = np.asfortranarray(B, dtype=np.float64)
    K, V = B.shape
    out = np.empty((K, V), dtype=np.int32)
    check(lib().tmvb_topic_order(ctx.handle, _pd(B), K, V, out.ctypes.data_as(P_i32)))
    return [out[i].astype(np.int64) for i in range(K)]


def _print_delbo(traj, baseline):
    """The printing half of check_elbo! (src/modelutils.jl:578-579): one line per checked iteration, the first one
    against the ELBO evaluated before the first iteration."""
    prev = baseline
    for k, e in enumerate(traj, start=1):
        if not np.isnan(e):
            print(k, " ∆elbo: ", round(e - prev, 3))
            prev = e


def _op(name):
    """The method of an operator that passes the handle alone: check(tmvb_<m>_<name>(handle))."""
    def op(self):
        self._call(name)
    op.__name__ = name
    return op


class DeviceModel:
    """A handle of libtmvb_hip.so with the host fields of its model next to it."""

    _ABI = None          # "lda": the functions are tmvb_lda_*
    _HOST = None         # the host (fp64) class whose fields the device model mirrors
    _check = None        # its check_model, as train! applies it to a device model
    _STATE = ()          # (field, shape) in tmvb_<m>_set_state / _get_state order, elbo (always last) left out; shape: "" a scalar,
    #                      "K" / "V" / "M" / "N" (= nnz) a vector, two letters a column-major matrix
    _ATTRS = ("corp", "K", "M", "V", "N", "C", "topics")    # what else comes over from the host model

    def __init__(self, corp, K: int, seed: int = 7, ctx: DeviceContext | None = None, device_id: int = 0, stream=None, _from=None):
        host = _from if _from is not None else self._HOST(corp, K, seed)
        for k in self._ATTRS + tuple(n for n, _ in self._STATE) + ("elbo",):
            setattr(self, k, getattr(host, k))
        self.ctx = ctx or DeviceContext(device_id, stream)
        self.dcorp = DeviceCorpus(self.ctx, self.corp)
        self.handle = VP()
        self._call("create", self.ctx.handle, self.dcorp.handle, self.K, C.byref(self.handle), handle=False)
        self.M_total = self.M
        self.update_buffer()

    def _call(self, op, *args, handle=True):
        fn = getattr(lib(), f"tmvb_{self._ABI}_{op}")
        check(fn(self.handle, *args) if handle else fn(*args))

    def _get(self, op, ctype):
        out = ctype(0)
        self._call(op, C.byref(out))
        return out.value

    def _default_tol(self, tol):
        return 1.0 / self.K ** 2 if tol is None else tol

    # ---- marshalling
    def _shape(self, letters):
        dims = {"K": self.K, "V": self.V, "M": self.M, "N": self.corp.nnz}
        return tuple(dims[c] for c in letters)

    def update_buffer(self):
        """State half of update_buffer! (src/modelutils.jl:390-431): host fields -> device."""
        vals = []                        # what the pointers below point into, alive until the call returns
        for name, letters in self._STATE:
            x, shape = getattr(self, name), self._shape(letters)
            if len(shape) == 2:
                vals.append(_F(x, shape))
            elif len(shape) == 1:
                a = np.ascontiguousarray(x, dtype=np.float64)
                if a.size != shape[0]:
                    raise TopicModelError(f"{name} must be of length {letters}.")
                vals.append(a.reshape(shape))
            else:
                vals.append(C.c_double(float(x)))
        vals.append(C.c_double(float(self.elbo)))
        self._call("set_state", *[_pd(v) if isinstance(v, np.ndarray) else C.byref(v) for v in vals])

    def update_host(self):
        """update_host! (src/modelutils.jl:501-537): device -> host fields (phi is never materialised)."""
        out = [np.empty(self._shape(letters), order="F") if letters else C.c_double(0.0) for _, letters in self._STATE]
        elbo = C.c_double(0.0)
        self._call("get_state", *[_pd(o) if isinstance(o, np.ndarray) else C.byref(o) for o in out], C.byref(elbo))
        for (name, _), o in zip(self._STATE, out):
            setattr(self, name, o if isinstance(o, np.ndarray) else o.value)
        self.elbo = elbo.value

    # ---- device operators every model has
    def update_elbo(self) -> float:
        self.elbo = self._get("update_elbo", C.c_double)
        return self.elbo

    def elbo_form(self) -> int:
        """1 if the last update_elbo! took the decomposed form (parts left behind by the iteration itself, nothing per token rebuilt),
        0 for the token walk (CTPF: the table form)."""
        return self._get("elbo_form", C.c_int32)

    def doc_sweeps(self):
        """Sweeps each document ran in the last E-step (uint8 per document, corpus order)."""
        out = np.zeros(max(self.M, 1), dtype=np.uint8)
        self._call("doc_sweeps", out.ctypes.data_as(C.POINTER(C.c_uint8)))
        return out[:self.M]

    def synchronize(self):
        self.ctx.synchronize()

    def _set_comm(self, comm, *totals):
        self._comm = comm
        self._call("set_comm", comm.handle if comm is not None else None, *totals)

    # ---- train!
    def _topic_weights(self):
        return self.beta

    def _train(self, iter, tol, inner, checkelbo, printelbo):
        """The body of train!: `inner` holds the model's own (iterations, tolerance) pairs, flat, in the order tmvb_<m>_train takes them
        between `tol` and `checkelbo`.  Returns the ELBO trajectory."""
        self._check(self)
        _validate_train_args([tol, *inner[1::2]], [iter, *inner[0::2]], checkelbo)
        self.update_buffer()
        ce = 0 if checkelbo == math.inf else int(checkelbo)
        traj = np.full(max(iter, 1), np.nan)
        done, base = C.c_int32(0), C.c_double(float(self.elbo))
        self._call("train", iter, tol, *inner, ce, _pd(traj), C.byref(done), C.byref(base))
        traj = traj[:done.value]
        self.elbo_baseline = base.value
        if iter > 0:
            self.update_host()
        if printelbo and ce:
            _print_delbo(traj, base.value)
        self.topics = _topic_orders(self.ctx, self._topic_weights())
        return traj

    def close(self):
        if getattr(self, "handle", None):
            getattr(lib(), f"tmvb_{self._ABI}_destroy")(self.handle)
            self.handle = VP()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PackedStats:
    """The models whose packed sufficient statistics a host may reduce itself (tmvb_<m>_stats / _bind_stats)."""

    def stats(self):
        """(device pointer, n_float32) of the packed sufficient statistics (layouts: include/tmvb.h)."""
        p, n = VP(), C.c_int64(0)
        self._call("stats", C.byref(p), C.byref(n))
        return p.value, n.value

    def bind_stats(self, dev_ptr: int, n_f32: int):
        self._call("bind_stats", dev_ptr, n_f32)


class EstepTimer:
    """The models that time their last E-step with HIP events (tmvb_<m>_last_estep_ms)."""

    def last_estep_ms(self) -> float:
        return self._get("last_estep_ms", C.c_float)
