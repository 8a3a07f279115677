"""
gendoc / gencorp (src/modelutils.jl:594-649): a model run as a generative process, on the device.

    gencorp(model, M, laplace_smooth=0.0, seed=0)   -> PackedCorpus of M synthetic documents over the model's vocabulary
    gendoc(model, laplace_smooth=0.0, seed=0)       -> Document (1-based terms, like every Document)

for LDA / gpuLDA / fLDA (theta ~ Dirichlet(alpha)) and CTM / gpuCTM / fCTM (theta = additive_logistic(N(mu, sigma))).  The reference has no
method for CTPF; neither has this module.  `gencorp_raw` is the C ABI call itself (tmvb_lda_gencorp / tmvb_ctm_gencorp, include/tmvb.h)
with the diagnostics and the per-stage device times.  Terms of a document come out sorted ascending (the reference returns a Dict's key
order).  The reference draws from Julia's global RNG; here `seed` names the corpus: same seed, same bytes, and documents [d0, d0 + m) of a
corpus are `doc_offset=d0, M=m` of the same seed.  All compute goes through libtmvb_hip.so; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._abi import GenCorpResult  # noqa: F401 (re-exported)
from ._lib import _copy, _handle, check, lib, P_dbl
from .corpus import Document, PackedCorpus
from .lda import call_context


def gencorp_raw(ctx, K, V, beta, M, mean_C, alpha=None, mu=None, sigma=None, laplace_smooth=0.0, seed=0, doc_offset=0, diagnostics=False):
    """The ABI call.  alpha -> tmvb_lda_gencorp, (mu, sigma) -> tmvb_ctm_gencorp.  ctx: a DeviceContext, or None for a NULL context (the
    library then answers TMVB_ENODEVICE on a machine without a GPU).  Returns (status, dict): nothing raises here."""
    L = lib()
    f64 = lambda a: np.asfortranarray(np.asarray(a, dtype=np.float64))
    beta = f64(beta)
    out = GenCorpResult()
    h = _handle(ctx)
    tail = (int(M), int(doc_offset), mean_C, laplace_smooth,
            np.uint64(int(seed) % 2 ** 64).astype(np.int64), 1 if diagnostics else 0, C.byref(out))
    if alpha is not None:
        alpha = f64(alpha)
        rc = L.tmvb_lda_gencorp(h, K, V, alpha.ctypes.data_as(P_dbl), beta.ctypes.data_as(P_dbl), *tail)
    else:
        mu, sigma = f64(mu), f64(sigma)
        rc = L.tmvb_ctm_gencorp(h, K, V, mu.ctypes.data_as(P_dbl), sigma.ctypes.data_as(P_dbl), beta.ctypes.data_as(P_dbl), *tail)
    if rc != 0:
        return rc, {"error": L.tmvb_last_error().decode("utf-8", "replace")}
    try:
        M = int(out.M)
        res = {"M": M, "nnz": int(out.nnz), "sum_counts": int(out.sum_counts),
               "doc_ptr": _copy(out.doc_ptr, M + 1, np.int64), "terms": _copy(out.terms, out.nnz, np.int32), "counts": _copy(out.counts, out.nnz, np.int32),
               "ms": {s: float(getattr(out, "ms_" + s)) for s in ("tables", "docs", "tokens", "condense")}}
        if diagnostics:
            res["log_theta"] = _copy(out.log_theta, M * K, np.float32).reshape(M, K)
            res["doc_topic"] = _copy(out.doc_topic, M * K, np.int32).reshape(M, K)
            res["topic_term"] = _copy(out.topic_term, K * V, np.int64).reshape(K, V)
    finally:
        L.tmvb_gencorp_free(C.byref(out))
    return rc, res


def _family(model):
    if hasattr(model, "alef"):
        raise TypeError("gendoc / gencorp have no method for CTPF models (src/modelutils.jl:594-633 covers LDA, fLDA, CTM, fCTM and their gpu forms).")
    if hasattr(model, "alpha"):
        return {"alpha": model.alpha}
    if hasattr(model, "mu") and hasattr(model, "sigma"):
        return {"mu": model.mu, "sigma": model.sigma}
    raise TypeError("gendoc / gencorp need an LDA, fLDA, CTM or fCTM model (or its gpu form).")


def gencorp(model, M, laplace_smooth: float = 0.0, seed: int = 0, doc_offset: int = 0, device_id: int = 0) -> PackedCorpus:
    """gencorp(model, M; laplace_smooth) (src/modelutils.jl:642-649)."""
    if not (isinstance(M, (int, np.integer)) and not isinstance(M, bool) and M > 0):
        raise ValueError("corp_size parameter must be a positive integer.")
    if not laplace_smooth >= 0:
        raise ValueError("laplace_smooth parameter must be nonnegative.")
    fam = _family(model)
    # like the reference, a gpu model is read through its HOST fields (alpha / mu / sigma / beta as train! left them)
    with call_context(device_id, getattr(model, "ctx", None)) as ctx:
        rc, res = gencorp_raw(ctx, model.K, model.V, model.beta, M, float(np.mean(model.C)), laplace_smooth=float(laplace_smooth), seed=seed,
                              doc_offset=doc_offset, **fam)
    check(rc)
    return PackedCorpus(res["doc_ptr"], res["terms"], res["counts"], model.V)


def gendoc(model, laplace_smooth: float = 0.0, seed: int = 0, device_id: int = 0) -> Document:
    """gendoc(model, laplace_smooth) (src/modelutils.jl:594-633): document 0 of the corpus `seed` names."""
    if not laplace_smooth >= 0:
        raise ValueError("laplace_smooth parameter must be nonnegative.")
    pc = gencorp(model, 1, laplace_smooth, seed, 0, device_id)
    return Document(terms=pc.terms.astype(np.int64) + 1, counts=pc.counts)
