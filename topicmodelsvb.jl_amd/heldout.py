"""
Held-out evaluation on the device: document-completion perplexity (the reference has no such function).

    split_corpus(corp, frac=0.5, seed=0)                 -> (observed, heldout): two PackedCorpus over the same M and V
    heldout_loglik(model, observed, heldout, ...)        -> HeldoutResult(ll[M], tokens[M], zero_prob_tokens, perplexity)
    perplexity(model, corp, frac=0.5, seed=0, ...)       -> split, fold the observed part in with predict, score the held-out part

The ELBO bounds the training corpus and cannot be compared across K or across model families; exp(-sum ll / sum tokens) of held-out
words can.  The split is a pure function of (seed, doc_offset + d, token occurrence): occurrence t of document d (CSR order, an entry's
occurrences consecutive) is held out iff word t & 3 of Philox4x32-10(key = seed, counter = (doc_offset + d, stage 5, t >> 2)) is below
floor(frac * 2^32).  `heldout_loglik_raw` is the C ABI call itself (tmvb_heldout_loglik, include/tmvb.h).  All compute goes through
libtmvb_hip.so; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._abi import SplitResult  # noqa: F401 (re-exported)
from ._lib import CorpusError, TopicModelError, _copy, _csr, _handle, check, lib, P_dbl, P_i32, P_i64
from .corpus import PackedCorpus
from .lda import _packed, call_context


class HeldoutResult:
    """ll[M] (log predictive likelihood of each document's held-out words; 0 for a document without any, -inf where a word has probability
    0), tokens[M], zero_prob_tokens, perplexity = exp(-sum ll / sum tokens): inf if any ll is -inf, nan if no token is held out."""

    def __init__(self, ll, tokens, zero_prob_tokens, ms_kernel=0.0):
        self.ll = np.asarray(ll, dtype=np.float64)
        self.tokens = np.asarray(tokens, dtype=np.int64)
        self.zero_prob_tokens = int(zero_prob_tokens)
        self.ms_kernel = float(ms_kernel)

    @property
    def perplexity(self) -> float:
        n = int(self.tokens.sum())
        if n == 0:
            return float("nan")
        if np.any(np.isneginf(self.ll)):
            return float("inf")
        return float(np.exp(-self.ll.sum() / n))

    def __repr__(self):
        return f"HeldoutResult(M={len(self.ll)}, tokens={int(self.tokens.sum())}, zero_prob_tokens={self.zero_prob_tokens}, perplexity={self.perplexity:.6g})"


def split_corpus_raw(ctx, M, V, doc_ptr, terms, counts, frac=0.5, seed=0, doc_offset=0):
    """The ABI call tmvb_corpus_split.  ctx: a DeviceContext, or None for a NULL context (the library then answers TMVB_ENODEVICE on a
    machine without a GPU).  Returns (status, dict): nothing raises here."""
    L = lib()
    doc_ptr, terms, counts = _csr(doc_ptr, terms, counts)
    out = SplitResult()
    rc = L.tmvb_corpus_split(_handle(ctx), int(M), int(V), doc_ptr.ctypes.data_as(P_i64), terms.ctypes.data_as(P_i32),
                             counts.ctypes.data_as(P_i32), frac, np.uint64(int(seed) % 2 ** 64).astype(np.int64),
                             int(doc_offset), C.byref(out))
    if rc != 0:
        return rc, {"error": L.tmvb_last_error().decode("utf-8", "replace")}
    try:
        M = int(out.M)
        res = {"M": M, "nnz_obs": int(out.nnz_obs), "nnz_held": int(out.nnz_held), "sum_obs": int(out.sum_obs), "sum_held": int(out.sum_held),
               "obs_ptr": _copy(out.obs_ptr, M + 1, np.int64), "obs_terms": _copy(out.obs_terms, out.nnz_obs, np.int32),
               "obs_counts": _copy(out.obs_counts, out.nnz_obs, np.int32),
               "held_ptr": _copy(out.held_ptr, M + 1, np.int64), "held_terms": _copy(out.held_terms, out.nnz_held, np.int32),
               "held_counts": _copy(out.held_counts, out.nnz_held, np.int32),
               "ms": {"draw": float(out.ms_draw), "compact": float(out.ms_compact)}}
    finally:
        L.tmvb_split_free(C.byref(out))
    return rc, res


def heldout_loglik_raw(ctx, K, V, theta, beta, pc, laplace_smooth=0.0):
    """The ABI call tmvb_heldout_loglik: theta K x M, beta K x V, pc the held-out PackedCorpus (anything with doc_ptr / terms / counts).
    Returns (status, HeldoutResult) or (status, message): nothing raises here."""
    L = lib()
    f64 = lambda a: np.asfortranarray(np.asarray(a, dtype=np.float64))
    theta, beta = f64(theta), f64(beta)
    doc_ptr, terms, counts = _csr(pc.doc_ptr, pc.terms, pc.counts)
    M = len(doc_ptr) - 1
    ll = np.zeros(max(M, 1)); tokens = np.zeros(max(M, 1), dtype=np.int64)
    zero, ms = C.c_int64(0), C.c_float(0.0)
    rc = L.tmvb_heldout_loglik(_handle(ctx), int(K), int(V), M, theta.ctypes.data_as(P_dbl), beta.ctypes.data_as(P_dbl),
                               doc_ptr.ctypes.data_as(P_i64), terms.ctypes.data_as(P_i32), counts.ctypes.data_as(P_i32), laplace_smooth,
                               ll.ctypes.data_as(P_dbl), tokens.ctypes.data_as(P_i64), C.byref(zero), C.byref(ms))
    if rc != 0:
        return rc, L.tmvb_last_error().decode("utf-8", "replace")
    return rc, HeldoutResult(ll[:M], tokens[:M], zero.value, ms.value)


def split_corpus(corp, frac: float = 0.5, seed: int = 0, doc_offset: int = 0, device_id: int = 0):
    """(observed, heldout): every token occurrence of `corp` (a Corpus or a PackedCorpus) goes to the held-out side with probability
    `frac`, by the draw rule above.  Both sides keep M and V, entries whose count became 0 are dropped, a document may be empty on either
    side, observed + heldout is the input.  Readers / ratings do not travel."""
    pc = _packed(corp)
    with call_context(device_id) as ctx:
        rc, res = split_corpus_raw(ctx, pc.M, pc.V, pc.doc_ptr, pc.terms, pc.counts, float(frac), seed, doc_offset)
    check(rc)
    return (PackedCorpus(res["obs_ptr"], res["obs_terms"], res["obs_counts"], pc.V),
            PackedCorpus(res["held_ptr"], res["held_terms"], res["held_counts"], pc.V))


def _additive_logistic_columns(x):
    x = np.exp(x - x.max(axis=0, keepdims=True))
    return x / x.sum(axis=0, keepdims=True)


def predicted_theta(model, observed, iter: int = 10, tol=None, niter: int = 1000, ntol=None, device_id: int = 0):
    """K x M topic proportions of `observed` under the trained `model`: the model family's own predict, then its own topicdist for every
    document (gamma / sum gamma for LDA / fLDA, additive_logistic(lambda + vsq / 2) for CTM / fCTM)."""
    from .ctm import predict_ctm
    from .fctm import predict_fctm
    from .flda import predict_flda
    from .lda import predict
    if hasattr(model, "alef"):
        raise TopicModelError("heldout_loglik has no method for CTPF models: the reference has no predict for them (src/modelutils.jl:831-943).")
    filtered = hasattr(model, "kappa")
    if hasattr(model, "alpha"):
        p = (predict_flda if filtered else predict)(observed, model, iter=iter, tol=tol, device_id=device_id)
        return p.gamma / p.gamma.sum(axis=0, keepdims=True)
    if hasattr(model, "mu") and hasattr(model, "sigma"):
        p = (predict_fctm if filtered else predict_ctm)(observed, model, iter=iter, tol=tol, niter=niter, ntol=ntol, device_id=device_id)
        return _additive_logistic_columns(p.lam + 0.5 * p.vsq)
    raise TopicModelError("heldout_loglik needs an LDA, fLDA, CTM or fCTM model (or its gpu form).")


def heldout_loglik(model, observed, heldout, iter: int = 10, tol=None, niter: int = 1000, ntol=None, laplace_smooth: float = 0.0,
                   device_id: int = 0) -> HeldoutResult:
    """Folds `observed` in with the model's predict (iter / tol, and niter / ntol for the CTM family), takes the model's topicdist of every
    document as Theta and scores `heldout` under model.beta: ll[d] = sum_n c_n log(sum_k Theta[k, d] beta'[k, w_n]), beta' = (beta +
    laplace_smooth) / (1 + laplace_smooth V).  The filtered models' kappa / tau take no part in the score, as in the reference's gendoc
    (src/modelutils.jl:594-633): a filtered model is scored through its topics alone.  CTPF raises TopicModelError (no predict in the
    reference); differing vocabularies raise CorpusError."""
    if hasattr(model, "alef"):
        raise TopicModelError("heldout_loglik has no method for CTPF models: the reference has no predict for them (src/modelutils.jl:831-943).")
    obs, held = _packed(observed), _packed(heldout)
    if obs.V != model.V or held.V != model.V:
        raise CorpusError("predict corpus and train_model corpus must have identical vocabularies.")
    if obs.M != held.M:
        raise CorpusError("observed and heldout corpora must hold the same documents.")
    if not laplace_smooth >= 0:
        raise ValueError("laplace_smooth parameter must be nonnegative.")
    theta = predicted_theta(model, obs, iter, tol, niter, ntol, device_id)
    with call_context(device_id) as ctx:
        rc, res = heldout_loglik_raw(ctx, model.K, model.V, theta, model.beta, held, float(laplace_smooth))
    check(rc)
    res.theta = theta
    return res


def perplexity(model, corp, frac: float = 0.5, seed: int = 0, **kw) -> float:
    """Document-completion perplexity of `corp` (unseen documents) under `model`: split_corpus(corp, frac, seed), heldout_loglik on the two
    sides (keywords go there), exp(-sum ll / sum tokens).  Lower is better; V is the uniform model."""
    pc = _packed(corp)
    if pc.V != model.V:
        raise CorpusError("predict corpus and train_model corpus must have identical vocabularies.")
    if hasattr(model, "alef"):
        raise TopicModelError("heldout_loglik has no method for CTPF models: the reference has no predict for them (src/modelutils.jl:831-943).")
    obs, held = split_corpus(pc, frac, seed, device_id=kw.get("device_id", 0))
    return heldout_loglik(model, obs, held, **kw).perplexity
