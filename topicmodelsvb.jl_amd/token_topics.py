"""
Word-topic assignments: which topic a word belongs to in a document (gensim's per_word_topics, MALLET's state file).

    token_topics(model, docs=None, top=1, corp=None)     -> TokenTopics: per entry the `top` best topics and their responsibilities, per
                                                            document the counts by best topic
    phi(model, d)                                        -> K x N_d float32, the reference's gpumodel.phi[d] (d 1-based); a list for a list
    token_factors(model)                                 -> (A, B): the two nonnegative factors of update_phi! by model family
    token_topics_raw(ctx, K, V, A, B, pc, ...)           -> the ABI call tmvb_token_topics itself (include/tmvb.h)

The engine never keeps phi; the reference fills model.phi for every document (src/modelutils.jl:514-515, :534-535, :559-560).  Here phi is
recomputed from the factors on the device, r_k = (eps + A[k, d] B[k, w]) / sum_j (eps + A[j, d] B[j, w]), the top topics are selected in
registers, and only what was asked for comes back.  All compute goes through libtmvb_hip.so; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import CorpusError, TokenTopicsInfo, TopicModelError, _csr, _handle, check, lib, P_dbl, P_f32, P_i32, P_i64
from .lda import _packed, call_context

EPSILON = 1.5777218104420236e-30        # the reference's EPSILON (src/utils.jl:3), added by @positive (src/macros.jl:34-39)
TOP_MAX = 8                             # TMVB_TT_TOP_MAX


def digamma(x):
    """psi(x) in fp64 by the library's host digamma (tmvb_digamma_f64; touches no device)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.empty_like(x)
    check(lib().tmvb_digamma_f64(x.ctypes.data_as(P_dbl), y.ctypes.data_as(P_dbl), x.size))
    return y


def token_topics_raw(ctx, K, V, A, B, pc, docs=None, top=1, eps=EPSILON, phi=False, hard=True, max_chunk_entries=0, select=True):
    """The ABI call tmvb_token_topics: A K x M, B K x V, pc anything with doc_ptr / terms / counts, docs 0-based ids (None: every document
    in order).  select=False passes NULL for top_idx / top_r.  Returns (status, dict) or (status, message): nothing raises here."""
    L = lib()
    try:
        f64 = lambda a: np.asfortranarray(np.asarray(a, dtype=np.float64))
        A, B = f64(A), f64(B)
        doc_ptr, terms, counts = _csr(pc.doc_ptr, pc.terms, pc.counts)
        M = len(doc_ptr) - 1
        K, V, t = int(K), int(V), int(top)
        if A.shape != (K, M) or B.shape != (K, V):
            return 1, f"token_topics_raw: A must be of size ({K}, {M}) and B of size ({K}, {V})"
        d32 = None if docs is None else np.ascontiguousarray(docs, dtype=np.int64)
        if d32 is not None and d32.size and (d32.min() < -2 ** 31 or d32.max() >= 2 ** 31):
            return 1, "token_topics_raw: a document id does not fit 32 bits"
        d32 = None if d32 is None else d32.astype(np.int32)
        Ms = M if d32 is None else len(d32)
        # sizes from the arguments alone, so that a bad doc_ptr or id reaches the library's own checks and not an allocation
        ok = M >= 1 and doc_ptr[0] == 0 and bool(np.all(np.diff(doc_ptr) >= 0)) and (d32 is None or bool(np.all((d32 >= 0) & (d32 < M))))
        lens = np.diff(doc_ptr) if ok else np.zeros(max(M, 0), dtype=np.int64)
        nsel = int(lens.sum() if d32 is None else lens[d32].sum()) if ok else 0
        tt = min(max(t, 1), TOP_MAX)
        top_idx = np.full((max(nsel, 1), tt), -1, dtype=np.int32) if select else None
        top_r = np.zeros((max(nsel, 1), tt), dtype=np.float32) if select else None
        dense = np.zeros((max(nsel, 1), K), dtype=np.float32) if phi and 1 <= K <= 1024 else None
        hd = np.zeros((max(Ms, 1), max(K, 1)), dtype=np.int64) if hard else None
    except (TypeError, ValueError, AttributeError) as e:
        return 1, f"token_topics_raw: {e}"
    info = TokenTopicsInfo()
    p = lambda a, ty: a.ctypes.data_as(ty) if a is not None else None
    rc = L.tmvb_token_topics(_handle(ctx), K, V, M, p(A, P_dbl), p(B, P_dbl), p(doc_ptr, P_i64), p(terms, P_i32),
                             p(counts, P_i32), p(d32, P_i32), Ms, float(eps), t, int(max_chunk_entries),
                             p(top_idx, P_i32), p(top_r, P_f32), p(dense, P_f32), p(hd, P_i64), C.byref(info))
    if rc != 0:
        return rc, L.tmvb_last_error().decode("utf-8", "replace")
    if d32 is None:                                        # the selection is the corpus
        zdocs, sel_ptr, sel_terms, sel_counts = np.arange(M, dtype=np.int64), doc_ptr, terms, counts
    else:
        zdocs = d32.astype(np.int64)
        sel_ptr = np.concatenate([[0], np.cumsum(lens[zdocs])]).astype(np.int64)
        take = np.concatenate([np.arange(doc_ptr[d], doc_ptr[d + 1]) for d in zdocs] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
        sel_terms, sel_counts = terms[take], counts[take]
    return rc, {"nsel": nsel, "doc_ptr": sel_ptr, "terms": sel_terms, "counts": sel_counts, "docs": zdocs,
                "top_idx": top_idx[:nsel] if select else None, "top_r": top_r[:nsel] if select else None,
                "phi": dense[:nsel] if dense is not None else None, "hard": hd[:Ms, :K] if hard else None,
                "info": {"nsel": int(info.nsel), "n_short": int(info.n_short), "n_long": int(info.n_long), "chunks": int(info.chunks),
                         "lanes_per_entry": int(info.lanes_per_entry), "ms_kernel": float(info.ms_kernel)}}


def _family(model):
    if hasattr(model, "kappa") or hasattr(model, "tau"):
        raise TopicModelError("token_topics has no method for fLDA / fCTM models: their phi carries tau (src/fLDA.jl:204-207), a different operator.")
    if hasattr(model, "alef"):
        return "ctpf"
    if hasattr(model, "mu") and hasattr(model, "sigma"):
        return "ctm"
    if hasattr(model, "alpha") and hasattr(model, "Elogtheta"):
        return "lda"
    raise TopicModelError("token_topics needs an LDA, CTM or CTPF model (or its gpu form).")


def token_factors(model):
    """(A, B), K x M and K x V fp64, with phi[:, n] of document d = normalise(eps + A[:, d] * B[:, w_n]) -- update_phi! of the model's family:
    LDA   A = exp(Elogtheta),                                          B = beta               (src/LDA.jl:150-154)
    CTM   A = exp(lambda_d - max_k lambda_d),                          B = beta               (src/CTM.jl:175-178)
    CTPF  A = exp(psi(gimel_d) - log dalet - log bet - column max),    B = exp(psi(alef_w) - column max)   (src/CTPF.jl:327-330)
    The shifts are taken in fp64; they are constant in k and cancel.  A gpu model's host fields are refreshed first (update_host)."""
    fam = _family(model)
    if getattr(model, "handle", None) and hasattr(model, "update_host"):
        model.update_host()
    f = lambda a: np.asarray(a, dtype=np.float64)
    if fam == "lda":
        return np.exp(f(model.Elogtheta)), f(model.beta)
    if fam == "ctm":
        lam = f(model.lam)
        return np.exp(lam - lam.max(axis=0, keepdims=True)), f(model.beta)
    a = digamma(f(model.gimel)) - np.log(f(model.dalet))[:, None] - np.log(f(model.bet))[:, None]
    b = digamma(f(model.alef))
    return np.exp(a - a.max(axis=0, keepdims=True)), np.exp(b - b.max(axis=0, keepdims=True))


class TokenTopics:
    """The selected documents' entries in CSR form (doc_ptr[Ms + 1], terms, counts; entry n of the selection belongs to document
    zero_based_docs[s] for doc_ptr[s] <= n < doc_ptr[s + 1]) with topic[nsel, top] (0-based, best first, -1 past K), prob[nsel, top] (the
    fp32 responsibilities) and hard[Ms, K] (the document's token counts by best topic); info: the library's tmvb_token_topics_info_t."""

    def __init__(self, raw):
        self.doc_ptr, self.terms, self.counts = raw["doc_ptr"], raw["terms"], raw["counts"]
        self.topic, self.prob, self.hard = raw["top_idx"], raw["top_r"], raw["hard"]
        self.zero_based_docs = raw["docs"]
        self.info = raw["info"]

    def __repr__(self):
        return f"TokenTopics(docs={len(self.zero_based_docs)}, entries={len(self.terms)}, top={self.topic.shape[1]})"


def _zero_based(docs, M):
    if docs is None:
        return None
    d = np.asarray(list(docs) if not isinstance(docs, np.ndarray) else docs)
    if d.ndim != 1 or (d.size and not np.issubdtype(d.dtype, np.integer)):
        raise ValueError("docs must be a list of 1-based document indices.")
    if d.size and (d.min() < 1 or d.max() > M):
        raise CorpusError("document index outside corpus range.")
    return d.astype(np.int64) - 1


def _folded_in(model, corp, iter, tol, device_id):
    """the model's family's own predict on a new corpus"""
    pc = _packed(corp)
    if pc.V != model.V:
        raise CorpusError("predict corpus and train_model corpus must have identical vocabularies.")
    fam = _family(model)
    if fam == "lda":
        from .lda import predict
        return predict(pc, model, iter=iter, tol=tol, device_id=device_id)
    if fam == "ctm":
        from .ctm import predict_ctm
        return predict_ctm(pc, model, iter=iter, tol=tol, device_id=device_id)
    from .ctpf_foldin import predict_ctpf
    return predict_ctpf(pc, model, viter=iter, vtol=tol, device_id=device_id)


def _run(model, docs, top, corp, iter, tol, device_id, phi, hard, select):
    if corp is not None:
        model = _folded_in(model, corp, iter, tol, device_id)
    A, B = token_factors(model)
    z = _zero_based(docs, model.M)
    with call_context(device_id) as ctx:
        rc, raw = token_topics_raw(ctx, model.K, model.V, A, B, model.corp, docs=z, top=top, phi=phi, hard=hard, select=select)
    check(rc)
    return raw


def token_topics(model, docs=None, top: int = 1, corp=None, iter: int = 10, tol=None, device_id: int = 0) -> TokenTopics:
    """For every entry of the documents `docs` (1-based indices, repeats and any order allowed; None: all) of the model's corpus the `top`
    <= 8 topics with the largest responsibility, best first (equal responsibilities: the lower topic first), and per document the token
    counts by best topic.  corp: a new corpus instead, folded in first with the family's own predict (predict, predict_ctm, predict_ctpf
    with iter / tol); a differing vocabulary raises CorpusError.  LDA, CTM, CTPF and their gpu forms; fLDA / fCTM raise TopicModelError."""
    if not (isinstance(top, (int, np.integer)) and 1 <= top <= TOP_MAX):
        raise ValueError(f"top must be an integer in [1, {TOP_MAX}].")
    return TokenTopics(_run(model, docs, int(top), corp, iter, tol, device_id, False, True, True))


def phi(model, d, device_id: int = 0):
    """phi of document d (1-based) as the reference keeps it in gpumodel.phi[d]: K x N_d float32, column n the responsibilities of the
    document's n-th entry.  A list / range of indices returns a list."""
    one = isinstance(d, (int, np.integer))
    raw = _run(model, [int(d)] if one else d, 1, None, 10, None, device_id, True, False, False)
    out = [np.ascontiguousarray(raw["phi"][raw["doc_ptr"][s]:raw["doc_ptr"][s + 1]].T) for s in range(len(raw["docs"]))]
    return out[0] if one else out
