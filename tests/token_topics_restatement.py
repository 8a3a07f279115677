"""
NumPy restatement of tmvb_token_topics (include/tmvb.h, "word-topic assignments"), in fp64 from the definition:

    y_k = eps + A[k, d] B[k, w],    r_k = y_k / sum_j y_j

for every entry (term w) of the selected documents, in docs order; top-t by lexsort on (-r, k); hard[s, k] = sum of the counts of the entries
of selected document s whose best topic is k.

cap(K) = (K + 12) 2^-24 bounds |r - r64| / r64 of the device's fp32 arithmetic (u = 2^-24), to first order:
    y_k:   two input roundings, the product, the add of eps and the underflow term (an underflowing product moves y_k by at most 2^-26
           relative when eps >= 2^-100)                                                    <= 4 1/4 u
    the same again through the sum of positives (a weighted mean of the y_j's errors)      <= 4 1/4 u
    the sum of K positives in any order                                                    <= (K - 1) u
    a division or a reciprocal-multiply                                                    <= 3 u
    total (K + 10 1/2) u < (K + 12) u.
A NumPy emulation of the fp32 arithmetic measured at most 0.37 x that cap (sequential and permuted sums, flushed and kept denormals,
factors with exact zeros, products down to e^-150, K in {1, 3, 5, 17, 50, 65, 130, 1024}, eps = EPSILON and 2^-100; worst 21 u at
K = 1024).  Every r64 is positive because eps > 0: the bound is purely relative and no case needs leaving out.
"""
import numpy as np

EPSILON = 1.5777218104420236e-30
U = 2.0 ** -24


def cap(K):
    return (K + 12) * U


def selected(doc_ptr, docs):
    """indices into the CSR of the selected documents' entries in docs order, and the selection's own doc_ptr"""
    doc_ptr = np.asarray(doc_ptr, dtype=np.int64)
    docs = np.arange(len(doc_ptr) - 1) if docs is None else np.asarray(docs, dtype=np.int64)
    take = np.concatenate([np.arange(doc_ptr[d], doc_ptr[d + 1]) for d in docs] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    ptr = np.concatenate([[0], np.cumsum(doc_ptr[docs + 1] - doc_ptr[docs])]).astype(np.int64)
    return take, ptr, docs


def responsibilities(A, B, doc_ptr, terms, docs=None, eps=EPSILON, rounded=True):
    """r64[nsel, K]; rounded: A, B and eps rounded once to fp32 first, as the library does on upload"""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    if rounded:
        A, B, eps = A.astype(np.float32).astype(np.float64), B.astype(np.float32).astype(np.float64), float(np.float32(eps))
    take, ptr, docs = selected(doc_ptr, docs)
    doc_of = np.repeat(docs, np.diff(ptr))
    y = eps + A[:, doc_of].T * B[:, np.asarray(terms)[take]].T
    return y / y.sum(axis=1, keepdims=True)


def top_t(r, t):
    """(idx[n, t], val[n, t]) under (r descending, topic ascending); slots past K hold -1 and 0.  r of any float type: ties are ties of its bits"""
    n, K = r.shape
    idx = np.full((n, t), -1, dtype=np.int32)
    val = np.zeros((n, t), dtype=r.dtype)
    if n == 0:
        return idx, val
    ks = np.broadcast_to(np.arange(K), r.shape)
    order = np.lexsort((ks, -r.astype(np.float64)), axis=1)[:, :t]
    m = min(t, K)
    idx[:, :m] = order[:, :m]
    val[:, :m] = np.take_along_axis(r, order[:, :m], axis=1)
    return idx, val


def hard_counts(best, counts, ptr, K):
    """hard[Ms, K] from the best topic of every selected entry"""
    Ms = len(ptr) - 1
    out = np.zeros((Ms, K), dtype=np.int64)
    for s in range(Ms):
        np.add.at(out[s], best[ptr[s]:ptr[s + 1]], counts[ptr[s]:ptr[s + 1]])
    return out


def restate(A, B, doc_ptr, terms, counts, docs=None, eps=EPSILON, t=1):
    """dict(r, top_idx, top_r, hard, ptr, take) in fp64"""
    r = responsibilities(A, B, doc_ptr, terms, docs, eps)
    take, ptr, _ = selected(doc_ptr, docs)
    idx, val = top_t(r, t)
    hard = hard_counts(idx[:, 0], np.asarray(counts, dtype=np.int64)[take], ptr, r.shape[1])
    return {"r": r, "top_idx": idx, "top_r": val, "hard": hard, "ptr": ptr, "take": take}
