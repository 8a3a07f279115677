"""
NumPy fp64 restatement of the CTPF fold-in of users (include/tmvb.h, "CTPF fold-in"), in its DIRECT form: per library
entry the 2K-row softmax of update_xi! (src/CTPF.jl:334-337), then xi_a + xi_b, then h_new = e + sum_d r_du (xi_a + xi_b)[:, d] -- the table W of
the device path does not occur here, so the two are independent formulations.  The exit rule and the sweep count are those of the document loop
(src/CTPF.jl:354-361) with he in the place of gimel.  Also: the states and libraries the fold-in tests share, computed once.
"""
import numpy as np


class State:
    """the frozen side of a CTPF state: gimel, zayin (K x M), dalet, het, vav (K), the hyperparameter e"""

    def __init__(self, gimel, zayin, dalet, het, vav, e=0.1):
        self.gimel, self.zayin = np.asarray(gimel, dtype=np.float64), np.asarray(zayin, dtype=np.float64)
        self.dalet, self.het, self.vav = (np.asarray(x, dtype=np.float64) for x in (dalet, het, vav))
        self.e = float(e)
        self.K, self.M = self.gimel.shape


def foldin_direct(digamma, st, lib_ptr, lib_docs, lib_ratings, he0=None, viter=10, vtol=None, sweeps=None, norms=None):
    """(he K x Un, sweeps[Un]).  lib_docs 0-based.  sweeps: an optional per-user override -- user u runs exactly sweeps[u] sweeps (viter = n_u,
    vtol = 0).  norms: an optional list that receives, per user, the exit norms of the sweeps it ran."""
    K = st.K
    Un = len(lib_ptr) - 1
    vtol = 1.0 / K ** 2 if vtol is None else vtol
    he = np.empty((K, Un), order="F")
    sw = np.zeros(Un, dtype=np.int32)
    lda, lhe, lva = np.log(st.dalet), np.log(st.het), np.log(st.vav)
    for u in range(Un):
        docs = np.asarray(lib_docs[lib_ptr[u]:lib_ptr[u + 1]], dtype=np.int64)
        r = np.asarray(lib_ratings[lib_ptr[u]:lib_ptr[u + 1]], dtype=np.float64)
        h = np.ones(K) if he0 is None else np.array(he0[:, u], dtype=np.float64)
        nv, tol = (viter, vtol) if sweeps is None else (int(sweeps[u]), 0.0)
        a = digamma(st.gimel[:, docs]) - lda[:, None] - lva[:, None]          # K x R: the halves of the softmax argument that do not move
        b = digamma(st.zayin[:, docs]) - lhe[:, None] - lva[:, None]
        seen = []
        for _ in range(nv):
            t = digamma(h)
            x = np.vstack([a + t[:, None], b + t[:, None]])                    # 2K x R
            x = np.exp(x - x.max(axis=0, keepdims=True)) if x.shape[1] else x  # additive_logistic(., dims=1)
            xi = x / x.sum(axis=0, keepdims=True) if x.shape[1] else x
            hn = st.e + (xi[:K] + xi[K:]) @ r
            nrm = float(np.linalg.norm(hn - h))
            h = hn
            sw[u] += 1
            seen.append(nrm)
            if nrm < tol:
                break
        he[:, u] = h
        if norms is not None:
            norms.append(seen)
    return he, sw


def transposed_libraries(rdr_ptr, readers, ratings, U):
    """the users' libraries of a corpus: (ptr[U + 1], docs 0-based ascending, ratings)"""
    rdr_ptr = np.asarray(rdr_ptr, dtype=np.int64); readers = np.asarray(readers, dtype=np.int64)
    docs = np.repeat(np.arange(len(rdr_ptr) - 1, dtype=np.int64), np.diff(rdr_ptr))
    order = np.lexsort((docs, readers))
    ptr = np.concatenate([[0], np.cumsum(np.bincount(readers, minlength=U))]).astype(np.int64)
    return ptr, docs[order].astype(np.int32), np.asarray(ratings)[order].astype(np.int32)


_CACHE = {}


def trained_oracle(tmvb, oracle, K, iters=5, seed=4):
    """(oracle model after `iters` estep + mstep from synth_case of tests/test_ctpf_gpu.py, its corpus dict, the users' libraries); computed once
    per (K, iters, seed) and shared: callers do not modify it"""
    key = (K, iters, seed)
    if key not in _CACHE:
        from test_ctpf_gpu import synth_case
        g = synth_case(tmvb, K, seed=seed)
        om = oracle.CTPF(oracle.CSR(g["doc_ptr"], g["terms"], g["counts"], g["V"], g["rdr_ptr"], g["readers"], g["ratings"], g["U"]), K, g["alef0"])
        for _ in range(iters):
            om.estep(); om.mstep()
        _CACHE[key] = (om, g, transposed_libraries(g["rdr_ptr"], g["readers"], g["ratings"], g["U"]))
    return _CACHE[key]


def state_of(om):
    return State(om.gimel.copy(), om.zayin.copy(), om.dalet.copy(), om.het.copy(), om.vav.copy(), 0.1)


def straddlers(norms, vtol, band=0.002):
    """users with an exit norm within +-band of vtol in fp64: the users whose fp32 exit may fall one sweep earlier or later"""
    return [u for u, s in enumerate(norms) if any(abs(n - vtol) <= band * vtol for n in s)]
