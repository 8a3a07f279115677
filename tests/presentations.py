"""
One corpus, seven presentations (a helper module of tests/test_corpus_presentations*.py: no fixtures, no test).

tmvb_corpus_create takes any CSR that passes check_doc / check_corp: ids in any order inside a document, ids repeated inside a document
(quirk Q1, SURVEY.md: the engine accumulates repeats, so a document means what its condensed form means), documents and ids in any order.  Every
other corpus of the suite is sorted, condensed and in generation order.  canonical() draws one such corpus with the shapes that matter to the
kernels and the host builders, present() re-presents it:

  P0  canonical
  P1  the entries of every document shuffled
  P2  the entries of every document descending
  P3  documents permuted: the empty and the two longest go last, the rest (equal lengths among them) at random
  P4  vocabulary (and users) relabelled by a random permutation
  P5  un-condensed: every entry with count >= 2 is split with probability 1/2 into two or three entries of the same id whose counts add up
      (reader entries with rating >= 2 likewise), then the document is shuffled; the one-entry count-7 document becomes three entries of one id
  P6  P5 o P4 o P3

A Presentation carries the maps that take results back: doc_of[i] = canonical document held at position i, term_to[j] = presented id of
canonical id j (user_to likewise), entry_of[q] = canonical entry behind presented entry q (rentry_of for reader entries).
"""
import types

import numpy as np
from scipy.special import gammaln

CHUNK = 256                         # TMVB_CHUNK (csrc/tmvb_internal.h): postings per partial-sum slot of the statistics pass
M_DEFAULT, V_DEFAULT = 320, 1000
SEED = 11                           # canonical seed of the GPU tests
P5_SEED = {}                        # filled below: per (seed, U) the presentation seed at which P5 straddles a chunk boundary
NAMES = ("P0", "P1", "P2", "P3", "P4", "P5", "P6")


class Presentation:
    def __init__(self, name, M, V, U, docs, doc_of, term_to, user_to, info):
        """docs[i] = (terms, counts, entry_of, readers, ratings, rentry_of), entry_of / rentry_of indexing the canonical flat arrays"""
        self.name, self.M, self.V, self.U, self.docs, self.info = name, M, V, U, docs, info
        self.doc_of = np.asarray(doc_of, dtype=np.int64)
        self.term_to = np.asarray(term_to, dtype=np.int64)
        self.user_to = np.asarray(user_to, dtype=np.int64)
        cat = lambda k, dt: np.concatenate([d[k] for d in docs]).astype(dt) if docs else np.zeros(0, dt)
        self.doc_ptr = np.concatenate([[0], np.cumsum([len(d[0]) for d in docs])]).astype(np.int64)
        self.terms, self.counts, self.entry_of = cat(0, np.int32), cat(1, np.int32), cat(2, np.int64)
        self.rdr_ptr = np.concatenate([[0], np.cumsum([len(d[3]) for d in docs])]).astype(np.int64)
        self.readers, self.ratings, self.rentry_of = cat(3, np.int32), cat(4, np.int32), cat(5, np.int64)

    # ---- what the tests need of it
    @property
    def canon(self):
        return self.info["canon"]

    @property
    def pos_of(self):
        """pos_of[d] = position of canonical document d"""
        p = np.empty(self.M, dtype=np.int64); p[self.doc_of] = np.arange(self.M)
        return p

    def case(self, **extra):
        """the dict the make_pair() of the model test files takes"""
        g = dict(V=self.V, doc_ptr=self.doc_ptr, terms=self.terms, counts=self.counts)
        if self.U:
            g.update(U=self.U, rdr_ptr=self.rdr_ptr, readers=self.readers, ratings=self.ratings)
        g.update(extra)
        return g

    def doc_lists(self, readers=False):
        """documents as oracle/oracle_np.py takes them"""
        return [((d[0], d[1], d[3], d[4]) if readers else (d[0], d[1])) for d in self.docs]

    def cols(self, a):
        """K x V of the canonical corpus -> as this presentation labels the vocabulary (and back: uncols)"""
        out = np.empty_like(np.asarray(a)); out[..., self.term_to] = a
        return out

    def uncols(self, a):
        return np.asarray(a)[..., self.term_to]

    def ucols(self, a):
        out = np.empty_like(np.asarray(a)); out[..., self.user_to] = a
        return out

    def unucols(self, a):
        return np.asarray(a)[..., self.user_to]

    def docs_fwd(self, a):
        """K x M (or M) in canonical document order -> in presented order (and back: docs_back)"""
        return np.asarray(a)[..., self.doc_of]

    def docs_back(self, a):
        return np.asarray(a)[..., self.pos_of]

    def entries_fwd(self, a):
        """a per-entry quantity that does not depend on the count (tau) in canonical entry order -> presented entry order"""
        return np.asarray(a)[self.entry_of]

    def condensed(self):
        """back to the canonical labelling, document order and condensed sorted form: (doc_ptr, terms, counts, rdr_ptr, readers, ratings)"""
        back_t = np.empty(max(self.V, 1), dtype=np.int64); back_t[self.term_to] = np.arange(self.V)
        back_u = np.empty(max(self.U, 1), dtype=np.int64)
        if self.U:
            back_u[self.user_to] = np.arange(self.U)
        T, Cn, R, Q = [], [], [], []
        for d in range(self.M):
            t, c, _, r, q, _ = self.docs[self.pos_of[d]]
            for ids, val, back, I, W in ((t, c, back_t, T, Cn), (r, q, back_u, R, Q)):
                u, inv = np.unique(back[np.asarray(ids, dtype=np.int64)], return_inverse=True)
                w = np.zeros(len(u), dtype=np.int64); np.add.at(w, inv, val)
                I.append(u); W.append(w)
        ptr = lambda L: np.concatenate([[0], np.cumsum([len(x) for x in L])]).astype(np.int64)
        cat = lambda L: np.concatenate(L).astype(np.int32) if L else np.zeros(0, np.int32)
        return ptr(T), cat(T), cat(Cn), ptr(R), cat(R), cat(Q)

    def numpy_info(self):
        """tmvb_corpus_info restated on the presented CSR"""
        dup = lambda ptr, ids: int(sum(len(np.unique(ids[ptr[d]:ptr[d + 1]])) < ptr[d + 1] - ptr[d] for d in range(self.M)))
        return dict(M=self.M, V=self.V, U=self.U, nnz=int(self.doc_ptr[-1]), nR=int(self.rdr_ptr[-1]),
                    max_doc_len=int(np.diff(self.doc_ptr).max(initial=0)), max_readers=int(np.diff(self.rdr_ptr).max(initial=0)),
                    n_empty_docs=int((np.diff(self.doc_ptr) == 0).sum()), sum_counts=int(self.counts.sum(dtype=np.int64)),
                    sum_ratings=int(self.ratings.sum(dtype=np.int64)), n_docs_with_duplicate_terms=dup(self.doc_ptr, self.terms),
                    n_docs_with_duplicate_readers=dup(self.rdr_ptr, self.readers))

    def postings(self, j, readers=False):
        """the posting list of id j in the order tmvb_build_inv_index gives it (a counting sort of the CSR: id-major, then document order, then
        entry order): (document position, entry index) per posting"""
        ptr, ids = (self.rdr_ptr, self.readers) if readers else (self.doc_ptr, self.terms)
        q = np.flatnonzero(ids == j)                                   # flat CSR order = document order, then entry order
        return np.searchsorted(ptr, q, side="right") - 1, q


def canonical(seed=SEED, M=M_DEFAULT, V=V_DEFAULT, U=0, cover=False):
    """The condensed, sorted corpus (a Presentation named P0 with identity maps).  At the default size: one empty document, a one-entry document of
    count 1 and one of count 7, two long documents of 300 and 700 unique terms (0.3 V and 0.7 V at other sizes), two hot ids -- each in every
    non-empty document but one of the two one-entry documents, which hold one hot id each: M - 2 postings, two chunks of the statistics pass at
    M = 320 --, the rest 2 - 90 entries with counts 1 - 5, 5 % of the ids unused.  cover=True appends the document that holds every unused id once
    (CTM / fCTM have no epsilon under their logarithm: every term must occur).  U > 0: readers with ratings 1 - 4, one hot reader in every
    document that has readers, a fifth of the documents without readers."""
    rng = np.random.default_rng(seed)
    ids = rng.permutation(V)
    n_unused = max(1, V // 20)
    unused, hot, pool = np.sort(ids[:n_unused]), ids[n_unused:n_unused + 2], ids[n_unused + 2:]
    special = dict(empty=M // 3, one=5 % M, seven=M // 2, long_a=17 % M, long_b=M - M // 8)
    assert len(set(special.values())) == 5
    kind = {v: k for k, v in special.items()}
    n_long = dict(long_a=(3 * V) // 10, long_b=(7 * V) // 10)
    hot_reader = int(rng.integers(U)) if U else -1
    docs = []
    for d in range(M):
        k = kind.get(d)
        if k == "empty":
            t, c = np.zeros(0, np.int64), np.zeros(0, np.int64)
        elif k == "one":
            t, c = hot[:1].copy(), np.array([1])
        elif k == "seven":
            t, c = hot[1:].copy(), np.array([7])
        else:
            n = n_long[k] if k else int(rng.integers(2, min(90, len(pool) // 2) + 1))
            t = np.sort(np.concatenate([hot, rng.choice(pool, size=n - 2, replace=False)]))
            c = rng.integers(1, 6, size=n)
            c[np.isin(t, hot)] = rng.integers(2, 6, size=2)             # the hot ids can always be split
        r, q = np.zeros(0, np.int64), np.zeros(0, np.int64)
        if U and d % 8 != 2:
            nr = int(rng.integers(1, min(40, U) + 1)) if k != "long_b" else min(U, 70)
            r = np.sort(np.unique(np.concatenate([[hot_reader], rng.choice(U, size=nr - 1, replace=False)]))) if nr > 1 else np.array([hot_reader])
            q = rng.integers(1, 5, size=len(r))
        docs.append([t, c, None, r, q, None])
    if cover:
        docs.append([unused.copy(), np.ones(n_unused, np.int64), None, np.zeros(0, np.int64), np.zeros(0, np.int64), None])
    a = b = 0
    for doc in docs:
        doc[2] = np.arange(a, a + len(doc[0])); a += len(doc[0])
        doc[5] = np.arange(b, b + len(doc[3])); b += len(doc[3])
    info = dict(special=special, hot=[int(h) for h in hot], hot_reader=hot_reader, unused=unused, cover=cover, seed=seed)
    info["canon"] = Presentation("P0", len(docs), V, U, [tuple(x) for x in docs], np.arange(len(docs)), np.arange(V), np.arange(U), info)
    return info["canon"]


def _take(doc, o, ro):
    return (doc[0][o], doc[1][o], doc[2][o], doc[3][ro], doc[4][ro], doc[5][ro])


def shuffled(p, rng, name="P1"):
    docs = [_take(d, rng.permutation(len(d[0])), rng.permutation(len(d[3]))) for d in p.docs]
    return Presentation(name, p.M, p.V, p.U, docs, p.doc_of, p.term_to, p.user_to, p.info)


def descending(p, name="P2"):
    docs = [_take(d, np.argsort(-d[0], kind="stable"), np.argsort(-d[3], kind="stable")) for d in p.docs]
    return Presentation(name, p.M, p.V, p.U, docs, p.doc_of, p.term_to, p.user_to, p.info)


def docs_permuted(p, rng, name="P3"):
    """the empty and the two longest documents last (with them the head of the longest-first processing order moves to the end of the corpus), the
    others at random: documents of equal length swap places, which the stable longest-first sort keeps"""
    sp = p.info["special"]
    last = [int(np.flatnonzero(p.doc_of == sp[k])[0]) for k in ("empty", "long_a", "long_b")]
    rest = np.array([i for i in range(p.M) if i not in last])
    order = np.concatenate([rng.permutation(rest), last]).astype(np.int64)
    return Presentation(name, p.M, p.V, p.U, [p.docs[i] for i in order], p.doc_of[order], p.term_to, p.user_to, p.info)


def relabelled(p, rng, name="P4"):
    tp, up = rng.permutation(p.V), rng.permutation(p.U)
    docs = [(tp[d[0]], d[1], d[2], up[d[3]] if p.U else d[3], d[4], d[5]) for d in p.docs]
    return Presentation(name, p.M, p.V, p.U, docs, p.doc_of, tp[p.term_to], up[p.user_to] if p.U else p.user_to, p.info)


def _split(ids, vals, emap, rng, force3):
    I, W, E = [], [], []
    for j, c, e in zip(ids, vals, emap):
        parts = [int(c)]
        if force3 or (c >= 2 and rng.random() < 0.5):
            n = 3 if force3 else (2 if c == 2 else int(rng.integers(2, 4)))
            cuts = np.sort(rng.choice(np.arange(1, c), size=n - 1, replace=False))
            parts = np.diff(np.concatenate([[0], cuts, [c]])).tolist()
        I += [j] * len(parts); W += parts; E += [e] * len(parts)
    o = rng.permutation(len(I))
    return np.asarray(I, np.int64)[o], np.asarray(W, np.int64)[o], np.asarray(E, np.int64)[o]


def uncondensed(p, rng, name="P5"):
    seven = p.info["special"]["seven"]
    docs = []
    for i, d in enumerate(p.docs):
        t, c, e = _split(d[0], d[1], d[2], rng, force3=(p.doc_of[i] == seven))
        r, q, re = _split(d[3], d[4], d[5], rng, force3=False)
        docs.append((t, c, e, r, q, re))
    return Presentation(name, p.M, p.V, p.U, docs, p.doc_of, p.term_to, p.user_to, p.info)


def straddle(p):
    """(hot id, document position) such that two entries of that document are postings CHUNK - 1 and CHUNK of the id -- one document in two partial-sum
    slots of termstats_multi_kernel -- or None"""
    for h in p.info["hot"]:
        doc, _ = p.postings(p.term_to[h])
        if len(doc) > CHUNK and doc[CHUNK - 1] == doc[CHUNK]:
            return int(h), int(doc[CHUNK])
    return None


def p5_seed(canon):
    """the first presentation seed at which P5 has the straddle (searched once per canonical corpus; the GPU tests assert the straddle itself)"""
    key = (canon.info["seed"], canon.M, canon.V, canon.U, canon.info["cover"])
    if canon.M < M_DEFAULT:                                            # a small corpus (the pure-Python oracle's): no id has CHUNK postings
        return 1000
    if key not in P5_SEED:
        for s in range(200):
            if straddle(uncondensed(canon, np.random.default_rng(1000 + s))) is not None:
                P5_SEED[key] = 1000 + s
                break
        else:
            raise AssertionError("no presentation seed gives P5 a posting-chunk straddle")
    return P5_SEED[key]


def present(canon, name):
    """presentation `name` of the canonical corpus"""
    if name == "P0":
        return canon
    if name == "P1":
        return shuffled(canon, np.random.default_rng(101))
    if name == "P2":
        return descending(canon)
    if name == "P3":
        return docs_permuted(canon, np.random.default_rng(103))
    if name == "P4":
        return relabelled(canon, np.random.default_rng(104))
    if name == "P5":
        p = uncondensed(canon, np.random.default_rng(p5_seed(canon)))
        if canon.M >= M_DEFAULT:
            assert straddle(p) is not None
        return p
    if name == "P6":
        p = relabelled(docs_permuted(canon, np.random.default_rng(103)), np.random.default_rng(104))
        return uncondensed(p, np.random.default_rng(106), name="P6")
    raise KeyError(name)


# ------------------------------------------------------------------------------------------------ oracle states across presentations
# the state fields of the five models (the names oracle/oracle.py and the device wrappers share) and what each is indexed by
FIELDS = {
    "lda": ("alpha", "beta", "beta_old", "gamma", "Elogtheta", "Elogtheta_old"),
    "ctm": ("mu", "sigma", "invsigma", "beta", "beta_old", "lam", "lam_old", "vsq", "logzeta"),
    "ctpf": ("alef", "alef_old", "he", "he_old", "bet", "bet_old", "vav", "vav_old", "dalet", "dalet_old", "het", "het_old", "gimel", "gimel_old", "zayin", "zayin_old"),
    "flda": ("eta", "alpha", "kappa", "kappa_old", "beta", "beta_old", "gamma", "Elogtheta", "Elogtheta_old", "tau", "tau_old"),
    "fctm": ("eta", "mu", "sigma", "invsigma", "kappa", "kappa_old", "beta", "beta_old", "lam", "lam_old", "vsq", "logzeta", "tau", "tau_old"),
}
KIND = dict(alpha="plain", eta="plain", mu="plain", sigma="plain", invsigma="plain", bet="plain", vav="plain", dalet="plain", het="plain",
            bet_old="plain", vav_old="plain", dalet_old="plain", het_old="plain",
            beta="vocab", beta_old="vocab", kappa="vocab", kappa_old="vocab", alef="vocab", alef_old="vocab", he="user", he_old="user",
            gamma="doc", Elogtheta="doc", Elogtheta_old="doc", lam="doc", lam_old="doc", vsq="doc", logzeta="doc", gimel="doc", gimel_old="doc",
            zayin="doc", zayin_old="doc", sw="doc", tau="entry", tau_old="entry")


def snapshot(om, names, **extra):
    s = {n: np.array(getattr(om, n), copy=True, order="F") if isinstance(getattr(om, n), np.ndarray) else getattr(om, n) for n in names}
    s.update(extra)
    return s


def view(s, p):
    """an oracle state in the labelling and order of presentation p: what force() takes and what the device is compared with"""
    o = types.SimpleNamespace()
    for n, v in s.items():
        k = KIND.get(n, "plain")
        v = p.cols(v) if k == "vocab" else p.ucols(v) if k == "user" else p.docs_fwd(v) if k == "doc" else p.entries_fwd(v) if k == "entry" else v
        setattr(o, n, np.asfortranarray(v) if isinstance(v, np.ndarray) and v.ndim == 2 else v)
    return o


def restore(om, s):
    for n, v in s.items():
        if n in KIND:
            setattr(om, n, np.array(v, copy=True, order="F") if isinstance(v, np.ndarray) else v)


def ctpf_elbo_shift(p):
    """what update_elbo! of a CTPF gains when entries are split (tests/test_corpus_presentations_gpu.py): sum over the canonical entries of
    lgamma(c + 1) - sum over its parts of lgamma(c_part + 1), term and reader entries"""
    c = p.canon
    out = 0.0
    for val, src, val0 in ((p.counts, p.entry_of, c.counts), (p.ratings, p.rentry_of, c.ratings)):
        out += float((gammaln(val0 + 1.0) - np.bincount(src, weights=gammaln(val + 1.0), minlength=len(val0))).sum())       # 0.0 exactly where nothing is split
        assert np.array_equal(np.bincount(src, weights=val, minlength=len(val0)), val0)
    return float(out)


