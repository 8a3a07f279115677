"""
Document partitions of the canonical corpus of tests/presentations.py for the sharded tests (a helper module of tests/test_shard_cuts.py and
tests/test_sharded_oracle_gpu.py: no fixtures, no test).

A partition is a list of cuts 0 = c_0 <= ... <= c_W = M: rank r holds the documents [c_r, c_{r+1}) of a presentation of the corpus.

  even2, even3, even8   PackedCorpus.shard_bounds(W) of the canonical presentation: what a sharded host asks for, near-even in nnz + nR
  ragged6               what shard_bounds gives at many ranks on a small corpus or beside one very long document, all at once:
                          rank 0  a third of the ordinary documents
                          rank 1  NO document (between two ranks that have some)
                          rank 2  only the corpus's empty document (M = 1, nnz = 0; it has no readers either)
                          rank 3  only the 700-term document
                          rank 4  only the one-entry document of count 1
                          rank 5  the rest
                        The canonical order holds those three documents far apart, so ragged6 lives on a presentation of its own: documents permuted
                        (kind P3) with the three side by side behind the first third of the others; the oracle's states are viewed through it
                        (presentations.view) like through any other presentation.
"""
import numpy as np

import presentations as P

NAMES = ("even2", "even3", "even8", "ragged6")
RAGGED_ROLES = ("third", "none", "empty_doc", "long_doc", "one_entry", "rest")


def packed(tmvb, p):
    """the presentation as the engine's PackedCorpus"""
    if p.U:
        return tmvb.PackedCorpus(p.doc_ptr, p.terms, p.counts, p.V, p.rdr_ptr, p.readers, p.ratings, p.U)
    return tmvb.PackedCorpus(p.doc_ptr, p.terms, p.counts, p.V)


def ragged_presentation(canon):
    """(presentation, position of the first of the three isolated documents)"""
    sp = canon.info["special"]
    trio = [sp["empty"], sp["long_b"], sp["one"]]
    rest = [d for d in range(canon.M) if d not in trio]
    a = len(rest) // 3
    order = np.array(rest[:a] + trio + rest[a:], dtype=np.int64)
    p = P.Presentation("P3", canon.M, canon.V, canon.U, [canon.docs[i] for i in order], canon.doc_of[order], canon.term_to, canon.user_to, canon.info)
    return p, a


def check_cuts(p, cuts, W):
    """the cuts cover [0, M) without overlap, in W ranks"""
    assert len(cuts) == W + 1 and cuts[0] == 0 and cuts[-1] == p.M, cuts
    assert all(0 <= cuts[r] <= cuts[r + 1] <= p.M for r in range(W)), cuts
    seen = np.concatenate([np.arange(cuts[r], cuts[r + 1]) for r in range(W)])
    assert np.array_equal(seen, np.arange(p.M))


def check_ragged(p, cuts):
    """the five properties of ragged6, on the presentation it was built on"""
    sp = p.canon.info["special"]
    n = np.diff(cuts)
    nnz = [int(p.doc_ptr[cuts[r + 1]] - p.doc_ptr[cuts[r]]) for r in range(6)]
    nr = [int(p.rdr_ptr[cuts[r + 1]] - p.rdr_ptr[cuts[r]]) for r in range(6)]
    assert n[1] == 0 and n[0] > 0 and n[2] > 0                                     # no document at all, between two ranks that have some
    assert n[2] == 1 and p.doc_of[cuts[2]] == sp["empty"] and nnz[2] == 0 and nr[2] == 0
    assert n[3] == 1 and p.doc_of[cuts[3]] == sp["long_b"] and nnz[3] == (7 * p.V) // 10
    assert n[4] == 1 and p.doc_of[cuts[4]] == sp["one"] and nnz[4] == 1 and p.counts[p.doc_ptr[cuts[4]]] == 1
    assert n[0] > 1 and n[5] > 1 and nnz[0] > 0 and nnz[5] > 0 and n[0] + n[5] == p.M - 3      # two ranks with the rest
    assert n[0] != n[5]


def partition(tmvb, canon, name):
    """(presentation, its PackedCorpus, cuts) of partition `name`; asserts what the partition promises"""
    if name == "ragged6":
        p, a = ragged_presentation(canon)
        cuts = [0, a, a, a + 1, a + 2, a + 3, p.M]
        check_cuts(p, cuts, 6)
        check_ragged(p, cuts)
        return p, packed(tmvb, p), cuts
    W = int(name[len("even"):])
    corpus = packed(tmvb, canon)
    bounds = corpus.shard_bounds(W)
    cuts = [b[0] for b in bounds] + [bounds[-1][1]]
    assert all(bounds[r][1] == bounds[r + 1][0] for r in range(W - 1)), bounds
    check_cuts(canon, cuts, W)
    return canon, corpus, cuts
