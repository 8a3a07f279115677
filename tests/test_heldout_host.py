"""
Held-out evaluation (tmvb_corpus_split / tmvb_heldout_loglik, include/tmvb.h), the part that needs no GPU -- and the NumPy oracle of
tests/test_heldout_gpu.py: the reference has no such function, so the yardstick is a restatement written here.

  * a Philox4x32-10 in pure NumPy equals the library's host entry tmvb_philox4x32_10 on 64 fixed (counter, key) pairs;
  * `host_split`, the draw rule of include/tmvb.h restated on that NumPy Philox, holds out the stated share of the occurrences of every
    count class (binomial z-tests, p >= 1e-6 each, 8 assertions; corpus and seed fixed before the first run);
  * every argument error of both entry points comes back with its status and message from a NULL context, valid arguments without a
    device give TMVB_ENODEVICE;
  * the Python structure mirrors the header, the Julia shim binds the entry points, and the tolerance literal of the GPU test lies
    within [1, 10] x its recorded MI355X measurement (profiles/heldout_tolerances_measured.json), the rule of DESIGN section 6.
"""
import ctypes as C
import json
import math
import os
import re
import sys

import numpy as np
import pytest
from scipy import stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

RNG_SPLIT = 5
MASK = np.uint64(0xFFFFFFFF)


# ------------------------------------------------------------------------------------------------------------------ NumPy Philox
def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11): counter uint32 [n, 4], key uint32 [n, 2] -> uint32 [n, 4]."""
    c = [np.asarray(counter)[:, i].astype(np.uint64) for i in range(4)]
    k = [np.asarray(key)[:, i].astype(np.uint64) for i in range(2)]
    M0, M1, W0, W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]                     # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> s32) ^ c[1] ^ k[0], p1 & MASK, (p0 >> s32) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + W0) & MASK, (k[1] + W1) & MASK]
    return np.stack(c, axis=1).astype(np.uint32)


def split_words(seed, docs, draws):
    """tmvb_rng(seed, doc, TMVB_RNG_SPLIT, 0, draw) for arrays of global document indices and draw indices -> uint32 [n, 4]"""
    docs = np.asarray(docs, dtype=np.uint64)
    seed = np.uint64(int(seed) % 2 ** 64)
    n = len(docs)
    ctr = np.stack([docs & MASK, docs >> np.uint64(32), np.full(n, RNG_SPLIT, dtype=np.uint64), np.asarray(draws, dtype=np.uint64)], axis=1)
    key = np.stack([np.full(n, seed & MASK), np.full(n, seed >> np.uint64(32))], axis=1)
    return philox4x32_10(ctr, key)


# ------------------------------------------------------------------------------------------------------------------ host restatement
def host_held_counts(doc_ptr, counts, frac, seed, doc_offset=0):
    """held[j]: how many of entry j's counts[j] occurrences the draw rule holds out"""
    doc_ptr = np.asarray(doc_ptr, dtype=np.int64); counts = np.asarray(counts, dtype=np.int64)
    M = len(doc_ptr) - 1
    if len(counts) == 0:
        return np.zeros(0, dtype=np.int64)
    thr = int(math.floor(frac * 2.0 ** 32))
    cs = np.concatenate([[0], np.cumsum(counts)])
    Cd = cs[doc_ptr[1:]] - cs[doc_ptr[:-1]]
    nblk = (Cd + 3) // 4
    first = np.concatenate([[0], np.cumsum(nblk)])
    doc_of = np.repeat(np.arange(M), nblk)
    blk = np.arange(first[-1]) - first[doc_of]
    words = split_words(seed, doc_of + doc_offset, blk).astype(np.uint64)
    t = blk[:, None] * 4 + np.arange(4)[None, :]
    valid = t < Cd[doc_of][:, None]
    flags = (words < np.uint64(thr) if thr < 2 ** 32 else np.ones_like(words, dtype=bool))[valid]      # row-major: document, then occurrence
    assert len(flags) == cs[-1]
    return np.add.reduceat(flags.astype(np.int64), cs[:-1])                    # counts >= 1: every segment is non-empty


def host_split(doc_ptr, terms, counts, frac, seed, doc_offset=0):
    """The six arrays of tmvb_split_t: (obs_ptr, obs_terms, obs_counts, held_ptr, held_terms, held_counts)."""
    doc_ptr = np.asarray(doc_ptr, dtype=np.int64); terms = np.asarray(terms, dtype=np.int32); counts = np.asarray(counts, dtype=np.int64)
    held = host_held_counts(doc_ptr, counts, frac, seed, doc_offset)
    out = []
    for c in (counts - held, held):
        keep = c > 0
        pos = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)
        out += [pos[doc_ptr], terms[keep], c[keep].astype(np.int32)]
    return tuple(out)


def np_loglik(theta, beta, doc_ptr, terms, counts, laplace_smooth=0.0):
    """(ll[M], tokens[M]) in fp64: ll[d] = sum_n c_n log(sum_k theta[k, d] beta'[k, w_n]), beta' = (beta + s) / (1 + s V)"""
    theta = np.asarray(theta, dtype=np.float64); beta = np.asarray(beta, dtype=np.float64)
    M = len(doc_ptr) - 1
    bs = (beta + laplace_smooth) / (1.0 + laplace_smooth * beta.shape[1])
    doc = np.repeat(np.arange(M), np.diff(doc_ptr))
    p = np.einsum("kn,kn->n", theta[:, doc], bs[:, terms])
    with np.errstate(divide="ignore"):
        lp = counts * np.log(p)
    ll = np.zeros(M)
    np.add.at(ll, doc, lp)
    return ll, np.bincount(doc, weights=counts, minlength=M).astype(np.int64)


def mixed_corpus(M, V, seed, big_count=True, long_doc=0):
    """Document lengths 0, 1, 3, 64, 65 and 700 entries (64 / 65 straddle one trip of a wave at four lanes per entry and the Philox
    blocks of a wave), counts 1 .. 7 with 4 and 5 (occurrences crossing Philox blocks) and, on request, one entry of 5 000 occurrences
    (a long run inside one entry); long_doc > 0 appends one document of that many entries."""
    rng = np.random.Generator(np.random.PCG64(seed))
    lens = rng.choice([0, 1, 3, 64, 65], size=M)
    lens[:6] = [0, 1, 3, 64, 65, 700]
    lens[M // 2] = 700; lens[M - 1] = 0; lens[M - 2] = 65
    if long_doc:
        lens = np.concatenate([lens, [long_doc]])
    doc_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(doc_ptr[-1])
    terms = rng.integers(0, V, size=n).astype(np.int32)
    counts = rng.choice([1, 1, 1, 2, 3, 4, 5, 7], size=n).astype(np.int32)
    if big_count:
        counts[doc_ptr[M - 2] + 17] = 5000
    return doc_ptr, terms, counts


def gamma_stochastic(rows, cols, seed):
    """rows x cols, every row a normalised Gamma(1) draw with every entry > 0"""
    rng = np.random.Generator(np.random.PCG64(seed))
    g = np.maximum(rng.gamma(1.0, size=(rows, cols)), 1e-9)
    return g / g.sum(axis=1, keepdims=True)


# ------------------------------------------------------------------------------------------------------------------ tests
def test_numpy_philox_equals_the_library(tmvb):
    L = tmvb.lib()
    rng = np.random.Generator(np.random.PCG64(20261017))
    ctr = rng.integers(0, 2 ** 32, size=(64, 4), dtype=np.uint64).astype(np.uint32)
    key = rng.integers(0, 2 ** 32, size=(64, 2), dtype=np.uint64).astype(np.uint32)
    ctr[0] = 0; key[0] = 0
    ctr[1] = 0xFFFFFFFF; key[1] = 0xFFFFFFFF
    ctr[2] = [7, 0, RNG_SPLIT, 3]; key[2] = [1234, 0]
    mine = philox4x32_10(ctr, key)
    P = C.POINTER(C.c_uint32)
    for i in range(64):
        out = np.zeros(4, dtype=np.uint32)
        c, k = np.ascontiguousarray(ctr[i]), np.ascontiguousarray(key[i])
        assert L.tmvb_philox4x32_10(c.ctypes.data_as(P), k.ctypes.data_as(P), out.ctypes.data_as(P)) == 0
        assert np.array_equal(out, mine[i]), (i, out, mine[i])
    # Random123's known answers for the all-zero and the all-ones input
    assert [f"{x:08x}" for x in mine[0]] == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    assert [f"{x:08x}" for x in mine[1]] == ["408f276d", "41c83b0e", "a20bc7c6", "6d5451fd"]
    assert np.array_equal(split_words(1234, [7], [3])[0], mine[2])


STAT_SEED = 20261017          # fixed before the first run
Z_LIMIT = stats.norm.isf(0.5e-6)          # two-sided p = 1e-6


def test_host_restatement_holds_out_the_stated_share():
    """M = 2 000, mean C about 40, frac = 0.3: the held share of every count class against Binomial(n, floor(0.3 2^32) / 2^32)."""
    rng = np.random.Generator(np.random.PCG64(STAT_SEED))
    M, V, frac = 2000, 500, 0.3
    lens = rng.poisson(16, size=M)
    doc_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(doc_ptr[-1])
    terms = rng.integers(0, V, size=n).astype(np.int32)
    counts = np.minimum(rng.geometric(0.4, size=n), 40).astype(np.int32)
    assert 30 < counts.sum() / M < 50
    held = host_held_counts(doc_ptr, counts, frac, STAT_SEED)
    assert np.all(held >= 0) and np.all(held <= counts)
    p = math.floor(frac * 2.0 ** 32) / 2.0 ** 32
    classes = [(1, 1), (2, 2), (3, 3), (4, 4), (5, 5), (6, 8), (9, 40)]
    n_assert = 0
    for lo, hi in classes + [(1, 40)]:
        m = (counts >= lo) & (counts <= hi)
        tot, h = int(counts[m].sum()), int(held[m].sum())
        assert tot > 1000
        z = (h - tot * p) / math.sqrt(tot * p * (1 - p))
        n_assert += 1
        assert abs(z) < Z_LIMIT, (lo, hi, tot, h, z)
    assert n_assert <= 10
    # the position inside an entry does not matter either: an entry of count c is Binomial(c, p), so the held counts of the count-4 entries spread
    c4 = held[counts == 4]
    assert set(np.unique(c4)) == {0, 1, 2, 3, 4}
    # the rule's edges and its structure
    assert host_held_counts(doc_ptr, counts, 0.0, 5).sum() == 0
    assert np.array_equal(host_held_counts(doc_ptr, counts, 1.0, 5), counts)
    six = host_split(doc_ptr, terms, counts, frac, STAT_SEED)
    assert six[0][-1] == len(six[1]) == len(six[2]) and six[3][-1] == len(six[4]) == len(six[5])
    assert six[2].sum() + six[5].sum() == counts.sum() and six[2].min() >= 1 and six[5].min() >= 1
    # a slice through doc_offset is the slice of the whole
    a, b = doc_ptr[700], doc_ptr[900]
    part = host_held_counts(doc_ptr[700:901] - a, counts[a:b], frac, STAT_SEED, doc_offset=700)
    assert np.array_equal(part, held[a:b])


EINVAL, ESHAPE, ENODEVICE = 1, 2, 7


def _split_base():
    return dict(M=3, V=6, doc_ptr=[0, 2, 2, 5], terms=[0, 5, 1, 2, 3], counts=[1, 4, 2, 1, 9], frac=0.5, seed=1, doc_offset=0)


def split_error_cases():
    b = _split_base()
    return [
        ("frac negative", dict(b, frac=-0.01), EINVAL, "frac"),
        ("frac above one", dict(b, frac=1.0000001), EINVAL, "frac"),
        ("frac nan", dict(b, frac=float("nan")), EINVAL, "frac"),
        ("frac infinite", dict(b, frac=float("inf")), EINVAL, "frac"),
        ("M zero", dict(b, M=0), EINVAL, "M must be a positive integer"),
        ("M negative", dict(b, M=-3), EINVAL, "M must be a positive integer"),
        ("V zero", dict(b, V=0), EINVAL, "V must be a positive integer"),
        ("doc_offset negative", dict(b, doc_offset=-1), EINVAL, "doc_offset"),
        ("document of 2^31 tokens", dict(b, counts=[1, 4, 2 ** 30, 2 ** 30 - 1, 1]), EINVAL, "tokens"),
        ("doc_ptr does not start at 0", dict(b, doc_ptr=[1, 2, 2, 5]), ESHAPE, "doc_ptr"),
        ("doc_ptr decreases", dict(b, doc_ptr=[0, 3, 2, 5]), ESHAPE, "doc_ptr"),
        ("term equal to V", dict(b, terms=[0, 6, 1, 2, 3]), ESHAPE, "term"),
        ("term negative", dict(b, terms=[0, 5, -1, 2, 3]), ESHAPE, "term"),
        ("count zero", dict(b, counts=[1, 4, 0, 1, 9]), ESHAPE, "count"),
        ("count negative", dict(b, counts=[1, 4, 2, -1, 9]), ESHAPE, "count"),
    ]


def _loglik_base():
    K, V = 3, 6
    return dict(K=K, V=V, theta=np.full((K, 3), 1.0 / K), beta=np.full((K, V), 1.0 / V), doc_ptr=[0, 2, 2, 5], terms=[0, 5, 1, 2, 3],
                counts=[1, 4, 2, 1, 9], laplace_smooth=0.0)


def loglik_error_cases():
    b = _loglik_base()
    K, V = b["K"], b["V"]
    bad_beta = b["beta"].copy(); bad_beta[1, 2] += 0.01
    neg_beta = b["beta"].copy(); neg_beta[0, 0] = -0.1; neg_beta[0, 1] += 0.1 + 1.0 / V
    th_sum = b["theta"].copy(); th_sum[0, 1] += 1e-5
    th_neg = b["theta"].copy(); th_neg[:, 2] = [-0.5, 1.0, 0.5]
    th_nan = b["theta"].copy(); th_nan[1, 0] = float("nan")
    return [
        ("K zero", dict(b, K=0, theta=np.zeros((0, 3)), beta=np.zeros((0, V))), EINVAL, "K = 0"),
        ("K above 1024", dict(b, K=1025, theta=np.full((1025, 3), 1 / 1025), beta=np.full((1025, V), 1.0 / V)), EINVAL, "K = 1025"),
        ("laplace_smooth negative", dict(b, laplace_smooth=-1e-3), EINVAL, "laplace_smooth parameter must be nonnegative."),
        ("laplace_smooth nan", dict(b, laplace_smooth=float("nan")), EINVAL, "laplace_smooth parameter must be nonnegative."),
        ("beta row does not sum to one", dict(b, beta=bad_beta), ESHAPE, "beta must be a right stochastic matrix."),
        ("beta negative entry", dict(b, beta=neg_beta), ESHAPE, "beta must be a right stochastic matrix."),
        ("theta column sums to 1 + 1e-5", dict(b, theta=th_sum), ESHAPE, "θ not a probability vector"),
        ("theta negative entry", dict(b, theta=th_neg), ESHAPE, "θ not a probability vector"),
        ("theta nan", dict(b, theta=th_nan), ESHAPE, "θ not a probability vector"),
        ("doc_ptr does not start at 0", dict(b, doc_ptr=[1, 2, 2, 5]), ESHAPE, "doc_ptr"),
        ("doc_ptr decreases", dict(b, doc_ptr=[0, 3, 2, 5]), ESHAPE, "doc_ptr"),
        ("term equal to V", dict(b, terms=[0, 6, 1, 2, 3]), ESHAPE, "term"),
        ("count zero", dict(b, counts=[1, 4, 0, 1, 9]), ESHAPE, "count"),
    ]


class _CSR:
    def __init__(self, doc_ptr, terms, counts):
        self.doc_ptr, self.terms, self.counts = doc_ptr, terms, counts


def call_split(tmvb, ctx, kw):
    kw = dict(kw)
    return tmvb.split_corpus_raw(ctx, kw.pop("M"), kw.pop("V"), kw.pop("doc_ptr"), kw.pop("terms"), kw.pop("counts"), **kw)


def call_loglik(tmvb, ctx, kw):
    return tmvb.heldout_loglik_raw(ctx, kw["K"], kw["V"], kw["theta"], kw["beta"], _CSR(kw["doc_ptr"], kw["terms"], kw["counts"]), kw["laplace_smooth"])


@pytest.mark.parametrize("case", split_error_cases(), ids=lambda c: c[0].replace(" ", "_"))
def test_split_argument_errors_without_a_context(tmvb, case):
    _, kw, status, msg = case
    rc, res = call_split(tmvb, None, kw)
    assert rc == status and msg in res["error"], (rc, res)


@pytest.mark.parametrize("case", loglik_error_cases(), ids=lambda c: c[0].replace(" ", "_"))
def test_loglik_argument_errors_without_a_context(tmvb, case):
    _, kw, status, msg = case
    rc, res = call_loglik(tmvb, None, kw)
    assert rc == status and isinstance(res, str) and msg in res, (rc, res)


def test_valid_arguments_without_a_device_are_enodevice(tmvb):
    """No silent CPU path: the arguments pass, then a NULL context on a machine without a GPU is TMVB_ENODEVICE."""
    if tmvb.lib().tmvb_device_count() > 0:
        pytest.skip("a GPU is visible: tests/test_heldout_gpu.py covers the live path")
    rc, res = call_split(tmvb, None, _split_base())
    assert rc == ENODEVICE and "no HIP device" in res["error"]
    rc, res = call_loglik(tmvb, None, _loglik_base())
    assert rc == ENODEVICE and "no HIP device" in res
    pc = tmvb.PackedCorpus([0, 2, 2, 5], [0, 5, 1, 2, 3], [1, 4, 2, 1, 9], 6)
    with pytest.raises(tmvb.EngineError):
        tmvb.split_corpus(pc)


def test_python_mirror_argument_errors(tmvb):
    pc = tmvb.PackedCorpus([0, 2, 2, 5], [0, 5, 1, 2, 3], [1, 4, 2, 1, 9], 6)
    other = tmvb.PackedCorpus([0, 2, 2, 5], [0, 5, 1, 2, 3], [1, 4, 2, 1, 9], 7)
    m = tmvb.LDA(pc, 3)
    with pytest.raises(tmvb.CorpusError, match="predict corpus and train_model corpus must have identical vocabularies."):
        tmvb.heldout_loglik(m, other, other)
    with pytest.raises(tmvb.CorpusError, match="identical vocabularies"):
        tmvb.perplexity(m, other)
    with pytest.raises(ValueError, match="laplace_smooth parameter must be nonnegative."):
        tmvb.heldout_loglik(m, pc, pc, laplace_smooth=-1.0)
    pf = tmvb.PackedCorpus([0, 2], [0, 1], [1, 1], 3, [0, 1], [0], [1], 2)
    with pytest.raises(tmvb.TopicModelError, match="CTPF"):
        tmvb.heldout_loglik(tmvb.CTPF(pf, 2), pf, pf)
    r = tmvb.HeldoutResult([-2.0, 0.0, -4.0], [1, 0, 2], 0)
    assert r.perplexity == pytest.approx(math.exp(2.0))
    assert tmvb.HeldoutResult([-2.0, -np.inf], [1, 3], 3).perplexity == math.inf
    assert math.isnan(tmvb.HeldoutResult([0.0, 0.0], [0, 0], 0).perplexity)


def test_header_structure_and_sources(tmvb):
    syms = tmvb.exported_symbols()
    L = C.CDLL(tmvb.LIB_PATH)
    for s in ("tmvb_corpus_split", "tmvb_split_free", "tmvb_heldout_loglik"):
        assert s in syms and hasattr(L, s)
    assert tmvb.lib().tmvb_abi_version() == 2
    for name in ("split_corpus", "heldout_loglik", "perplexity", "heldout_loglik_raw"):
        assert name in tmvb.__all__ and callable(getattr(tmvb, name))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tmvb.h")).read(), flags=re.S)
    fields = re.search(r"typedef struct \{([^}]*)\} tmvb_split_t;", hdr).group(1)
    names = re.findall(r"\b(\w+)\s*[;,]", fields)
    assert names == [f[0] for f in sys.modules[tmvb.__name__ + ".heldout"].SplitResult._fields_]
    assert "tmvb_heldout.hip" in tmvb._lib.SOURCES
    philox = open(os.path.join(ROOT, "topicmodelsvb.jl_amd", "csrc", "tmvb_philox.h")).read()
    assert re.search(r"TMVB_RNG_SPLIT = %d\b" % RNG_SPLIT, philox)


def test_julia_shim_binds_the_entry_points():
    src = open(os.path.join(ROOT, "topicmodelsvb.jl_amd", "julia", "TMVBHip.jl")).read()
    for s in (":tmvb_corpus_split", ":tmvb_split_free", ":tmvb_heldout_loglik", "function split_corp(", "function heldout_loglik(", "mutable struct TmvbSplit"):
        assert s in src, s
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tmvb.h")).read(), flags=re.S)
    names = re.findall(r"\b(\w+)\s*[;,]", re.search(r"typedef struct \{([^}]*)\} tmvb_split_t;", hdr).group(1))
    body = src[src.index("mutable struct TmvbSplit"):]
    body = body[:body.index("TmvbSplit() =")]
    assert re.findall(r"(\w+)::", body) == names


def test_the_gpu_tolerance_is_frozen_from_its_measurement():
    """a tolerance is at least 1 x and at most 10 x the worst deviation measured on the MI355X."""
    import test_heldout_gpu as g
    ev = json.load(open(os.path.join(ROOT, "profiles", "heldout_tolerances_measured.json")))
    measured = ev["heldout.ll_rel"]["measured"]
    assert measured > 0
    assert 1.0 <= g.LL_REL_TOL / measured <= 10.0, (g.LL_REL_TOL, measured)
