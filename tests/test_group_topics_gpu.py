"""
tmvb_group_topics on the device (include/tmvb.h, "topics by group and over time") against tests/group_topics_restatement.py.

  1. exact         on admissible inputs dense, mass and tokens equal BIT FOR BIT the sums of (double)c * (double)r over the device's own r bits, which
                   tmvb_token_topics(phi=...) returns through an entry point that is already pinned.  Admissible: every r >= 2^-11 and every
                   group's token total < 2^18 -- every addend is then a multiple of 2^-34 and every sum below 2^18, so fp64 addition is exact in
                   any order.  The test asserts both on the phi bits and the totals; the construction gives them: A, B in [1, 2] give r > 1 / (4 K)
                   for K <= 256, constant factors at K = 1024 give r = 2^-10.  K covers every lanes_per_entry, the runs of group 0 have 1, SEG - 1,
                   SEG, SEG + 1 and 2 SEG + 1 entries ("long"; "short" stops at SEG: the control of tests/test_group_topics_mutant_gpu.py), G in
                   {1, 2, 7} with an empty group, -1 documents, an empty document, a document with a repeated id, unused terms.
  2. selection     top_idx / top_p = the lexsort of the device's own dense / mass quotient bits, on inputs full of ties: constant factors,
                   n > the number of used terms, n = V
  3. floating      Dirichlet-like A columns, a sparse B with zeros, eps = 1e-30: S within n_run 2^-53 S of the fsum at the device's phi bits, mass
                   within (n_max + V) 2^-53, shift and drift within (V + 16) 2^-52 of the restatement at the device's own normalised rows
  4. identities    bit for bit: two calls, max_chunk_groups in {0, 1, 2, G}, with and without dense / shift / drift, permuted labels, one
                   document as a group, drift across an empty group
  5. planted       two groups drawn by gencorp from two different rows for topic 0: its shift exceeds every other topic's, each group's top words
                   for topic 0 are its own planted ones
  6. models        group_topics(model, labels) on the trained LDA, CTM and CTPF golden corpora, corp= fold-in, fLDA raises

sum_k mass[g][k] == tokens[g]: exact only where sum_k r_k is exactly 1 in fp32 (constant factors at a power-of-two K: asserted at K = 1024); for the
random factors of case 1 the fp32 division leaves sum_k r_k within K 2^-24 of 1, so there the test asserts the exact fp64 value
sum over entries of c * (sum_k r_k) bit for bit, and the distance from tokens[g] under K 2^-24 tokens[g].

Largest measured fraction of each cap of case 3 on an MI355X: profiles/group_topics_tolerances_measured.json (a run with TMVB_GT_RECORD=<file>
writes such a record at the module's end).
"""
import json
import math
import os

import numpy as np
import pytest

import group_topics_restatement as gr
import token_topics_restatement as tr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEG = gr.SEG
V = 40
KS = [1, 3, 4, 5, 16, 17, 50, 64, 65, 130, 256, 1024]
LANES = {1: 1, 3: 1, 4: 1, 5: 1, 16: 1, 17: 2, 50: 4, 64: 4, 65: 8, 130: 16, 256: 16, 1024: 64}
CASES = [(K, 7, "long") for K in KS] + [(5, 1, "long"), (50, 2, "long"), (5, 1, "short"), (50, 2, "short"), (17, 7, "short"), (1024, 7, "short")]
FRACTION = {"S": 0.0, "mass": 0.0, "shift": 0.0, "drift": 0.0}
CACHE = {}


@pytest.fixture(scope="module")
def ctx(tmvb):
    c = tmvb.DeviceContext(0)
    yield c
    c.close()
    out = os.environ.get("TMVB_GT_RECORD", "")
    if not out:
        return
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump({"group_topics.cap_fraction": {"measured": FRACTION, "caps": {"S": "n_run 2^-53 S", "mass": "(n_max + V) 2^-53 mass",
                                                                                 "shift": "(V + 16) 2^-52", "drift": "(V + 16) 2^-52"},
                                                 "what": "largest |device - restatement| / cap over the floating cases of tests/test_group_topics_gpu.py"}}, f, indent=1)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def run(tmvb, ctx, A, B, pc, group, G, **kw):
    rc, res = tmvb.group_topics_raw(ctx, A.shape[0], B.shape[1], A, B, pc, group, G, **kw)
    assert rc == 0, res
    return res


def device_phi(tmvb, ctx, A, B, pc, eps):
    rc, res = tmvb.token_topics_raw(ctx, A.shape[0], B.shape[1], A, B, pc, eps=eps, phi=True, hard=False, select=False)
    assert rc == 0, res
    return res["phi"]


def same_outputs(a, b, keys=("docs", "tokens", "mass", "top_idx", "top_p", "shift", "drift", "dense")):
    for k in keys:
        if a[k] is None or b[k] is None:
            continue
        assert a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


# ------------------------------------------------------------------------------------------------------------------ 1. exact
def exact_corpus(tmvb, G, kind, seed=1):
    """group 0: D documents, term 0 in all of them, term 1 in the first SEG + 1 (long), term 2 in the first SEG, term 3 in the first SEG - 1, term 4 in
    one; every document 0 - 2 more terms of 5 .. 31 (32 .. 39 stay unused), one document the same id twice; then 30 documents of the other groups
    (group 5 of 7 stays empty), four left out, one empty; all shuffled"""
    rng = np.random.default_rng(seed)
    D = 2 * SEG + 1 if kind == "long" else SEG
    docs, labels = [], []
    for i in range(D):
        t = [0] + ([1] if kind == "long" and i < SEG + 1 else []) + ([2] if i < SEG else []) + ([3] if i < SEG - 1 else []) + ([4] if i == 7 else [])
        t += rng.integers(5, 32, size=int(rng.integers(0, 3))).tolist()
        if i == 3:
            t += [9, 9]
        docs.append(rng.permutation(t)); labels.append(0)
    others = [g for g in range(1, G) if g != 5]
    for i in range(30):
        docs.append(rng.integers(5, 32, size=int(rng.integers(1, 12))))
        labels.append(others[i % len(others)] if others else 0)
    for i in range(4):
        docs.append(rng.integers(0, 32, size=5)); labels.append(-1)
    docs.append(np.zeros(0, dtype=np.int64)); labels.append(0)
    o = rng.permutation(len(docs))
    docs, labels = [docs[i] for i in o], np.array(labels, dtype=np.int32)[o]
    ptr = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.int64)
    terms = np.concatenate(docs).astype(np.int32)
    return tmvb.PackedCorpus(ptr, terms, rng.integers(1, 6, size=len(terms)).astype(np.int32), V), labels


def exact_factors(K, M, seed):
    if K == 1024:
        return np.full((K, M), 1.5), np.full((K, V), 1.25)
    rng = np.random.default_rng(seed)
    return rng.uniform(1.0, 2.0, size=(K, M)), rng.uniform(1.0, 2.0, size=(K, V))


def exact_case(tmvb, ctx, K, G, kind):
    key = (K, G, kind)
    if key not in CACHE:
        pc, group = exact_corpus(tmvb, G, kind)
        A, B = exact_factors(K, len(group), 100 + K)
        phi = device_phi(tmvb, ctx, A, B, pc, tr.EPSILON)
        CACHE[key] = (pc, group, A, B, phi, gr.stats(phi, pc.doc_ptr, pc.terms, pc.counts, group, G, V))
    return CACHE[key]


@pytest.mark.parametrize("K,G,kind", CASES)
def test_exact(tmvb, ctx, K, G, kind):
    pc, group, A, B, phi, ref = exact_case(tmvb, ctx, K, G, kind)
    # admissibility, on the phi bits themselves
    assert phi.dtype == np.float32 and float(phi.min()) >= 2.0 ** -11 and int(ref["tokens"].max()) < 2 ** 18
    lens = np.diff(gr.index(pc.doc_ptr, pc.terms, group)["run_ptr"])
    want = {1, SEG - 1, SEG} | ({SEG + 1, 2 * SEG + 1} if kind == "long" else set())
    assert want <= set(lens.tolist()) and (lens.max() > SEG) == (kind == "long")
    res = run(tmvb, ctx, A, B, pc, group, G, dense=True)
    assert res["info"]["lanes_per_entry"] == LANES[K] and res["info"]["nsel"] == int(np.diff(pc.doc_ptr)[group >= 0].sum()) and res["info"]["runs"] == len(lens)
    assert res["info"]["segments"] == int(np.sum(-(-lens // SEG)))
    assert np.array_equal(res["tokens"], ref["tokens"]) and np.array_equal(res["docs"], ref["docs"])
    S = ref["S"]
    bad = np.argwhere(bits(res["dense"]) != bits(S))
    assert len(bad) == 0, (len(bad), bad[:5], res["dense"][tuple(bad[0])], S[tuple(bad[0])])
    mass = S.sum(axis=2)                                    # exact in any order
    assert np.array_equal(bits(res["mass"]), bits(mass))
    # sum_k mass against the tokens (module docstring)
    ix_doc = np.repeat(np.arange(len(group)), np.diff(pc.doc_ptr))
    rowsum = phi.astype(np.float64).sum(axis=1) * np.asarray(pc.counts, dtype=np.float64)
    for g in range(G):
        tot = float(rowsum[group[ix_doc] == g].sum())
        assert float(res["mass"][g].sum()) == tot and abs(tot - ref["tokens"][g]) <= K * 2.0 ** -24 * max(int(ref["tokens"][g]), 1)
        if K == 1024:
            assert float(res["mass"][g].sum()) == float(ref["tokens"][g])
    if G == 7:
        assert ref["tokens"][5] == 0 and np.all(res["mass"][5] == 0) and np.all(res["top_idx"][5] == -1) and np.all(res["top_p"][5] == 0)
        assert np.all(res["shift"][5] == 0) and np.all(res["drift"][5] == 0) and np.all(res["drift"][0] == 0) and np.all(res["drift"][6] > 0)
    assert np.all(res["dense"][:, :, 32:] == 0)             # unused terms


def test_the_r_are_token_topics_bits(tmvb, ctx):
    """G = 1 on a corpus with one entry per term: dense[0][k][w] = c_w * phi[entry of w][k], no addition at all"""
    K, Vv = 50, 33
    rng = np.random.default_rng(3)
    perm = rng.permutation(Vv)
    pc = tmvb.PackedCorpus(np.array([0, 10, 10, 21, Vv]), perm.astype(np.int32), rng.integers(1, 2 ** 27, size=Vv).astype(np.int32), Vv)      # a document stays below 2^31 tokens
    A, B = rng.gamma(0.5, size=(K, 4)), rng.gamma(0.5, size=(K, Vv))
    phi = device_phi(tmvb, ctx, A, B, pc, tr.EPSILON)
    res = run(tmvb, ctx, A, B, pc, np.zeros(4, dtype=np.int32), 1, dense=True)
    want = np.zeros((K, Vv))
    want[:, perm] = (phi.astype(np.float64) * np.asarray(pc.counts, dtype=np.float64)[:, None]).T
    assert np.array_equal(bits(res["dense"][0]), bits(want))


# ------------------------------------------------------------------------------------------------------------------ 2. selection
def assert_selection(res, n):
    beta = gr.normalise(res["dense"], res["mass"])
    idx, p = gr.select(beta, res["mass"], n)
    assert np.array_equal(res["top_idx"], idx), np.argwhere(res["top_idx"] != idx)[:5]
    assert np.array_equal(bits(res["top_p"]), bits(p))


@pytest.mark.parametrize("K,n", [(5, 40), (50, 33), (17, 1), (64, 10)])
def test_selection_with_ties(tmvb, ctx, K, n):
    pc, group = exact_corpus(tmvb, 7, "short")
    M = len(group)
    res = run(tmvb, ctx, np.full((K, M), 0.5), np.full((K, V), 2.0), pc, group, 7, topn=n, dense=True)      # constant factors: every r equal
    used = int((res["dense"][0, 0] > 0).sum())
    assert used <= 32 and (n <= used or np.all(res["top_p"][0, :, used:] == 0))                             # n = 40 = V and n = 33 pass the used terms
    ties = int(sum(len(np.unique(res["top_p"][g, 0])) < n for g in (0, 1, 2, 3, 4, 6)))
    assert n == 1 or ties > 0
    assert_selection(res, n)
    if n > used:
        assert res["top_idx"][0, 0, used:].tolist() == sorted(set(range(V)) - set(np.flatnonzero(res["dense"][0, 0] > 0).tolist()))[:n - used]


# ------------------------------------------------------------------------------------------------------------------ 3. floating inputs
FV = 70


def floating_case(tmvb, ctx, K, G=4, seed=5):
    """group 0 holds a hot term in 600 documents (a run longer than SEG); group 2 of 4 stays empty; some documents are left out or empty"""
    key = ("float", K, G, seed)
    if key in CACHE:
        return CACHE[key]
    rng = np.random.default_rng(seed + K)
    M = 760
    lens = rng.integers(0, 12, size=M)
    group = np.where(np.arange(M) < 600, 0, rng.choice([1, 3, -1], size=M)).astype(np.int32)
    docs = [np.concatenate([[1] if (group[d] == 0 or d % 3 == 0) else [], rng.integers(0, FV - 6, size=lens[d])]).astype(np.int32) for d in range(M)]
    docs[5] = np.zeros(0, dtype=np.int32)
    o = rng.permutation(M)
    docs, group = [docs[i] for i in o], group[o]
    ptr = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.int64)
    terms = np.concatenate(docs).astype(np.int32)
    pc = tmvb.PackedCorpus(ptr, terms, rng.integers(1, 40, size=len(terms)).astype(np.int32), FV)
    A = rng.dirichlet(np.full(max(K, 2), 0.1), size=M).T[:K].copy()           # Dirichlet-like columns: most of the mass on a few topics
    B = rng.gamma(0.3, size=(K, FV)) * (rng.random((K, FV)) > 0.3)            # sparse, exact zeros
    phi = device_phi(tmvb, ctx, A, B, pc, 1e-30)
    CACHE[key] = (pc, group, A, B, phi)
    return CACHE[key]


def fsum_stats(phi, pc, group, G, Vv):
    """S and mass by math.fsum of the exact products: correctly rounded"""
    ix = gr.index(pc.doc_ptr, pc.terms, group)
    K = phi.shape[1]
    prod = phi.astype(np.float64) * np.asarray(pc.counts, dtype=np.float64)[:, None]
    S, n_run = np.zeros((G, K, Vv)), np.zeros((G, Vv), dtype=np.int64)
    for u in range(len(ix["run_group"])):
        e = ix["entry"][ix["run_ptr"][u]:ix["run_ptr"][u + 1]]
        g, w = ix["run_group"][u], ix["run_term"][u]
        n_run[g, w] = len(e)
        S[g, :, w] = [math.fsum(prod[e, k]) for k in range(K)]
    mass = np.zeros((G, K))
    for g in range(G):
        e = ix["entry"][ix["run_ptr"][np.searchsorted(ix["run_group"], g, "left")]:ix["run_ptr"][np.searchsorted(ix["run_group"], g, "right")]]
        mass[g] = [math.fsum(prod[e, k]) for k in range(K)]
    return S, mass, n_run


def device_rowsum(x):
    """the order of the library's row sums: lane t of 256 adds w = t, t + 256, ... ascending from 0, then the halving tree"""
    x = np.asarray(x, dtype=np.float64)
    pad = np.zeros(-(-len(x) // 256) * 256)
    pad[:len(x)] = x
    s = np.zeros(256)
    for row in pad.reshape(-1, 256):
        s = s + row
    o = 128
    while o:
        s[:o] = s[:o] + s[o:2 * o]
        o //= 2
    return float(s[0])


@pytest.mark.parametrize("K", [3, 50, 130])
def test_floating_inputs(tmvb, ctx, K):
    G = 4
    pc, group, A, B, phi = floating_case(tmvb, ctx, K)
    res = run(tmvb, ctx, A, B, pc, group, G, eps=1e-30, dense=True)
    S64, mass64, n_run = fsum_stats(phi, pc, group, G, FV)
    assert n_run.max() > SEG and np.any(B == 0) and res["tokens"][2] == 0 and res["info"]["segments"] > res["info"]["runs"]
    capS = gr.cap_S(n_run)[:, None, :] * S64
    errS = np.abs(res["dense"] - S64)
    fS = float((errS[capS > 0] / capS[capS > 0]).max())
    assert np.all(errS <= capS), fS                         # capS = 0 where S64 = 0: the device holds an exact 0 there
    capM = gr.cap_mass(n_run.max(axis=1), FV)[:, None] * mass64
    errM = np.abs(res["mass"] - mass64)
    fM = float((errM[capM > 0] / capM[capM > 0]).max())
    assert np.all(errM <= capM), fM
    # the device's mass is the fixed-order sum of the device's own S
    assert np.array_equal(bits(res["mass"]), bits(np.array([[device_rowsum(res["dense"][g, k]) for k in range(K)] for g in range(G)])))
    # shift and drift at the device's own normalised rows
    beta = gr.normalise(res["dense"], res["mass"])
    pool = np.zeros((K, FV))
    for g in range(G):
        pool = pool + res["dense"][g]
    tot = np.array([device_rowsum(pool[k]) for k in range(K)])
    shift, drift = gr.shift_drift(beta, res["tokens"] > 0, gr.normalise(pool[None], tot[None])[0])
    fs, fd = float(np.abs(res["shift"] - shift).max() / gr.cap_js(FV)), float(np.abs(res["drift"] - drift).max() / gr.cap_js(FV))
    print(f"group_topics floating K = {K}: largest fraction of the cap  S {fS:.3f}  mass {fM:.3f}  shift {fs:.3f}  drift {fd:.3f}")
    for k, v in (("S", fS), ("mass", fM), ("shift", fs), ("drift", fd)):
        FRACTION[k] = max(FRACTION[k], v)
    assert fs <= 1.0 and fd <= 1.0
    assert np.all(res["shift"][[0, 1, 3]] > 0) and np.all(res["shift"] <= math.log(2.0)) and np.all(res["drift"][0] == 0) and np.all(res["drift"][2] == 0)
    assert_selection(res, 10)


# ------------------------------------------------------------------------------------------------------------------ 4. identities
@pytest.mark.parametrize("K", [5, 50])
def test_identities(tmvb, ctx, K):
    G = 4
    pc, group, A, B, phi = floating_case(tmvb, ctx, K)
    kw = dict(eps=1e-30, topn=7)
    full = run(tmvb, ctx, A, B, pc, group, G, dense=True, **kw)
    same_outputs(run(tmvb, ctx, A, B, pc, group, G, dense=True, **kw), full)
    for chunk, n_chunks in ((0, 1), (1, 4), (2, 2), (G, 1)):
        c = run(tmvb, ctx, A, B, pc, group, G, dense=True, max_chunk_groups=chunk, **kw)
        assert c["info"]["group_chunks"] == n_chunks
        same_outputs(c, full)
    for sh, dr, dn, chunk in ((False, False, False, 0), (True, False, False, 1), (False, True, True, 1), (True, True, False, 2), (False, False, True, 0)):
        c = run(tmvb, ctx, A, B, pc, group, G, shift=sh, drift=dr, dense=dn, max_chunk_groups=chunk, **kw)
        assert (c["shift"] is None) == (not sh) and (c["drift"] is None) == (not dr) and (c["dense"] is None) == (not dn)
        same_outputs(c, full)
    # permuted labels permute every per-group output; shift agrees within the cap (the pooled sum is added in another order)
    perm = np.array([2, 0, 3, 1])                           # new label of old group g
    p = run(tmvb, ctx, A, B, pc, np.where(group >= 0, perm[np.maximum(group, 0)], -1), G, dense=True, **kw)
    for k in ("docs", "tokens", "mass", "top_idx", "top_p", "dense"):
        assert np.array_equal(p[k][perm].view(np.uint8), full[k].view(np.uint8)), k
    assert np.all(np.abs(p["shift"][perm] - full["shift"]) <= gr.cap_js(FV))
    # drift skips a group without entries: the same rows with the empty group 2 taken out
    comp = np.array([0, 1, -1, 2])
    c = run(tmvb, ctx, A, B, pc, np.where(group >= 0, comp[np.maximum(group, 0)], -1), 3, **kw)
    assert np.array_equal(bits(c["drift"]), bits(full["drift"][[0, 1, 3]])) and np.array_equal(bits(c["shift"]), bits(full["shift"][[0, 1, 3]]))
    assert np.all(full["drift"][3] > 0) and np.all(full["drift"][2] == 0)


def test_identities_under_the_exact_conditions(tmvb, ctx):
    """permuted labels leave shift unchanged bit for bit when every sum is exact; a group made of one document reproduces that document's phi column sums"""
    K, G = 50, 7
    pc, group, A, B, phi, ref = exact_case(tmvb, ctx, K, G, "long")
    full = run(tmvb, ctx, A, B, pc, group, G)
    perm = np.array([3, 0, 6, 1, 2, 4, 5])
    p = run(tmvb, ctx, A, B, pc, np.where(group >= 0, perm[np.maximum(group, 0)], -1), G)
    assert np.array_equal(bits(p["shift"][perm]), bits(full["shift"])) and np.array_equal(bits(p["mass"][perm]), bits(full["mass"]))
    ptr = np.asarray(pc.doc_ptr)
    for d in (int(np.argmax(np.diff(ptr))), int(np.flatnonzero(np.diff(ptr) == 0)[0]), 0):
        one = run(tmvb, ctx, A, B, pc, np.where(np.arange(len(group)) == d, 0, -1), 1)
        sums = (phi[ptr[d]:ptr[d + 1]].astype(np.float64) * np.asarray(pc.counts[ptr[d]:ptr[d + 1]], dtype=np.float64)[:, None]).sum(axis=0)
        assert np.array_equal(bits(one["mass"][0]), bits(sums)) and one["docs"].tolist() == [1] and one["tokens"][0] == int(pc.counts[ptr[d]:ptr[d + 1]].sum())


# ------------------------------------------------------------------------------------------------------------------ 5. planted structure
def test_planted_structure(tmvb, ctx):
    K, Vp, Mg = 4, 60, 150
    rng = np.random.default_rng(11)
    base = np.full((K, Vp), 1e-3)
    for k in range(1, K):
        base[k, 10 + 12 * k:22 + 12 * k] += 1.0             # topics 1 .. 3: blocks of their own
    planted = (np.arange(0, 5), np.arange(5, 10))
    betas = []
    for words in planted:
        b = base.copy()
        b[0, words] += np.linspace(2.0, 1.0, 5)              # topic 0 is written with other words in each group
        betas.append(b / b.sum(axis=1, keepdims=True))
    alpha = np.full(K, 0.3)
    parts = []
    for g, b in enumerate(betas):
        rc, res = tmvb.gencorp_raw(ctx, K, Vp, b, Mg, 80.0, alpha=alpha, seed=100 + g, diagnostics=True)
        assert rc == 0, res
        parts.append(res)
    ptr = np.concatenate([parts[0]["doc_ptr"], parts[0]["doc_ptr"][-1] + parts[1]["doc_ptr"][1:]])
    pc = tmvb.PackedCorpus(ptr, np.concatenate([p["terms"] for p in parts]), np.concatenate([p["counts"] for p in parts]), Vp)
    A = np.exp(np.concatenate([p["log_theta"] for p in parts]).astype(np.float64)).T
    B = 0.5 * (betas[0] + betas[1])                          # the model sees one pooled topic 0
    group = np.repeat([0, 1], Mg).astype(np.int32)
    res = run(tmvb, ctx, A, B, pc, group, 2, topn=5)
    assert np.all(res["shift"][:, 0] > res["shift"][:, 1:].max(axis=1)), res["shift"]
    assert np.all(res["drift"][1, 0] > res["drift"][1, 1:]) and np.all(res["drift"][0] == 0)
    for g in (0, 1):
        assert sorted(res["top_idx"][g, 0].tolist()) == planted[g].tolist(), (g, res["top_idx"][g, 0])
    prev = res["mass"] / res["mass"].sum(axis=1, keepdims=True)
    assert np.all(np.abs(prev.sum(axis=1) - 1.0) < 1e-12) and np.all(prev > 0.05)


# ------------------------------------------------------------------------------------------------------------------ 6. models
def load(name):
    return np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))


def check_model(tmvb, m, K):
    pc = m.corp
    M = pc.M
    labels = [("y%d" % (1990 + d % 3)) if d % 7 != 4 else None for d in range(M)]
    gt = tmvb.group_topics(m, labels, topn=5, dense=True)
    assert gt.labels == ["y1990", "y1991", "y1992"] and gt.mass.shape == (3, K) and gt.idx.shape == (3, K, 5) and len(gt.words) == 3 and len(gt.words[0][0]) == 5
    g = np.array([-1 if x is None else gt.labels.index(x) for x in labels])
    ptr = np.asarray(pc.doc_ptr)
    phis = tmvb.phi(m, list(range(1, M + 1)))
    theta = tmvb.topic_proportions(m)
    for i in range(3):
        docs = np.flatnonzero(g == i)
        assert gt.docs[i] == len(docs) and gt.tokens[i] == sum(int(pc.counts[ptr[d]:ptr[d + 1]].sum()) for d in docs)
        prod = np.concatenate([phis[d].astype(np.float64) * np.asarray(pc.counts[ptr[d]:ptr[d + 1]], dtype=np.float64) for d in docs], axis=1)      # exact products, K x entries
        want = np.array([math.fsum(row) for row in prod])   # correctly rounded, as in the floating case
        n_max = int(np.bincount(np.concatenate([pc.terms[ptr[d]:ptr[d + 1]] for d in docs]), minlength=1).max())
        assert np.all(np.abs(gt.mass[i] - want) <= gr.cap_mass(n_max, pc.V) * want)
        assert np.allclose(gt.theta_mean[i], theta[:, docs].mean(axis=1), rtol=1e-14)
        b = gt.beta(i)
        assert b.shape == (K, pc.V) and np.allclose(b.sum(axis=1), 1.0, rtol=1e-12)
        assert np.array_equal(gt.idx[i], gr.select(b[None], gt.mass[i][None], 5)[0][0])
    assert np.allclose(gt.prevalence.sum(axis=1), 1.0) and np.all(np.isnan(gt.drift[0])) and not np.any(np.isnan(gt.drift[1:])) and not np.any(np.isnan(gt.shift))
    assert gt.trend.shape == (K,) and sorted(gt.hot(K).tolist()) == list(range(K)) and gt.hot(1)[0] == int(np.argmax(gt.trend)) and gt.cold(1)[0] == int(np.argmin(gt.trend))
    rev = tmvb.group_topics(m, labels, topn=5, order=["y1992", "y1991", "y1990"])
    assert np.array_equal(bits(rev.mass[::-1].copy()), bits(gt.mass)) and np.allclose(rev.trend, -gt.trend, atol=1e-13)
    return gt


def test_group_topics_of_a_trained_lda(tmvb):
    g = load("lda_m40_v60_k7")
    K, Vg = int(g["K"]), int(g["V"])
    m = tmvb.LDA(tmvb.PackedCorpus(g["doc_ptr"], g["terms"], g["counts"], Vg), K)
    m.beta = np.asfortranarray(g["beta0"]); m.beta_old = m.beta.copy(order="F")
    tmvb.gpu_train(m, iter=3, tol=0.0, checkelbo=1, printelbo=False)
    check_model(tmvb, m, K)
    # a new corpus goes through predict first
    rng = np.random.default_rng(41)
    lens = [4, 0, 9, 6]
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    new = tmvb.PackedCorpus(ptr, rng.integers(0, Vg, size=int(ptr[-1])).astype(np.int32), rng.integers(1, 6, size=int(ptr[-1])).astype(np.int32), Vg)
    gt = tmvb.group_topics(m, [2.0, 1.0, float("nan"), 1.0], corp=new, topn=3)
    assert gt.labels == [1.0, 2.0] and gt.docs.tolist() == [2, 1] and gt.tokens.tolist() == [int(new.counts[13:].sum()), int(new.counts[:4].sum())]
    p = tmvb.predict(new, m)
    r = tr.responsibilities(np.exp(p.Elogtheta), m.beta, new.doc_ptr, new.terms, None, tr.EPSILON)
    want = (r[:4] * np.asarray(new.counts[:4], dtype=np.float64)[:, None]).sum(axis=0)
    assert np.all(np.abs(gt.mass[1] - want) <= (tr.cap(K) + 1e-12) * want)
    with pytest.raises(tmvb.CorpusError):
        tmvb.group_topics(m, [1], corp=tmvb.PackedCorpus(np.array([0, 1]), np.array([0], dtype=np.int32), np.array([1], dtype=np.int32), Vg + 1))
    with pytest.raises(ValueError):
        tmvb.group_topics(m, [1] * 39)
    with pytest.raises(ValueError):
        tmvb.group_topics(m, [1] * 40, topn=65)


def test_group_topics_of_a_trained_ctm(tmvb):
    g = load("ctm_m40_v60_k5")
    K, Vg = int(g["K"]), int(g["V"])
    m = tmvb.CTM(tmvb.PackedCorpus(g["doc_ptr"], g["terms"], g["counts"], Vg), K)
    m.beta = np.asfortranarray(g["beta0"]); m.beta_old = m.beta.copy(order="F")
    tmvb.gpu_train_ctm(m, iter=3, tol=0.0, checkelbo=1, printelbo=False)
    check_model(tmvb, m, K)


def test_group_topics_of_a_trained_ctpf(tmvb):
    g = load("ctpf_m40_v60_u15_k4")
    K, Vg, U = int(g["K"]), int(g["V"]), int(g["U"])
    m = tmvb.CTPF(tmvb.PackedCorpus(g["doc_ptr"], g["terms"], g["counts"], Vg, g["rdr_ptr"], g["readers"], g["ratings"], U), K)
    m.alef = np.asfortranarray(g["alef0"]); m.alef_old = m.alef.copy(order="F")
    tmvb.gpu_train_ctpf(m, iter=3, tol=0.0, checkelbo=1, printelbo=False)
    check_model(tmvb, m, K)


def test_a_filtered_model_raises(tmvb):
    g = load("flda_m40_v60_k5")
    m = tmvb.fLDA(tmvb.PackedCorpus(g["doc_ptr"], g["terms"], g["counts"], int(g["V"])), int(g["K"]))
    with pytest.raises(tmvb.TopicModelError, match="tau"):
        tmvb.group_topics(m, [0] * m.M)
