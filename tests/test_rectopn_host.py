"""
Top-n recommendations (tmvb_score_topn; include/tmvb.h), the part that needs no GPU -- and the NumPy checker and the inputs of
tests/test_rectopn_gpu.py: the reference has no such function (showurecs / showdrecs read the head of a full ranking), so the yardstick is a
restatement written here.

  * `np_topn`: the first n rows of [0, Md) \\ excl(q) under the order of reverse(sortperm(.)) -- score descending, index DESCENDING on equal
    scores -- from a score matrix, checked against a brute-force `sorted` on three hand-written cases with ties;
  * `topn_case`: the exact inputs of the GPU file (the integer features of tests/test_recranks_host.py's exact_case with exclusion lists of
    its own);
  * every error of the contract comes back with its status and message from a NULL context, valid arguments without a device give
    TMVB_ENODEVICE;
  * the header, the structure, SOURCES, the Julia shim, the mutant's flag, the call scope, the kernel-resource table;
  * recommend_topn's argument errors and the slice rule of `ids`.
"""
import contextlib
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import tmvb_amd  # noqa: E402
from test_call_scope_host import test_units_own_no_device_scratch as _units_own_no_device_scratch  # noqa: E402
from test_recranks_host import T, csr_of, exact_case  # noqa: E402

# the mirror module of the feature: a tree without it fails here, at import, and with it every test of this module and of the two GPU modules
TOPN = sys.modules[tmvb_amd.pkg.__name__ + ".recs_topn"]
EINVAL, ESHAPE, ENODEVICE = 1, 2, 7
EXCL = ["none", "random", "all-but-three", "all"]


# ------------------------------------------------------------------------------------------------------------------ NumPy checker
def np_topn(S, excl, n):
    """(idx int32 [Mq, n], score float32 [Mq, n], count int32 [Mq]) from the score matrix S[Mq, Md]: per query the first n rows outside
    its exclusion list, score descending, index descending on equal scores; -1 / -inf past count"""
    Mq, Md = S.shape
    eptr, eidx = excl
    idx = np.full((Mq, n), -1, dtype=np.int32)
    score = np.full((Mq, n), -np.inf, dtype=np.float32)
    count = np.zeros(Mq, dtype=np.int32)
    for q in range(Mq):
        cand = np.ones(Md, dtype=bool)
        cand[eidx[eptr[q]:eptr[q + 1]]] = False
        ids = np.flatnonzero(cand)
        order = ids[np.lexsort((ids, S[q, ids]))[::-1]][:n]              # ascending by (score, index), reversed: reverse(sortperm(.))
        count[q] = len(order)
        idx[q, :len(order)] = order
        score[q, :len(order)] = S[q, order]
    return idx, score, count


def brute_topn(S, excl_rows, n):
    out = []
    for q in range(S.shape[0]):
        ex = set(excl_rows[q])
        out.append(sorted((e for e in range(S.shape[1]) if e not in ex), key=lambda e: (S[q, e], e), reverse=True)[:n])
    return out


@pytest.mark.parametrize("S,excl_rows,n,want", [
    # all scores equal: the highest indices outside the list, descending
    (np.full((1, 6), 2.0), [[5, 2]], 3, [[4, 3, 1]]),
    # ties around the cut: 7 7 7 at rows 0, 2, 4 -> 4, 2 enter at n = 3 behind the 9; the excluded 9 at row 5 does not
    (np.array([[7.0, 1.0, 7.0, 9.0, 7.0, 9.0]]), [[5]], 3, [[3, 4, 2]]),
    # fewer candidates than n, an empty list, and a query with everything excluded
    (np.array([[1.0, 1.0, 3.0], [0.0, 5.0, 5.0], [4.0, 4.0, 4.0]]), [[1], [], [0, 1, 2]], 4, [[2, 0], [2, 1, 0], []]),
])
def test_the_restatement_against_brute_force(S, excl_rows, n, want):
    idx, score, count = np_topn(S, csr_of(excl_rows), n)
    assert brute_topn(S, excl_rows, n) == want                           # the hand-written answer is what `sorted` says
    for q, w in enumerate(want):
        assert count[q] == len(w) and idx[q, :len(w)].tolist() == w and np.all(idx[q, len(w):] == -1)
        assert score[q, :len(w)].tolist() == [S[q, e] for e in w] and np.all(np.isneginf(score[q, len(w):]))
    assert idx.dtype == np.int32 and score.dtype == np.float32 and count.dtype == np.int32


def test_the_restatement_on_random_ties():
    rng = np.random.Generator(np.random.PCG64(4))
    S = rng.integers(0, 3, size=(6, 40)).astype(np.float64)
    rows = [np.flatnonzero(rng.random(40) < 0.3) for _ in range(6)]
    idx, _, count = np_topn(S, csr_of(rows), 7)
    assert [idx[q, :count[q]].tolist() for q in range(6)] == brute_topn(S, rows, 7)


# ------------------------------------------------------------------------------------------------------------------ inputs of the GPU file
def excl_lists(Mq, Md, mode, seed):
    """none; random: every row with probability 0.4, and query 0 always lists the planted last row; all-but-three: every row but (up to) three
    of [0, Md - 1), the planted last row always listed; all"""
    rng = np.random.Generator(np.random.PCG64(seed))
    rows = []
    for q in range(Mq):
        if mode == "none":
            e = np.zeros(0, dtype=np.int64)
        elif mode == "random":
            e = np.flatnonzero(rng.random(Md) < 0.4)
            if q == 0:
                e = np.union1d(e, [Md - 1])
        elif mode == "all-but-three":
            keep = rng.choice(Md - 1, size=min(3, Md - 1), replace=False) if Md > 1 else []
            e = np.setdiff1d(np.arange(Md), keep)
        else:
            e = np.arange(Md)
        rows.append(e)
    return csr_of(rows)


def topn_case(Md, Mq, K, mode):
    """the integer features of exact_case (every score an integer below 2^24, ties everywhere, the last database row all 15: it comes before
    every other row of every query) with exclusion lists of this feature's own: exact_case's never name the last row"""
    xd, xq, _, _ = exact_case(Md, Mq, K, "none", "one_each")
    return xd, xq, excl_lists(Mq, Md, mode, seed=13 * Md + 7 * Mq + K)


def test_the_exact_inputs_are_what_the_gpu_file_relies_on():
    for mode in EXCL:
        xd, xq, excl = topn_case(2 * T + 2, 65, 50, mode)
        S = xq.T @ xd
        assert S.max() < 2 ** 24 and np.array_equal(S, S.astype(np.float32).astype(np.float64)) and np.all(S[:, -1] > S[:, :-1].max(axis=1))
        lens = np.diff(excl[0])
        last = np.array([lens[q] > 0 and excl[1][excl[0][q + 1] - 1] == 2 * T + 1 for q in range(65)])
        assert {"none": not lens.any(), "random": last[0] and 0 < last.sum() < 65, "all-but-three": last.all() and np.all(lens == 2 * T - 1),
                "all": np.all(lens == 2 * T + 2)}[mode]
    for Md in (1, 2):                                                # the smallest databases: all-but-three keeps nothing / row 0
        _, _, excl = topn_case(Md, 3, 2, "all-but-three")
        assert np.all(np.diff(excl[0]) == 1) and np.all(excl[1] == Md - 1)


# ------------------------------------------------------------------------------------------------------------------ tmvb_score_topn: errors
def _base():
    return dict(K=3, xd=np.arange(15, dtype=np.float64).reshape(3, 5), xq=np.ones((3, 2)), excl=([0, 1, 1], [2]), n=2, splits=0)


def topn_error_cases():
    b = _base()
    return [
        ("K above 1024", dict(b, K=1025, xd=np.ones((1025, 5)), xq=np.ones((1025, 2))), EINVAL, "K = 1025"),
        ("n zero", dict(b, n=0), EINVAL, "n = 0 outside [1, 64]"),
        ("n above 64", dict(b, n=65), EINVAL, "n = 65 outside [1, 64]"),
        ("splits negative", dict(b, splits=-1), EINVAL, "splits = -1"),
        ("splits above Md", dict(b, splits=6), EINVAL, "splits = 6"),
        ("nan in the database", dict(b, xd=np.where(np.arange(15).reshape(3, 5) == 7, np.nan, 1.0)), ESHAPE, "non-finite entry (database row 2)"),
        ("inf in the queries", dict(b, xq=np.array([[1.0, 1.0], [1.0, np.inf], [0.0, 0.0]])), ESHAPE, "non-finite entry (query row 1)"),
        ("pointer not from 0", dict(b, excl=([1, 1, 1], [2])), ESHAPE, "excl_ptr must start at 0"),
        ("pointer decreases", dict(b, excl=([0, 1, 0], [2])), ESHAPE, "excl_ptr decreases at query 1"),
        ("id out of range", dict(b, excl=([0, 1, 2], [2, 5])), ESHAPE, "query 1 holds excluded id 5 outside [0, 5)"),
        ("id negative", dict(b, excl=([0, 1, 1], [-1])), ESHAPE, "query 0 holds excluded id -1 outside [0, 5)"),
        ("ids repeated", dict(b, excl=([0, 2, 2], [2, 2])), ESHAPE, "the excluded ids of query 0 are not strictly ascending"),
        ("ids descending", dict(b, excl=([0, 0, 2], [3, 1])), ESHAPE, "the excluded ids of query 1 are not strictly ascending"),
    ]


def call(tmvb, ctx, kw):
    return tmvb.rec_topn_raw(ctx, kw["K"], kw["xd"], kw["xq"], kw["excl"], kw["n"], kw["splits"])


@pytest.mark.parametrize("case", topn_error_cases(), ids=lambda c: c[0].replace(" ", "_"))
def test_score_topn_argument_errors_without_a_context(tmvb, case):
    _, kw, status, msg = case
    rc, res = call(tmvb, None, kw)
    assert rc == status and isinstance(res, str) and msg in res, (rc, res)


def test_score_topn_shape_errors_through_the_abi(tmvb):
    """K = 0, Md = 0, Mq = 0, Md = 2^31, a NULL argument and 2^31 - 1 listed ids cannot be said with an array: the C call itself (no entry is
    read before these are judged)"""
    L = tmvb.lib()
    PD, P32, P64, PF = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_float)
    x = np.ones(8); ptr = np.zeros(3, dtype=np.int64); idx = np.zeros(2, dtype=np.int32); out = np.zeros(8, dtype=np.int32); sc = np.zeros(8, dtype=np.float32)
    a = [x.ctypes.data_as(PD), x.ctypes.data_as(PD), ptr.ctypes.data_as(P64), idx.ctypes.data_as(P32), out.ctypes.data_as(P32), sc.ctypes.data_as(PF),
         out.ctypes.data_as(P32)]

    def go(K, Md, Mq, p=a):
        rc = L.tmvb_score_topn(None, K, Md, p[0], Mq, p[1], p[2], p[3], 2, 0, p[4], p[5], p[6], None)
        return rc, L.tmvb_last_error().decode()

    for K, Md, Mq, msg in ((0, 2, 2, "K = 0"), (-1, 2, 2, "K = -1"), (2, 0, 1, "Md and Mq must be positive"), (2, 2, 0, "Md and Mq must be positive"),
                           (2, -4, 1, "Md and Mq must be positive"), (2, 2 ** 31, 1, "2^31 or more")):
        rc, err = go(K, Md, Mq)
        assert rc == EINVAL and msg in err, (K, Md, Mq, rc, err)
    for hole in (0, 1, 2, 4, 5, 6):                                  # xd, xq, excl_ptr, idx, score, count (the id array may be NULL when empty)
        rc, err = go(2, 2, 2, [None if q == hole else v for q, v in enumerate(a)])
        assert rc == EINVAL and "NULL argument" in err, (hole, rc, err)
    ptr1 = np.array([0, 1, 1], dtype=np.int64)                       # ... and not when the pointers say there are ids
    rc, err = go(2, 2, 2, a[:2] + [ptr1.ctypes.data_as(P64), None] + a[4:])
    assert rc == EINVAL and "NULL argument" in err
    big = np.array([0, 2 ** 31 - 1, 2 ** 31 - 1], dtype=np.int64)    # judged from the pointers alone: no id is read
    rc, err = go(2, 2, 2, a[:2] + [big.ctypes.data_as(P64)] + a[3:])
    assert rc == EINVAL and "2147483647 excluded ids" in err, (rc, err)


def test_valid_arguments_without_a_device_are_enodevice(tmvb):
    """No silent CPU path: the arguments pass, then a NULL context on a machine without a GPU is TMVB_ENODEVICE."""
    if tmvb.lib().tmvb_device_count() > 0:
        pytest.skip("a GPU is visible: tests/test_rectopn_gpu.py covers the live path")
    xd, xq, excl = topn_case(33, 5, 3, "random")
    for kw in (_base(), dict(_base(), splits=5, n=64), dict(K=3, xd=xd, xq=xq, excl=excl, n=15, splits=0)):
        rc, res = call(tmvb, None, kw)
        assert rc == ENODEVICE and "no HIP device" in res, (rc, res)
    with pytest.raises(tmvb.EngineError):
        tmvb.recommend_topn(tmvb.CTPF(tmvb.syn_citeu(M=12, V=30, U=6, seed=1), 3))


# ------------------------------------------------------------------------------------------------------------------ the mirror
def test_recommend_topn_argument_errors(tmvb):
    m = tmvb.CTPF(tmvb.syn_citeu(M=12, V=30, U=6, seed=1), 3)
    with pytest.raises(tmvb.TopicModelError, match="CTPF"):
        tmvb.recommend_topn(tmvb.LDA(tmvb.syn_nsf(M=6, V=20, seed=1), 3))
    with pytest.raises(ValueError, match="by must be"):
        tmvb.recommend_topn(m, by="rows")
    for bad in (0, 65, -1, 2.5):
        with pytest.raises(ValueError, match="topn must be"):
            tmvb.recommend_topn(m, topn=bad)
    for by, bad in (("user", [0]), ("user", [7]), ("doc", [13]), ("doc", [])):
        with pytest.raises(tmvb.CorpusError, match="outside corpus range"):
            tmvb.recommend_topn(m, by=by, ids=bad)


def test_slice_csr():
    ptr, idx = csr_of([[1, 4], [], [0, 2, 3], [5]])
    for sel in ([2, 0, 3], [1], [3, 3, 1, 0], [0, 1, 2, 3]):
        p, i = TOPN.slice_csr(ptr, idx, sel)
        want = csr_of([idx[ptr[s]:ptr[s + 1]] for s in sel])
        assert p.dtype == np.int64 and i.dtype == np.int32 and p[0] == 0 and np.array_equal(p, want[0]) and np.array_equal(i, want[1])


@pytest.mark.parametrize("by", ["user", "doc"])
def test_ids_make_the_call_on_the_slice(tmvb, by, monkeypatch):
    """recommend_topn hands the library the selected queries only -- their factors and their own exclusion lists, rebased to 0, in the order
    asked for --, the whole database, and returns the 1-based ids beside the rows.  The call itself is replaced by a recorder."""
    m = tmvb.CTPF(tmvb.syn_citeu(M=14, V=30, U=9, seed=2), 3)
    seen = {}

    def recorder(ctx, K, xd, xq, excl, n, splits=0):
        seen.update(K=K, xd=xd, xq=xq, excl=excl, n=n, splits=splits)
        Mq = xq.shape[1]
        return 0, {"idx": np.zeros((Mq, n), dtype=np.int32), "score": np.zeros((Mq, n), dtype=np.float32), "count": np.zeros(Mq, dtype=np.int32),
                   "splits": 1, "kp": 4, "ms_prep": 0.0, "ms_scan": 0.0, "ms_merge": 0.0}

    monkeypatch.setattr(TOPN, "rec_topn_raw", recorder)
    monkeypatch.setattr(TOPN, "call_context", lambda device_id, ctx=None: contextlib.nullcontext(None))
    X, Y = TOPN.ctpf_factors(m)
    xd, xq = (X, Y) if by == "user" else (Y, X)
    pc = m.corp
    if by == "user":
        lists = [sorted({d for d in range(pc.M) if u in pc.readers[pc.rdr_ptr[d]:pc.rdr_ptr[d + 1]]}) for u in range(pc.U)]
    else:
        lists = [sorted(set(pc.readers[pc.rdr_ptr[d]:pc.rdr_ptr[d + 1]].tolist())) for d in range(pc.M)]
    for ids in ([3, 1, xq.shape[1]], 2, None):
        r = tmvb.recommend_topn(m, topn=5, by=by, ids=ids, splits=2)
        sel = np.arange(xq.shape[1]) if ids is None else np.atleast_1d(ids) - 1
        assert r.by == by and np.array_equal(r.ids, sel + 1) and r.idx.shape == (len(sel), 5)
        assert seen["K"] == 3 and seen["n"] == 5 and seen["splits"] == 2 and np.array_equal(seen["xd"], xd) and np.array_equal(seen["xq"], xq[:, sel])
        want = csr_of([lists[s] for s in sel])
        assert np.array_equal(seen["excl"][0], want[0]) and np.array_equal(seen["excl"][1], want[1]) and seen["excl"][0][0] == 0


# ------------------------------------------------------------------------------------------------------------------ static checks
def test_the_new_unit_owns_no_device_scratch():
    _units_own_no_device_scratch("tmvb_rectopn.hip")


def test_header_structure_sources_and_exports(tmvb):
    syms = tmvb.exported_symbols()
    assert "tmvb_score_topn" in syms and hasattr(C.CDLL(tmvb.LIB_PATH), "tmvb_score_topn")
    assert tmvb.lib().tmvb_abi_version() == 2                        # a new function does not break an existing caller
    for name in ("rec_topn_raw", "recommend_topn", "RecTopN"):
        assert name in tmvb.__all__ and getattr(tmvb, name) is not None
    assert callable(getattr(tmvb.gpuCTPF, "recommend_topn"))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tmvb.h")).read(), flags=re.S)
    assert int(re.search(r"#define TMVB_NB_TOPN_MAX (\d+)", hdr).group(1)) == TOPN.TOPN_MAX == 64
    fields = re.search(r"typedef struct \{([^}]*)\} tmvb_rectopn_info_t;", hdr).group(1)
    assert re.findall(r"\b(\w+)\s*[;,]", fields) == [f[0] for f in tmvb._lib.RecTopNInfo._fields_]
    args = re.search(r"int tmvb_score_topn\(([^;]*)\);", hdr).group(1)
    assert len(args.split(",")) == len(tmvb.lib().tmvb_score_topn.argtypes) == 14
    csrc = os.path.join(ROOT, "topicmodelsvb.jl_amd", "csrc")
    assert "tmvb_rectopn.hip" in tmvb._lib.SOURCES and "tmvb_rectopn.hip" in open(os.path.join(ROOT, "Makefile")).read()
    assert "tmvb_score_topn" in open(os.path.join(csrc, "tmvb_call.h")).read().split("#pragma once")[0]
    assert "TMVB_MUTANT_TOPN_MISS_LAST_EXCL" in open(os.path.join(csrc, "tmvb_internal.h")).read()
    assert "tmvb_rectopn.hip -DTMVB_MUTANT_TOPN_MISS_LAST_EXCL=1" in open(os.path.join(ROOT, "tools", "build_mutants.sh")).read()
    # the tile loop and the layout are shared, not copied; no atomics on global memory (the one atomicAdd is the LDS append counter)
    src = open(os.path.join(csrc, "tmvb_rectopn.hip")).read()
    assert '#include "tmvb_nbtile.h"' in src and "nb_tile_scores(" in src and "nb_feature_row(" in src
    assert "__builtin_amdgcn_mfma" not in src and "nb_perm(int k)" not in src
    assert re.findall(r"atomic\w+\(([^,]*),", src) == ["s_cnt"]


def test_julia_shim_binds_the_entry_point():
    src = open(os.path.join(ROOT, "topicmodelsvb.jl_amd", "julia", "TMVBHip.jl")).read()
    assert ":tmvb_score_topn" in src and "function score_topn(" in src and "mutable struct TmvbRecTopNInfo" in src
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tmvb.h")).read(), flags=re.S)
    names = re.findall(r"\b(\w+)\s*[;,]", re.search(r"typedef struct \{([^}]*)\} tmvb_rectopn_info_t;", hdr).group(1))
    body = src[src.index("mutable struct TmvbRecTopNInfo"):]
    assert re.findall(r"(\w+)::", body[:body.index("TmvbRecTopNInfo() =")]) == names


def test_the_kernels_are_in_the_resource_table_without_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    names = ("rt_feature_kernel", "rt_scan_kernel", "rt_merge_kernel")
    assert all(kr.BENCHED.get(k) == 0 for k in names)
    recorded = open(os.path.join(ROOT, "profiles", "rectopn_kernel_resources.txt")).read()
    assert all(k in recorded for k in names)
    lib = os.path.join(ROOT, "topicmodelsvb.jl_amd", "libtmvb_hip.so")
    if not (os.path.exists(lib) and os.path.exists(kr.READELF)):
        pytest.skip("needs the built library and llvm-readelf")
    rows = [r for r in kr.kernels(lib) if r["demangled"].startswith(names)]
    assert len(rows) == 3 and all(r["scratch"] == 0 and r["vgpr_spills"] == 0 for r in rows), rows
