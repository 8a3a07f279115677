// tmvb_estep_plan.h -- the E-step launch plans of LDA and CTPF (host only).
// A plan is the processing order of the documents plus one record per kernel launch: which kernel, which documents of the order, which stream.
// The builders are functions of the document lengths, KP and the path flags alone; tmvb_lda_create / tmvb_ctpf_create call them once and
// the E-steps walk the records.
#pragma once
#include "tmvb_common_kernels.h"

// Stream of a launch.  CHAIN: the critical chain document kernels -> statistics pass -> M-step: the context's stream (LDA without a register
// path: aux[0]).  LONG: aux[1], the latency-bound long documents next to the chain.  BESIDE: aux[0], CTPF's wide single-wave classes.
// A model without a register path has LDS-tile launches only and alternates them LONG / BESIDE.
enum class tmvb_role : int32_t { CHAIN, LONG, BESIDE };
static inline tmvb_role tmvb_lds_role(bool reg_path, size_t i) { return (reg_path || (i & 1) == 0) ? tmvb_role::LONG : tmvb_role::BESIDE; }

// ------------------------------------------------------------------------------------ LDA
// long documents: one workgroup of TMVB_LONG_WAVES waves per document (see lda_estep_reg_body, W > 1)
#define TMVB_LONG_WAVES 4

static constexpr bool lda_reg_lpr_supported(int lpr) { return lpr >= 1 && lpr <= 25 && (lpr & 1); }   // every KP = 4 * odd <= 100
// 64-token register tiles per document: the tile costs T * KP VGPRs of the 512 available per lane
// tiles * KP + KP / 4 + ~35 VGPRs must stay within the 256 architectural VGPRs (beyond that the tile spills to AGPRs;
// measured still ahead of the LDS-tile kernel at KP = 100, T = 3)
static constexpr int lda_reg_max_tiles(int lpr) { return lpr <= 13 ? 4 : (lpr <= 17 || lpr == 25) ? 3 : 2; }
// token pairs per lane of the widest grid-tile instantiation: 2 NP LPR tile registers + 2 LPR accumulators + ~40 must stay
// within the 256 architectural VGPRs.  KP <= 60: 6 pairs (documents of <= 192 unique terms per wave), KP <= 76: 4, KP <= 100: 3.
constexpr int lda_grid_np_max(int lpr) { return lpr <= 15 ? 6 : lpr <= 19 ? 4 : 3; }
// token-pair classes of the grid-tile kernel: a document runs the smallest instantiated NP (2, 3, 4, 6 up to the maximum) that holds it
static inline int lda_grid_np_class(int64_t n, int np_max)
{
    const int64_t np = (n + 31) / 32;
    const int c = np <= 2 ? 2 : np <= 3 ? 3 : np <= 4 ? 4 : 6;
    return c <= np_max ? c : np_max;
}

enum class lda_kind : int32_t {
    LDS_TILE,     // lda_estep_kernel, tile_rows rows in LDS (the last bucket streams chunks)
    REG,          // lda_estep_reg_kernel<LPR, n>: n 64-token tiles
    REG_ANY,      // lda_estep_reg_any_kernel: mixed tile counts
    REG_LONG,     // lda_estep_reg_long_kernel<LPR, n>: TMVB_LONG_WAVES waves per document
    GRID,         // lda_estep_grid_kernel<LPR, n>: n token pairs per lane (tmvb_gridtile.h)
    GRID_ANY,     // lda_estep_grid_any_kernel: mixed lengths
    GRID_LONG,    // lda_estep_grid_long_kernel<LPR, NPmax, waves>
    TWO_COPY      // lda_estep_tt_kernel: documents of <= 64 unique terms (KP <= 60)
};
struct lda_launch {
    lda_kind kind = lda_kind::LDS_TILE;
    tmvb_role role = tmvb_role::LONG;
    int64_t first = 0, count = 0;      // documents [first, first + count) of the order
    int32_t tile_rows = 0;             // LDS_TILE
    int32_t n = 0;                     // REG / REG_LONG: tiles T;  GRID: token pairs NP
    int32_t waves = 1;                 // per document
    int32_t piece = 0;                 // pipelined E-step: which statistics pass consumes these documents
};
struct lda_plan_flags {
    bool reg_path, grid_path;
    bool one_launch;                   // small corpora (one statistics pass, KP <= 60): every single-wave document in one mixed launch
    bool two_copy;                     // TMVB_LDA_TT=1
};

static inline void lda_build_plan(const std::vector<int64_t>& len, int KP, const lda_plan_flags& f, std::vector<int32_t>& order, std::vector<lda_launch>& plan)
{
    const int64_t M = (int64_t)len.size();
    order.resize((size_t)M);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return len[x] > len[y]; });
    plan.clear();
    const int max_tiles = lda_reg_max_tiles(KP / 4), np_max = lda_grid_np_max(KP / 4);
    const int64_t reg_max = f.grid_path ? 32 * np_max : f.reg_path ? 64 * max_tiles : -1;
    auto put = [&](lda_kind kind, tmvb_role role, int64_t first, int64_t count, int n, int waves) {
        lda_launch b; b.kind = kind; b.role = role; b.first = first; b.count = count; b.n = n; b.waves = waves;
        plan.push_back(b);
    };
    // documents longer than reg_max: LDS-tile kernel
    // long documents get up to 156 KiB of LDS (one workgroup per CU): a tile that holds the whole document is
    // gathered once per E-step, a streamed one once per sweep
    // Documents between 64 T and 64 T W unique terms keep the register-tile arithmetic with one workgroup of
    // W = TMVB_LONG_WAVES waves each (lda_estep_reg_long_kernel); only what is longer still goes through LDS.
    const int64_t long_max = f.reg_path ? (int64_t)64 * max_tiles * TMVB_LONG_WAVES : reg_max;
    std::vector<tmvb_bucket> lds;
    int64_t pos = tmvb_build_lds_buckets(len, order, M, KP, long_max, 3, lds, TMVB_BIG_TILE_BYTES);
    for (size_t i = 0; i < lds.size(); ++i) {
        put(lda_kind::LDS_TILE, tmvb_lds_role(f.reg_path, i), lds[i].first, lds[i].count, 0, 1);
        plan.back().tile_rows = lds[i].tile_rows;
    }
    auto longer_than = [&](int64_t lo) { int64_t cnt = 0; while (pos + cnt < M && len[order[pos + cnt]] > lo) ++cnt; return cnt; };
    // grid-tile kernel with 4 / 2 waves per document: up to 768 / 384 unique terms
    const int64_t grid_long_max = (f.grid_path && f.reg_path) ? (int64_t)32 * np_max * 4 : 0;
    if (f.reg_path) {
        for (int T = max_tiles; T >= 1 && pos < M; --T) {   // (KP = 100, T = 3 spills to AGPRs and is still 2.8x the LDS kernel)
            const int64_t cnt = longer_than(std::max<int64_t>(std::max<int64_t>(64 * TMVB_LONG_WAVES * (int64_t)(T - 1), reg_max), grid_long_max));
            if (cnt) put(lda_kind::REG_LONG, tmvb_role::LONG, pos, cnt, T, TMVB_LONG_WAVES);
            pos += cnt;
        }
        for (int Wv = 4; Wv >= 2 && grid_long_max > 0 && pos < M; Wv >>= 1) {
            const int64_t cnt = longer_than((int64_t)32 * np_max * (Wv / 2));
            if (cnt) put(lda_kind::GRID_LONG, tmvb_role::LONG, pos, cnt, np_max, Wv);
            pos += cnt;
        }
    }
    // small corpora (one statistics pass): ONE launch for all register-tile documents, longest first
    // (KP <= 60 only: with two result slots per lane the widest body costs the short documents a wave per SIMD --
    //  measured at KP = 100, 16 k documents: 2.14 k it/s merged, 2.26 k separate)
    if (f.one_launch && pos < M) {
        put(f.grid_path ? lda_kind::GRID_ANY : lda_kind::REG_ANY, tmvb_role::CHAIN, pos, M - pos, 0, 1);
        return;
    }
    if (f.grid_path) {
        // grid-tile launches, longest first: one per instantiated pair count (0 here: the two-copy kernel)
        auto cls = [&](int64_t n) { return (f.two_copy && n <= 64) ? 0 : lda_grid_np_class(n, np_max); };
        while (pos < M) {
            const int np = cls(len[order[pos]]);
            int64_t cnt = 0;
            while (pos + cnt < M && cls(len[order[pos + cnt]]) == np) ++cnt;
            put(np ? lda_kind::GRID : lda_kind::TWO_COPY, tmvb_role::CHAIN, pos, cnt, np, 1);
            pos += cnt;
        }
        return;
    }
    // register-tile launches: T = ceil(N / 64) tiles of 64 tokens
    for (int T = max_tiles; T >= 1 && pos < M; --T) {
        const int64_t cnt = T == 1 ? M - pos : longer_than(64 * (int64_t)(T - 1));
        if (cnt) put(lda_kind::REG, tmvb_role::CHAIN, pos, cnt, T, 1);
        pos += cnt;
    }
}

// Cut the chain's launches where the running token count crosses a multiple of nnz / P.  The launches beside the chain
// (long documents) go with the LAST piece: they are issued first, on their own stream, and have the
// whole E-step to finish.  Fills doc_piece[d] and replaces the plan.
static inline void lda_cut_pieces(const std::vector<int64_t>& len, int64_t nnz, const std::vector<int32_t>& order, int P, std::vector<lda_launch>& plan,
                                  std::vector<int32_t>& doc_piece)
{
    nnz = std::max<int64_t>(nnz, 1);
    // cumulative token fractions at which a piece ends: the last pieces are smaller, because the statistics
    // pass of the last piece has no document kernels left to hide under
    std::vector<double> cum(P);
    {
        double tot = 0.0;
        for (int q = 0; q < P; ++q) { cum[q] = 1.0 + 0.5 * (double)(P - 1 - q) / (double)std::max(P - 1, 1); tot += cum[q]; }
        double run = 0.0;
        for (int q = 0; q < P; ++q) { run += cum[q] / tot; cum[q] = run; }
        cum[P - 1] = 2.0;
    }
    auto piece_of = [&](int64_t run) { const double x = (double)run / (double)nnz; int q = 0; while (q < P - 1 && x >= cum[q]) ++q; return q; };
    doc_piece.assign(len.size(), 0);
    std::vector<lda_launch> cut;
    int64_t run = 0;
    for (const lda_launch& b : plan) {
        auto put = [&](int64_t first, int64_t end, int piece) { lda_launch c = b; c.first = first; c.count = end - first; c.piece = piece; cut.push_back(c); };
        if (b.role != tmvb_role::CHAIN) {
            for (int64_t q = b.first; q < b.first + b.count; ++q) doc_piece[order[q]] = P - 1;
            put(b.first, b.first + b.count, P - 1);
            continue;
        }
        int64_t start = b.first;
        int piece = piece_of(run);
        for (int64_t q = b.first; q < b.first + b.count; ++q) {
            const int pq = piece_of(run);
            if (pq != piece) {
                if (q > start) put(start, q, piece);
                start = q; piece = pq;
            }
            doc_piece[order[q]] = pq;
            run += len[order[q]];
        }
        if (b.first + b.count > start) put(start, b.first + b.count, piece);
    }
    plan.swap(cut);
}

// ------------------------------------------------------------------------------------ CTPF
// length classes of the grid-tile kernels (term pairs, reader pairs per lane): single-wave (2, 1) (3, 1) (4, 1) (6, 1) = documents of <= 32 readers
// by their terms (<= 64 / 96 / 128 / 192), and (4, 2) = <= 128 terms with <= 64 readers;
// multi-wave classes, four waves per document: (2 term pairs, 4 reader pairs) = <= 256 terms, <= 512 readers, and (3, 3) = <= 384, <= 384
struct ctpf_grid_cls { int waves = 0, npt = 0, npr = 0; };          // waves = 0: no grid-tile class holds the document
static inline bool operator==(const ctpf_grid_cls& x, const ctpf_grid_cls& y) { return x.waves == y.waves && x.npt == y.npt && x.npr == y.npr; }
static inline ctpf_grid_cls ctpf_grid_class(int64_t n, int64_t r)
{
    if (r <= 32 && n <= 192) return {1, n <= 64 ? 2 : n <= 96 ? 3 : n <= 128 ? 4 : 6, 1};
    if (r <= 64 && n <= 128) return {1, 4, 2};
    if (n <= 256 && r <= 512) return {4, 2, 4};
    if (n <= 384 && r <= 384) return {4, 3, 3};
    return {};
}

enum class ctpf_kind : int32_t {
    LDS_TILE,       // ctpf_estep_kernel, tile_rows rows (terms + readers) in LDS
    REG,            // ctpf_estep_reg_kernel<LPR, n>: n 64-term tiles
    REG_ANY,        // ctpf_estep_reg_any_kernel: both tile counts
    GRID_NARROW,    // ctpf_estep_grid_narrow_kernel: classes (2, 1) (3, 1)
    GRID_WIDE,      // ctpf_estep_grid_wide_kernel: classes (4, 1) (6, 1) (4, 2)
    GRID_LONG,      // ctpf_estep_grid_long_kernel<LPR, npt, npr, 4>: one four-wave class
    GRID_LONG2      // ctpf_estep_grid_long2_kernel: the first count_a documents (3, 3), the others (2, 4)
};
struct ctpf_launch {
    ctpf_kind kind = ctpf_kind::LDS_TILE;
    tmvb_role role = tmvb_role::LONG;
    int64_t first = 0, count = 0;      // documents [first, first + count) of the order
    int32_t count_a = 0;               // GRID_LONG2
    int32_t tile_rows = 0;             // LDS_TILE
    int32_t n = 0;                     // REG: tiles T
    int32_t npt = 0, npr = 0;          // GRID_LONG
    int32_t waves = 1;                 // per document
};

// processing order: first the documents of the LDS-tile kernel by rows (terms + readers), longest first, in LDS
// buckets on the combined row count; then the register-tile documents (<= 128 terms and <= 64 readers) by tiles; then the grid-tile
// classes, longest class first.  Classes that share a kernel leave as ONE launch: the two four-wave classes (ctpf_estep_grid_long2_kernel),
// the narrow and the wide single-wave classes, the two register-tile tile counts.
static inline void ctpf_build_plan(const std::vector<int64_t>& doc_len, const std::vector<int64_t>& rdr_len, int KP, bool reg_path, bool grid_path,
                                   std::vector<int32_t>& order, std::vector<ctpf_launch>& plan)
{
    const int64_t M = (int64_t)doc_len.size();
    std::vector<int64_t> len((size_t)M);
    std::vector<int32_t> reg2, reg1;
    std::vector<std::pair<ctpf_grid_cls, int32_t>> gdocs;
    order.clear(); plan.clear();
    for (int64_t d = 0; d < M; ++d) {
        len[d] = doc_len[d] + rdr_len[d];
        const ctpf_grid_cls c = grid_path ? ctpf_grid_class(doc_len[d], rdr_len[d]) : ctpf_grid_cls{};
        if (c.waves) { gdocs.emplace_back(c, (int32_t)d); continue; }
        const bool reg = reg_path && !grid_path && doc_len[d] <= 128 && rdr_len[d] <= 64;
        if (!reg) order.push_back((int32_t)d);
        else if (doc_len[d] > 64) reg2.push_back((int32_t)d);
        else reg1.push_back((int32_t)d);
    }
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return len[x] > len[y]; });
    std::vector<tmvb_bucket> lds;
    tmvb_build_lds_buckets(len, order, (int64_t)order.size(), KP, -1, 3, lds, reg_path ? TMVB_BIG_TILE_BYTES : TMVB_MAX_TILE_BYTES);
    auto put = [&](ctpf_kind kind, tmvb_role role, int64_t count) -> ctpf_launch& {
        ctpf_launch b; b.kind = kind; b.role = role; b.first = (int64_t)order.size(); b.count = count;
        plan.push_back(b);
        return plan.back();
    };
    for (size_t i = 0; i < lds.size(); ++i) {
        ctpf_launch& b = put(ctpf_kind::LDS_TILE, tmvb_lds_role(reg_path, i), lds[i].count);
        b.first = lds[i].first; b.tile_rows = lds[i].tile_rows;
    }
    auto by_terms = [&](int32_t x, int32_t y) { return doc_len[x] > doc_len[y]; };
    std::stable_sort(reg2.begin(), reg2.end(), by_terms);
    std::stable_sort(reg1.begin(), reg1.end(), by_terms);
    if (!reg2.empty() && !reg1.empty()) put(ctpf_kind::REG_ANY, tmvb_role::CHAIN, (int64_t)(reg2.size() + reg1.size()));
    else if (!reg2.empty()) put(ctpf_kind::REG, tmvb_role::CHAIN, (int64_t)reg2.size()).n = 2;
    else if (!reg1.empty()) put(ctpf_kind::REG, tmvb_role::CHAIN, (int64_t)reg1.size()).n = 1;
    order.insert(order.end(), reg2.begin(), reg2.end());
    order.insert(order.end(), reg1.begin(), reg1.end());
    std::stable_sort(gdocs.begin(), gdocs.end(), [&](const std::pair<ctpf_grid_cls, int32_t>& x, const std::pair<ctpf_grid_cls, int32_t>& y) {
        const ctpf_grid_cls &a = x.first, &b = y.first;
        if (a.waves != b.waves) return a.waves > b.waves;
        if (a.npt != b.npt) return a.npt > b.npt;
        if (a.npr != b.npr) return a.npr > b.npr;
        return len[x.second] > len[y.second]; });
    for (size_t q = 0, e = 0; q < gdocs.size(); q = e) {
        const ctpf_grid_cls c = gdocs[q].first;
        while (e < gdocs.size() && gdocs[e].first == c) ++e;
        const int64_t cnt = (int64_t)(e - q);
        // the multi-wave (long) documents on aux[1] next to the chain, the single-wave classes as two mixed-class launches by register need:
        // narrow on the chain, wide on aux[0]
        const ctpf_kind kind = c.waves > 1 ? ctpf_kind::GRID_LONG : c.npt >= 4 ? ctpf_kind::GRID_WIDE : ctpf_kind::GRID_NARROW;
        ctpf_launch* prev = plan.empty() ? nullptr : &plan.back();       // (its documents end where this class begins)
        if (prev && kind != ctpf_kind::GRID_LONG && prev->kind == kind) {
            prev->count += cnt;
        } else if (prev && kind == ctpf_kind::GRID_LONG && c.npt == 2 && prev->kind == ctpf_kind::GRID_LONG && prev->npt == 3) {
            // (count_a is the kernel's int argument: a document id is an int32, so a class holds fewer than 2^31 documents)
            prev->kind = ctpf_kind::GRID_LONG2; prev->count_a = (int32_t)prev->count; prev->count += cnt; prev->npt = prev->npr = 0;
        } else {
            ctpf_launch& b = put(kind, c.waves > 1 ? tmvb_role::LONG : kind == ctpf_kind::GRID_WIDE ? tmvb_role::BESIDE : tmvb_role::CHAIN, cnt);
            b.waves = c.waves;
            if (kind == ctpf_kind::GRID_LONG) { b.npt = c.npt; b.npr = c.npr; }
        }
        for (size_t u = q; u < e; ++u) order.push_back(gdocs[u].second);
    }
}
