// tmvb_token_topics.hip -- word-topic assignments: the per-token responsibilities phi of update_phi! (src/LDA.jl:150-154, src/CTM.jl:175-178,
// src/CTPF.jl:327-330), recomputed from the factors, with the top-t topics of every entry selected in registers.  The engine
// never keeps phi (include/tmvb.h: update_host!); the reference fills model.phi for every document (src/modelutils.jl:514-515, :534-535, :559-560).
//
//   y_k = eps + A[k, d] B[k, w]        r_k = y_k / sum_j y_j        entry (w, c) of document d, k = 0 .. K - 1
//
// The kernel is a sibling of heldout_loglik_kernel (tmvb_heldout.hip): B staged as [V][KP] rows, the selected documents' A columns as [Ms][KP]
// rows, the document's A row in LDS, L = 2^logL lanes per entry (lane r takes the 16-byte chunks r, r + L, ... of the row, at most four), one
// workgroup per work item -- a run of entries of one selected document: 64 lanes up to TT_SHORT_TRIPS trips of a wave, 256 lanes beyond.
// What is new: a lane keeps its <= 16 values in registers across the sum, because they are needed again after it.
//   sum        (tmvb_token_phi.h, shared with tmvb_group_topics.hip) per lane ((y0 + y1) + (y2 + y3)) per chunk, chunks in ascending order; the L partial sums meet in a fixed xor butterfly, so every
//              lane of the entry holds the same bits of S; r = y / S is the IEEE fp32 division.
//   top-t      t rounds: a lane offers the best of its values not yet taken as a packed key (r bits << 32 | ~k: larger key = larger r, on equal
//              r the lower topic), the L keys meet in an xor butterfly of max, the lane that owned the winner marks it taken.  No LDS, no
//              scratch, no atomics.
//   hard       the leading lane of an entry adds c to bin (group, best topic) of an LDS table private to its lane group -- a plain read-modify-write,
//              no two lanes share a bin --; the groups' tables are summed per topic in group order at the end.  Integers: exact in any order.
//   dense      float4 stores into a padded [chunk][KP] device buffer, the pattern of the loads; compacted to [nsel][K] by the strided copy-out.
// Entries are processed in chunks of at most max_chunk_entries (a document is cut where a chunk ends; hard adds up over the cuts, chunks run in
// stream order): the result does not depend on the cuts.
#include "tmvb_internal.h"
#include "tmvb_call.h"
#include "tmvb_token_phi.h"

#include <algorithm>
#include <cstring>

#define TT_MAX_K 1024
#define TT_SHORT_TRIPS 4            // work items of at most this many trips of a wave stay on one wave
#define TT_DENSE_BYTES ((int64_t)1 << 28)   // default bound of the padded dense buffer: 256 MiB
#define TT_MAX_ENTRIES ((int64_t)INT32_MAX - 1)   // entries of the CSR and selected entries of one call: below this (tmvb_check_host_csr's limit)

// a run of entries of one selected document inside one chunk
struct tt_item {
    int64_t sel0;                   // number of its first entry among the selected entries (outputs top_*, staged terms / counts)
    int64_t loc0;                   // the same inside the chunk (dense buffer)
    int32_t slot;                   // position in docs (A row, hard row)
    int32_t n;                      // entries
};

// One workgroup of WG lanes per work item items[blockIdx.x].  A: [Ms][KP], B: [V][KP] (pads 0), rows 16-byte aligned.  t_sel = 0: no selection.
template <int WG, bool DENSE>
static __global__ __launch_bounds__(WG) void token_topics_kernel(int K, int KP, int logL, int t, int t_sel, float eps, const tt_item* __restrict__ items,
                                                                 const float* __restrict__ A, const float* __restrict__ B,
                                                                 const int32_t* __restrict__ terms, const int32_t* __restrict__ counts,
                                                                 int32_t* __restrict__ top_idx, float* __restrict__ top_r, float* __restrict__ phi,
                                                                 long long* __restrict__ hard)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char tt_lds[];      // KP floats of A, then (hard only) G K bins: tt_lds_bytes
    float* s_a = reinterpret_cast<float*>(tt_lds);
    unsigned* s_hard = reinterpret_cast<unsigned*>(tt_lds + (size_t)KP * sizeof(float));      // [G][K]; a document has fewer than 2^31 tokens
    const int tid = threadIdx.x, L = 1 << logL, r = tid & (L - 1), g = tid >> logL, G = WG >> logL;
    const tt_item it = items[blockIdx.x];
    const int n = it.n;
    const int nch = (K + 3) >> 2;                      // chunks that hold topics; a chunk of pads only (KP = 4 * odd) is never touched
    const float4* a4 = reinterpret_cast<const float4*>(A + (int64_t)it.slot * KP);
    float4* s4 = reinterpret_cast<float4*>(s_a);
    for (int c = tid; c < (KP >> 2); c += WG) s4[c] = a4[c];
    if (hard)
        for (int j = tid; j < G * K; j += WG) s_hard[j] = 0;
    __syncthreads();
    const unsigned vmask = tt_value_mask(K, r, L);     // bit 4 q + j: value j of the lane's q-th chunk is a topic
    for (int64_t i0 = 0; i0 < n; i0 += G) {            // uniform trip count: every lane takes part in the butterflies
        const int64_t i = i0 + g;
        const bool live = i < n;
        float y[16];
        int c_n = 0;
        const float4* row = nullptr;
        if (live) {
            c_n = counts[it.sel0 + i];
            row = reinterpret_cast<const float4*>(B + (int64_t)terms[it.sel0 + i] * KP);
        }
        float4 av[4], bv[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int c = r + q * L;
            bv[q] = make_float4(0.0f, 0.0f, 0.0f, 0.0f); av[q] = bv[q];
            if (live && c < nch) { bv[q] = row[c]; av[q] = s4[c]; }
        }
        tt_responsibilities(y, av, bv, vmask, eps, L, live);           // tmvb_token_phi.h; y is r from here on
        if (DENSE) {
            if (live) {
                float4* out = reinterpret_cast<float4*>(phi + (it.loc0 + i) * (int64_t)KP);
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int c = r + q * L;
                    if (c < nch) out[c] = make_float4(y[4 * q + 0], y[4 * q + 1], y[4 * q + 2], y[4 * q + 3]);
                }
            }
        }
        unsigned taken = ~vmask;
        for (int j = 0; j < t_sel; j++) {
            long long best = 0;                        // 0: nothing left (a real key has r bits or inverted id above 0)
#pragma unroll
            for (int e = 0; e < 16; e++) {
                const int k = 4 * (r + (e >> 2) * L) + (e & 3);
                const long long key = (taken >> e) & 1u ? 0ll : (long long)(((unsigned long long)__float_as_uint(y[e]) << 32) | (unsigned)~k);
                best = key > best ? key : best;
            }
            long long m = best;
            for (int o = L >> 1; o; o >>= 1) {
                const long long other = __shfl_xor(m, o);
#ifdef TMVB_MUTANT_TT_TIE_LAST
                // MUTANT: on equal r bits the HIGHER topic id wins the merge across lanes
                const bool take = (other >> 32) > (m >> 32) || ((other >> 32) == (m >> 32) && other != 0 && (m == 0 || other < m));
#else
                const bool take = other > m;
#endif
                m = take ? other : m;
            }
            const int kw = (int)~(unsigned)m;
            if (m != 0 && ((kw >> 2) & (L - 1)) == r) taken |= 1u << ((((kw >> 2) >> logL) << 2) | (kw & 3));
            if (live && r == 0) {
                if (top_idx && j < t) {
                    top_idx[(it.sel0 + i) * t + j] = m != 0 ? kw : -1;
                    top_r[(it.sel0 + i) * t + j] = m != 0 ? __uint_as_float((unsigned)(m >> 32)) : 0.0f;
                }
                if (hard && j == 0 && m != 0) s_hard[g * K + kw] += (unsigned)c_n;
            }
        }
    }
    if (hard) {
        __syncthreads();
        for (int k = tid; k < K; k += WG) {
            long long s = 0;
            for (int gg = 0; gg < G; gg++) s += (long long)s_hard[gg * K + k];
            hard[(int64_t)it.slot * K + k] += s;        // a slot has one work item per chunk, chunks run in stream order
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------ host
namespace {
// dynamic LDS of a workgroup of wg lanes: the A row, and with hard the G = wg / L tables of K bins (G K <= 16 wg: K <= 16 L)
size_t tt_lds_bytes(int wg, int K, int KP, int logL, bool hard)
{
    return (size_t)KP * sizeof(float) + (hard ? (size_t)(wg >> logL) * K * sizeof(unsigned) : 0);
}

template <bool DENSE>
void tt_launch(hipStream_t st, int64_t n_short, int64_t n_long, int K, int KP, int logL, int t, int t_sel, float eps, const tt_item* items, const float* A,
               const float* B, const int32_t* terms, const int32_t* counts, int32_t* top_idx, float* top_r, float* phi, long long* hard)
{
    if (n_short > 0)
        hipLaunchKernelGGL((token_topics_kernel<64, DENSE>), dim3((unsigned)n_short), dim3(64), (unsigned)tt_lds_bytes(64, K, KP, logL, hard != nullptr), st, K, KP, logL, t, t_sel, eps, items, A, B, terms, counts,
                           top_idx, top_r, phi, hard);
    if (n_long > 0)
        hipLaunchKernelGGL((token_topics_kernel<256, DENSE>), dim3((unsigned)n_long), dim3(256), (unsigned)tt_lds_bytes(256, K, KP, logL, hard != nullptr), st, K, KP, logL, t, t_sel, eps, items + n_short, A, B, terms,
                           counts, top_idx, top_r, phi, hard);
}

int tt_run(tmvb_ctx* ctx, int32_t K, int64_t V, const double* A, const double* B, const int64_t* doc_ptr, const int32_t* terms, const int32_t* counts,
           const int32_t* docs, int64_t Ms, int64_t nsel, float eps, int32_t t, int64_t cap, int32_t* top_idx, float* top_r, float* phi, int64_t* hard,
           tmvb_token_topics_info_t* info)
{
    const int KP = tmvb_kpad(K), logL = tt_log_lanes(K);
    const int64_t short_max = (int64_t)TT_SHORT_TRIPS * (64 >> logL);
    // host staging, declared in front of the call's scope: fp32 A rows of the selected documents, fp32 B rows, the selected entries, the work items
    std::vector<float> h_a((size_t)Ms * KP, 0.0f), h_b((size_t)V * KP, 0.0f);
    std::vector<int32_t> h_terms, h_counts;
    for (int64_t s = 0; s < Ms; s++) {
        const int64_t d = docs ? docs[s] : s;
        for (int k = 0; k < K; k++) h_a[(size_t)s * KP + k] = (float)A[k + (int64_t)K * d];
    }
    for (int64_t v = 0; v < V; v++)
        for (int k = 0; k < K; k++) h_b[(size_t)v * KP + k] = (float)B[k + (int64_t)K * v];
    if (docs) {                                        // the selected entries in docs order; with docs == NULL the caller's arrays are that already
        h_terms.reserve((size_t)nsel); h_counts.reserve((size_t)nsel);
        for (int64_t s = 0; s < Ms; s++) {
            h_terms.insert(h_terms.end(), terms + doc_ptr[docs[s]], terms + doc_ptr[docs[s] + 1]);
            h_counts.insert(h_counts.end(), counts + doc_ptr[docs[s]], counts + doc_ptr[docs[s] + 1]);
        }
        terms = h_terms.data(); counts = h_counts.data();
    }
    // chunks of at most cap entries; inside a chunk the short items first, then the long ones
    struct chunk { int64_t first, n_short, n_long, entries; };
    std::vector<chunk> chunks;
    std::vector<tt_item> h_items;
    {
        std::vector<tt_item> cur;
        int64_t fill = 0, sel = 0;
        auto flush = [&]() {
            chunk c{(int64_t)h_items.size(), 0, 0, fill};
            for (const tt_item& x : cur) if (x.n <= short_max) { h_items.push_back(x); c.n_short++; }
            for (const tt_item& x : cur) if (x.n > short_max) { h_items.push_back(x); c.n_long++; }
            chunks.push_back(c);
            cur.clear(); fill = 0;
        };
        for (int64_t s = 0; s < Ms; s++) {
            const int64_t d = docs ? docs[s] : s;
            int64_t left = doc_ptr[d + 1] - doc_ptr[d];
            while (left > 0) {
                const int64_t take = std::min(left, cap - fill);
                cur.push_back(tt_item{sel, fill, (int32_t)s, (int32_t)take});
                sel += take; fill += take; left -= take;
                if (fill == cap) flush();
            }
        }
        if (fill > 0) flush();
    }
    int64_t n_short = 0, n_long = 0;
    for (const chunk& c : chunks) { n_short += c.n_short; n_long += c.n_long; }
    const int t_sel = top_idx ? t : (hard ? 1 : 0);
    const int64_t dense_rows = phi ? std::min(cap, std::max<int64_t>(nsel, 1)) : 0;

    hipStream_t st = ctx->stream;
    tmvb_call c("token_topics", ctx->device, st);
    TMVB_CALL_TRY(c, c.begin());
    TMVB_CALL_TRY(c, c.events(2));
    float *d_a, *d_b, *d_top_r = nullptr, *d_phi = nullptr;
    int32_t *d_terms, *d_counts, *d_top_idx = nullptr;
    tt_item* d_items;
    long long* d_hard = nullptr;
    TMVB_CALL_TRY(c, c.upload(&d_a, (const float*)h_a.data(), h_a.size()));
    TMVB_CALL_TRY(c, c.upload(&d_b, (const float*)h_b.data(), h_b.size()));
    TMVB_CALL_TRY(c, c.upload(&d_terms, terms, (size_t)nsel));
    TMVB_CALL_TRY(c, c.upload(&d_counts, counts, (size_t)nsel));
    TMVB_CALL_TRY(c, c.upload(&d_items, (const tt_item*)h_items.data(), h_items.size()));
    if (top_idx) {
        TMVB_CALL_TRY(c, c.alloc(&d_top_idx, (size_t)nsel * t));
        TMVB_CALL_TRY(c, c.alloc(&d_top_r, (size_t)nsel * t));
    }
    if (phi) TMVB_CALL_TRY(c, c.alloc(&d_phi, (size_t)dense_rows * KP));
    if (hard) {
        TMVB_CALL_TRY(c, c.alloc(&d_hard, (size_t)Ms * K));
        TMVB_CALL_HIP(c, hipMemsetAsync(d_hard, 0, std::max<size_t>((size_t)Ms * K, 1) * sizeof(long long), st));
    }
    float ms_total = 0.0f;
    int64_t done = 0;
    for (const chunk& ch : chunks) {
        TMVB_CALL_HIP(c, hipEventRecord(c.ev(0), st));
        if (phi)
            tt_launch<true>(st, ch.n_short, ch.n_long, (int)K, KP, logL, (int)t, t_sel, eps, (const tt_item*)d_items + ch.first, d_a, d_b, d_terms, d_counts,
                            d_top_idx, d_top_r, d_phi, d_hard);
        else
            tt_launch<false>(st, ch.n_short, ch.n_long, (int)K, KP, logL, (int)t, t_sel, eps, (const tt_item*)d_items + ch.first, d_a, d_b, d_terms, d_counts,
                             d_top_idx, d_top_r, d_phi, d_hard);
        TMVB_CALL_HIP(c, hipGetLastError());
        TMVB_CALL_HIP(c, hipEventRecord(c.ev(1), st));
        if (phi)                                       // compaction: rows of KP floats on the device, of K floats at the caller's
            TMVB_CALL_HIP(c, hipMemcpy2DAsync(phi + (size_t)done * K, (size_t)K * sizeof(float), d_phi, (size_t)KP * sizeof(float), (size_t)K * sizeof(float),
                                              (size_t)ch.entries, hipMemcpyDeviceToHost, st));
        TMVB_CALL_HIP(c, hipStreamSynchronize(st));    // the dense buffer and the two events are used again by the next chunk
        float ms = 0.0f;
        TMVB_CALL_TRY(c, c.elapsed(&ms, 0, 1));
        ms_total += ms;
        done += ch.entries;
    }
    if (top_idx && nsel > 0) {
        TMVB_CALL_HIP(c, hipMemcpyAsync(top_idx, d_top_idx, (size_t)nsel * t * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        TMVB_CALL_HIP(c, hipMemcpyAsync(top_r, d_top_r, (size_t)nsel * t * sizeof(float), hipMemcpyDeviceToHost, st));
    }
    static_assert(sizeof(long long) == sizeof(int64_t), "hard counts travel as 64-bit integers");
    if (hard && Ms > 0) TMVB_CALL_HIP(c, hipMemcpyAsync(hard, d_hard, (size_t)Ms * K * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    TMVB_CALL_HIP(c, hipStreamSynchronize(st));
    if (info) {
        info->nsel = nsel; info->n_short = n_short; info->n_long = n_long;
        info->chunks = (int32_t)chunks.size(); info->lanes_per_entry = 1 << logL; info->ms_kernel = ms_total;
    }
    return TMVB_OK;
}
}  // namespace

extern "C" int tmvb_token_topics(tmvb_ctx* ctx, int32_t K, int64_t V, int64_t M, const double* A, const double* B, const int64_t* doc_ptr,
                                 const int32_t* terms, const int32_t* counts, const int32_t* docs, int64_t Ms, double eps, int32_t t,
                                 int64_t max_chunk_entries, int32_t* top_idx, float* top_r, float* phi, int64_t* hard, tmvb_token_topics_info_t* info)
{
    const char* fn = "tmvb_token_topics";
    if (info) memset(info, 0, sizeof(*info));
    TMVB_REQUIRE(K >= 1 && K <= TT_MAX_K, TMVB_EINVAL, "%s: K = %d outside [1, %d]", fn, K, TT_MAX_K);
    TMVB_REQUIRE(t >= 1 && t <= TMVB_TT_TOP_MAX, TMVB_EINVAL, "%s: t = %d outside [1, %d]", fn, t, TMVB_TT_TOP_MAX);
    TMVB_REQUIRE(eps >= 0x1p-100 && eps <= 1.0, TMVB_EINVAL, "%s: eps must lie in [2^-100, 1]", fn);      // NaN fails both
    TMVB_REQUIRE(M > 0 && V > 0 && M < (int64_t)INT32_MAX && V < (int64_t)INT32_MAX, TMVB_EINVAL, "%s: M and V must be positive integers below 2^31 - 1", fn);
    TMVB_REQUIRE(A && B && doc_ptr && terms && counts, TMVB_EINVAL, "%s: NULL argument", fn);
    TMVB_REQUIRE(top_idx || phi || hard, TMVB_EINVAL, "%s: every output is NULL", fn);
    TMVB_REQUIRE((top_idx == nullptr) == (top_r == nullptr), TMVB_EINVAL, "%s: top_idx and top_r are given together or not at all", fn);
    TMVB_REQUIRE(max_chunk_entries >= 0, TMVB_EINVAL, "%s: max_chunk_entries must be nonnegative", fn);
    TMVB_REQUIRE(docs ? Ms >= 0 && Ms < (int64_t)INT32_MAX : (Ms == M || Ms == 0), TMVB_EINVAL, "%s: Ms = %lld (with docs == NULL: M or 0)", fn, (long long)Ms);
    TMVB_REQUIRE(doc_ptr[0] == 0, TMVB_EINVAL, "%s: doc_ptr must start at 0", fn);
    for (int64_t d = 0; d < M; d++) TMVB_REQUIRE(doc_ptr[d + 1] >= doc_ptr[d], TMVB_EINVAL, "%s: doc_ptr decreases at document %lld", fn, (long long)d);
    TMVB_REQUIRE(doc_ptr[M] < TT_MAX_ENTRIES, TMVB_EINVAL, "%s: %lld entries in one call (limit 2^31 - 2)", fn, (long long)doc_ptr[M]);
    for (int64_t j = 0; j < doc_ptr[M]; j++) {
        TMVB_REQUIRE(terms[j] >= 0 && terms[j] < V, TMVB_EINVAL, "%s: entry %lld holds term %d outside [0, %lld)", fn, (long long)j, terms[j], (long long)V);
        TMVB_REQUIRE(counts[j] >= 1, TMVB_EINVAL, "%s: entry %lld holds a count below 1", fn, (long long)j);
    }
    if (!docs) Ms = M;
    int64_t nsel = 0;
    for (int64_t s = 0; s < Ms; s++) {
        const int64_t d = docs ? docs[s] : s;
        TMVB_REQUIRE(d >= 0 && d < M, TMVB_EINVAL, "%s: docs[%lld] = %lld outside [0, %lld)", fn, (long long)s, (long long)d, (long long)M);
        nsel += doc_ptr[d + 1] - doc_ptr[d];
        int64_t C = 0;
        for (int64_t j = doc_ptr[d]; j < doc_ptr[d + 1]; j++) C += counts[j];
        TMVB_REQUIRE(C < ((int64_t)1 << 31), TMVB_EINVAL, "%s: document %lld has %lld tokens (limit 2^31 - 1)", fn, (long long)d, (long long)C);
        TMVB_REQUIRE(nsel < TT_MAX_ENTRIES, TMVB_EINVAL, "%s: more than 2^31 - 2 selected entries in one call", fn);
        for (int k = 0; k < K; k++) {                  // a value that fp32 cannot hold is refused with the negative and the NaN
            const double x = A[k + (int64_t)K * d];
            TMVB_REQUIRE(x >= 0.0 && x <= 3.4028234663852886e38, TMVB_EINVAL, "%s: A[%d, %lld] is negative, NaN or beyond fp32", fn, k, (long long)d);
        }
    }
    for (int64_t j = 0; j < (int64_t)K * V; j++)
        TMVB_REQUIRE(B[j] >= 0.0 && B[j] <= 3.4028234663852886e38, TMVB_EINVAL, "%s: B[%lld, %lld] is negative, NaN or beyond fp32", fn, (long long)(j % K),
                     (long long)(j / K));
    int rc = tmvb_check_ctx_or_device(fn, ctx);
    if (rc != TMVB_OK) return rc;
    int64_t cap = max_chunk_entries;
    if (cap == 0) cap = phi ? std::max<int64_t>(TT_DENSE_BYTES / ((int64_t)tmvb_kpad(K) * 4), 1) : TT_MAX_ENTRIES;
    return tt_run(ctx, K, V, A, B, doc_ptr, terms, counts, docs, Ms, nsel, (float)eps, t, cap, top_idx, top_r, phi, hard, info);
}

extern "C" int tmvb_digamma_f64(const double* x, double* y, int64_t n)
{
    TMVB_REQUIRE(n >= 0 && (n == 0 || (x && y)), TMVB_EINVAL, "tmvb_digamma_f64: NULL argument or negative n");
    // Near its positive root x0 = 1.46163... psi is small against the terms of the recurrence and tmvb_digamma_host loses relative accuracy
    // (4e-14 at psi = -0.02): within 1/4 of the root the Taylor series about the double nearest to x0 is used, c[n - 1] = psi^(n)(x0) / n!.
    static const double x0 = 1.4616321449683622, psi_x0 = -9.241265521729427e-17;
    static const double c[26] = {0.9676722454476212, -0.4427631689835922, 0.2584997609556511, -0.16394270544240658, 0.10782405069126241, -0.07219956125645474,
                                 0.04880428816414313, -0.033161126474847376, 0.022597648232218118, -0.01542476590494897, 0.010538791616612184,
                                 -0.007204534386356875, 0.004926781395729858, -0.0033698016554393312, 0.00230512632673493, -0.001576936771430199,
                                 0.0010788252019162978, -0.000738070938996006, 0.0005049532658346027, -0.0003454680251063082, 0.00023635601564027086,
                                 -0.00016170622091974827, 0.00011063372768747428, -7.569179582195078e-05, 5.17857579522209e-05, -3.543007094765967e-05};
    for (int64_t i = 0; i < n; i++) {
        const double h = x[i] - x0;
        if (std::fabs(h) <= 0.25) {
            double s = c[25];
            for (int j = 24; j >= 0; j--) s = s * h + c[j];
            y[i] = psi_x0 + s * h;
        } else {
            y[i] = tmvb_digamma_host(x[i]);
        }
    }
    return TMVB_OK;
}
