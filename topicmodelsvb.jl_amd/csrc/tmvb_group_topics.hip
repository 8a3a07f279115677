// tmvb_group_topics.hip -- topics by group and over time: for every group g of documents S_g[k, w] = sum over the entries (w, c) of the documents of
// g of c r_k(d, w), with r the responsibilities of tmvb_token_topics (include/tmvb.h states the definitions and the order of every sum).
//
//   index     host: the selected entries ordered by (group, term, document, position) by two stable counting sorts (term, then group: LSD), each
//             on up to 16 threads over contiguous ranges, the scheme of tmvb_build_inv_index.  A run = the entries of one (group, term).
//   accum     group_topics_kernel, a sibling of token_topics_kernel: the same fp32 staging of B as [V][KP] rows and the same lanes_per_entry rule
//             (tmvb_token_phi.h); A as [Ms][KA] rows of the selected documents, KA = K rounded up to 32 floats, so that a gathered row starts a 128-byte line.  The work item
//             is a segment of a run (<= TMVB_GT_SEG entries), one WAVE per item, GT_WAVES items per workgroup (1: a 64-lane workgroup), no LDS and no barrier.  The term's B
//             chunks are loaded once and stay in registers; every trip gathers the A rows of 64 / L entries with 16-byte loads, calls the shared
//             tt_responsibilities and adds (double)c * (double)r_k into <= 16 fp64 accumulators per lane (32 VGPRs).  At the item's end the
//             64 / L slots meet in an xor butterfly; slot 0 writes: a single-segment run straight into S, a segment of a longer run into its row
//             of the call's partial buffer.
//   combine   one lane per (long run, topic) adds the run's partial rows in segment order and writes S.
//   small     row sums (mass, the pooled row), the normalisation to beta_g with the sort's values, the running pooled sum over ascending g, the
//             selection of the n heads, the Jensen-Shannon rows: plain fixed-order fp64 kernels, one workgroup per row where a row is summed.
// Groups are processed in chunks of chunk_groups whose [K][V] blocks fit the device buffer; no sum crosses a chunk except the pooled row, which one
// kernel continues in ascending g, and drift's previous row, which is kept in a buffer of its own: the bytes do not depend on the chunks.
// fp contraction is OFF in this unit (tmvb_divergence_terms.h).  No atomics; no scratch (tools/kernel_resources.py holds the kernels to that).
#include "tmvb_internal.h"
#include "tmvb_call.h"
#include "tmvb_token_phi.h"
#include "tmvb_divergence_terms.h"

#include <algorithm>
#include <chrono>
#include <cstring>
#include <thread>
#include <vector>

#pragma clang fp contract(off)

#define GT_MAX_K 1024
#ifndef GT_WAVES
#define GT_WAVES 1                  // work items (waves) per workgroup: 1 measured fastest; -DGT_WAVES / -DGT_UNROLL / -DTMVB_GT_SEG: the variants timed there
#endif
#ifdef GT_UNROLL                    // explicit unrolling of the trip loop (the A-row prefetch depth); default: the compiler's choice
#define GT_STR2(x) #x
#define GT_STR(x) GT_STR2(x)
#define GT_TRIP_PRAGMA _Pragma(GT_STR(unroll GT_UNROLL))
#else
#define GT_TRIP_PRAGMA
#endif
#define GT_WG (64 * GT_WAVES)
#define GT_S_BYTES ((int64_t)1 << 28)            // default bound of the [chunk_groups][K][V] fp64 buffer: 256 MiB
#define GT_MAX_ENTRIES ((int64_t)INT32_MAX - 1)
#define GT_THREADS_MIN ((int64_t)1 << 20)        // entries from which the index build uses more than one thread

// a segment of a run
struct gt_item {
    int64_t e0;                     // its first entry in the index order
    int64_t dst;                    // to_part == 0: element (g - g0) K V + w of S, topic stride V; else: first element of its row of part, stride 1
    int32_t n;                      // entries, 1 .. TMVB_GT_SEG
    int32_t term;
    int32_t to_part;
    int32_t pad;
};

// a run of more than one segment
struct gt_multi {
    int64_t dst;                    // element (g - g0) K V + w of S
    int64_t p0;                     // its first row of part
    int32_t nseg;
    int32_t pad;
};

// ------------------------------------------------------------------------------------------------------------------ accumulation
// A: [Ms][KA] (the selected documents), B: [V][KP] (pads 0), rows 16-byte aligned.  ent_doc / ent_cnt: A row and count of every entry in the index order.
static __global__ __launch_bounds__(GT_WG) void group_topics_kernel(int K, int KP, int KA, int logL, float eps, int64_t V, int64_t n_items,
                                                                    const gt_item* __restrict__ items, const float* __restrict__ A, const float* __restrict__ B,
                                                                    const int32_t* __restrict__ ent_doc, const int32_t* __restrict__ ent_cnt,
                                                                    double* __restrict__ S, double* __restrict__ part)
{
    const int lane = threadIdx.x & 63;
    const int64_t item = (int64_t)blockIdx.x * GT_WAVES + (threadIdx.x >> 6);
    if (item >= n_items) return;                       // wave-uniform
    const int L = 1 << logL, r = lane & (L - 1), g = lane >> logL, E = 64 >> logL;
    const gt_item it = items[item];
    const int nch = (K + 3) >> 2;                      // chunks that hold topics
    const unsigned vmask = tt_value_mask(K, r, L);
    const float4 zero4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float4* brow = reinterpret_cast<const float4*>(B + (int64_t)it.term * KP);
    float4 bv[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int c = r + q * L;
        bv[q] = c < nch ? brow[c] : zero4;
    }
    double acc[16];
#pragma unroll
    for (int j = 0; j < 16; j++) acc[j] = 0.0;
    GT_TRIP_PRAGMA
    for (int i0 = 0; i0 < it.n; i0 += E) {             // uniform trip count: every lane takes part in the butterfly of the sum
        const int i = i0 + g;
        const bool live = i < it.n;
        float4 av[4];
#pragma unroll
        for (int q = 0; q < 4; q++) av[q] = zero4;
        int c_n = 0;
        if (live) {
            c_n = ent_cnt[it.e0 + i];
            const float4* arow = reinterpret_cast<const float4*>(A + (int64_t)ent_doc[it.e0 + i] * KA);
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int c = r + q * L;
                if (c < nch) av[q] = arow[c];
            }
        }
        float y[16];
        tt_responsibilities(y, av, bv, vmask, eps, L, live);           // tmvb_token_phi.h: the bits of tmvb_token_topics
        const double cd = (double)c_n;                 // 0 in a slot without an entry: adds +0
#pragma unroll
        for (int j = 0; j < 16; j++) acc[j] += cd * (double)y[j];
    }
    for (int o = L; o < 64; o <<= 1) {                 // the E slots: xor butterfly over the slot number, every lane ends with the same bits
#pragma unroll
        for (int j = 0; j < 16; j++) acc[j] += __shfl_xor(acc[j], o);
    }
    if (g != 0) return;
    double* out = (it.to_part ? part : S) + it.dst;
    const int64_t stride = it.to_part ? 1 : V;
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int k = 4 * (r + q * L) + j;
            if (k < K) out[(int64_t)k * stride] = acc[4 * q + j];
        }
}

// one lane per (long run, topic): the partial rows in segment order
static __global__ __launch_bounds__(256) void gt_combine_kernel(int K, int64_t V, int64_t n_multi, const gt_multi* __restrict__ multi, const double* __restrict__ part,
                                                                double* __restrict__ S)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_multi * K) return;
    const int64_t m = q / K;
    const int k = (int)(q - m * K);
    const gt_multi mu = multi[m];
#ifdef TMVB_MUTANT_GT_SEG_CUT
    const int nseg = mu.nseg - 1;                      // MUTANT: the last segment of a run is left out
#else
    const int nseg = mu.nseg;
#endif
    double s = part[mu.p0 * K + k];
    for (int j = 1; j < nseg; j++) s += part[(mu.p0 + j) * K + k];
    S[mu.dst + (int64_t)k * V] = s;
}

// ------------------------------------------------------------------------------------------------------------------ small fixed-order kernels
// the 256 lane sums of a row meet in a halving tree; every lane returns the total
__device__ __forceinline__ double gt_block_sum(double a, double* s)
{
    const int tid = threadIdx.x;
    s[tid] = a;
    __syncthreads();
    for (int o = 128; o; o >>= 1) {
        if (tid < o) s[tid] += s[tid + o];
        __syncthreads();
    }
    return s[0];
}

// out[row] = sum_w X[row][w]: lane t adds w = t, t + 256, ... ascending from 0
static __global__ __launch_bounds__(256) void gt_rowsum_kernel(int64_t V, const double* __restrict__ X, double* __restrict__ out)
{
    __shared__ double s[256];
    const double* x = X + (int64_t)blockIdx.x * V;
    double a = 0.0;
    for (int64_t w = threadIdx.x; w < V; w += 256) a += x[w];
    const double t = gt_block_sum(a, s);
    if (threadIdx.x == 0) out[blockIdx.x] = t;
}

// P[row][w] = X[row][w] / sum[row] (0 where the sum is 0); vals[row][w] = w where given.  P may be X (the pooled row): no __restrict__ on the two
static __global__ __launch_bounds__(256) void gt_norm_kernel(int64_t rows, int64_t V, const double* X, const double* __restrict__ sum, double* P,
                                                             int32_t* __restrict__ vals)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= rows * V) return;
    const int64_t row = q / V;
    const double m = sum[row];
    P[q] = m > 0.0 ? X[q] / m : 0.0;
    if (vals) vals[q] = (int32_t)(q - row * V);
}

// pool[k][w] += S[0][k][w], then S[1][k][w], ...: the pooled sum continues in ascending g over the chunks
static __global__ __launch_bounds__(256) void gt_pool_kernel(int64_t KV, int ng, const double* __restrict__ S, double* __restrict__ pool)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= KV) return;
    double s = pool[q];
    for (int g = 0; g < ng; g++) s += S[(int64_t)g * KV + q];
    pool[q] = s;
}

static __global__ __launch_bounds__(256) void gt_select_kernel(int64_t rows, int64_t V, int n, const double* __restrict__ mass, const double* __restrict__ skeys,
                                                               const int32_t* __restrict__ svals, int32_t* __restrict__ idx, double* __restrict__ p)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= rows * n) return;
    const int64_t row = q / n, s = q - row * n;
    const bool any = mass[row] > 0.0;
    idx[q] = any ? svals[row * V + s] : -1;
    p[q] = any ? skeys[row * V + s] : 0.0;
}

// One workgroup per row (g, k) of P[ng][K][V].  qsel[g] = -2: out = 0; -1: the other row is ext[k][.]; >= 0: row k of that group of P.
static __global__ __launch_bounds__(256) void gt_js_kernel(int K, int64_t V, const double* __restrict__ P, const double* __restrict__ ext, const int32_t* __restrict__ qsel,
                                                           double* __restrict__ out)
{
    __shared__ double s[256];
    const int64_t row = blockIdx.x;
    const int g = (int)(row / K), k = (int)(row - (int64_t)g * K);
    const int sel = qsel[g];
    if (sel == -2) {                                   // workgroup-uniform
        if (threadIdx.x == 0) out[row] = 0.0;
        return;
    }
    const double* p = P + row * V;
    const double* q = sel < 0 ? ext + (int64_t)k * V : P + ((int64_t)sel * K + k) * V;
    double a = 0.0;
    for (int64_t w = threadIdx.x; w < V; w += 256) a += td_term<TMVB_TD_JS>(p[w], q[w]);
    const double t = gt_block_sum(a, s);
    if (threadIdx.x == 0) out[row] = td_finish<TMVB_TD_JS>(t);
}

// ------------------------------------------------------------------------------------------------------------------ host: the index
namespace {
struct gt_index {
    std::vector<int32_t> pos, doc;                     // per selected entry in the index order: position in the CSR, document
    std::vector<int64_t> run_ptr;
    std::vector<int32_t> run_group, run_term;
};

// One stable counting sort over T contiguous ranges: per-range histograms, one prefix over (key, range), then every range scatters its own elements
// from its own cursors -- the positions the one-thread loop assigns.  each(t, f) calls f(key, pos, doc) for the elements of range t in order.
template <class Each>
void gt_counting_pass(int T, int64_t n_keys, Each each, int32_t* out_pos, int32_t* out_doc)
{
    std::vector<std::vector<int64_t>> cur((size_t)T);
    auto run_ranges = [&](auto&& fn) {
        std::vector<std::thread> workers;
        for (int t = 1; t < T; ++t) workers.emplace_back(fn, t);
        fn(0);
        for (std::thread& w : workers) w.join();
    };
    run_ranges([&](int t) {
        std::vector<int64_t>& H = cur[(size_t)t];
        H.assign((size_t)n_keys, 0);
        each(t, [&](int64_t key, int32_t, int32_t) { H[(size_t)key]++; });
    });
    int64_t w = 0;
    for (int64_t j = 0; j < n_keys; ++j)
        for (int t = 0; t < T; ++t) {
            const int64_t c = cur[(size_t)t][(size_t)j];
            cur[(size_t)t][(size_t)j] = w;
            w += c;
        }
    run_ranges([&](int t) {
        std::vector<int64_t>& C = cur[(size_t)t];
        each(t, [&](int64_t key, int32_t pos, int32_t doc) {
            const int64_t at = C[(size_t)key]++;
            out_pos[at] = pos; out_doc[at] = doc;
        });
    });
}

// the arguments are checked by the caller
void gt_build_index(int64_t M, int64_t V, const int64_t* doc_ptr, const int32_t* terms, const int32_t* group, int32_t G, gt_index* ix)
{
    int64_t nsel = 0;
    for (int64_t d = 0; d < M; d++)
        if (group[d] >= 0) nsel += doc_ptr[d + 1] - doc_ptr[d];
    int T = 1;
    if (nsel >= GT_THREADS_MIN) {
        const unsigned hw = std::thread::hardware_concurrency();
        T = (int)std::max(1u, std::min(hw ? hw : 1u, 16u));
    }
    // pass 1, by term: the documents in T contiguous ranges of about equal entries
    std::vector<int64_t> dcut((size_t)T + 1, M);
    dcut[0] = 0;
    for (int t = 1; t < T; ++t) {
        const int64_t target = doc_ptr[M] / T * t;
        const int64_t d = std::lower_bound(doc_ptr, doc_ptr + M + 1, target) - doc_ptr;
        dcut[(size_t)t] = std::min<int64_t>(std::max(d, dcut[(size_t)t - 1]), M);
    }
    std::vector<int32_t> pos1((size_t)nsel), doc1((size_t)nsel);
    gt_counting_pass(T, V, [&](int t, auto&& f) {
        for (int64_t d = dcut[(size_t)t]; d < dcut[(size_t)t + 1]; ++d)
            if (group[d] >= 0)
                for (int64_t q = doc_ptr[d]; q < doc_ptr[d + 1]; ++q) f((int64_t)terms[q], (int32_t)q, (int32_t)d);
    }, pos1.data(), doc1.data());
    // pass 2, by group: the output of pass 1 in T contiguous ranges
    ix->pos.resize((size_t)nsel); ix->doc.resize((size_t)nsel);
    gt_counting_pass(T, (int64_t)G, [&](int t, auto&& f) {
        const int64_t a = nsel / T * t, b = t + 1 == T ? nsel : nsel / T * (t + 1);
        for (int64_t i = a; i < b; ++i) f((int64_t)group[doc1[(size_t)i]], pos1[(size_t)i], doc1[(size_t)i]);
    }, ix->pos.data(), ix->doc.data());
    ix->run_ptr.clear(); ix->run_group.clear(); ix->run_term.clear();
    for (int64_t i = 0; i < nsel; ++i) {
        const int32_t g = group[ix->doc[(size_t)i]], w = terms[ix->pos[(size_t)i]];
        if (i == 0 || g != ix->run_group.back() || w != ix->run_term.back()) {
            ix->run_ptr.push_back(i); ix->run_group.push_back(g); ix->run_term.push_back(w);
        }
    }
    ix->run_ptr.push_back(nsel);
}

// what both entry points ask of the CSR and the labels
int gt_check_corpus(const char* fn, int64_t M, int64_t V, const int64_t* doc_ptr, const int32_t* terms, const int32_t* counts, const int32_t* group, int32_t G)
{
    TMVB_REQUIRE(doc_ptr[0] == 0, TMVB_EINVAL, "%s: doc_ptr must start at 0", fn);
    for (int64_t d = 0; d < M; d++) TMVB_REQUIRE(doc_ptr[d + 1] >= doc_ptr[d], TMVB_EINVAL, "%s: doc_ptr decreases at document %lld", fn, (long long)d);
    TMVB_REQUIRE(doc_ptr[M] < GT_MAX_ENTRIES, TMVB_EINVAL, "%s: %lld entries in one call (limit 2^31 - 2)", fn, (long long)doc_ptr[M]);
    for (int64_t j = 0; j < doc_ptr[M]; j++) {
        TMVB_REQUIRE(terms[j] >= 0 && terms[j] < V, TMVB_EINVAL, "%s: entry %lld holds term %d outside [0, %lld)", fn, (long long)j, terms[j], (long long)V);
        if (counts) {
            TMVB_REQUIRE(counts[j] >= 1, TMVB_EINVAL, "%s: entry %lld holds a count below 1", fn, (long long)j);
            TMVB_REQUIRE(counts[j] < (1 << 29), TMVB_EINVAL, "%s: entry %lld holds a count of 2^29 or more", fn, (long long)j);
        }
    }
    for (int64_t d = 0; d < M; d++)
        TMVB_REQUIRE(group[d] >= -1 && group[d] < G, TMVB_EINVAL, "%s: group[%lld] = %d outside [-1, %d)", fn, (long long)d, group[d], G);
    return TMVB_OK;
}

// ------------------------------------------------------------------------------------------------------------------ host: the call
struct gt_chunk { int32_t g0, g1; int64_t item0, items, multi0, multis; };

int gt_run(tmvb_ctx* ctx, int32_t K, int64_t V, int64_t M, const double* A, const double* B, const int32_t* counts, const int32_t* group, int32_t G, float eps,
           int32_t n, int32_t cg, const gt_index& ix, float ms_index, double* mass, int32_t* top_idx, double* top_p, double* shift, double* drift, double* dense,
           tmvb_group_topics_info_t* info)
{
    const int KP = tmvb_kpad(K), KA = (K + 31) & ~31, logL = tt_log_lanes(K);
    const int64_t KV = (int64_t)K * V, nsel = (int64_t)ix.pos.size(), runs = (int64_t)ix.run_group.size();
    // host staging, declared in front of the call's scope
    // A: only the columns of the selected documents, in document order; slot[d] = the row of document d
    std::vector<int32_t> slot((size_t)M, -1);
    int64_t Ms = 0;
    for (int64_t d = 0; d < M; d++)
        if (group[d] >= 0) slot[(size_t)d] = (int32_t)Ms++;
    std::vector<float> h_a((size_t)Ms * KA, 0.0f), h_b((size_t)V * KP, 0.0f);
    for (int64_t d = 0; d < M; d++)
        if (group[d] >= 0)
            for (int k = 0; k < K; k++) h_a[(size_t)slot[(size_t)d] * KA + k] = (float)A[k + (int64_t)K * d];
    for (int64_t v = 0; v < V; v++)
        for (int k = 0; k < K; k++) h_b[(size_t)v * KP + k] = (float)B[k + (int64_t)K * v];
    std::vector<int32_t> h_cnt((size_t)nsel), h_row((size_t)nsel);
    for (int64_t i = 0; i < nsel; i++) {
        h_cnt[(size_t)i] = counts[ix.pos[(size_t)i]];
        h_row[(size_t)i] = slot[(size_t)ix.doc[(size_t)i]];
    }
    std::vector<char> has((size_t)G, 0);               // groups with entries
    for (int64_t u = 0; u < runs; u++) has[(size_t)ix.run_group[(size_t)u]] = 1;
    // work items and long runs, chunk by chunk (runs ascend in g)
    std::vector<gt_chunk> chunks;
    std::vector<gt_item> h_items;
    std::vector<gt_multi> h_multi;
    int64_t n_part = 0;
    {
        int64_t u = 0;
        for (int32_t g0 = 0; g0 < G; g0 += cg) {
            gt_chunk ch{g0, std::min<int32_t>(g0 + cg, G), (int64_t)h_items.size(), 0, (int64_t)h_multi.size(), 0};
            for (; u < runs && ix.run_group[(size_t)u] < ch.g1; u++) {
                const int64_t e0 = ix.run_ptr[(size_t)u], len = ix.run_ptr[(size_t)u + 1] - e0;
                const int64_t dst = (int64_t)(ix.run_group[(size_t)u] - g0) * KV + ix.run_term[(size_t)u];
                const int64_t nseg = (len + TMVB_GT_SEG - 1) / TMVB_GT_SEG;
                if (nseg == 1) { h_items.push_back(gt_item{e0, dst, (int32_t)len, ix.run_term[(size_t)u], 0, 0}); continue; }
                h_multi.push_back(gt_multi{dst, n_part, (int32_t)nseg, 0});
                for (int64_t s = 0; s < nseg; s++)
                    h_items.push_back(gt_item{e0 + s * TMVB_GT_SEG, (n_part + s) * K, (int32_t)std::min<int64_t>(TMVB_GT_SEG, len - s * TMVB_GT_SEG), ix.run_term[(size_t)u], 1, 0});
                n_part += nseg;
            }
            ch.items = (int64_t)h_items.size() - ch.item0; ch.multis = (int64_t)h_multi.size() - ch.multi0;
            chunks.push_back(ch);
        }
    }
    const bool two_pass = shift && chunks.size() > 1;  // the pooled row needs every group: the statistics are accumulated again for shift
    std::vector<int32_t> h_qsel((size_t)cg);

    hipStream_t st = ctx->stream;
    tmvb_call c("group_topics", ctx->device, st);
    TMVB_CALL_TRY(c, c.begin());
    TMVB_CALL_TRY(c, c.events(6));
    float *d_a, *d_b;
    int32_t *d_doc, *d_cnt, *d_vals, *d_idx, *d_qsel;
    gt_item* d_items;
    gt_multi* d_multi;
    double *d_S, *d_P, *d_part, *d_mass, *d_p, *d_pool = nullptr, *d_poolsum = nullptr, *d_prev = nullptr, *d_shift = nullptr, *d_drift = nullptr;
    const size_t block = (size_t)cg * KV, GK = (size_t)G * K;
    TMVB_CALL_TRY(c, c.upload(&d_a, (const float*)h_a.data(), h_a.size()));
    TMVB_CALL_TRY(c, c.upload(&d_b, (const float*)h_b.data(), h_b.size()));
    TMVB_CALL_TRY(c, c.upload(&d_doc, (const int32_t*)h_row.data(), (size_t)nsel));
    TMVB_CALL_TRY(c, c.upload(&d_cnt, (const int32_t*)h_cnt.data(), (size_t)nsel));
    TMVB_CALL_TRY(c, c.upload(&d_items, (const gt_item*)h_items.data(), h_items.size()));
    TMVB_CALL_TRY(c, c.upload(&d_multi, (const gt_multi*)h_multi.data(), h_multi.size()));
    TMVB_CALL_TRY(c, c.alloc(&d_S, block)); TMVB_CALL_TRY(c, c.alloc(&d_P, block)); TMVB_CALL_TRY(c, c.alloc(&d_vals, block));
    TMVB_CALL_TRY(c, c.alloc(&d_part, (size_t)n_part * K));
    TMVB_CALL_TRY(c, c.alloc(&d_mass, GK)); TMVB_CALL_TRY(c, c.alloc(&d_idx, GK * n)); TMVB_CALL_TRY(c, c.alloc(&d_p, GK * n));
    TMVB_CALL_TRY(c, c.alloc(&d_qsel, (size_t)cg));
    if (shift) {
        TMVB_CALL_TRY(c, c.alloc(&d_pool, (size_t)KV)); TMVB_CALL_TRY(c, c.alloc(&d_poolsum, (size_t)K)); TMVB_CALL_TRY(c, c.alloc(&d_shift, GK));
        TMVB_CALL_HIP(c, hipMemsetAsync(d_pool, 0, (size_t)KV * sizeof(double), st));
    }
    if (drift) { TMVB_CALL_TRY(c, c.alloc(&d_prev, (size_t)KV)); TMVB_CALL_TRY(c, c.alloc(&d_drift, GK)); }

    auto grid = [](int64_t n_el) { return dim3((unsigned)((n_el + 255) / 256)); };
    // S of the chunk's groups: cleared, the segments, the long runs
    auto accumulate = [&](const gt_chunk& ch) -> hipError_t {
        const int ng = ch.g1 - ch.g0;
        hipError_t e = hipMemsetAsync(d_S, 0, (size_t)ng * KV * sizeof(double), st);
        if (e != hipSuccess) return e;
        if (ch.items > 0)
            hipLaunchKernelGGL(group_topics_kernel, dim3((unsigned)((ch.items + GT_WAVES - 1) / GT_WAVES)), dim3(GT_WG), 0, st, (int)K, KP, KA, logL, eps, V, ch.items,
                               (const gt_item*)d_items + ch.item0, (const float*)d_a, (const float*)d_b, (const int32_t*)d_doc, (const int32_t*)d_cnt, d_S, d_part);
        if (ch.multis > 0)
            hipLaunchKernelGGL(gt_combine_kernel, grid(ch.multis * K), dim3(256), 0, st, (int)K, V, ch.multis, (const gt_multi*)d_multi + ch.multi0, (const double*)d_part, d_S);
        return hipGetLastError();
    };
    // shift of the chunk's groups from the pooled row (d_pool holds it normalised); d_P holds the chunk's beta_g
    auto shift_rows = [&](const gt_chunk& ch) -> hipError_t {
        const int ng = ch.g1 - ch.g0;
        for (int g = 0; g < ng; g++) h_qsel[(size_t)g] = has[(size_t)(ch.g0 + g)] ? -1 : -2;
        hipError_t e = hipMemcpyAsync(d_qsel, h_qsel.data(), (size_t)ng * sizeof(int32_t), hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(gt_js_kernel, dim3((unsigned)(ng * K)), dim3(256), 0, st, (int)K, V, (const double*)d_P, (const double*)d_pool, (const int32_t*)d_qsel,
                           d_shift + (size_t)ch.g0 * K);
        e = hipGetLastError();
        return e != hipSuccess ? e : hipStreamSynchronize(st);         // h_qsel is written again
    };
    auto pool_rows = [&]() -> hipError_t {             // the pooled sum -> the pooled row, in place
        hipLaunchKernelGGL(gt_rowsum_kernel, dim3((unsigned)K), dim3(256), 0, st, V, (const double*)d_pool, d_poolsum);
        hipLaunchKernelGGL(gt_norm_kernel, grid(KV), dim3(256), 0, st, (int64_t)K, V, (const double*)d_pool, (const double*)d_poolsum, d_pool, (int32_t*)nullptr);
        return hipGetLastError();
    };

    float ms_accum = 0.0f, ms_select = 0.0f, ms_shift = 0.0f;
    int32_t prev_g = -1;                               // the last group with entries so far; its beta is in d_prev once its chunk is done
    for (const gt_chunk& ch : chunks) {
        const int ng = ch.g1 - ch.g0;
        const int64_t rows = (int64_t)ng * K;
        tmvb_call cs("group_topics", ctx->device, st); // the sort's buffers live for one chunk
        TMVB_CALL_HIP(c, hipEventRecord(c.ev(0), st));
        TMVB_CALL_HIP(c, accumulate(ch));
        hipLaunchKernelGGL(gt_rowsum_kernel, dim3((unsigned)rows), dim3(256), 0, st, V, (const double*)d_S, d_mass + (size_t)ch.g0 * K);
        TMVB_CALL_HIP(c, hipGetLastError());
        TMVB_CALL_HIP(c, hipEventRecord(c.ev(1), st));
        if (dense) TMVB_CALL_HIP(c, hipMemcpyAsync(dense + (size_t)ch.g0 * KV, d_S, (size_t)rows * V * sizeof(double), hipMemcpyDeviceToHost, st));
        TMVB_CALL_HIP(c, hipEventRecord(c.ev(2), st));
        hipLaunchKernelGGL(gt_norm_kernel, grid(rows * V), dim3(256), 0, st, rows, V, (const double*)d_S, (const double*)d_mass + (size_t)ch.g0 * K, d_P, d_vals);
        TMVB_CALL_HIP(c, hipGetLastError());
        double* d_skeys;
        int32_t* d_svals;
        const int rc = tmvb_segmented_sort_pairs(cs, (int)rows, V, d_P, d_vals, true, &d_skeys, &d_svals);
        if (rc != TMVB_OK) return c.fail(rc);
        hipLaunchKernelGGL(gt_select_kernel, grid(rows * n), dim3(256), 0, st, rows, V, (int)n, (const double*)d_mass + (size_t)ch.g0 * K, (const double*)d_skeys,
                           (const int32_t*)d_svals, d_idx + (size_t)ch.g0 * K * n, d_p + (size_t)ch.g0 * K * n);
        TMVB_CALL_HIP(c, hipGetLastError());
        TMVB_CALL_HIP(c, hipEventRecord(c.ev(3), st));
        TMVB_CALL_HIP(c, hipEventRecord(c.ev(4), st));
        if (shift) {
            hipLaunchKernelGGL(gt_pool_kernel, grid(KV), dim3(256), 0, st, KV, ng, (const double*)d_S, d_pool);
            TMVB_CALL_HIP(c, hipGetLastError());
        }
        if (drift) {
            int32_t last = prev_g;
            for (int g = 0; g < ng; g++) {
                const int32_t gg = ch.g0 + g;
                if (!has[(size_t)gg]) { h_qsel[(size_t)g] = -2; continue; }
                h_qsel[(size_t)g] = last < 0 ? -2 : (last < ch.g0 ? -1 : last - ch.g0);
                last = gg;
            }
            TMVB_CALL_HIP(c, hipMemcpyAsync(d_qsel, h_qsel.data(), (size_t)ng * sizeof(int32_t), hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(gt_js_kernel, dim3((unsigned)rows), dim3(256), 0, st, (int)K, V, (const double*)d_P, (const double*)d_prev, (const int32_t*)d_qsel,
                               d_drift + (size_t)ch.g0 * K);
            TMVB_CALL_HIP(c, hipGetLastError());
            if (last >= ch.g0)
                TMVB_CALL_HIP(c, hipMemcpyAsync(d_prev, d_P + (size_t)(last - ch.g0) * KV, (size_t)KV * sizeof(double), hipMemcpyDeviceToDevice, st));
            prev_g = last;
            TMVB_CALL_HIP(c, hipStreamSynchronize(st));                // h_qsel is written again
        }
        if (shift && !two_pass) {
            TMVB_CALL_HIP(c, pool_rows());
            TMVB_CALL_HIP(c, shift_rows(ch));
        }
        TMVB_CALL_HIP(c, hipEventRecord(c.ev(5), st));
        TMVB_CALL_HIP(c, hipStreamSynchronize(st));                    // the chunk's buffers and the events are used again
        float ms = 0.0f;
        TMVB_CALL_TRY(c, c.elapsed(&ms, 0, 1)); ms_accum += ms;
        TMVB_CALL_TRY(c, c.elapsed(&ms, 2, 3)); ms_select += ms;
        TMVB_CALL_TRY(c, c.elapsed(&ms, 4, 5)); ms_shift += ms;
    }
    if (two_pass) {
        TMVB_CALL_HIP(c, hipEventRecord(c.ev(4), st));
        TMVB_CALL_HIP(c, pool_rows());
        for (const gt_chunk& ch : chunks) {
            const int64_t rows = (int64_t)(ch.g1 - ch.g0) * K;
            TMVB_CALL_HIP(c, accumulate(ch));
            hipLaunchKernelGGL(gt_norm_kernel, grid(rows * V), dim3(256), 0, st, rows, V, (const double*)d_S, (const double*)d_mass + (size_t)ch.g0 * K, d_P, (int32_t*)nullptr);
            TMVB_CALL_HIP(c, hipGetLastError());
            TMVB_CALL_HIP(c, shift_rows(ch));
        }
        TMVB_CALL_HIP(c, hipEventRecord(c.ev(5), st));
        TMVB_CALL_HIP(c, hipStreamSynchronize(st));
        float ms = 0.0f;
        TMVB_CALL_TRY(c, c.elapsed(&ms, 4, 5)); ms_shift += ms;
    }
    TMVB_CALL_HIP(c, hipMemcpyAsync(mass, d_mass, GK * sizeof(double), hipMemcpyDeviceToHost, st));
    TMVB_CALL_HIP(c, hipMemcpyAsync(top_idx, d_idx, GK * n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    TMVB_CALL_HIP(c, hipMemcpyAsync(top_p, d_p, GK * n * sizeof(double), hipMemcpyDeviceToHost, st));
    if (shift) TMVB_CALL_HIP(c, hipMemcpyAsync(shift, d_shift, GK * sizeof(double), hipMemcpyDeviceToHost, st));
    if (drift) TMVB_CALL_HIP(c, hipMemcpyAsync(drift, d_drift, GK * sizeof(double), hipMemcpyDeviceToHost, st));
    TMVB_CALL_HIP(c, hipStreamSynchronize(st));
    if (info) {
        info->nsel = nsel; info->runs = runs; info->segments = (int64_t)h_items.size(); info->group_chunks = (int32_t)chunks.size();
        info->lanes_per_entry = 1 << logL; info->ms_index = ms_index; info->ms_accum = ms_accum; info->ms_select = ms_select; info->ms_shift = ms_shift;
    }
    return TMVB_OK;
}
}  // namespace

extern "C" int tmvb_group_topics(tmvb_ctx* ctx, int32_t K, int64_t V, int64_t M, const double* A, const double* B, const int64_t* doc_ptr, const int32_t* terms,
                                 const int32_t* counts, const int32_t* group, int32_t G, double eps, int32_t n, int32_t max_chunk_groups, int64_t* docs,
                                 int64_t* tokens, double* mass, int32_t* top_idx, double* top_p, double* shift, double* drift, double* dense,
                                 tmvb_group_topics_info_t* info)
{
    const char* fn = "tmvb_group_topics";
    if (info) memset(info, 0, sizeof(*info));
    TMVB_REQUIRE(K >= 1 && K <= GT_MAX_K, TMVB_EINVAL, "%s: K = %d outside [1, %d]", fn, K, GT_MAX_K);
    TMVB_REQUIRE(G >= 1 && G <= TMVB_GT_GMAX, TMVB_EINVAL, "%s: G = %d outside [1, %d]", fn, G, TMVB_GT_GMAX);
    TMVB_REQUIRE(eps >= 0x1p-100 && eps <= 1.0, TMVB_EINVAL, "%s: eps must lie in [2^-100, 1]", fn);      // NaN fails both
    TMVB_REQUIRE(M > 0 && V > 0 && M < (int64_t)INT32_MAX && V < (int64_t)INT32_MAX, TMVB_EINVAL, "%s: M and V must be positive integers below 2^31 - 1", fn);
    TMVB_REQUIRE(n >= 1 && (int64_t)n <= std::min<int64_t>(V, TMVB_GT_TOP_MAX), TMVB_EINVAL, "%s: n = %d outside [1, min(V, %d)]", fn, n, TMVB_GT_TOP_MAX);
    TMVB_REQUIRE((int64_t)K * V < ((int64_t)1 << 31), TMVB_EINVAL, "%s: K V is 2^31 or more", fn);
    TMVB_REQUIRE(A && B && doc_ptr && terms && counts && group && docs && tokens && mass && top_idx && top_p, TMVB_EINVAL, "%s: NULL argument", fn);
    TMVB_REQUIRE(max_chunk_groups >= 0, TMVB_EINVAL, "%s: max_chunk_groups must be nonnegative", fn);
    int rc = gt_check_corpus(fn, M, V, doc_ptr, terms, counts, group, G);
    if (rc != TMVB_OK) return rc;
    for (int64_t j = 0; j < (int64_t)K * V; j++)
        TMVB_REQUIRE(B[j] >= 0.0 && B[j] <= 3.4028234663852886e38, TMVB_EINVAL, "%s: B[%lld, %lld] is negative, NaN or beyond fp32", fn, (long long)(j % K),
                     (long long)(j / K));
    for (int32_t g = 0; g < G; g++) docs[g] = tokens[g] = 0;
    for (int64_t d = 0; d < M; d++) {
        if (group[d] < 0) continue;
        for (int k = 0; k < K; k++) {                  // a value that fp32 cannot hold is refused with the negative and the NaN
            const double x = A[k + (int64_t)K * d];
            TMVB_REQUIRE(x >= 0.0 && x <= 3.4028234663852886e38, TMVB_EINVAL, "%s: A[%d, %lld] is negative, NaN or beyond fp32", fn, k, (long long)d);
        }
        docs[group[d]]++;
        for (int64_t j = doc_ptr[d]; j < doc_ptr[d + 1]; j++) tokens[group[d]] += counts[j];
    }
    if ((rc = tmvb_check_ctx_or_device(fn, ctx)) != TMVB_OK) return rc;
    const int64_t KV = (int64_t)K * V;
    int64_t cg = std::min<int64_t>(std::max<int64_t>(GT_S_BYTES / (KV * 8), 1), (((int64_t)1 << 31) - 1) / KV);      // cg K V < 2^31: the sort's int offsets
    if (max_chunk_groups > 0) cg = std::min<int64_t>(cg, max_chunk_groups);
    cg = std::min<int64_t>(cg, G);
    const auto t0 = std::chrono::steady_clock::now();
    gt_index ix;
    gt_build_index(M, V, doc_ptr, terms, group, G, &ix);
    const float ms_index = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return gt_run(ctx, K, V, M, A, B, counts, group, G, (float)eps, n, (int32_t)cg, ix, ms_index, mass, top_idx, top_p, shift, drift, dense, info);
}

extern "C" int tmvb_group_index(int64_t M, int64_t V, const int64_t* doc_ptr, const int32_t* terms, const int32_t* group, int32_t G, int64_t* n_runs,
                                int64_t* run_ptr, int32_t* run_group, int32_t* run_term, int64_t* entry)
{
    const char* fn = "tmvb_group_index";
    TMVB_REQUIRE(M > 0 && V > 0 && M < (int64_t)INT32_MAX && V < (int64_t)INT32_MAX, TMVB_EINVAL, "%s: M and V must be positive integers below 2^31 - 1", fn);
    TMVB_REQUIRE(G >= 1 && G <= TMVB_GT_GMAX, TMVB_EINVAL, "%s: G = %d outside [1, %d]", fn, G, TMVB_GT_GMAX);
    TMVB_REQUIRE(doc_ptr && terms && group && n_runs && run_ptr && run_group && run_term && entry, TMVB_EINVAL, "%s: NULL argument", fn);
    const int rc = gt_check_corpus(fn, M, V, doc_ptr, terms, nullptr, group, G);
    if (rc != TMVB_OK) return rc;
    gt_index ix;
    gt_build_index(M, V, doc_ptr, terms, group, G, &ix);
    *n_runs = (int64_t)ix.run_group.size();
    std::copy(ix.run_ptr.begin(), ix.run_ptr.end(), run_ptr);
    std::copy(ix.run_group.begin(), ix.run_group.end(), run_group);
    std::copy(ix.run_term.begin(), ix.run_term.end(), run_term);
    for (size_t i = 0; i < ix.pos.size(); i++) entry[i] = ix.pos[i];
    return TMVB_OK;
}
