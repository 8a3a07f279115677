// tmvb_coherence.hip -- topic coherence on the device: co-document counts of the top words of every topic, and UMass / NPMI from them on the
// host (include/tmvb.h states the definition; the reference has no such function).
//
// tmvb_corpus_codocfreq.  codf[k][i][j] = number of documents that contain both top[k][i] and top[k][j].  Exact integers, the same bits on
// every call, additive over document shards.
//   slots     (host) the distinct ids of the batch's rows of top get slots 0 .. T - 1; a V-sized map term -> slot (-1: not selected) and a
//             [K][N] slot table are uploaded.  A term shared by several topics has one slot.
//   bitset    bits[T][Ws] 64-bit words, Ws = W = ceil(M / 64) rounded up to even (rows 16-byte aligned); bit d of row s is set iff document d
//             contains the term of slot s.  One thread per CSR entry (grid-stride): gather the map first -- most entries are not selected
//             and end there --, then find the entry's document by a binary search in doc_ptr (the library has no CSR-order entry -> document
//             array: the inverted index is id-major), then one 64-bit atomic OR.  OR is idempotent and commutative: the result does not
//             depend on the order or on repeated ids.  The pad bits of the last word and the pad word stay zero (memset).
//   pairs     grid (document chunk c, topic k), 256 lanes.  A chunk is TMVB_CODF_CHUNK_DOCS = 4096 documents = 64 words of a row: N = 64 rows
//             are 32 KB of LDS, five workgroups per CU by LDS, and a wave covers a row of the chunk with one 8-byte read per lane
//             (ds_read_b64: 256 B / clk, lanes on consecutive banks).  The workgroup stages its N rows with 16-byte loads; the N (N + 1) / 2
//             pairs i >= j are dealt to the four waves; lane l takes popcount(row_i[l] & row_j[l]); a xor butterfly sums the wave, and
//             lane 0 adds the sum to codf[k][i][j] with one 64-bit integer atomic per pair and chunk (order-independent).  The host mirrors
//             the lower triangle.
//   batches   if T W 8 bytes exceed the budget, consecutive topics whose distinct ids fit form a batch with its own build pass.
//
// tmvb_coherence_from_counts.  fp64 on the host, compensated sums; touches no device.
#include "tmvb_internal.h"
#include "tmvb_call.h"

#include <algorithm>
#include <cstring>
#include <limits>

#define CODF_MAX_K 1024
#define CODF_MIN_N 2
#define CODF_MAX_N 64
#define CODF_CHUNK_WORDS (TMVB_CODF_CHUNK_DOCS / 64)
#define CODF_WG 256
static_assert(CODF_CHUNK_WORDS == 64, "the pair kernel gives every lane of a wave one word of a chunk's row");

// ------------------------------------------------------------------------------------------------------------------ bitset
// bits: [T][Ws], zeroed.  slot_of: [V].  One thread per CSR entry, grid-stride.
static __global__ __launch_bounds__(CODF_WG) void codf_bitset_kernel(int64_t M, int64_t nnz, int64_t Ws, const int64_t* __restrict__ doc_ptr,
                                                                     const int32_t* __restrict__ terms, const int32_t* __restrict__ slot_of,
                                                                     unsigned long long* __restrict__ bits)
{
    const int64_t stride = (int64_t)gridDim.x * CODF_WG;
    for (int64_t e = (int64_t)blockIdx.x * CODF_WG + threadIdx.x; e < nnz; e += stride) {
        const int32_t s = slot_of[terms[e]];
        if (s < 0) continue;
        int64_t lo = 0, hi = M;                         // the last d with doc_ptr[d] <= e: doc_ptr[0] = 0 <= e < nnz = doc_ptr[M]
        while (hi - lo > 1) {
            const int64_t mid = (lo + hi) >> 1;
            if (doc_ptr[mid] <= e) lo = mid; else hi = mid;
        }
        atomicOr(&bits[(int64_t)s * Ws + (lo >> 6)], 1ull << (lo & 63));
    }
}

// ------------------------------------------------------------------------------------------------------------------ pairs
// slots: [Kb][N] of this batch; codf: [Kb][N][N] of this batch (entries i >= j are written).  W = ceil(M / 64) words hold documents.
static __global__ __launch_bounds__(CODF_WG) void codf_pairs_kernel(int64_t M, int64_t Ws, int N, const int32_t* __restrict__ slots,
                                                                    const unsigned long long* __restrict__ bits, unsigned long long* __restrict__ codf)
{
    __shared__ __attribute__((aligned(16))) unsigned long long s_rows[CODF_MAX_N * CODF_CHUNK_WORDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t w0 = (int64_t)blockIdx.x * CODF_CHUNK_WORDS;
    const int k = blockIdx.y;
#ifdef TMVB_MUTANT_CODF_DROP_TAIL
    const int64_t W = M >> 6;                           // MUTANT: the last, partial 64-document word is skipped
#else
    const int64_t W = (M + 63) >> 6;
#endif
    // stage: 16-byte units, CODF_CHUNK_WORDS / 2 per row; words at or past W read as zero (also the rows' pad word, never loaded past Ws)
    for (int u = tid; u < N * (CODF_CHUNK_WORDS / 2); u += CODF_WG) {
        const int row = u / (CODF_CHUNK_WORDS / 2), q = u % (CODF_CHUNK_WORDS / 2);
        const int64_t w = w0 + 2 * q;
        ulonglong2 v = make_ulonglong2(0ull, 0ull);
        if (w < Ws) v = *reinterpret_cast<const ulonglong2*>(bits + (int64_t)slots[k * N + row] * Ws + w);
        if (w >= W) v.x = 0ull;
        if (w + 1 >= W) v.y = 0ull;
        *reinterpret_cast<ulonglong2*>(&s_rows[row * CODF_CHUNK_WORDS + 2 * q]) = v;
    }
    __syncthreads();
    const int np = N * (N + 1) / 2;
    for (int p = wave; p < np; p += CODF_WG / 64) {     // wave-uniform: pair p = (i, j), i >= j, p = i (i + 1) / 2 + j
        int i = (int)((sqrtf(8.0f * (float)p + 1.0f) - 1.0f) * 0.5f);
        while (i * (i + 1) / 2 > p) i--;
        while ((i + 1) * (i + 2) / 2 <= p) i++;
        const int j = p - i * (i + 1) / 2;
        int c = __popcll(s_rows[i * CODF_CHUNK_WORDS + lane] & s_rows[j * CODF_CHUNK_WORDS + lane]);
        for (int o = 32; o; o >>= 1) c += __shfl_xor(c, o);
        if (lane == 0 && c) atomicAdd(&codf[((int64_t)k * N + i) * N + j], (unsigned long long)c);
    }
}

// ------------------------------------------------------------------------------------------------------------------ host
namespace {
// the K, N, M rules both entry points share
int codf_check_shape(const char* fn, int32_t K, int32_t N, int64_t M)
{
    TMVB_REQUIRE(K >= 1 && K <= CODF_MAX_K, TMVB_EINVAL, "%s: K = %d outside [1, %d]", fn, K, CODF_MAX_K);
    TMVB_REQUIRE(N >= CODF_MIN_N && N <= CODF_MAX_N, TMVB_EINVAL, "%s: N = %d outside [%d, %d]", fn, N, CODF_MIN_N, CODF_MAX_N);
    TMVB_REQUIRE(M > 0, TMVB_EINVAL, "%s: M must be a positive integer", fn);
    return TMVB_OK;
}

// how many ids of `row` the open batch has not seen yet; stamp[v] == k0 + 1 marks "seen in the batch that starts at topic k0"
int64_t codf_count_new(const int32_t* row, int N, std::vector<int32_t>& stamp, int32_t mark)
{
    int64_t n = 0;
    for (int i = 0; i < N; i++)
        if (stamp[(size_t)row[i]] != mark) n++;
    return n;
}

int codf_run(tmvb_ctx* ctx, int64_t M, int64_t V, const int64_t* doc_ptr, const int32_t* terms, int32_t K, int32_t N, const int32_t* top, int64_t budget,
             int64_t* codf, tmvb_codf_info_t* info)
{
    const int64_t nnz = doc_ptr[M], W = (M + 63) >> 6, Ws = (W + 1) & ~(int64_t)1, row_bytes = W * 8;
    // ---- batches of consecutive topics whose distinct ids fit the budget (the caller has checked that one topic fits: max_slots >= N)
    const int64_t max_slots = budget / row_bytes;
    std::vector<int32_t> stamp((size_t)V, 0), batch_first;      // stamp: 0 = never seen
    std::vector<int64_t> batch_slots;
    int64_t T_batch = 0;
    for (int32_t k = 0; k < K; k++) {
        const int32_t* row = top + (int64_t)k * N;
        const bool open = !batch_first.empty();
        if (!open || T_batch + codf_count_new(row, N, stamp, batch_first.back() + 1) > max_slots) {
            if (open) batch_slots.push_back(T_batch);
            batch_first.push_back(k);
            T_batch = 0;
        }
        const int32_t mark = batch_first.back() + 1;
        for (int i = 0; i < N; i++)
            if (stamp[(size_t)row[i]] != mark) { stamp[(size_t)row[i]] = mark; T_batch++; }
    }
    batch_slots.push_back(T_batch);
    const int n_batches = (int)batch_first.size();
    batch_first.push_back(K);
    const int64_t T_max = *std::max_element(batch_slots.begin(), batch_slots.end());
    int32_t Kb_max = 0;
    for (int b = 0; b < n_batches; b++) Kb_max = std::max(Kb_max, batch_first[b + 1] - batch_first[b]);
    int64_t T_all = 0;
    {
        std::vector<char> seen((size_t)V, 0);
        for (int64_t q = 0; q < (int64_t)K * N; q++)
            if (!seen[(size_t)top[q]]) { seen[(size_t)top[q]] = 1; T_all++; }
    }

    // host staging, declared in front of the call's scope
    std::vector<int32_t> h_map((size_t)V), h_slots((size_t)Kb_max * N);
    std::vector<int64_t> h_codf((size_t)Kb_max * N * N);

    hipStream_t st = ctx->stream;
    tmvb_call c("codocfreq", ctx->device, st);
    TMVB_CALL_TRY(c, c.begin());
    TMVB_CALL_TRY(c, c.events(3));
    int64_t* d_ptr;
    int32_t *d_terms, *d_map, *d_slots;
    unsigned long long *d_bits, *d_codf;
    TMVB_CALL_TRY(c, c.alloc(&d_ptr, (size_t)M + 1)); TMVB_CALL_TRY(c, c.alloc(&d_terms, (size_t)nnz)); TMVB_CALL_TRY(c, c.alloc(&d_map, (size_t)V));
    TMVB_CALL_TRY(c, c.alloc(&d_slots, (size_t)Kb_max * N)); TMVB_CALL_TRY(c, c.alloc(&d_bits, (size_t)(T_max * Ws)));
    TMVB_CALL_TRY(c, c.alloc(&d_codf, (size_t)Kb_max * N * N));
    TMVB_CALL_HIP(c, hipMemcpyAsync(d_ptr, doc_ptr, ((size_t)M + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    if (nnz > 0) TMVB_CALL_HIP(c, hipMemcpyAsync(d_terms, terms, (size_t)nnz * sizeof(int32_t), hipMemcpyHostToDevice, st));
    static_assert(sizeof(unsigned long long) == sizeof(int64_t), "counts travel as 64-bit integers");
    const int64_t chunks = (W + CODF_CHUNK_WORDS - 1) / CODF_CHUNK_WORDS;
    const unsigned build_blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>((nnz + CODF_WG - 1) / CODF_WG, (int64_t)ctx->num_cu * 8));
    float ms_bitset = 0.0f, ms_pairs = 0.0f;
    for (int b = 0; b < n_batches; b++) {
        const int32_t k0 = batch_first[b], Kb = batch_first[b + 1] - k0;
        std::fill(h_map.begin(), h_map.end(), -1);
        int32_t T = 0;
        for (int64_t q = 0; q < (int64_t)Kb * N; q++) {
            int32_t& s = h_map[(size_t)top[(int64_t)k0 * N + q]];
            if (s < 0) s = T++;
            h_slots[(size_t)q] = s;
        }
        TMVB_CALL_HIP(c, hipMemcpyAsync(d_map, h_map.data(), (size_t)V * sizeof(int32_t), hipMemcpyHostToDevice, st));
        TMVB_CALL_HIP(c, hipMemcpyAsync(d_slots, h_slots.data(), (size_t)Kb * N * sizeof(int32_t), hipMemcpyHostToDevice, st));
        TMVB_CALL_HIP(c, hipMemsetAsync(d_bits, 0, (size_t)(T * Ws) * sizeof(unsigned long long), st));
        TMVB_CALL_HIP(c, hipMemsetAsync(d_codf, 0, (size_t)Kb * N * N * sizeof(unsigned long long), st));
        // stage times: the events bracket the two kernels only; allocations, copies and memsets lie outside
        TMVB_CALL_HIP(c, hipEventRecord(c.ev(0), st));
        if (nnz > 0)
            hipLaunchKernelGGL(codf_bitset_kernel, dim3(build_blocks), dim3(CODF_WG), 0, st, M, nnz, Ws, (const int64_t*)d_ptr, (const int32_t*)d_terms,
                               (const int32_t*)d_map, d_bits);
        TMVB_CALL_HIP(c, hipGetLastError());
        TMVB_CALL_HIP(c, hipEventRecord(c.ev(1), st));
        hipLaunchKernelGGL(codf_pairs_kernel, dim3((unsigned)chunks, (unsigned)Kb), dim3(CODF_WG), 0, st, M, Ws, (int)N, (const int32_t*)d_slots,
                           (const unsigned long long*)d_bits, d_codf);
        TMVB_CALL_HIP(c, hipGetLastError());
        TMVB_CALL_HIP(c, hipEventRecord(c.ev(2), st));
        TMVB_CALL_HIP(c, hipMemcpyAsync(h_codf.data(), d_codf, (size_t)Kb * N * N * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        TMVB_CALL_HIP(c, hipStreamSynchronize(st));             // the next batch rewrites the map, the slot table and the bit matrix
        float ms_b = 0.0f, ms_p = 0.0f;
        TMVB_CALL_TRY(c, c.elapsed(&ms_b, 0, 1));
        TMVB_CALL_TRY(c, c.elapsed(&ms_p, 1, 2));
        ms_bitset += ms_b; ms_pairs += ms_p;
        for (int32_t k = 0; k < Kb; k++)                // mirror the lower triangle
            for (int i = 0; i < N; i++)
                for (int j = 0; j <= i; j++) {
                    const int64_t x = h_codf[((size_t)k * N + i) * N + j];
                    codf[((int64_t)(k0 + k) * N + i) * N + j] = x;
                    codf[((int64_t)(k0 + k) * N + j) * N + i] = x;
                }
    }
    if (info) { info->n_slots = T_all; info->n_batches = n_batches; info->ms_bitset = ms_bitset; info->ms_pairs = ms_pairs; }
    return TMVB_OK;
}

struct neumaier {                   // compensated sum: the result is the exact sum rounded, to first order
    double s = 0.0, c = 0.0;
    void add(double x)
    {
        const double t = s + x;
        c += std::fabs(s) >= std::fabs(x) ? (s - t) + x : (x - t) + s;
        s = t;
    }
    double value() const { return s + c; }
};
}  // namespace

extern "C" int tmvb_corpus_codocfreq(tmvb_ctx* ctx, int64_t M, int64_t V, const int64_t* doc_ptr, const int32_t* terms, const int32_t* counts, int32_t K,
                                     int32_t N, const int32_t* top, int64_t max_bitset_bytes, int64_t* codf, tmvb_codf_info_t* info)
{
    const char* fn = "tmvb_corpus_codocfreq";
    if (info) memset(info, 0, sizeof(*info));
    int rc = codf_check_shape(fn, K, N, M);
    if (rc != TMVB_OK) return rc;
    TMVB_REQUIRE(V > 0, TMVB_EINVAL, "%s: V must be a positive integer", fn);
    TMVB_REQUIRE((int64_t)N <= V, TMVB_EINVAL, "%s: N = %d top words of a vocabulary of %lld", fn, N, (long long)V);
    TMVB_REQUIRE(top && codf, TMVB_EINVAL, "%s: NULL argument", fn);
    TMVB_REQUIRE(max_bitset_bytes >= 0, TMVB_EINVAL, "%s: max_bitset_bytes must be nonnegative (0 = the default of %lld bytes)", fn,
                 (long long)TMVB_CODF_DEFAULT_BITSET_BYTES);
    if ((rc = tmvb_check_host_csr(fn, M, V, doc_ptr, terms, counts, false)) != TMVB_OK) return rc;
    {
        std::vector<int32_t> seen((size_t)V, -1);       // seen[v] = last topic whose row holds v
        for (int32_t k = 0; k < K; k++)
            for (int i = 0; i < N; i++) {
                const int32_t v = top[(int64_t)k * N + i];
                TMVB_REQUIRE(v >= 0 && v < V, TMVB_ESHAPE, "%s: top[%d][%d] = %d outside [0, %lld)", fn, k, i, v, (long long)V);
                TMVB_REQUIRE(seen[(size_t)v] != k, TMVB_ESHAPE, "%s: term %d is repeated in row %d of top", fn, v, k);
                seen[(size_t)v] = k;
            }
    }
    const int64_t budget = max_bitset_bytes > 0 ? max_bitset_bytes : (int64_t)TMVB_CODF_DEFAULT_BITSET_BYTES;
    // a topic that cannot fit is an argument error too, judged before the device
    const int64_t need = (int64_t)N * (((M + 63) >> 6) * 8);
    TMVB_REQUIRE(need <= budget, TMVB_EINVAL, "%s: one topic needs %lld bytes of bit matrix (N = %d rows of %lld bytes), max_bitset_bytes is %lld", fn,
                 (long long)need, N, (long long)(need / N), (long long)budget);
    if ((rc = tmvb_check_ctx_or_device(fn, ctx)) != TMVB_OK) return rc;
    return codf_run(ctx, M, V, doc_ptr, terms, K, N, top, budget, codf, info);
}

extern "C" int tmvb_coherence_from_counts(int32_t K, int32_t N, int64_t M, const int64_t* codf, double* umass, double* npmi, int32_t* undefined_pairs)
{
    const char* fn = "tmvb_coherence_from_counts";
    int rc = codf_check_shape(fn, K, N, M);
    if (rc != TMVB_OK) return rc;
    TMVB_REQUIRE(codf && umass && npmi && undefined_pairs, TMVB_EINVAL, "%s: NULL argument", fn);
    for (int32_t k = 0; k < K; k++) {
        const int64_t* D = codf + (int64_t)k * N * N;
        for (int i = 0; i < N; i++) {
            TMVB_REQUIRE(D[i * N + i] >= 0 && D[i * N + i] <= M, TMVB_ESHAPE, "%s: codf[%d][%d][%d] = %lld is no document frequency of %lld documents", fn, k, i, i,
                         (long long)D[i * N + i], (long long)M);
            for (int j = 0; j < i; j++) {
                const int64_t x = D[i * N + j];
                TMVB_REQUIRE(x == D[j * N + i], TMVB_ESHAPE, "%s: codf[%d] is not symmetric at (%d, %d)", fn, k, i, j);
                TMVB_REQUIRE(x >= 0, TMVB_ESHAPE, "%s: codf[%d][%d][%d] is negative", fn, k, i, j);
                // the other diagonal entry is checked against M when its row comes; compare with both here
                TMVB_REQUIRE(x <= D[i * N + i] && x <= D[j * N + j], TMVB_ESHAPE, "%s: codf[%d][%d][%d] = %lld exceeds a document frequency of its pair (%lld, %lld)", fn,
                             k, i, j, (long long)x, (long long)D[i * N + i], (long long)D[j * N + j]);
            }
        }
    }
    const double Md = (double)M;
    for (int32_t k = 0; k < K; k++) {
        const int64_t* D = codf + (int64_t)k * N * N;
        neumaier su, sn;
        int32_t undef = 0, def = 0;
        for (int i = 1; i < N; i++)
            for (int j = 0; j < i; j++) {               // j is the higher-ranked word
                const int64_t Dij = D[i * N + j], Di = D[i * N + i], Dj = D[j * N + j];
                if (Dj == 0) undef++;
                else { su.add(std::log((double)(Dij + 1) / (double)Dj)); def++; }
                if (Dij == 0) sn.add(-1.0);
                else if (Dij != M) sn.add(std::log(((double)Dij * Md) / ((double)Di * (double)Dj)) / -std::log((double)Dij / Md));
            }
        umass[k] = def > 0 ? su.value() / (double)def : std::numeric_limits<double>::quiet_NaN();
        npmi[k] = sn.value() / (double)(N * (N - 1) / 2);
        undefined_pairs[k] = undef;
    }
    return TMVB_OK;
}
