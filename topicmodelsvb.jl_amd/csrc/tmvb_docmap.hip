// tmvb_docmap.hip -- map documents in two dimensions: exact t-SNE over the topic kNN graph (include/tmvb.h states the definition; the reference
// has no such function).
//
// tmvb_map_affinity.
//   affinity  one wave per point, a lane per neighbour, fp64: the fixed schedule of TMVB_MAP_BISECT entropy evaluations (xor-butterfly sums, so every
//             lane holds the same bits and the branch is wave-uniform), then p_{j|i}.  Not hot.
//   symmetry  host C++: a counting sort by column gives the transposed lists (ascending by source, because the sources are walked ascending), each
//             row's own list is sorted by column, the two are merged; (a + b) / (2 M) in fp64, one rounding.
// tmvb_map_layout, per iteration:
//   repulse   grid = (tiles of MAP_PTS x 256 points, j_split).  A lane keeps MAP_PTS points in registers; the j's of a run of TMVB_MAP_RUN are
//             staged in LDS and read at one address by the whole wave (a broadcast read); the fp32 chain of the header runs over them in order;
//             the run sums are widened into the fp64 accumulators of the segment, and a segment's sums go to seg[segment][i][3].  A workgroup owns
//             whole segments (segment s goes to blockIdx.y = s mod j_split), so the cut of the sums never depends on the launch.
//   finish    one workgroup per block of TMVB_MAP_RUN rows: a lane adds its row's segment sums ascending (rep, zrow), lane 0 adds the block's zrow
//             sequentially.  map_total_kernel adds the block sums sequentially: Z.
//   attract   one wave per row: lane = slot (edge number mod 64), fp64; then every lane adds the 64 slot sums in order (shuffles).
//   update    one workgroup per block of rows: gradient, gains, velocity, y'; lanes 0 / 64 / 128 add the block's y'_x, y'_y and |g|^2 sequentially;
//             map_total_kernel gives the means, map_centre_kernel subtracts them.
//   KL        repulse / finish / total on the new state into buffers of their own, the attraction kernel's KL form, one more blocked sum.
// No floating-point atomics, no atomics at all.  #pragma clang fp contract(off) wherever the header promises separately rounded operations.
#include "tmvb_internal.h"
#include "tmvb_call.h"
#include "tmvb_philox.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <utility>
#include <vector>

#define MAP_RUN TMVB_MAP_RUN
#define MAP_SEG TMVB_MAP_SEG
#define MAP_PTS 2                   // points per lane of the repulsion kernel
#define MAP_TILE (MAP_PTS * 256)    // points per workgroup
#define MAP_CHUNK 512               // block sums staged per pass of the sequential adds
#define MAP_RING 32                 // iterations whose timing events are in flight
static_assert(MAP_RUN == 256, "a workgroup of the repulsion kernel stages one run; a workgroup of the blocked sums is one block");
static_assert(TMVB_MAP_SLOTS == 64, "a slot of the edge sums is a lane");

// ------------------------------------------------------------------------------------------------------------------ affinity
static __global__ __launch_bounds__(256) void map_affinity_kernel(int64_t M, int n, const float* __restrict__ d2, const int32_t* __restrict__ count, double u,
                                                                  double* __restrict__ beta, double* __restrict__ p)
{
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= M) return;                                 // wave-uniform
    const int ni = count[i];
    const bool valid = lane < ni;
    const double D = valid ? (double)d2[i * n + lane] : INFINITY;
    double mn = D;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mn = fmin(mn, __shfl_xor(mn, o, 64));
    const double delta = valid ? D - mn : 0.0;
    double b = 0.0, pj = 0.0;
    if (ni > 0 && (double)ni <= u) {
        pj = 1.0 / (double)ni;
    } else if (ni > 0) {
        const double logu = log(u);
        double lo = 0.0, hi = INFINITY;
        b = 1.0;
        for (int s = 0; s < TMVB_MAP_BISECT; s++) {
            const double e = valid ? exp(-b * delta) : 0.0;
            const double S = wave_sum_d(e), T = wave_sum_d(delta * e);
            const double H = log(S) + b * T / S;
            if (H > logu) { lo = b; b = hi == INFINITY ? 2.0 * b : 0.5 * (b + hi); }
            else { hi = b; b = 0.5 * (lo + b); }
        }
        const double e = valid ? exp(-b * delta) : 0.0;
        pj = e / wave_sum_d(e);
    }
    if (lane < n) p[i * n + lane] = valid ? pj : 0.0;
    if (lane == 0) beta[i] = b;
}

// ------------------------------------------------------------------------------------------------------------------ fixed-order sums
// one workgroup of 256 = one block of rows: v of the block's first nv rows (lane order) added sequentially ascending by lane `who`
__device__ __forceinline__ void map_block_seq(double v, int nv, double* sh, int who, double* out)
{
    sh[threadIdx.x] = v;
    __syncthreads();
    if ((int)threadIdx.x == who) {
        double s = 0.0;
        for (int q = 0; q < nv; q++) s += sh[q];
        *out = s;
    }
}

// one workgroup; wave c adds column c of part[ncols][nblk] sequentially ascending.  mode 0: outd[0] = sum - Md (Z); 1: outf[c] = (float)(sum / Md)
// (the means); 2: outd[c] = sum
static __global__ __launch_bounds__(256) void map_total_kernel(int64_t nblk, int ncols, const double* __restrict__ part, int mode, double Md, double* __restrict__ outd,
                                                               float* __restrict__ outf)
{
    __shared__ double buf[4][MAP_CHUNK];
    const int lane = threadIdx.x & 63, c = threadIdx.x >> 6;
    double s = 0.0;
    for (int64_t c0 = 0; c0 < nblk; c0 += MAP_CHUNK) {
        const int m = (int)min((int64_t)MAP_CHUNK, nblk - c0);
        __syncthreads();
        if (c < ncols)
            for (int q = lane; q < m; q += 64) buf[c][q] = part[(int64_t)c * nblk + c0 + q];
        __syncthreads();
        if (lane == 0 && c < ncols)
            for (int q = 0; q < m; q++) s += buf[c][q];
    }
    if (lane == 0 && c < ncols) {
        if (mode == 0) {
#ifdef TMVB_MUTANT_MAP_Z_SELF
            outd[0] = s;                                // MUTANT: the M self terms stay in Z
#else
            outd[0] = s - Md;
#endif
        } else if (mode == 1) outf[c] = (float)(s / Md);
        else outd[c] = s;
    }
}

// part[b] = v of block b added sequentially ascending
static __global__ __launch_bounds__(256) void map_block_sum_kernel(int64_t M, const double* __restrict__ v, double* __restrict__ part)
{
    __shared__ double sh[256];
    const int64_t i = (int64_t)blockIdx.x * MAP_RUN + threadIdx.x;
    const int nv = (int)min((int64_t)MAP_RUN, M - (int64_t)blockIdx.x * MAP_RUN);
    map_block_seq(i < M ? v[i] : 0.0, nv, sh, 0, part + blockIdx.x);
}

// ------------------------------------------------------------------------------------------------------------------ repulsion
__device__ __forceinline__ void map_pair(const float2 yi, const float2 yj, float& z, float& rx, float& ry)
{
    const float dx = yi.x - yj.x, dy = yi.y - yj.y;
    const float d = fmaf(dy, dy, fmaf(dx, dx, 1.0f));
    const float q = __builtin_amdgcn_rcpf(d);           // <= 1 ulp; d >= 1
    z += q;
    const float w = q * q;
    rx = fmaf(w, dx, rx);
    ry = fmaf(w, dy, ry);
}

// seg: [nseg][M][3] = (z, rx, ry) of segment s and point i
static __global__ __launch_bounds__(256) void map_repulse_kernel(int64_t M, int nruns, int nseg, const float2* __restrict__ y, double* __restrict__ seg)
{
    __shared__ __attribute__((aligned(16))) float2 sy[MAP_RUN];
    const int tid = threadIdx.x;
    int64_t ip[MAP_PTS];
    float2 yi[MAP_PTS];
#pragma unroll
    for (int p = 0; p < MAP_PTS; p++) {
        ip[p] = (int64_t)blockIdx.x * MAP_TILE + p * 256 + tid;
        yi[p] = ip[p] < M ? y[ip[p]] : make_float2(0.0f, 0.0f);
    }
    for (int s = blockIdx.y; s < nseg; s += gridDim.y) {                  // workgroup-uniform
        double Z[MAP_PTS], RX[MAP_PTS], RY[MAP_PTS];
#pragma unroll
        for (int p = 0; p < MAP_PTS; p++) Z[p] = RX[p] = RY[p] = 0.0;
        const int r1 = min(nruns, (s + 1) * MAP_SEG);
        for (int r = s * MAP_SEG; r < r1; r++) {
            const int64_t j0 = (int64_t)r * MAP_RUN;
            const int nj = (int)min((int64_t)MAP_RUN, M - j0);
            __syncthreads();
            if (tid < nj) sy[tid] = y[j0 + tid];
            __syncthreads();
            float z[MAP_PTS], rx[MAP_PTS], ry[MAP_PTS];
#pragma unroll
            for (int p = 0; p < MAP_PTS; p++) z[p] = rx[p] = ry[p] = 0.0f;
            if (nj == MAP_RUN) {
#pragma unroll 8
                for (int j = 0; j < MAP_RUN; j++) {
                    const float2 yj = sy[j];                              // one address for the wave: a broadcast read
#pragma unroll
                    for (int p = 0; p < MAP_PTS; p++) map_pair(yi[p], yj, z[p], rx[p], ry[p]);
                }
            } else {
                for (int j = 0; j < nj; j++) {
                    const float2 yj = sy[j];
#pragma unroll
                    for (int p = 0; p < MAP_PTS; p++) map_pair(yi[p], yj, z[p], rx[p], ry[p]);
                }
            }
#pragma unroll
            for (int p = 0; p < MAP_PTS; p++) { Z[p] += (double)z[p]; RX[p] += (double)rx[p]; RY[p] += (double)ry[p]; }
        }
#pragma unroll
        for (int p = 0; p < MAP_PTS; p++)
            if (ip[p] < M) {
                double* o = seg + ((int64_t)s * M + ip[p]) * 3;
                o[0] = Z[p]; o[1] = RX[p]; o[2] = RY[p];
            }
    }
}

static __global__ __launch_bounds__(256) void map_finish_kernel(int64_t M, int nseg, const double* __restrict__ seg, double* __restrict__ rep, double* __restrict__ zrow,
                                                                double* __restrict__ bsum)
{
    __shared__ double sh[256];
    const int64_t i = (int64_t)blockIdx.x * MAP_RUN + threadIdx.x;
    double z = 0.0, rx = 0.0, ry = 0.0;
    if (i < M) {
        for (int s = 0; s < nseg; s++) {
            const double* o = seg + ((int64_t)s * M + i) * 3;
            z += o[0]; rx += o[1]; ry += o[2];
        }
        zrow[i] = z; rep[2 * i] = rx; rep[2 * i + 1] = ry;
    }
    const int nv = (int)min((int64_t)MAP_RUN, M - (int64_t)blockIdx.x * MAP_RUN);
    map_block_seq(z, nv, sh, 0, bsum + blockIdx.x);
}

// ------------------------------------------------------------------------------------------------------------------ attraction, KL
template <bool KL>
static __global__ __launch_bounds__(256) void map_attract_kernel(int64_t M, const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col, const float* __restrict__ val,
                                                                 const float2* __restrict__ y, const double* __restrict__ Zp, double* __restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= M) return;                                 // wave-uniform
    const float2 yi = y[i];
    const double xi = (double)yi.x, wi = (double)yi.y, Z = KL ? *Zp : 0.0;
    double a0 = 0.0, a1 = 0.0;
    const int64_t e1 = row_ptr[i + 1];
    for (int64_t m = row_ptr[i] + lane; m < e1; m += 64) {
        const float2 yj = y[col[m]];
        const double p = (double)val[m], dx = xi - (double)yj.x, dy = wi - (double)yj.y;
        const double d1 = 1.0 + (dx * dx + dy * dy);
        if (KL) {
            if (p > 0.0) a0 += p * log((p * Z) * d1);
        } else {
            a0 += (p * dx) / d1;
            a1 += (p * dy) / d1;
        }
    }
    double s0 = 0.0, s1 = 0.0;
    for (int q = 0; q < 64; q++) {                      // the slots in order, in every lane
        s0 += __shfl(a0, q, 64);
        if (!KL) s1 += __shfl(a1, q, 64);
    }
    if (lane == 0) {
        if (KL) out[i] = s0;
        else { out[2 * i] = s0; out[2 * i + 1] = s1; }
    }
}

// ------------------------------------------------------------------------------------------------------------------ update
// bsum: [3][nblk] = the block sums of y'_x, y'_y and |g|^2
static __global__ __launch_bounds__(256) void map_update_kernel(int64_t M, int64_t nblk, double e, float mu, float eta, float min_gain, const double* __restrict__ Zp,
                                                                const double* __restrict__ att, const double* __restrict__ rep, float* __restrict__ grad,
                                                                float* __restrict__ y, float* __restrict__ vel, float* __restrict__ gain, double* __restrict__ bsum)
{
#pragma clang fp contract(off)
    __shared__ double sh[3][256];
    const int64_t i = (int64_t)blockIdx.x * MAP_RUN + threadIdx.x;
    const double Z = *Zp;
    double yn[2] = {0.0, 0.0}, g2 = 0.0;
    if (i < M) {
        double gg[2];
#pragma unroll
        for (int c = 0; c < 2; c++) {
            const int64_t k = 2 * i + c;
            const double t = e * att[k];
            const double r = rep[k] / Z;
            const float g = (float)(4.0 * (t - r));
            grad[k] = g;
            const float v0 = vel[k];
            const bool differ = (v0 > 0.0f && g < 0.0f) || (v0 < 0.0f && g > 0.0f);
            float ga = gain[k];
            ga = differ ? ga + 0.2f : ga * 0.8f;
            ga = fmaxf(ga, min_gain);
            const float step = (eta * ga) * g;
            const float mv = mu * v0;
            const float v1 = mv - step;
            const float y1 = y[k] + v1;
            gain[k] = ga; vel[k] = v1; y[k] = y1;
            yn[c] = (double)y1;
            gg[c] = (double)g * (double)g;
        }
        g2 = gg[0] + gg[1];
    }
    const int nv = (int)min((int64_t)MAP_RUN, M - (int64_t)blockIdx.x * MAP_RUN);
    sh[0][threadIdx.x] = yn[0]; sh[1][threadIdx.x] = yn[1]; sh[2][threadIdx.x] = g2;
    __syncthreads();
    if ((threadIdx.x & 63) == 0 && threadIdx.x < 192) {
        const int c = threadIdx.x >> 6;
        double s = 0.0;
        for (int q = 0; q < nv; q++) s += sh[c][q];
        bsum[(int64_t)c * nblk + blockIdx.x] = s;
    }
}

static __global__ __launch_bounds__(256) void map_centre_kernel(int64_t M, const float* __restrict__ mean, float* __restrict__ y)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k < 2 * M) y[k] = y[k] - mean[k & 1];
}

static __global__ __launch_bounds__(256) void map_init_kernel(int64_t M, uint64_t seed, float* __restrict__ y)
{
#pragma clang fp contract(off)
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= 2 * M) return;
    const tmvb_philox4 r = tmvb_rng(seed, (uint64_t)(k >> 1), TMVB_RNG_MAP, (uint32_t)(k & 1), 0);
    const double u = tmvb_u53(r.x[0], r.x[1]);
    y[k] = (float)(1e-4 * (2.0 * u - 1.0));
}

// ------------------------------------------------------------------------------------------------------------------ host
namespace {
struct map_fwd { int32_t j; int32_t slot; };

int map_affinity_run(tmvb_ctx* ctx, int64_t M, int32_t n, const int32_t* idx, const float* d2, const int32_t* count, double u, const std::vector<map_fwd>& fwd,
                     const std::vector<int64_t>& tptr, double* beta, double* p_cond, int64_t* row_ptr, int32_t* col, float* val)
{
    hipStream_t st = ctx->stream;
    {
        tmvb_call c("map_affinity", ctx->device, st);
        TMVB_CALL_TRY(c, c.begin());
        float* d_d2; int32_t* d_count; double *d_beta, *d_p;
        TMVB_CALL_TRY(c, c.upload(&d_d2, d2, (size_t)M * n));
        TMVB_CALL_TRY(c, c.upload(&d_count, count, (size_t)M));
        TMVB_CALL_TRY(c, c.alloc(&d_beta, (size_t)M)); TMVB_CALL_TRY(c, c.alloc(&d_p, (size_t)M * n));
        hipLaunchKernelGGL(map_affinity_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, M, (int)n, (const float*)d_d2, (const int32_t*)d_count, u, d_beta, d_p);
        TMVB_CALL_HIP(c, hipGetLastError());
        TMVB_CALL_HIP(c, hipMemcpyAsync(beta, d_beta, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, st));
        TMVB_CALL_HIP(c, hipMemcpyAsync(p_cond, d_p, (size_t)M * n * sizeof(double), hipMemcpyDeviceToHost, st));
        TMVB_CALL_HIP(c, hipStreamSynchronize(st));
    }
    if (!row_ptr) return TMVB_OK;
    // ---- the transposed lists: row j of T = (source i, p_{j|i}), ascending by i because i is walked ascending
    const int64_t nf = tptr[(size_t)M];
    std::vector<int32_t> tsrc((size_t)nf);
    std::vector<double> tval((size_t)nf);
    std::vector<int64_t> fill(tptr.begin(), tptr.end() - 1);
    for (int64_t i = 0; i < M; i++)
        for (int s = 0; s < count[i]; s++) {
            const int64_t j = idx[i * n + s], at = fill[(size_t)j]++;
            tsrc[(size_t)at] = (int32_t)i;
            tval[(size_t)at] = p_cond[i * n + s];
        }
    // ---- merge row i of the sorted own list (a) with row i of T (b)
    const double two_m = 2.0 * (double)M;
    int64_t o = 0;
    for (int64_t i = 0; i < M; i++) {
        row_ptr[i] = o;
        const map_fwd* f = fwd.data() + i * n;
        const int nf_i = count[i];
        int a = 0;
        int64_t b = tptr[(size_t)i];
        const int64_t b1 = tptr[(size_t)i + 1];
        while (a < nf_i || b < b1) {
            const int32_t ja = a < nf_i ? f[a].j : INT32_MAX, jb = b < b1 ? tsrc[(size_t)b] : INT32_MAX;
            double pa = 0.0, pb = 0.0;
            const int32_t j = std::min(ja, jb);
            if (ja == j) pa = p_cond[i * n + f[a++].slot];
            if (jb == j) pb = tval[(size_t)b++];
            col[o] = j;
            val[o] = (float)((pa + pb) / two_m);
            o++;
        }
    }
    row_ptr[M] = o;
    return TMVB_OK;
}

int map_layout_run(tmvb_ctx* ctx, int64_t M, const int64_t* row_ptr, const int32_t* col, const float* val, const tmvb_map_params_t& P, const float* y0, const float* vel0,
                   const float* gain0, float* y, float* vel, float* gain, double* kl, int32_t* kl_iter, double* rep, double* zrow, double* att, float* grad,
                   tmvb_map_info_t* info)
{
    const int64_t nnz = row_ptr[M], nblk = (M + MAP_RUN - 1) / MAP_RUN, tiles = (M + MAP_TILE - 1) / MAP_TILE;
    const int nruns = (int)nblk, nseg = (nruns + MAP_SEG - 1) / MAP_SEG;
    int js = P.j_split > 0 ? P.j_split : (int)std::max<int64_t>(1, (2048 + tiles - 1) / tiles);       // about eight workgroups per CU in flight
    js = std::min(js, nseg);
    const double Md = (double)M;
    const unsigned gblk = (unsigned)nblk, gwave = (unsigned)((M + 3) / 4), gflat = (unsigned)((2 * M + 255) / 256);

    std::vector<float> h_gain;
    std::vector<double> h_kl;
    hipStream_t st = ctx->stream;
    tmvb_call c("map_layout", ctx->device, st);
    TMVB_CALL_TRY(c, c.begin());
    TMVB_CALL_TRY(c, c.events(4 * MAP_RING));
    int64_t* d_ptr; int32_t* d_col; float *d_val, *d_y, *d_vel, *d_gain, *d_grad, *d_mean;
    double *d_seg, *d_rep[2], *d_zrow[2], *d_Z, *d_att, *d_klrow, *d_bsum, *d_bsum3, *d_kl, *d_gn;
    TMVB_CALL_TRY(c, c.upload(&d_ptr, row_ptr, (size_t)M + 1));
    TMVB_CALL_TRY(c, c.upload(&d_col, col, (size_t)nnz));
    TMVB_CALL_TRY(c, c.upload(&d_val, val, (size_t)nnz));
    if (y0) TMVB_CALL_TRY(c, c.upload(&d_y, y0, (size_t)2 * M));
    else {
        TMVB_CALL_TRY(c, c.alloc(&d_y, (size_t)2 * M));
        hipLaunchKernelGGL(map_init_kernel, dim3(gflat), dim3(256), 0, st, M, (uint64_t)P.seed, d_y);
        TMVB_CALL_HIP(c, hipGetLastError());
    }
    if (vel0) TMVB_CALL_TRY(c, c.upload(&d_vel, vel0, (size_t)2 * M));
    else {
        TMVB_CALL_TRY(c, c.alloc(&d_vel, (size_t)2 * M));
        TMVB_CALL_HIP(c, hipMemsetAsync(d_vel, 0, (size_t)2 * M * sizeof(float), st));
    }
    if (!gain0) h_gain.assign((size_t)2 * M, 1.0f);
    TMVB_CALL_TRY(c, c.upload(&d_gain, gain0 ? gain0 : (const float*)h_gain.data(), (size_t)2 * M));
    TMVB_CALL_TRY(c, c.alloc(&d_grad, (size_t)2 * M)); TMVB_CALL_TRY(c, c.alloc(&d_mean, 2));
    TMVB_CALL_TRY(c, c.alloc(&d_seg, (size_t)nseg * M * 3));
    for (int k = 0; k < 2; k++) { TMVB_CALL_TRY(c, c.alloc(&d_rep[k], (size_t)2 * M)); TMVB_CALL_TRY(c, c.alloc(&d_zrow[k], (size_t)M)); }
    TMVB_CALL_TRY(c, c.alloc(&d_Z, 2)); TMVB_CALL_TRY(c, c.alloc(&d_att, (size_t)2 * M)); TMVB_CALL_TRY(c, c.alloc(&d_klrow, (size_t)M));
    TMVB_CALL_TRY(c, c.alloc(&d_bsum, (size_t)nblk)); TMVB_CALL_TRY(c, c.alloc(&d_bsum3, (size_t)3 * nblk));
    const int kl_max = (P.check > 0 ? P.iters / P.check : 0) + 2;
    TMVB_CALL_TRY(c, c.alloc(&d_kl, (size_t)kl_max)); TMVB_CALL_TRY(c, c.alloc(&d_gn, 1));
    TMVB_CALL_HIP(c, hipMemsetAsync(d_rep[0], 0, (size_t)2 * M * sizeof(double), st));
    TMVB_CALL_HIP(c, hipMemsetAsync(d_zrow[0], 0, (size_t)M * sizeof(double), st));
    TMVB_CALL_HIP(c, hipMemsetAsync(d_att, 0, (size_t)2 * M * sizeof(double), st));
    TMVB_CALL_HIP(c, hipMemsetAsync(d_grad, 0, (size_t)2 * M * sizeof(float), st));
    TMVB_CALL_HIP(c, hipMemsetAsync(d_Z, 0, 2 * sizeof(double), st));
    TMVB_CALL_HIP(c, hipMemsetAsync(d_gn, 0, sizeof(double), st));

    // Z(y) with its rows: set k = 0 for the gradient, 1 for the KL
    auto repulse = [&](int k) -> int {
        hipLaunchKernelGGL(map_repulse_kernel, dim3((unsigned)tiles, (unsigned)js), dim3(256), 0, st, M, nruns, nseg, (const float2*)d_y, d_seg);
        hipLaunchKernelGGL(map_finish_kernel, dim3(gblk), dim3(256), 0, st, M, nseg, (const double*)d_seg, d_rep[k], d_zrow[k], d_bsum);
        hipLaunchKernelGGL(map_total_kernel, dim3(1), dim3(256), 0, st, nblk, 1, (const double*)d_bsum, 0, Md, d_Z + k, (float*)nullptr);
        TMVB_CALL_HIP(c, hipGetLastError());
        return TMVB_OK;
    };
    int n_kl = 0;
    auto kl_eval = [&](int done_global) -> int {
        TMVB_CALL_TRY(c, repulse(1));
        hipLaunchKernelGGL(map_attract_kernel<true>, dim3(gwave), dim3(256), 0, st, M, (const int64_t*)d_ptr, (const int32_t*)d_col, (const float*)d_val, (const float2*)d_y,
                           (const double*)(d_Z + 1), d_klrow);
        hipLaunchKernelGGL(map_block_sum_kernel, dim3(gblk), dim3(256), 0, st, M, (const double*)d_klrow, d_bsum);
        hipLaunchKernelGGL(map_total_kernel, dim3(1), dim3(256), 0, st, nblk, 1, (const double*)d_bsum, 2, Md, d_kl + n_kl, (float*)nullptr);
        TMVB_CALL_HIP(c, hipGetLastError());
        kl_iter[n_kl++] = done_global;
        return TMVB_OK;
    };

    float ms_rep = 0.0f, ms_att = 0.0f, ms_upd = 0.0f, ms = 0.0f;
    auto collect = [&](int slot) -> int {                                  // the slot's last event has completed
        TMVB_CALL_TRY(c, c.elapsed(&ms, 4 * slot, 4 * slot + 1)); ms_rep += ms;
        TMVB_CALL_TRY(c, c.elapsed(&ms, 4 * slot + 1, 4 * slot + 2)); ms_att += ms;
        TMVB_CALL_TRY(c, c.elapsed(&ms, 4 * slot + 2, 4 * slot + 3)); ms_upd += ms;
        return TMVB_OK;
    };
    int done = 0, stop = 0, last_kl = -1;
    for (int t = 0; t < P.iters; t++) {
        const int T = P.iter0 + t, slot = t % MAP_RING;
        const bool early = T < P.exag_iters;
        if (t >= MAP_RING) {
            TMVB_CALL_HIP(c, hipEventSynchronize(c.ev(4 * slot + 3)));
            TMVB_CALL_TRY(c, collect(slot));
        }
        TMVB_CALL_HIP(c, hipEventRecord(c.ev(4 * slot), st));
        TMVB_CALL_TRY(c, repulse(0));
        TMVB_CALL_HIP(c, hipEventRecord(c.ev(4 * slot + 1), st));
        hipLaunchKernelGGL(map_attract_kernel<false>, dim3(gwave), dim3(256), 0, st, M, (const int64_t*)d_ptr, (const int32_t*)d_col, (const float*)d_val,
                           (const float2*)d_y, (const double*)nullptr, d_att);
        TMVB_CALL_HIP(c, hipEventRecord(c.ev(4 * slot + 2), st));
        hipLaunchKernelGGL(map_update_kernel, dim3(gblk), dim3(256), 0, st, M, nblk, early ? P.exaggeration : 1.0, early ? P.momentum0 : P.momentum1, P.eta, P.min_gain,
                           (const double*)d_Z, (const double*)d_att, (const double*)d_rep[0], d_grad, d_y, d_vel, d_gain, d_bsum3);
        hipLaunchKernelGGL(map_total_kernel, dim3(1), dim3(256), 0, st, nblk, 2, (const double*)d_bsum3, 1, Md, (double*)nullptr, d_mean);
        hipLaunchKernelGGL(map_centre_kernel, dim3(gflat), dim3(256), 0, st, M, (const float*)d_mean, d_y);
        TMVB_CALL_HIP(c, hipGetLastError());
        TMVB_CALL_HIP(c, hipEventRecord(c.ev(4 * slot + 3), st));
        done = t + 1;
        if (P.check > 0 && (T + 1) % P.check == 0) {
            TMVB_CALL_TRY(c, kl_eval(T + 1));
            last_kl = T + 1;
            if (P.min_grad_norm > 0.0) {
                double g2 = 0.0;
                hipLaunchKernelGGL(map_total_kernel, dim3(1), dim3(256), 0, st, nblk, 1, (const double*)(d_bsum3 + 2 * nblk), 2, Md, d_gn, (float*)nullptr);
                TMVB_CALL_HIP(c, hipGetLastError());
                TMVB_CALL_HIP(c, hipMemcpyAsync(&g2, d_gn, sizeof(double), hipMemcpyDeviceToHost, st));
                TMVB_CALL_HIP(c, hipStreamSynchronize(st));
                if (std::sqrt(g2) < P.min_grad_norm) { stop = 1; break; }
            }
        }
    }
    if (last_kl != P.iter0 + done) TMVB_CALL_TRY(c, kl_eval(P.iter0 + done));
    if (done > 0) {
        hipLaunchKernelGGL(map_total_kernel, dim3(1), dim3(256), 0, st, nblk, 1, (const double*)(d_bsum3 + 2 * nblk), 2, Md, d_gn, (float*)nullptr);
        TMVB_CALL_HIP(c, hipGetLastError());
    }

    // ---- results
    double h_Z = 0.0, h_g2 = 0.0;
    h_kl.resize((size_t)n_kl);
    TMVB_CALL_HIP(c, hipMemcpyAsync(y, d_y, (size_t)2 * M * sizeof(float), hipMemcpyDeviceToHost, st));
    TMVB_CALL_HIP(c, hipMemcpyAsync(vel, d_vel, (size_t)2 * M * sizeof(float), hipMemcpyDeviceToHost, st));
    TMVB_CALL_HIP(c, hipMemcpyAsync(gain, d_gain, (size_t)2 * M * sizeof(float), hipMemcpyDeviceToHost, st));
    TMVB_CALL_HIP(c, hipMemcpyAsync(h_kl.data(), d_kl, (size_t)n_kl * sizeof(double), hipMemcpyDeviceToHost, st));
    TMVB_CALL_HIP(c, hipMemcpyAsync(&h_Z, d_Z, sizeof(double), hipMemcpyDeviceToHost, st));
    TMVB_CALL_HIP(c, hipMemcpyAsync(&h_g2, d_gn, sizeof(double), hipMemcpyDeviceToHost, st));
    if (rep) TMVB_CALL_HIP(c, hipMemcpyAsync(rep, d_rep[0], (size_t)2 * M * sizeof(double), hipMemcpyDeviceToHost, st));
    if (zrow) TMVB_CALL_HIP(c, hipMemcpyAsync(zrow, d_zrow[0], (size_t)M * sizeof(double), hipMemcpyDeviceToHost, st));
    if (att) TMVB_CALL_HIP(c, hipMemcpyAsync(att, d_att, (size_t)2 * M * sizeof(double), hipMemcpyDeviceToHost, st));
    if (grad) TMVB_CALL_HIP(c, hipMemcpyAsync(grad, d_grad, (size_t)2 * M * sizeof(float), hipMemcpyDeviceToHost, st));
    TMVB_CALL_HIP(c, hipStreamSynchronize(st));
    for (int s = 0; s < std::min(done, MAP_RING); s++) TMVB_CALL_TRY(c, collect(s));
    for (int k = 0; k < n_kl; k++) kl[k] = h_kl[(size_t)k];
    if (info) {
        info->iters = done; info->stop = stop; info->n_kl = n_kl; info->j_split = js; info->Z = h_Z; info->grad_norm = std::sqrt(h_g2);
        info->ms_rep = ms_rep; info->ms_att = ms_att; info->ms_upd = ms_upd;
    }
    for (int64_t k = 0; k < 2 * M; k++)
        if (!std::isfinite(y[k]) || !std::isfinite(vel[k]) || !std::isfinite(gain[k])) {
            tmvb_set_error("tmvb_map_layout: the state is not finite after %d iterations (entry %lld)", done, (long long)k);
            return TMVB_ENONFINITE;
        }
    return TMVB_OK;
}
}  // namespace

extern "C" int tmvb_map_affinity(tmvb_ctx* ctx, int64_t M, int64_t Mc, int32_t n, const int32_t* idx, const float* d2, const int32_t* count, double perplexity,
                                 double* beta, double* p_cond, int64_t* row_ptr, int32_t* col, float* val)
{
    const char* fn = "tmvb_map_affinity";
    const bool sym = row_ptr || col || val;             // else: the conditional form, rows = new points against Mc mapped ones
    TMVB_REQUIRE(M >= (sym ? 2 : 1) && M < ((int64_t)1 << 31), TMVB_EINVAL, "%s: M = %lld outside [%d, 2^31)", fn, (long long)M, sym ? 2 : 1);
    TMVB_REQUIRE(sym ? Mc == M : (Mc >= 1 && Mc < ((int64_t)1 << 31)), TMVB_EINVAL, "%s: Mc = %lld (M with the symmetric matrix, else in [1, 2^31))", fn, (long long)Mc);
    TMVB_REQUIRE(n >= 1 && n <= TMVB_NB_TOPN_MAX, TMVB_EINVAL, "%s: n = %d outside [1, %d]", fn, n, TMVB_NB_TOPN_MAX);
    TMVB_REQUIRE(2 * M * n < ((int64_t)1 << 31), TMVB_EINVAL, "%s: 2 M n = %lld entries, not below 2^31", fn, (long long)(2 * M * n));
    TMVB_REQUIRE(std::isfinite(perplexity) && perplexity >= 1.0, TMVB_EINVAL, "%s: the perplexity must be a finite number >= 1", fn);
    TMVB_REQUIRE(idx && d2 && count && beta && p_cond && (!sym || (row_ptr && col && val)), TMVB_EINVAL, "%s: NULL argument", fn);
    // the own lists sorted by column (slot = where the entry stands in the caller's row) and the in-degrees
    std::vector<map_fwd> fwd((size_t)M * n);
    std::vector<int64_t> tptr((size_t)M + 1, 0);
    for (int64_t i = 0; i < M; i++) {
        const int ni = count[i];
        TMVB_REQUIRE(ni >= 0 && ni <= n, TMVB_ESHAPE, "%s: count = %d outside [0, n] (row %lld)", fn, ni, (long long)i);
        map_fwd* f = fwd.data() + i * n;
        for (int s = 0; s < ni; s++) {
            const int32_t j = idx[i * n + s];
            const float d = d2[i * n + s];
            TMVB_REQUIRE(j >= 0 && j < Mc, TMVB_ESHAPE, "%s: neighbour index %d outside [0, Mc) (row %lld)", fn, j, (long long)i);
            TMVB_REQUIRE(!sym || j != i, TMVB_ESHAPE, "%s: a point among its own neighbours (row %lld)", fn, (long long)i);
            TMVB_REQUIRE(std::isfinite(d) && d >= 0.0f, TMVB_ESHAPE, "%s: negative or non-finite distance (row %lld)", fn, (long long)i);
            f[s].j = j; f[s].slot = s;
        }
        std::sort(f, f + ni, [](const map_fwd& a, const map_fwd& b) { return a.j < b.j; });
        for (int s = 1; s < ni; s++) TMVB_REQUIRE(f[s].j != f[s - 1].j, TMVB_ESHAPE, "%s: neighbour %d listed twice (row %lld)", fn, f[s].j, (long long)i);
        if (sym)
            for (int s = 0; s < ni; s++) tptr[(size_t)f[s].j + 1]++;
    }
    for (int64_t j = 0; j < M; j++) tptr[(size_t)j + 1] += tptr[(size_t)j];
    const int rc = tmvb_check_ctx_or_device(fn, ctx);
    if (rc != TMVB_OK) return rc;
    return map_affinity_run(ctx, M, n, idx, d2, count, perplexity, fwd, tptr, beta, p_cond, row_ptr, col, val);
}

extern "C" int tmvb_map_layout(tmvb_ctx* ctx, int64_t M, const int64_t* row_ptr, const int32_t* col, const float* val, const tmvb_map_params_t* params, const float* y0,
                               const float* vel0, const float* gain0, float* y, float* vel, float* gain, int32_t kl_cap, double* kl, int32_t* kl_iter, double* rep,
                               double* zrow, double* att, float* grad, tmvb_map_info_t* info)
{
    const char* fn = "tmvb_map_layout";
    if (info) memset(info, 0, sizeof(*info));
    TMVB_REQUIRE(M >= 2 && M < ((int64_t)1 << 31), TMVB_EINVAL, "%s: M = %lld outside [2, 2^31)", fn, (long long)M);
    TMVB_REQUIRE(row_ptr && col && val && params && y && vel && gain && kl && kl_iter, TMVB_EINVAL, "%s: NULL argument", fn);
    const tmvb_map_params_t& P = *params;
    TMVB_REQUIRE(P.iters >= 0 && P.iters <= 100000, TMVB_EINVAL, "%s: iters = %d outside [0, 100000]", fn, P.iters);
    TMVB_REQUIRE(P.iter0 >= 0 && P.iter0 <= (1 << 30), TMVB_EINVAL, "%s: iter0 = %d outside [0, 2^30]", fn, P.iter0);
    TMVB_REQUIRE(P.exag_iters >= 0 && P.check >= 0 && P.j_split >= 0, TMVB_EINVAL, "%s: exag_iters, check and j_split must not be negative", fn);
    TMVB_REQUIRE(std::isfinite(P.exaggeration) && P.exaggeration >= 1.0, TMVB_EINVAL, "%s: exaggeration must be a finite number >= 1", fn);
    TMVB_REQUIRE(std::isfinite(P.eta) && P.eta > 0.0f, TMVB_EINVAL, "%s: eta must be a finite positive number", fn);
    TMVB_REQUIRE(P.momentum0 >= 0.0f && P.momentum0 < 1.0f && P.momentum1 >= 0.0f && P.momentum1 < 1.0f, TMVB_EINVAL, "%s: momentum outside [0, 1)", fn);
    TMVB_REQUIRE(std::isfinite(P.min_gain) && P.min_gain > 0.0f, TMVB_EINVAL, "%s: min_gain must be a finite positive number", fn);
    TMVB_REQUIRE(std::isfinite(P.min_grad_norm) && P.min_grad_norm >= 0.0, TMVB_EINVAL, "%s: min_grad_norm must be a finite nonnegative number", fn);
    TMVB_REQUIRE(kl_cap >= (P.check > 0 ? P.iters / P.check : 0) + 2, TMVB_EINVAL, "%s: kl_cap = %d, need iters / check + 2", fn, kl_cap);
    TMVB_REQUIRE(y0 || P.iter0 == 0, TMVB_EINVAL, "%s: y0 == NULL (the seeded start) needs iter0 == 0", fn);
    TMVB_REQUIRE(row_ptr[0] == 0, TMVB_ESHAPE, "%s: row_ptr[0] != 0", fn);
    for (int64_t i = 0; i < M; i++) {
        TMVB_REQUIRE(row_ptr[i + 1] >= row_ptr[i] && row_ptr[i + 1] < ((int64_t)1 << 31), TMVB_ESHAPE, "%s: row_ptr not ascending or beyond 2^31 (row %lld)", fn, (long long)i);
        for (int64_t m = row_ptr[i]; m < row_ptr[i + 1]; m++) {
            TMVB_REQUIRE(col[m] >= 0 && col[m] < M && col[m] != i, TMVB_ESHAPE, "%s: column %d outside [0, M) or on the diagonal (row %lld)", fn, col[m], (long long)i);
            TMVB_REQUIRE(m == row_ptr[i] || col[m] > col[m - 1], TMVB_ESHAPE, "%s: columns not strictly ascending (row %lld)", fn, (long long)i);
            TMVB_REQUIRE(std::isfinite(val[m]) && val[m] >= 0.0f, TMVB_ESHAPE, "%s: negative or non-finite value (row %lld)", fn, (long long)i);
        }
    }
    for (int64_t k = 0; k < 2 * M; k++)
        TMVB_REQUIRE((!y0 || std::isfinite(y0[k])) && (!vel0 || std::isfinite(vel0[k])) && (!gain0 || std::isfinite(gain0[k])), TMVB_ESHAPE,
                     "%s: non-finite state (entry %lld)", fn, (long long)k);
    const int rc = tmvb_check_ctx_or_device(fn, ctx);
    if (rc != TMVB_OK) return rc;
    return map_layout_run(ctx, M, row_ptr, col, val, P, y0, vel0, gain0, y, vel, gain, kl, kl_iter, rep, zrow, att, grad, info);
}
