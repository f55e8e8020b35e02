// pca.hip -- principal components of resident embedding rows: the column means, the scatter matrix S = sum_rows xc xc^T of the centred
// rows on the fp32 matrix cores, and the projection onto given components and back (include/l3hip.h, "Principal components"; DESIGN.md
// section 8v).  The eigendecomposition of S / (n - 1) is the caller's (l3embedding_amd/pca.py: numpy.linalg.eigh in float64).
//
// The contract is the arithmetic, rounding by rounding, and this file is compiled with -ffp-contract=off (_build.py):
//   mean      column sums in float64: the rows in segments of L3_PCA_MEAN_SEG, a segment summed sequentially from 0.0 in ascending row
//             order, the segment sums added sequentially in ascending order, the total divided by (double)n.  m32 = (float)m64.
//   scatter   xc = fl32(x - m32), one float32 subtraction as a row is staged.  The rows are cut into chains of L3_PCA_CHAIN consecutive
//             rows; within a chain an entry is one v_mfma_f32_32x32x2_f32 accumulator taking the rows in ascending order from 0, which is
//             the ascending fmaf chain; a chain's result is widened and added to a float64 sum in ascending chain order, per split of
//             consecutive chains, from 0.0; the splits' float64 partials are added in ascending split order by a second kernel, which
//             computes the entries i <= j only and writes each to (i, j) and (j, i).  No float atomics.
//   project   y[i][c] = the ascending fmaf chain over d of fl32(x[i][d] - mean[d]) w[c][d] (the tile of knn_tile.h, with the centring in
//             its fetch), times scale[c] once when there is a scale.  The inverse is the same kernel on the transposed components:
//             fl32(chain over c of fl32(y[i][c] / scale[c]) w[c][d]) + mean[d].
//
// The scatter tile.  A workgroup of 4 waves owns one 128 x 128 tile (a-features x b-features, a-tile <= b-tile) of one split.  A chunk
// of 16 rows is staged as [row][256 features] (the a panel, then the b panel), so the lanes (r, h) of k-step s read rows 2 s + h at 32
// consecutive features: every ds_read_b32 is conflict-free and the global loads run along the row.  Wave w holds the a-features 32 w ..
// 32 w + 31 against the four 32-wide groups of b: 64 float32 accumulator registers and, beside them, the 64 float64 sums of the same
// entries (128 registers).  The stage is double buffered: one barrier per chunk.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/l3hip.h"
#include "device_common.h"
#include "featprep.h"
#include "host_common.h"
#include "knn_tile.h"
#include "pca.h"

namespace l3 {
namespace {

using namespace knn_tile;          // BLOCK, TQ, TC, LDK, the pre-operations of a fetch and the tile's dot products

constexpr int R = L3_PCA_CHAIN;                 // rows of a float32 chain
constexpr int SEG = L3_PCA_MEAN_SEG;            // rows of a segment of the mean's sums
constexpr int TD = 128;                         // features of a side of the scatter tile
constexpr int KR = 16;                          // rows of a staged chunk
constexpr int NPRE = KR / 4;                    // float4 a lane stages per chunk
constexpr int LDS_LD = 2 * TD;                  // floats of a staged row: the a panel, then the b panel
constexpr int CHUNKS = R / KR;                  // chunks of a chain
constexpr int FB = 32;                          // side of a block of the finishing kernel
constexpr int64_t MAX_ROWS = INT32_MAX;
constexpr unsigned long long NO_ROW = ULLONG_MAX;
static_assert(R % KR == 0 && (R & (R - 1)) == 0, "a chain is a power of two and a whole number of chunks");
static_assert(KR * LDS_LD == NPRE * 4 * BLOCK, "a chunk is NPRE float4 a lane");

// ---- the rows ----------------------------------------------------------------------------------------------------------------------
// *bad = the lowest row that holds a NaN or an infinity (integer atomicMin; NO_ROW before)
__global__ __launch_bounds__(BLOCK) void pca_finite_kernel(const float* __restrict__ x, int64_t n, int D, unsigned long long* __restrict__ bad) {
    const int64_t total = n * D;
    unsigned long long first = NO_ROW;
    for (int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x; e < total; e += (int64_t)gridDim.x * BLOCK)
        if (!isfinite(x[e])) {
            first = (unsigned long long)(e / D);
            break;          // (a lane's elements ascend)
        }
    if (first != NO_ROW) atomicMin(bad, first);
}

// seg[g][d] = the sequential float64 sum of column d over the rows of segment g, in ascending order from 0.0
__global__ __launch_bounds__(BLOCK) void pca_segsum_kernel(const float* __restrict__ x, int64_t n, int D, double* __restrict__ seg) {
    const int d = blockIdx.x * BLOCK + threadIdx.x;
    if (d >= D) return;
    const int64_t lo = (int64_t)blockIdx.y * SEG, hi = lo + SEG < n ? lo + SEG : n;
    double acc = 0.0;
    for (int64_t i = lo; i < hi; ++i) acc += (double)x[i * D + d];
    seg[(int64_t)blockIdx.y * D + d] = acc;
}

__global__ __launch_bounds__(BLOCK) void pca_mean_kernel(const double* __restrict__ seg, int64_t segs, int D, int64_t n, double* __restrict__ m64,
                                                         float* __restrict__ m32) {
    const int d = blockIdx.x * BLOCK + threadIdx.x;
    if (d >= D) return;
    double acc = 0.0;
    for (int64_t g = 0; g < segs; ++g) acc += seg[g * D + d];
    const double m = acc / (double)n;
    m64[d] = m;
    m32[d] = (float)m;
}

// ---- the scatter tile ----------------------------------------------------------------------------------------------------------------
// Lane tid stages the float4 of features 4 (tid & 31) .. + 3 of panel (tid >> 5) & 1 in the rows (tid >> 6) + 4 i of a chunk of KR rows,
// i < NPRE: its features, and so its four means, are the same in every chunk.
struct ScatterLane {
    int f;               // the first of its four features
    float4 m;            // their means (0 past D)
    bool vec, any;       // the four features are inside a row together and 16-byte aligned; at least one is inside
};

__device__ __forceinline__ void scatter_fetch(float4 (&pre)[NPRE], const float* __restrict__ X, int D, const ScatterLane& ln, int64_t row0,
                                              int64_t row_end, int tid) {
#pragma unroll
    for (int i = 0; i < NPRE; ++i) {
        const int64_t g = row0 + (tid >> 6) + 4 * i;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (g < row_end && ln.any) {
            const float* p = X + g * D + ln.f;
            if (ln.vec) {
                v = *reinterpret_cast<const float4*>(p);
                v.x = __fsub_rn(v.x, ln.m.x), v.y = __fsub_rn(v.y, ln.m.y), v.z = __fsub_rn(v.z, ln.m.z), v.w = __fsub_rn(v.w, ln.m.w);
            } else {
                v.x = __fsub_rn(p[0], ln.m.x);
                if (ln.f + 1 < D) v.y = __fsub_rn(p[1], ln.m.y);
                if (ln.f + 2 < D) v.z = __fsub_rn(p[2], ln.m.z);
                if (ln.f + 3 < D) v.w = __fsub_rn(p[3], ln.m.w);
            }
        }
        pre[i] = v;
    }
}

// Workgroup (u, y): the u-th tile on or above the diagonal, rows of split y -> part[y][a][b] for the tile's entries inside D x D.
// Two workgroups a compute unit (241 registers a lane, 32 KiB of LDS): with one, even with chunks of 32 rows and two chunks' loads in
// flight, a SIMD's only wave leaves the matrix core idle at every barrier and the kernel runs at 0.6 of this one's rate
// (profiles/r38_pca.txt).
__global__ __launch_bounds__(BLOCK, 2) void pca_scatter_kernel(const float* __restrict__ X, const float* __restrict__ m32, int D, int64_t n, int T,
                                                               int splits, int64_t chains, double* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float stage[2 * KR * LDS_LD];
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5, w = tid >> 6;
    int ti = 0, u = blockIdx.x;
    while (u >= T - ti) u -= T - ti, ++ti;
    const int a0 = ti * TD, b0 = (ti + u) * TD;
    const int64_t c_lo = (int64_t)blockIdx.y * chains / splits, c_hi = ((int64_t)blockIdx.y + 1) * chains / splits;
    const int64_t row_end = c_hi * R < n ? c_hi * R : n;
    const int64_t q_lo = c_lo * CHUNKS, q_hi = (row_end + KR - 1) / KR;          // (at least one chunk: a split holds a chain)

    ScatterLane ln;
    ln.f = (((tid >> 5) & 1) ? b0 : a0) + 4 * (tid & 31);
    ln.any = ln.f < D;
    ln.vec = (D & 3) == 0;
    ln.m = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (ln.any) {
        ln.m.x = m32[ln.f];
        if (ln.f + 1 < D) ln.m.y = m32[ln.f + 1];
        if (ln.f + 2 < D) ln.m.z = m32[ln.f + 2];
        if (ln.f + 3 < D) ln.m.w = m32[ln.f + 3];
    }

    f32x16 acc[4] = {};
    double sum[4][16];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) sum[t][i] = 0.0;

    float4 pre[NPRE];
    scatter_fetch(pre, X, D, ln, q_lo * KR, row_end, tid);
    for (int64_t q = q_lo; q < q_hi; ++q) {
        float* st = stage + (q & 1) * (KR * LDS_LD);
        // (this buffer was last read two chunks ago, and every wave has passed the barrier of the chunk between)
#pragma unroll
        for (int i = 0; i < NPRE; ++i) *reinterpret_cast<float4*>(st + ((tid >> 6) + 4 * i) * LDS_LD + 4 * (tid & 63)) = pre[i];
        __syncthreads();
        if (q + 1 < q_hi) scatter_fetch(pre, X, D, ln, (q + 1) * KR, row_end, tid);
        const float* arow = st + h * LDS_LD + 32 * w + r;
        const float* brow = st + h * LDS_LD + TD + r;
#pragma unroll
        for (int s = 0; s < KR / 2; ++s) {          // k-step s: rows 2 s (lanes h = 0) and 2 s + 1 (h = 1) of the chunk, in that order
            const float a = arow[2 * s * LDS_LD];
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, brow[2 * s * LDS_LD + 32 * t], acc[t], 0, 0, 0);
        }
        if (((q + 1) & (CHUNKS - 1)) == 0 || q + 1 == q_hi) {          // the chain ends: into the float64 sums, and from 0 again
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    sum[t][i] += (double)acc[t][i];
                    acc[t][i] = 0.0f;
                }
        }
    }
    double* out = part + (int64_t)blockIdx.y * D * D;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int b = b0 + 32 * t + r;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int a = a0 + 32 * w + mfma_row(i, h);
            if (a < D && b < D) out[(int64_t)a * D + b] = sum[t][i];
        }
    }
}

// S[i][j] = S[j][i] = the splits' partials of entry (i, j), i <= j, added in ascending split order.  Workgroup (bj, bi), bi <= bj, owns
// the 32 x 32 block (bi, bj) and its mirror image, which it writes from LDS so that both writes run along a row.
__global__ __launch_bounds__(BLOCK) void pca_scatter_finish_kernel(const double* __restrict__ part, int splits, int D, double* __restrict__ S) {
    __shared__ double tile[FB][FB + 1];
    const int bi = blockIdx.y, bj = blockIdx.x;
    if (bi > bj) return;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int64_t DD = (int64_t)D * D;
    for (int rr = ty; rr < FB; rr += BLOCK / FB) {
        const int i = FB * bi + rr, j = FB * bj + tx;
        double v = 0.0;
        if (i < D && j < D && i <= j) {
            v = part[(int64_t)i * D + j];
            for (int s = 1; s < splits; ++s) v += part[s * DD + (int64_t)i * D + j];
        }
        tile[rr][tx] = v;
    }
    __syncthreads();
    for (int rr = ty; rr < FB; rr += BLOCK / FB) {
        const int i = FB * bi + rr, j = FB * bj + tx;
        if (i < D && j < D) S[(int64_t)i * D + j] = (bi == bj && rr > tx) ? tile[tx][rr] : tile[rr][tx];
        const int i2 = FB * bj + rr, j2 = FB * bi + tx;
        if (bi != bj && i2 < D && j2 < D) S[(int64_t)i2 * D + j2] = tile[tx][rr];
    }
}

// ---- projection ------------------------------------------------------------------------------------------------------------------------
// out[i][c] = post(chain over d of pre(x[i][d]) w[c][d]) for the rows i of X (n, D) and the rows c of Wd (K, D).  PRE: knn_tile.h's
// pre-operation of the fetch with qp (D).  POST 0 nothing, 1 times post[c], 2 plus post[c].  Lane (r, h) of wave w holds the rows
// i0 + 32 w + mfma_row(., h) at the columns j0 + 32 t + r, so a store runs along a row of out.
template <int PRE, int POST>
__global__ __launch_bounds__(BLOCK) void pca_project_kernel(const float* __restrict__ X, const float* __restrict__ qp, const float* __restrict__ Wd,
                                                            const float* __restrict__ post, int D, int64_t n, int K, float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float stage[(TQ + TC) * LDK];
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5, w = tid >> 6;
    const int64_t i0 = (int64_t)blockIdx.x * TQ, j0 = (int64_t)blockIdx.y * TC;
    f32x16 acc[4] = {};
    accumulate_tile<PRE>(acc, stage, X, Wd, D, i0, n, j0, K, tid, qp);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int64_t c = j0 + 32 * t + r;
        if (c >= K) continue;
        const float p = POST ? post[c] : 0.0f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int64_t row = i0 + 32 * w + mfma_row(i, h);
            if (row >= n) continue;
            const float v = acc[t][i];
            out[row * K + c] = POST == 1 ? __fmul_rn(v, p) : POST == 2 ? __fadd_rn(v, p) : v;
        }
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
bool finished(hipStream_t s) { return hipStreamSynchronize(s) == hipSuccess && hipGetLastError() == hipSuccess; }

unsigned blocks_of(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

int64_t chains_of(int64_t n) { return (n + R - 1) / R; }

// the function of l3hip.h: the splits of a scatter over n rows of D features when the caller leaves the count to the library
int default_splits(int64_t n, int D) {
    const int64_t T = (D + TD - 1) / TD, tiles = T * (T + 1) / 2;
    const int64_t want = L3_PCA_FILL / tiles;          // (rounded down: one round of workgroups, not one and a few more)
    return (int)std::max<int64_t>(1, std::min<int64_t>({want, chains_of(n), (int64_t)L3_PCA_MAX_SPLITS}));
}

template <class T>
int grow(l3_pca* h, T** buf, size_t* cap, size_t count, const char* fn) {
    if (*buf && count <= *cap) return L3_OK;
    // whatever read the old buffer has finished: every call on the handle waits for its stream before it returns
    h->bufs.grow(buf, cap, count);
    if (*buf) return L3_OK;
    return fail(L3_ENOMEM, std::string(fn) + ": device allocation of " + std::to_string(DeviceBufs::bytes_of<T>(count)) + " bytes failed");
}

int enter(l3_pca* h, const char* fn) {
    if (!h) return fail(L3_EINVAL, std::string(fn) + ": NULL handle");
    if (hipSetDevice(h->device) != hipSuccess) return fail(L3_EHIP, no_gpu_message(fn, h->device));
    return L3_OK;
}

int need_rows(const l3_pca* h, const char* fn) {
    if (h->n < 2) return fail(L3_ESTATE, std::string(fn) + ": the rows come first (l3_pca_set_rows)");
    return L3_OK;
}

int need_model(const l3_pca* h, const char* fn) {
    if (h->k < 1) return fail(L3_ESTATE, std::string(fn) + ": the model comes first (l3_pca_set_model)");
    return L3_OK;
}

int check_count(int64_t n, int64_t least, const char* fn) {
    if (n < least || n > MAX_ROWS) return fail(L3_EINVAL, std::string(fn) + ": need " + std::to_string(least) + " <= n <= 2^31 - 1 rows, not " + std::to_string(n));
    return L3_OK;
}

int check_feat(const l3_pca* h, const l3_feat* f, int64_t lo, int64_t hi, int64_t width, int64_t least, const char* fn) {
    if (!f) return fail(L3_EINVAL, std::string(fn) + ": the feature matrix is NULL");
    if (f->device != h->device)
        return fail(L3_EINVAL, std::string(fn) + ": the features are on device " + std::to_string(f->device) + ", the handle on device " + std::to_string(h->device));
    if (f->D != width) return fail(L3_EINVAL, std::string(fn) + ": the features have " + std::to_string(f->D) + " columns, not " + std::to_string(width));
    if (lo < 0 || hi > f->n || lo >= hi)
        return fail(L3_EINVAL, std::string(fn) + ": rows [" + std::to_string(lo) + ", " + std::to_string(hi) + ") are empty or outside the " +
                                   std::to_string(f->n) + " rows of the features");
    return check_count(hi - lo, least, fn);
}

// the fitted rows: x_host or x_dev (n, D) -> the handle's copy, refused if a row is not finite; voids the mean
int set_rows(l3_pca* h, const float* x_host, const float* x_dev, int64_t n, const char* fn) {
    h->n = 0, h->has_mean = false, h->has_S = false;
    if (int rc = grow(h, &h->X, &h->cap_X, (size_t)n * h->D, fn)) return rc;
    const hipMemcpyKind kind = x_host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
    unsigned long long bad = NO_ROW;
    if (hipMemcpyAsync(h->X, x_host ? x_host : x_dev, (size_t)n * h->D * sizeof(float), kind, h->s) != hipSuccess ||
        hipMemsetAsync(h->bad, 0xFF, sizeof(bad), h->s) != hipSuccess)
        return fail(L3_EHIP, std::string(fn) + ": copy to the handle's rows failed");
    const unsigned grid = std::min<unsigned>(blocks_of(n * h->D, BLOCK), 4096u);
    hipLaunchKernelGGL(pca_finite_kernel, dim3(grid), dim3(BLOCK), 0, h->s, h->X, n, h->D, h->bad);
    if (hipMemcpyAsync(&bad, h->bad, sizeof(bad), hipMemcpyDeviceToHost, h->s) != hipSuccess || !finished(h->s))
        return fail(L3_EHIP, std::string(fn) + ": the check of the rows failed on the device");
    if (bad != NO_ROW)
        return fail(L3_EINVAL, std::string(fn) + ": row " + std::to_string(bad) + " holds a NaN or an infinity (a mean of such rows is not a model)");
    h->n = n;
    return L3_OK;
}

void launch_mean(l3_pca* h) {
    const int64_t segs = (h->n + SEG - 1) / SEG;
    hipLaunchKernelGGL(pca_segsum_kernel, dim3(blocks_of(h->D, BLOCK), (unsigned)segs), dim3(BLOCK), 0, h->s, h->X, h->n, h->D, h->seg);
    hipLaunchKernelGGL(pca_mean_kernel, dim3(blocks_of(h->D, BLOCK)), dim3(BLOCK), 0, h->s, h->seg, segs, h->D, h->n, h->m64, h->m32);
}

int prepare_scatter(l3_pca* h, int splits, const char* fn) {
    const size_t DD = (size_t)h->D * h->D;
    if (int rc = grow(h, &h->part, &h->cap_part, DD * splits, fn)) return rc;
    return grow(h, &h->S, &h->cap_S, DD, fn);
}

void launch_tiles(l3_pca* h, int splits) {
    const int T = (h->D + TD - 1) / TD;
    hipLaunchKernelGGL(pca_scatter_kernel, dim3((unsigned)(T * (T + 1) / 2), (unsigned)splits), dim3(BLOCK), 0, h->s, h->X, h->m32, h->D, h->n, T, splits,
                       chains_of(h->n), h->part);
}

void launch_scatter(l3_pca* h, int splits) {
    const int F = (h->D + FB - 1) / FB;
    launch_tiles(h, splits);
    hipLaunchKernelGGL(pca_scatter_finish_kernel, dim3((unsigned)F, (unsigned)F), dim3(BLOCK), 0, h->s, h->part, splits, h->D, h->S);
}

// y (n, k) = the projection of x (n, D), both on the device
void launch_transform(l3_pca* h, const float* x, int64_t n, float* y) {
    const dim3 grid(blocks_of(n, TQ), blocks_of(h->k, TC));
    if (h->has_scale)
        hipLaunchKernelGGL((pca_project_kernel<PRE_SUB, 1>), grid, dim3(BLOCK), 0, h->s, x, h->mean, h->W, h->scale, h->D, n, h->k, y);
    else
        hipLaunchKernelGGL((pca_project_kernel<PRE_SUB, 0>), grid, dim3(BLOCK), 0, h->s, x, h->mean, h->W, (const float*)nullptr, h->D, n, h->k, y);
}

// x (n, D) = the rows that project to y (n, k), both on the device
void launch_inverse(l3_pca* h, const float* y, int64_t n, float* x) {
    const dim3 grid(blocks_of(n, TQ), blocks_of(h->D, TC));
    if (h->has_scale)
        hipLaunchKernelGGL((pca_project_kernel<PRE_DIV, 2>), grid, dim3(BLOCK), 0, h->s, y, h->scale, h->WT, h->mean, h->k, n, h->D, x);
    else
        hipLaunchKernelGGL((pca_project_kernel<PRE_NONE, 2>), grid, dim3(BLOCK), 0, h->s, y, (const float*)nullptr, h->WT, h->mean, h->k, n, h->D, x);
}

// One projection, forward or back: the input is in_host (copied to the handle) or in_dev; the result goes to out_host, or into a new
// l3_feat (*out_feat), or both.
int project(l3_pca* h, bool forward, const float* in_host, const float* in_dev, int64_t n, float* out_host, l3_feat** out_feat, const char* fn) {
    const int win = forward ? h->D : h->k, wout = forward ? h->k : h->D;
    if (out_feat) *out_feat = nullptr;
    if (!out_host && !out_feat) return fail(L3_EINVAL, std::string(fn) + ": no output is asked for");
    const float* x = in_dev;
    if (in_host) {
        if (int rc = grow(h, &h->P, &h->cap_P, (size_t)n * win, fn)) return rc;
        if (hipMemcpyAsync(h->P, in_host, (size_t)n * win * sizeof(float), hipMemcpyHostToDevice, h->s) != hipSuccess)
            return fail(L3_EHIP, std::string(fn) + ": copy to the device failed");
        x = h->P;
    }
    l3_feat* f = nullptr;
    float* y = nullptr;
    if (out_feat) {
        if (int rc = l3_feat_alloc(h->device, n, wout, &f)) return rc;          // (zero-filled on its own stream, and finished)
        y = f->x;
    } else {
        if (int rc = grow(h, &h->Y, &h->cap_Y, (size_t)n * wout, fn)) return rc;
        y = h->Y;
    }
    if (forward) launch_transform(h, x, n, y);
    else launch_inverse(h, x, n, y);
    bool ok = true;
    if (out_host) ok = hipMemcpyAsync(out_host, y, (size_t)n * wout * sizeof(float), hipMemcpyDeviceToHost, h->s) == hipSuccess;
    if (!ok || !finished(h->s)) {
        l3_feat_destroy(f);
        return fail(L3_EHIP, std::string(fn) + ": the kernel or the copy from the device failed");
    }
    if (out_feat) *out_feat = f;
    return L3_OK;
}

}  // namespace
}  // namespace l3

using namespace l3;

extern "C" {

int l3_pca_create(int device, int D, l3_pca** out) {
    const char* fn = "l3_pca_create";
    if (!out) return fail(L3_EINVAL, std::string(fn) + ": out is NULL");
    *out = nullptr;
    if (D < 1 || D > L3_PCA_MAX_D) return fail(L3_EINVAL, std::string(fn) + ": need 1 <= D <= " + std::to_string(L3_PCA_MAX_D) + " features, not " + std::to_string(D));
    if (!device_ok(device)) return fail(L3_EHIP, no_gpu_message(fn, device));
    l3_pca* h = new l3_pca();
    h->device = device, h->D = D;
    if (hipStreamCreateWithFlags(&h->s, hipStreamNonBlocking) != hipSuccess) {
        h->s = nullptr;
        l3_pca_destroy(h);
        return fail(L3_EHIP, std::string(fn) + ": hipStreamCreate failed");
    }
    h->m64 = h->bufs.alloc<double>((size_t)D);
    h->m32 = h->bufs.alloc<float>((size_t)D);
    h->mean = h->bufs.alloc<float>((size_t)D);
    h->bad = h->bufs.alloc<unsigned long long>(1);
    if (!h->bufs.ok()) {
        l3_pca_destroy(h);
        return fail(L3_ENOMEM, std::string(fn) + ": device allocation of the means failed");
    }
    *out = h;
    return L3_OK;
}

void l3_pca_destroy(l3_pca* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->s) (void)hipStreamSynchronize(h->s);
    if (h->s) (void)hipStreamDestroy(h->s);
    delete h;
}

int l3_pca_splits(int64_t n, int D, int* splits) {
    const char* fn = "l3_pca_splits";
    if (!splits) return fail(L3_EINVAL, std::string(fn) + ": splits is NULL");
    if (D < 1 || D > L3_PCA_MAX_D) return fail(L3_EINVAL, std::string(fn) + ": need 1 <= D <= " + std::to_string(L3_PCA_MAX_D));
    if (int rc = check_count(n, 2, fn)) return rc;
    *splits = default_splits(n, D);
    return L3_OK;
}

int l3_pca_set_rows(l3_pca* h, const float* rows, int64_t n) {
    const char* fn = "l3_pca_set_rows";
    if (int rc = enter(h, fn)) return rc;
    if (!rows) return fail(L3_EINVAL, std::string(fn) + ": rows is NULL");
    if (int rc = check_count(n, 2, fn)) return rc;
    return set_rows(h, rows, nullptr, n, fn);
}

int l3_pca_set_rows_dev(l3_pca* h, const l3_feat* f, int64_t lo, int64_t hi) {
    const char* fn = "l3_pca_set_rows_dev";
    if (int rc = enter(h, fn)) return rc;
    if (int rc = check_feat(h, f, lo, hi, h->D, 2, fn)) return rc;
    // (every l3_feat call has finished on its handle's stream when it returns: the rows hold their final values)
    return set_rows(h, nullptr, f->x + lo * f->D, hi - lo, fn);
}

int l3_pca_mean(l3_pca* h, double* mean_out, float* mean32_out) {
    const char* fn = "l3_pca_mean";
    if (int rc = enter(h, fn)) return rc;
    if (int rc = need_rows(h, fn)) return rc;
    h->has_mean = false, h->has_S = false;
    if (int rc = grow(h, &h->seg, &h->cap_seg, (size_t)((h->n + SEG - 1) / SEG) * h->D, fn)) return rc;
    launch_mean(h);
    bool ok = true;
    if (mean_out) ok = ok && hipMemcpyAsync(mean_out, h->m64, (size_t)h->D * sizeof(double), hipMemcpyDeviceToHost, h->s) == hipSuccess;
    if (mean32_out) ok = ok && hipMemcpyAsync(mean32_out, h->m32, (size_t)h->D * sizeof(float), hipMemcpyDeviceToHost, h->s) == hipSuccess;
    if (!ok || !finished(h->s)) return fail(L3_EHIP, std::string(fn) + ": the kernels or the copy from the device failed");
    h->has_mean = true;
    return L3_OK;
}

int l3_pca_set_mean(l3_pca* h, const float* mean32) {
    const char* fn = "l3_pca_set_mean";
    if (int rc = enter(h, fn)) return rc;
    if (!mean32) return fail(L3_EINVAL, std::string(fn) + ": mean32 is NULL");
    h->has_mean = false, h->has_S = false;
    std::vector<double> wide((size_t)h->D);
    for (int d = 0; d < h->D; ++d) {
        if (!std::isfinite(mean32[d])) return fail(L3_EINVAL, std::string(fn) + ": the mean of column " + std::to_string(d) + " is not finite");
        wide[d] = (double)mean32[d];
    }
    if (hipMemcpyAsync(h->m32, mean32, (size_t)h->D * sizeof(float), hipMemcpyHostToDevice, h->s) != hipSuccess ||
        hipMemcpyAsync(h->m64, wide.data(), (size_t)h->D * sizeof(double), hipMemcpyHostToDevice, h->s) != hipSuccess || !finished(h->s))
        return fail(L3_EHIP, std::string(fn) + ": copy to the device failed");
    h->has_mean = true;
    return L3_OK;
}

int l3_pca_scatter(l3_pca* h, int splits, double* S_out) {
    const char* fn = "l3_pca_scatter";
    if (int rc = enter(h, fn)) return rc;
    if (splits < 0 || splits > L3_PCA_MAX_SPLITS)
        return fail(L3_EINVAL, std::string(fn) + ": splits must be in [0, " + std::to_string(L3_PCA_MAX_SPLITS) + "], not " + std::to_string(splits));
    if (int rc = need_rows(h, fn)) return rc;
    if (!h->has_mean) return fail(L3_ESTATE, std::string(fn) + ": the mean comes first (l3_pca_mean or l3_pca_set_mean)");
    const int count = splits == 0 ? default_splits(h->n, h->D) : (int)std::min<int64_t>(splits, chains_of(h->n));
    h->has_S = false;
    if (int rc = prepare_scatter(h, count, fn)) return rc;
    launch_scatter(h, count);
    // (S_out may be NULL: S then stays on the device, where l3_eig_set_matrix_pca takes it from)
    if ((S_out && hipMemcpyAsync(S_out, h->S, (size_t)h->D * h->D * sizeof(double), hipMemcpyDeviceToHost, h->s) != hipSuccess) || !finished(h->s))
        return fail(L3_EHIP, std::string(fn) + ": the kernels or the copy from the device failed");
    h->has_S = true;          // (for l3_eig_set_matrix_pca: pca.h)
    return L3_OK;
}

int l3_pca_set_model(l3_pca* h, int k, const float* mean32, const float* components, const float* scale) {
    const char* fn = "l3_pca_set_model";
    if (int rc = enter(h, fn)) return rc;
    if (!mean32 || !components) return fail(L3_EINVAL, std::string(fn) + ": mean32 and components must not be NULL");
    if (k < 1 || k > h->D) return fail(L3_EINVAL, std::string(fn) + ": need 1 <= k <= D = " + std::to_string(h->D) + " components, not " + std::to_string(k));
    if (scale)
        for (int c = 0; c < k; ++c)
            if (!(std::isfinite(scale[c]) && scale[c] > 0.0f))
                return fail(L3_EINVAL, std::string(fn) + ": the scale of component " + std::to_string(c) + " is not a positive finite number");
    h->k = 0;
    const size_t kD = (size_t)k * h->D;
    if (int rc = grow(h, &h->W, &h->cap_W, kD, fn)) return rc;
    if (int rc = grow(h, &h->WT, &h->cap_WT, kD, fn)) return rc;
    if (int rc = grow(h, &h->scale, &h->cap_scale, (size_t)k, fn)) return rc;
    std::vector<float> wt(kD);          // the transpose, once: the inverse reduces over the components
    for (int c = 0; c < k; ++c)
        for (int d = 0; d < h->D; ++d) wt[(size_t)d * k + c] = components[(size_t)c * h->D + d];
    bool ok = hipMemcpyAsync(h->W, components, kD * sizeof(float), hipMemcpyHostToDevice, h->s) == hipSuccess &&
              hipMemcpyAsync(h->WT, wt.data(), kD * sizeof(float), hipMemcpyHostToDevice, h->s) == hipSuccess &&
              hipMemcpyAsync(h->mean, mean32, (size_t)h->D * sizeof(float), hipMemcpyHostToDevice, h->s) == hipSuccess;
    if (scale) ok = ok && hipMemcpyAsync(h->scale, scale, (size_t)k * sizeof(float), hipMemcpyHostToDevice, h->s) == hipSuccess;
    if (!ok || !finished(h->s)) return fail(L3_EHIP, std::string(fn) + ": copy to the device failed");
    h->k = k, h->has_scale = scale != nullptr;
    return L3_OK;
}

int l3_pca_transform(l3_pca* h, const float* rows, int64_t n, float* out) {
    const char* fn = "l3_pca_transform";
    if (int rc = enter(h, fn)) return rc;
    if (!rows || !out) return fail(L3_EINVAL, std::string(fn) + ": rows and out must not be NULL");
    if (int rc = need_model(h, fn)) return rc;
    if (int rc = check_count(n, 1, fn)) return rc;
    return project(h, true, rows, nullptr, n, out, nullptr, fn);
}

int l3_pca_transform_dev(l3_pca* h, const l3_feat* f, int64_t lo, int64_t hi, float* out, l3_feat** out_feat) {
    const char* fn = "l3_pca_transform_dev";
    if (int rc = enter(h, fn)) return rc;
    if (int rc = need_model(h, fn)) return rc;
    if (int rc = check_feat(h, f, lo, hi, h->D, 1, fn)) return rc;
    return project(h, true, nullptr, f->x + lo * f->D, hi - lo, out, out_feat, fn);
}

int l3_pca_inverse(l3_pca* h, const float* Y, int64_t n, float* out) {
    const char* fn = "l3_pca_inverse";
    if (int rc = enter(h, fn)) return rc;
    if (!Y || !out) return fail(L3_EINVAL, std::string(fn) + ": Y and out must not be NULL");
    if (int rc = need_model(h, fn)) return rc;
    if (int rc = check_count(n, 1, fn)) return rc;
    return project(h, false, Y, nullptr, n, out, nullptr, fn);
}

int l3_pca_inverse_dev(l3_pca* h, const l3_feat* f, int64_t lo, int64_t hi, float* out, l3_feat** out_feat) {
    const char* fn = "l3_pca_inverse_dev";
    if (int rc = enter(h, fn)) return rc;
    if (int rc = need_model(h, fn)) return rc;
    if (int rc = check_feat(h, f, lo, hi, h->k, 1, fn)) return rc;
    return project(h, false, nullptr, f->x + lo * f->D, hi - lo, out, out_feat, fn);
}

// Device time of `reps` rounds on the resident rows, in ms per round (hipEvents; one untimed round first).  what 0: the mean's two
// kernels; 1: the scatter's two kernels at the library's split count; 2: the projection of the fitted rows onto the model's components;
// 3: the scatter's tile kernel alone.  For profiles/ records; no test asserts a time.
int l3_pca_time(l3_pca* h, int what, int reps, double* ms) {
    const char* fn = "l3_pca_time";
    if (int rc = enter(h, fn)) return rc;
    if (!ms || reps < 1 || what < 0 || what > 3) return fail(L3_EINVAL, std::string(fn) + ": need ms, reps >= 1 and what in [0, 3]");
    if (int rc = need_rows(h, fn)) return rc;
    const int splits = default_splits(h->n, h->D);
    if (what == 0) {
        h->has_mean = false, h->has_S = false;
        if (int rc = grow(h, &h->seg, &h->cap_seg, (size_t)((h->n + SEG - 1) / SEG) * h->D, fn)) return rc;
    } else if (what == 2) {
        if (int rc = need_model(h, fn)) return rc;
        if (int rc = grow(h, &h->Y, &h->cap_Y, (size_t)h->n * h->k, fn)) return rc;
    } else {
        if (!h->has_mean) return fail(L3_ESTATE, std::string(fn) + ": the mean comes first (l3_pca_mean or l3_pca_set_mean)");
        if (int rc = prepare_scatter(h, splits, fn)) return rc;
    }
    hipEvent_t a, b;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return fail(L3_EHIP, std::string(fn) + ": hipEventCreate failed");
    auto run = [&](int count) {
        for (int r = 0; r < count; ++r) {
            if (what == 0) launch_mean(h);
            else if (what == 1) launch_scatter(h, splits);
            else if (what == 2) launch_transform(h, h->X, h->n, h->Y);
            else launch_tiles(h, splits);
        }
    };
    run(1);
    float t = 0.0f;
    int rc = L3_OK;
    if (hipEventRecord(a, h->s) != hipSuccess) rc = fail(L3_EHIP, std::string(fn) + ": hipEventRecord failed");
    if (rc == L3_OK) run(reps);
    if (rc == L3_OK && (hipEventRecord(b, h->s) != hipSuccess || !finished(h->s) || hipEventElapsedTime(&t, a, b) != hipSuccess))
        rc = fail(L3_EHIP, std::string(fn) + ": the timed launches failed");
    if (rc != L3_OK) (void)hipStreamSynchronize(h->s);
    if (what == 0 && rc == L3_OK) h->has_mean = true;
    *ms = (double)t / reps;
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    return rc;
}

}  // extern "C"
