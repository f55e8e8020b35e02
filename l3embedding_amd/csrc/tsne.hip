// tsne.hip -- exact t-SNE of n points in the plane over a sparse symmetric P: the calibration of the conditional probabilities, the
// repulsive and attractive passes, the update and the loop that chains them.
//
// The arithmetic, which is the contract (include/l3hip.h, "t-SNE"; tests/tsne_ref.py has the float64 oracle and the derived bounds):
//     calibration   a lane per row, everything float64, the neighbours in ascending list position in every sum, exactly
//                   L3_TSNE_SEARCH_STEPS moves of the bracket and then one evaluation at the beta they left
//     repulsive     per pair dx = y_i - y_j, d2 = fmaf(dx, dx, dy dy), q = rcp(1 + d2) (the hardware's approximate reciprocal),
//                   R += fmaf(q q, dx, .), z += q; j ascending in runs of L3_TSNE_RUN, a run a float32 chain from 0, the run sums added
//                   into float64 in ascending order, per segment of runs; the segments' partials added in ascending order
//     attractive    float64 from the float32 coordinates; lane l of the row's wave takes the entries l, l + 64, ... in order; the
//                   lanes are folded by the xor butterfly 32, 16, ..., 1
//     sums over rows (Z, the KL part)   rows ascending in runs of L3_TSNE_RUN, a run summed sequentially from 0.0 in float64, the run
//                   sums added sequentially in ascending order
//     update        the counted float32 roundings of l3hip.h
// No float atomics: the only atomic is the integer count of rejected rows in the calibration.  The file is compiled with
// -ffp-contract=off (_build.py), so every fused multiply-add is one that is written as fmaf / fma here.
//
//   tsne_conditional_kernel   128 rows a workgroup, the distances staged through LDS as [neighbour][row] (a lane's column: no bank
//                             conflicts), a lane per row
//   tsne_repulsive_kernel<RPL>  workgroup (x, y): the rows [row_block x, row_block (x + 1)), RPL = row_block / 256 per lane with y_i in
//                             registers, against the runs of segment y.  A run's 256 points are staged in LDS and read at one address
//                             per wave (a broadcast), each read serving RPL pairs.  The run that holds a lane's own row skips that one
//                             term; every other run carries no test.
//   tsne_finish_kernel        a lane per row: the segments' partials added in ascending order -> R (n, 2), z (n)
//   tsne_runsum / total_kernel  the two levels of a sum over rows
//   tsne_attractive_kernel    a wave per row of P
//   tsne_update_kernel        a lane per coordinate
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/l3hip.h"
#include "host_common.h"
#include "tsne.h"

namespace l3 {
namespace {

constexpr int BLOCK = 256;
constexpr int RUN = L3_TSNE_RUN;
static_assert(RUN == BLOCK, "a run is staged by one workgroup, a point per lane");
constexpr int STEPS = L3_TSNE_SEARCH_STEPS;
constexpr int K_MAX = L3_KNN_TOPK_MAX;
constexpr int CAL_ROWS = 128;               // rows of a calibration workgroup: 64 x 128 floats of LDS
constexpr int SMALL_N = 8192;               // up to here a lane owns one row, beyond it four
constexpr int TARGET_BLOCKS = 1024;         // workgroups of the repulsive pass the segments aim at
constexpr int64_t MAX_POINTS = 1 << 24;
constexpr int SCAN_LDS = 2048;              // run totals a single workgroup stages at a time

// ---- calibration -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CAL_ROWS) void tsne_conditional_kernel(const float* __restrict__ dist, int64_t n, int k, double target,
                                                                    double* __restrict__ p_out, double* __restrict__ beta_out,
                                                                    unsigned long long* __restrict__ bad) {
    __shared__ float sd[K_MAX * CAL_ROWS];
    const int tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * CAL_ROWS;
    const int rows = (int)min((int64_t)CAL_ROWS, n - row0), total = rows * k;
    for (int e = tid; e < total; e += CAL_ROWS) {
        const int r = e / k, j = e - r * k;
        sd[j * CAL_ROWS + r] = dist[row0 * k + e];
    }
    __syncthreads();
    if (tid >= rows) return;
    const int64_t i = row0 + tid;
    const float* mine = sd + tid;
    float dmin = mine[0];
    bool ok = true;
    for (int j = 0; j < k; ++j) {
        const float v = mine[j * CAL_ROWS];
        ok = ok && isfinite(v);
        dmin = v < dmin ? v : dmin;
    }
    if (!ok) {          // a distance that is NaN or infinite: a NaN row, and the caller hears of it
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        for (int j = 0; j < k; ++j) p_out[i * k + j] = nan;
        beta_out[i] = nan;
        atomicAdd(bad, 1ull);
        return;
    }
    const double inf = __longlong_as_double(0x7ff0000000000000ll), m = (double)dmin;
    double beta = 1.0, lo = -inf, hi = inf, sum_p = 0.0;
    for (int step = 0; step <= STEPS; ++step) {
        sum_p = 0.0;
        double sum_dp = 0.0;
        for (int j = 0; j < k; ++j) {
            const double d = (double)mine[j * CAL_ROWS] - m;
            const double p = exp(-d * beta);
            sum_p += p;
            sum_dp += d * p;
        }
        if (step == STEPS) break;          // the evaluation at the beta the moves left
        const double H = log(sum_p) + beta * sum_dp / sum_p;
        if (H > target) {
            lo = beta;
            beta = hi == inf ? beta * 2.0 : (beta + hi) / 2.0;
        } else {
            hi = beta;
            beta = lo == -inf ? beta / 2.0 : (beta + lo) / 2.0;
        }
    }
    for (int j = 0; j < k; ++j) {
        const double d = (double)mine[j * CAL_ROWS] - m;
        p_out[i * k + j] = exp(-d * beta) / sum_p;
    }
    beta_out[i] = beta;
}

// ---- the repulsive pass --------------------------------------------------------------------------------------------------------------
// One run of `cnt` staged points against the lane's RPL rows.  OWN: this is the run that holds row `own` of the lane, at position
// `tid`: that pair adds nothing to z (0.0f added to a sum that is >= 0 leaves its bits) and its R term is q^2 * 0 = 0 by itself.
template <int RPL, bool OWN>
__device__ __forceinline__ void run_pairs(const float2* __restrict__ pts, int cnt, int tid, int own, const float (&yx)[RPL], const float (&yy)[RPL],
                                          float (&ax)[RPL], float (&ay)[RPL], float (&az)[RPL]) {
#pragma unroll 8
    for (int jj = 0; jj < cnt; ++jj) {
        const float2 p = pts[jj];          // one address for the whole wave
#pragma unroll
        for (int r = 0; r < RPL; ++r) {
            const float dx = yx[r] - p.x, dy = yy[r] - p.y;
            const float t = dy * dy;
            const float d2 = __fmaf_rn(dx, dx, t);
            const float w = 1.0f + d2;
            const float q = __builtin_amdgcn_rcpf(w);
            const float q2 = q * q;
            ax[r] = __fmaf_rn(q2, dx, ax[r]);
            ay[r] = __fmaf_rn(q2, dy, ay[r]);
            az[r] += (OWN && r == own && jj == tid) ? 0.0f : q;
        }
    }
}

// part: (segments, 3, n) float64: Rx, Ry, z of segment y for every row
template <int RPL>
__global__ __launch_bounds__(BLOCK) void tsne_repulsive_kernel(const float* __restrict__ Y, int64_t n, int rps, double* __restrict__ part) {
    __shared__ float2 pts[RUN];
    const int tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * (BLOCK * RPL), n_runs = (n + RUN - 1) / RUN;
    const int64_t run_lo = (int64_t)blockIdx.y * rps, run_hi = min(n_runs, run_lo + rps);
    const float2* Y2 = reinterpret_cast<const float2*>(Y);
    float yx[RPL], yy[RPL];
    double Rx[RPL], Ry[RPL], Zs[RPL];
#pragma unroll
    for (int r = 0; r < RPL; ++r) {
        const int64_t i = row0 + r * BLOCK + tid;
        const float2 v = i < n ? Y2[i] : make_float2(0.0f, 0.0f);
        yx[r] = v.x, yy[r] = v.y;
        Rx[r] = Ry[r] = Zs[r] = 0.0;
    }
    for (int64_t run = run_lo; run < run_hi; ++run) {
        const int64_t j0 = run * RUN;
        const int cnt = (int)min((int64_t)RUN, n - j0);
        __syncthreads();          // the run before has been read
        if (tid < cnt) pts[tid] = Y2[j0 + tid];
        __syncthreads();
        float ax[RPL], ay[RPL], az[RPL];
#pragma unroll
        for (int r = 0; r < RPL; ++r) ax[r] = ay[r] = az[r] = 0.0f;
        // row row0 + 256 r + tid lies in run RPL x + r, at position tid
        const int64_t own = run - (int64_t)blockIdx.x * RPL;
        if (own >= 0 && own < RPL) run_pairs<RPL, true>(pts, cnt, tid, (int)own, yx, yy, ax, ay, az);
        else if (cnt == RUN) run_pairs<RPL, false>(pts, RUN, tid, -1, yx, yy, ax, ay, az);
        else run_pairs<RPL, false>(pts, cnt, tid, -1, yx, yy, ax, ay, az);
#pragma unroll
        for (int r = 0; r < RPL; ++r) Rx[r] += (double)ax[r], Ry[r] += (double)ay[r], Zs[r] += (double)az[r];
    }
    double* p = part + (int64_t)blockIdx.y * 3 * n;
#pragma unroll
    for (int r = 0; r < RPL; ++r) {
        const int64_t i = row0 + r * BLOCK + tid;
        if (i < n) p[i] = Rx[r], p[n + i] = Ry[r], p[2 * n + i] = Zs[r];
    }
}

__global__ __launch_bounds__(BLOCK) void tsne_finish_kernel(const double* __restrict__ part, int64_t n, int segments, double* __restrict__ R,
                                                            double* __restrict__ z) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    double rx = 0.0, ry = 0.0, zz = 0.0;
    for (int s = 0; s < segments; ++s) {
        const double* p = part + (int64_t)s * 3 * n;
        rx += p[i], ry += p[n + i], zz += p[2 * n + i];
    }
    R[2 * i] = rx, R[2 * i + 1] = ry, z[i] = zz;
}

// ---- a sum over rows in the run order -------------------------------------------------------------------------------------------------
// a lane per run of 256 rows: the run's total
__global__ __launch_bounds__(BLOCK) void tsne_runsum_kernel(const double* __restrict__ v, int64_t n, double* __restrict__ runs) {
    const int64_t r = (int64_t)blockIdx.x * BLOCK + threadIdx.x, m0 = r * RUN;
    if (m0 >= n) return;
    const int64_t m1 = min(n, m0 + RUN);
    double acc = 0.0;
    for (int64_t q = m0; q < m1; ++q) acc += v[q];
    runs[r] = acc;
}

// One workgroup: the run totals added in order by one lane, staged through LDS by all
__global__ __launch_bounds__(BLOCK) void tsne_total_kernel(const double* __restrict__ runs, int64_t R, double* __restrict__ out) {
    __shared__ double buf[SCAN_LDS];
    double acc = 0.0;
    for (int64_t base = 0; base < R; base += SCAN_LDS) {
        const int cnt = (int)min((int64_t)SCAN_LDS, R - base);
        __syncthreads();
        for (int q = threadIdx.x; q < cnt; q += BLOCK) buf[q] = runs[base + q];
        __syncthreads();
        if (threadIdx.x == 0)
            for (int q = 0; q < cnt; ++q) acc += buf[q];
    }
    if (threadIdx.x == 0) *out = acc;
}

// ---- the attractive pass ----------------------------------------------------------------------------------------------------------------
// Wave w of workgroup x: row 4 x + w of P
__global__ __launch_bounds__(BLOCK) void tsne_attractive_kernel(const float* __restrict__ Y, int64_t n, const int64_t* __restrict__ indptr,
                                                                const int32_t* __restrict__ cols, const float* __restrict__ vals,
                                                                double* __restrict__ A, double* __restrict__ klrow) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
    if (i >= n) return;          // (the whole wave)
    const double yx = (double)Y[2 * i], yy = (double)Y[2 * i + 1];
    double ax = 0.0, ay = 0.0, kl = 0.0;
    const int64_t e1 = indptr[i + 1];
    for (int64_t e = indptr[i] + lane; e < e1; e += 64) {
        const int64_t j = cols[e];
        const double P = (double)vals[e];
        const double dx = yx - (double)Y[2 * j], dy = yy - (double)Y[2 * j + 1];
        const double d2 = fma(dx, dx, dy * dy);
        const double pq = P * (1.0 / (1.0 + d2));
        ax = fma(pq, dx, ax);
        ay = fma(pq, dy, ay);
        kl = fma(P, log1p(d2), kl);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        ax += __shfl_xor(ax, m);
        ay += __shfl_xor(ay, m);
        kl += __shfl_xor(kl, m);
    }
    if (lane == 0) A[2 * i] = ax, A[2 * i + 1] = ay, klrow[i] = kl;
}

// ---- the update ----------------------------------------------------------------------------------------------------------------------
// a lane per coordinate e of the 2 n
__global__ __launch_bounds__(BLOCK) void tsne_update_kernel(float* __restrict__ Y, float* __restrict__ U, float* __restrict__ G,
                                                            const double* __restrict__ A, const double* __restrict__ R,
                                                            const l3_tsne_scalars* __restrict__ sc, int64_t m, double exaggeration, float momentum,
                                                            float lr) {
    const int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (e >= m) return;
    const double Z = sc->Z;
    const float g = (float)(4.0 * (exaggeration * A[e] - R[e] / Z));
    const float u = U[e];
    float gain = G[e];
    const float ug = u * g;
    gain = ug < 0.0f ? gain + 0.2f : gain * 0.8f;
    gain = gain < 0.01f ? 0.01f : gain;
    const float a = momentum * u, s = lr * gain;
    const float b = s * g;
    const float un = a - b;
    U[e] = un, G[e] = gain, Y[e] = Y[e] + un;
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
bool finished(hipStream_t s) { return hipStreamSynchronize(s) == hipSuccess && hipGetLastError() == hipSuccess; }

unsigned blocks_of(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

// the function of l3hip.h: rows per workgroup, runs per segment and segments of the repulsive pass at n points
void geometry(int64_t n, int* row_block, int* rps, int* segments) {
    *row_block = n <= SMALL_N ? BLOCK : 4 * BLOCK;
    const int64_t row_blocks = (n + *row_block - 1) / *row_block, n_runs = (n + RUN - 1) / RUN;
    *rps = (int)std::max<int64_t>(1, (n_runs * row_blocks + TARGET_BLOCKS - 1) / TARGET_BLOCKS);
    *segments = (int)((n_runs + *rps - 1) / *rps);
}

int enter(l3_tsne* h, const char* fn) {
    if (!h) return fail(L3_EINVAL, std::string(fn) + ": NULL handle");
    if (hipSetDevice(h->device) != hipSuccess) return fail(L3_EHIP, no_gpu_message(fn, h->device));
    return L3_OK;
}

int need_embedding(const l3_tsne* h, const char* fn) {
    if (!h->has_embedding) return fail(L3_ESTATE, std::string(fn) + ": the embedding comes first (l3_tsne_set_embedding)");
    return L3_OK;
}

int need_affinities(const l3_tsne* h, const char* fn) {
    if (!h->has_affinities) return fail(L3_ESTATE, std::string(fn) + ": the affinities come first (l3_tsne_set_affinities)");
    return L3_OK;
}

void launch_sum(l3_tsne* h, const double* v, double* out) {
    const int64_t R = (h->n + RUN - 1) / RUN;
    hipLaunchKernelGGL(tsne_runsum_kernel, dim3(blocks_of(R, BLOCK)), dim3(BLOCK), 0, h->s, v, h->n, h->runs);
    hipLaunchKernelGGL(tsne_total_kernel, dim3(1), dim3(BLOCK), 0, h->s, h->runs, R, out);
}

// the segments' partials of the current embedding
void launch_pairs(l3_tsne* h) {
    const dim3 grid(blocks_of(h->n, h->row_block), (unsigned)h->segments);
    if (h->row_block == BLOCK) hipLaunchKernelGGL(tsne_repulsive_kernel<1>, grid, dim3(BLOCK), 0, h->s, h->Y, h->n, h->runs_per_segment, h->part);
    else hipLaunchKernelGGL(tsne_repulsive_kernel<4>, grid, dim3(BLOCK), 0, h->s, h->Y, h->n, h->runs_per_segment, h->part);
}

// R, z and Z of the current embedding
void launch_repulsive(l3_tsne* h) {
    launch_pairs(h);
    hipLaunchKernelGGL(tsne_finish_kernel, dim3(blocks_of(h->n, BLOCK)), dim3(BLOCK), 0, h->s, h->part, h->n, h->segments, h->R, h->z);
    launch_sum(h, h->z, &h->scal->Z);
}

// A and the rows' KL parts of the current embedding
void launch_attractive(l3_tsne* h) {
    hipLaunchKernelGGL(tsne_attractive_kernel, dim3(blocks_of(h->n, BLOCK / 64)), dim3(BLOCK), 0, h->s, h->Y, h->n, h->indptr, h->cols, h->vals, h->A,
                       h->klrow);
}

void launch_update(l3_tsne* h, double exaggeration, double momentum, double lr) {
    hipLaunchKernelGGL(tsne_update_kernel, dim3(blocks_of(2 * h->n, BLOCK)), dim3(BLOCK), 0, h->s, h->Y, h->U, h->G, h->A, h->R, h->scal, 2 * h->n,
                       exaggeration, (float)momentum, (float)lr);
}

int check_schedule(double exaggeration, double momentum, double lr, const char* fn) {
    if (!(exaggeration > 0.0) || !std::isfinite(exaggeration) || !(momentum >= 0.0 && momentum < 1.0) || !(lr > 0.0) || !std::isfinite(lr))
        return fail(L3_EINVAL, std::string(fn) + ": need exaggeration > 0, 0 <= momentum < 1 and learning_rate > 0, all finite");
    return L3_OK;
}

int check_csr(int64_t n, const int64_t* indptr, const int32_t* cols, const float* vals, const char* fn) {
    if (!indptr) return fail(L3_EINVAL, std::string(fn) + ": indptr is NULL");
    if (indptr[0] != 0) return fail(L3_EINVAL, std::string(fn) + ": indptr[0] must be 0");
    for (int64_t i = 0; i < n; ++i)
        if (indptr[i + 1] < indptr[i]) return fail(L3_EINVAL, std::string(fn) + ": indptr descends at row " + std::to_string(i));
    if (indptr[n] > 0 && (!cols || !vals)) return fail(L3_EINVAL, std::string(fn) + ": cols and vals must not be NULL");
    for (int64_t i = 0; i < n; ++i)
        for (int64_t e = indptr[i]; e < indptr[i + 1]; ++e) {
            const int64_t j = cols[e];
            if (j < 0 || j >= n) return fail(L3_EINVAL, std::string(fn) + ": row " + std::to_string(i) + " holds the column " + std::to_string(j) + ", outside the " + std::to_string(n) + " points");
            if (j == i) return fail(L3_EINVAL, std::string(fn) + ": row " + std::to_string(i) + " holds a diagonal entry");
            if (e > indptr[i] && cols[e - 1] >= j) return fail(L3_EINVAL, std::string(fn) + ": the columns of row " + std::to_string(i) + " are not sorted (strictly ascending)");
            if (!(vals[e] >= 0.0f) || !std::isfinite(vals[e])) return fail(L3_EINVAL, std::string(fn) + ": row " + std::to_string(i) + " holds an entry that is negative or not finite");
        }
    return L3_OK;
}

}  // namespace
}  // namespace l3

using namespace l3;

extern "C" {

int l3_tsne_geometry(int64_t n, int* row_block, int* segments) {
    const char* fn = "l3_tsne_geometry";
    if (n < 1 || n > MAX_POINTS || !row_block || !segments) return fail(L3_EINVAL, std::string(fn) + ": need 1 <= n <= 2^24 and two outputs");
    int rps = 0;
    geometry(n, row_block, &rps, segments);
    return L3_OK;
}

int l3_op_tsne_conditional(int device, const float* dist, int64_t n, int k, double perplexity, double* p_out, double* beta_out, int64_t* bad_rows) {
    const char* fn = "l3_op_tsne_conditional";
    if (!dist || !p_out || !beta_out) return fail(L3_EINVAL, std::string(fn) + ": dist, p_out and beta_out must not be NULL");
    if (n < 1 || n > MAX_POINTS) return fail(L3_EINVAL, std::string(fn) + ": need 1 <= n <= 2^24 rows, not " + std::to_string(n));
    if (k < 2 || k > K_MAX) return fail(L3_EINVAL, std::string(fn) + ": need 2 <= k <= " + std::to_string(K_MAX) + " neighbours, not " + std::to_string(k));
    if (!(perplexity > 1.0 && perplexity < (double)k))
        return fail(L3_EINVAL, std::string(fn) + ": need 1 < perplexity < k = " + std::to_string(k) + ", not " + std::to_string(perplexity));
    if (!device_ok(device)) return fail(L3_EHIP, no_gpu_message(fn, device));
    DeviceBufs bufs;
    const size_t cells = (size_t)n * k;
    float* d = bufs.put(dist, cells, nullptr);
    double* p = bufs.alloc<double>(cells);
    double* beta = bufs.alloc<double>((size_t)n);
    unsigned long long* bad = bufs.alloc<unsigned long long>(1);
    if (!bufs.ok()) return fail(L3_ENOMEM, std::string(fn) + ": device allocation failed");
    unsigned long long got = 0;
    if (hipMemset(bad, 0, 8) != hipSuccess) return fail(L3_EHIP, std::string(fn) + ": hipMemset failed");
    hipLaunchKernelGGL(tsne_conditional_kernel, dim3(blocks_of(n, CAL_ROWS)), dim3(CAL_ROWS), 0, nullptr, d, n, k, std::log(perplexity), p, beta, bad);
    if (hipMemcpy(p_out, p, cells * 8, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(beta_out, beta, (size_t)n * 8, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(&got, bad, 8, hipMemcpyDeviceToHost) != hipSuccess || hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess)
        return fail(L3_EHIP, std::string(fn) + ": the kernel or the copy from the device failed");
    if (bad_rows) *bad_rows = (int64_t)got;
    return L3_OK;
}

int l3_tsne_create(int device, int64_t n, l3_tsne** out) {
    const char* fn = "l3_tsne_create";
    if (!out) return fail(L3_EINVAL, std::string(fn) + ": out is NULL");
    *out = nullptr;
    if (n < 1 || n > MAX_POINTS) return fail(L3_EINVAL, std::string(fn) + ": need 1 <= n <= 2^24 points, not " + std::to_string(n));
    if (!device_ok(device)) return fail(L3_EHIP, no_gpu_message(fn, device));
    l3_tsne* h = new l3_tsne();
    h->device = device, h->n = n;
    geometry(n, &h->row_block, &h->runs_per_segment, &h->segments);
    if (hipStreamCreateWithFlags(&h->s, hipStreamNonBlocking) != hipSuccess) {
        h->s = nullptr;
        l3_tsne_destroy(h);
        return fail(L3_EHIP, std::string(fn) + ": hipStreamCreate failed");
    }
    const size_t m = (size_t)n;
    h->Y = h->bufs.alloc<float>(2 * m), h->U = h->bufs.alloc<float>(2 * m), h->G = h->bufs.alloc<float>(2 * m);
    h->indptr = h->bufs.alloc<int64_t>(m + 1);
    h->part = h->bufs.alloc<double>((size_t)h->segments * 3 * m);
    h->R = h->bufs.alloc<double>(2 * m), h->A = h->bufs.alloc<double>(2 * m);
    h->z = h->bufs.alloc<double>(m), h->klrow = h->bufs.alloc<double>(m);
    h->runs = h->bufs.alloc<double>((m + RUN - 1) / RUN);
    h->scal = h->bufs.alloc<l3_tsne_scalars>(1);
    if (!h->bufs.ok() || hipMemset(h->scal, 0, sizeof(l3_tsne_scalars)) != hipSuccess) {
        l3_tsne_destroy(h);
        return fail(L3_ENOMEM, std::string(fn) + ": device allocation for " + std::to_string(n) + " points failed");
    }
    *out = h;
    return L3_OK;
}

void l3_tsne_destroy(l3_tsne* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->s) (void)hipStreamSynchronize(h->s);
    if (h->s) (void)hipStreamDestroy(h->s);
    delete h;
}

int l3_tsne_set_affinities(l3_tsne* h, const int64_t* indptr, const int32_t* cols, const float* vals) {
    const char* fn = "l3_tsne_set_affinities";
    if (!h) return fail(L3_EINVAL, std::string(fn) + ": NULL handle");
    if (int rc = check_csr(h->n, indptr, cols, vals, fn)) return rc;          // before the device is touched
    if (int rc = enter(h, fn)) return rc;
    h->has_affinities = false;
    const size_t nnz = (size_t)indptr[h->n];
    double plogp = 0.0;
    for (size_t e = 0; e < nnz; ++e)
        if (vals[e] > 0.0f) plogp += (double)vals[e] * std::log((double)vals[e]);
    h->bufs.grow(&h->cols, &h->cap_cols, nnz);
    h->bufs.grow(&h->vals, &h->cap_vals, nnz);
    if (!h->cols || !h->vals) return fail(L3_ENOMEM, std::string(fn) + ": device allocation of " + std::to_string(nnz) + " entries failed");
    bool ok = hipMemcpyAsync(h->indptr, indptr, ((size_t)h->n + 1) * 8, hipMemcpyHostToDevice, h->s) == hipSuccess;
    if (nnz) {
        ok = ok && hipMemcpyAsync(h->cols, cols, nnz * 4, hipMemcpyHostToDevice, h->s) == hipSuccess;
        ok = ok && hipMemcpyAsync(h->vals, vals, nnz * 4, hipMemcpyHostToDevice, h->s) == hipSuccess;
    }
    if (!ok || !finished(h->s)) return fail(L3_EHIP, std::string(fn) + ": copy to the device failed");
    h->plogp = plogp, h->has_affinities = true;
    return L3_OK;
}

int l3_tsne_set_embedding(l3_tsne* h, const float* y) {
    const char* fn = "l3_tsne_set_embedding";
    if (int rc = enter(h, fn)) return rc;
    if (!y) return fail(L3_EINVAL, std::string(fn) + ": y is NULL");
    h->has_embedding = false;
    const size_t m = 2 * (size_t)h->n;
    std::vector<float> ones(m, 1.0f);
    if (hipMemcpyAsync(h->Y, y, m * 4, hipMemcpyHostToDevice, h->s) != hipSuccess || hipMemsetAsync(h->U, 0, m * 4, h->s) != hipSuccess ||
        hipMemcpyAsync(h->G, ones.data(), m * 4, hipMemcpyHostToDevice, h->s) != hipSuccess || !finished(h->s))
        return fail(L3_EHIP, std::string(fn) + ": copy to the device failed");
    h->has_embedding = true, h->iteration = 0;
    return L3_OK;
}

int l3_tsne_get_embedding(l3_tsne* h, float* y) {
    const char* fn = "l3_tsne_get_embedding";
    if (int rc = enter(h, fn)) return rc;
    if (!y) return fail(L3_EINVAL, std::string(fn) + ": y is NULL");
    if (int rc = need_embedding(h, fn)) return rc;
    if (hipMemcpyAsync(y, h->Y, 2 * (size_t)h->n * 4, hipMemcpyDeviceToHost, h->s) != hipSuccess || !finished(h->s))
        return fail(L3_EHIP, std::string(fn) + ": copy from the device failed");
    return L3_OK;
}

int l3_tsne_run(l3_tsne* h, int n_iter, double exaggeration, double momentum, double learning_rate, int kl_every, double* history_out,
                int* n_records) {
    const char* fn = "l3_tsne_run";
    if (n_records) *n_records = 0;
    if (int rc = enter(h, fn)) return rc;
    if (n_iter < 1 || kl_every < 1) return fail(L3_EINVAL, std::string(fn) + ": need n_iter >= 1 and kl_every >= 1");
    if (int rc = check_schedule(exaggeration, momentum, learning_rate, fn)) return rc;
    if (int rc = need_affinities(h, fn)) return rc;
    if (int rc = need_embedding(h, fn)) return rc;
    int records = 0;
    for (int it = 0; it < n_iter; ++it, ++h->iteration) {
        launch_repulsive(h);
        launch_attractive(h);
        if ((it + 1) % kl_every == 0 || it == n_iter - 1) {          // the only read-back: two scalars
            launch_sum(h, h->klrow, &h->scal->kl_rows);
            l3_tsne_scalars got;
            if (hipMemcpyAsync(&got, h->scal, sizeof(got), hipMemcpyDeviceToHost, h->s) != hipSuccess || !finished(h->s))
                return fail(L3_EHIP, std::string(fn) + ": the kernels or the copy from the device failed");
            if (!std::isfinite(got.Z) || got.Z == 0.0)
                return fail(L3_EINVAL, std::string(fn) + ": Z = " + std::to_string(got.Z) + " at iteration " + std::to_string(h->iteration) +
                                           ": the map has a single point, or it diverged (lower the learning rate)");
            if (history_out) {
                double* rec = history_out + 3 * records;
                rec[0] = (double)h->iteration, rec[1] = h->plogp + got.kl_rows + std::log(got.Z), rec[2] = got.Z;
            }
            ++records;
            if (n_records) *n_records = records;
        }
        launch_update(h, exaggeration, momentum, learning_rate);
    }
    if (!finished(h->s)) return fail(L3_EHIP, std::string(fn) + ": the kernels failed on the device");
    return L3_OK;
}

// Device time of `reps` rounds on the resident map, in ms per round (hipEvents; one untimed round first).  what 0: the repulsive pass
// (the pair kernel, the finish and Z); 1: the attractive pass; 2: the update; 3: one whole iteration; 4: the pair kernel alone.  The
// map moves on under 2 and 3 (exaggeration 1, momentum 0.5, learning rate 1).  For profiles/ records; no test asserts a time.
int l3_tsne_time(l3_tsne* h, int what, int reps, double* ms) {
    const char* fn = "l3_tsne_time";
    if (int rc = enter(h, fn)) return rc;
    if (!ms || reps < 1 || what < 0 || what > 4) return fail(L3_EINVAL, std::string(fn) + ": need ms, reps >= 1 and what in [0, 4]");
    if (int rc = need_embedding(h, fn)) return rc;
    if (what != 0 && what != 4)
        if (int rc = need_affinities(h, fn)) return rc;
    if (what == 2) launch_repulsive(h), launch_attractive(h);
    hipEvent_t a, b;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return fail(L3_EHIP, std::string(fn) + ": hipEventCreate failed");
    auto run = [&](int count) {
        for (int r = 0; r < count; ++r) {
            if (what == 0 || what == 3) launch_repulsive(h);
            if (what == 1 || what == 3) launch_attractive(h);
            if (what == 2 || what == 3) launch_update(h, 1.0, 0.5, 1.0);
            if (what == 4) launch_pairs(h);
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
    *ms = (double)t / reps;
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    return rc;
}

int l3_op_tsne_repulsive(int device, const float* y, int64_t n, double* R_out, double* z_out, double* Z_out) {
    const char* fn = "l3_op_tsne_repulsive";
    if (!y) return fail(L3_EINVAL, std::string(fn) + ": y is NULL");
    l3_tsne* h = nullptr;
    int rc = l3_tsne_create(device, n, &h);
    if (rc == L3_OK) rc = l3_tsne_set_embedding(h, y);
    if (rc == L3_OK) {
        launch_repulsive(h);
        l3_tsne_scalars got;
        bool ok = hipMemcpyAsync(&got, h->scal, sizeof(got), hipMemcpyDeviceToHost, h->s) == hipSuccess;
        if (R_out) ok = ok && hipMemcpyAsync(R_out, h->R, 2 * (size_t)n * 8, hipMemcpyDeviceToHost, h->s) == hipSuccess;
        if (z_out) ok = ok && hipMemcpyAsync(z_out, h->z, (size_t)n * 8, hipMemcpyDeviceToHost, h->s) == hipSuccess;
        if (!ok || !finished(h->s)) rc = fail(L3_EHIP, std::string(fn) + ": the kernels or the copy from the device failed");
        else if (Z_out) *Z_out = got.Z;
    }
    l3_tsne_destroy(h);
    return rc;
}

int l3_op_tsne_attractive(int device, const float* y, int64_t n, const int64_t* indptr, const int32_t* cols, const float* vals, double* A_out,
                          double* kl_rows_out, double* plogp_out) {
    const char* fn = "l3_op_tsne_attractive";
    if (!y) return fail(L3_EINVAL, std::string(fn) + ": y is NULL");
    if (n < 1 || n > MAX_POINTS) return fail(L3_EINVAL, std::string(fn) + ": need 1 <= n <= 2^24 points, not " + std::to_string(n));
    if (int rc = check_csr(n, indptr, cols, vals, fn)) return rc;
    l3_tsne* h = nullptr;
    int rc = l3_tsne_create(device, n, &h);
    if (rc == L3_OK) rc = l3_tsne_set_affinities(h, indptr, cols, vals);
    if (rc == L3_OK) rc = l3_tsne_set_embedding(h, y);
    if (rc == L3_OK) {
        launch_attractive(h);
        launch_sum(h, h->klrow, &h->scal->kl_rows);
        l3_tsne_scalars got;
        bool ok = hipMemcpyAsync(&got, h->scal, sizeof(got), hipMemcpyDeviceToHost, h->s) == hipSuccess;
        if (A_out) ok = ok && hipMemcpyAsync(A_out, h->A, 2 * (size_t)n * 8, hipMemcpyDeviceToHost, h->s) == hipSuccess;
        if (!ok || !finished(h->s)) rc = fail(L3_EHIP, std::string(fn) + ": the kernel or the copy from the device failed");
        else {
            if (kl_rows_out) *kl_rows_out = got.kl_rows;
            if (plogp_out) *plogp_out = h->plogp;
        }
    }
    l3_tsne_destroy(h);
    return rc;
}

int l3_op_tsne_update(int device, int64_t n, float* y, float* update, float* gains, const double* A, const double* R, double Z, double exaggeration,
                      double momentum, double learning_rate) {
    const char* fn = "l3_op_tsne_update";
    if (!y || !update || !gains || !A || !R) return fail(L3_EINVAL, std::string(fn) + ": y, update, gains, A and R must not be NULL");
    if (int rc = check_schedule(exaggeration, momentum, learning_rate, fn)) return rc;
    l3_tsne* h = nullptr;
    int rc = l3_tsne_create(device, n, &h);
    if (rc == L3_OK) {
        const size_t m = 2 * (size_t)n;
        l3_tsne_scalars sc = {Z, 0.0};
        bool ok = hipMemcpyAsync(h->Y, y, m * 4, hipMemcpyHostToDevice, h->s) == hipSuccess && hipMemcpyAsync(h->U, update, m * 4, hipMemcpyHostToDevice, h->s) == hipSuccess &&
                  hipMemcpyAsync(h->G, gains, m * 4, hipMemcpyHostToDevice, h->s) == hipSuccess && hipMemcpyAsync(h->A, A, m * 8, hipMemcpyHostToDevice, h->s) == hipSuccess &&
                  hipMemcpyAsync(h->R, R, m * 8, hipMemcpyHostToDevice, h->s) == hipSuccess &&
                  hipMemcpyAsync(h->scal, &sc, sizeof(sc), hipMemcpyHostToDevice, h->s) == hipSuccess && hipStreamSynchronize(h->s) == hipSuccess;
        if (ok) {
            launch_update(h, exaggeration, momentum, learning_rate);
            ok = hipMemcpyAsync(y, h->Y, m * 4, hipMemcpyDeviceToHost, h->s) == hipSuccess && hipMemcpyAsync(update, h->U, m * 4, hipMemcpyDeviceToHost, h->s) == hipSuccess &&
                 hipMemcpyAsync(gains, h->G, m * 4, hipMemcpyDeviceToHost, h->s) == hipSuccess && finished(h->s);
        }
        if (!ok) rc = fail(L3_EHIP, std::string(fn) + ": the kernel or a copy failed");
    }
    l3_tsne_destroy(h);
    return rc;
}

}  // extern "C"
