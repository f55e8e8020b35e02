// mlp.hip -- the downstream MLP classifier (classifier/train.py:230-391): construct_mlp_model's fp32 training step on the fp32
// matrix cores (v_mfma_f32_32x32x2_f32: exact fp32 products, one rounding per fmaf), and the l3_mlp engine of the C ABI.
//
// One training step is seven launches on one stream:
//   3 x mlp_dense_fwd   h1 = relu(X[idx] W1 + b1) (gathered rows, split-K), h2 = relu(h1 W2 + b2), z = h2 W3 + b3
//   mlp_softmax_ce      dz, per-row cross-entropy and correctness
//   2 x mlp_dense_bwd_x dh2 = dz W3^T [h2 > 0], dh1 = dh2 W2^T [h1 > 0]
//   mlp_wgrad           dW = X^T dY of the three layers, + 2 wd W, keras Adam, tile by tile (dW never reaches HBM); batch loss
// Both data-gradient launches read the old W2 / W3 before the one launch that updates every weight: the ordering hazard of a
// per-layer update cannot arise.  No host synchronisation inside an epoch.
//
// Every kernel of the step has a member dimension (mlp.h): block row y of a launch works on one model of a group of up to 16 of
// one shape, with its own weights, moments, activations, partials and counters and the group's rows, labels and permutation.  The
// l3_mlp_group handle trains a parameter search's grid that way, seven launches per step whatever the number of live members, and
// l3_mlp is a group of one: there is one copy of each kernel, and a member's arithmetic does not depend on the group.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/l3hip.h"
#include "device_common.h"
#include "featprep.h"
#include "kernels.h"
#include "mlp.h"

namespace l3 {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// ---- forward: Y = act(X[idx] W + b) ------------------------------------------------------------------------------------------
// One wave per (split, 32x32 output tile).  Step of 8 k: lane (r, h) holds A = X[row r][k0 + 4h + j] and B = W[k0 + 4h + j][col r]
// for j = 0..3 (one float4 of its row of X), and MFMA j sums k0 + j and k0 + 4 + j.
struct MlpFwdArgs {
    const float* x;
    const int* idx;
    int64_t ldx;
    const float *w, *b;
    float *y, *part;
    int* ctr;
    int rows, K, N, S, kc, relu, vec;
    MlpMembers mem;
    MlpFwdStride m;
};
__global__ __launch_bounds__(256) void mlp_fwd_kernel(MlpFwdArgs a) {
    // the block row's member: its own weights, output, partials and counters (a stride of 0 shares a buffer)
    const int64_t mb = mlp_member(a.mem, blockIdx.y);
    a.x += mb * a.m.x, a.w += mb * a.m.w, a.b += mb * a.m.b, a.y += mb * a.m.y, a.part += mb * a.m.part, a.ctr += mb * a.m.ctr;
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int ct_n = (a.N + 31) >> 5, tiles = ((a.rows + 31) >> 5) * ct_n;
    const int wv = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wv >= tiles * a.S) return;
    const int s = wv / tiles, t = wv - s * tiles;
    const int rt = t / ct_n, ct = t - rt * ct_n;
    const int arow = rt * 32 + r, col = ct * 32 + r;
    const bool rv = arow < a.rows, cv = col < a.N;
    const float* xr = a.x + (rv ? (int64_t)(a.idx ? a.idx[arow] : arow) * a.ldx : 0);
    const float* wc = a.w + (cv ? col : 0);
    const int kb = s * a.kc, ke = min(a.K, kb + a.kc);
    f32x16 acc = {};
    for (int k0 = kb; k0 < ke; k0 += 8) {
        const int k = k0 + 4 * h;
        float av[4], bv[4];
        if (a.vec && k + 4 <= ke && rv) {
            const float4 q = *reinterpret_cast<const float4*>(xr + k);
            av[0] = q.x, av[1] = q.y, av[2] = q.z, av[3] = q.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) av[j] = (rv && k + j < ke) ? xr[k + j] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) bv[j] = (cv && k + j < ke) ? wc[(int64_t)(k + j) * a.N] : 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j], bv[j], acc, 0, 0, 0);
    }
    const float bias = cv ? a.b[col] : 0.f;
    if (a.S == 1) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int row = rt * 32 + mfma_row(i, h);
            if (row < a.rows && cv) {
                const float v = acc[i] + bias;
                a.y[(int64_t)row * a.N + col] = a.relu ? fmaxf(v, 0.f) : v;
            }
        }
        return;
    }
    const int64_t plane = (int64_t)a.rows * a.N;
    float* P = a.part + s * plane;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int row = rt * 32 + mfma_row(i, h);
        if (row < a.rows && cv) P[(int64_t)row * a.N + col] = acc[i];
    }
    // the last of the tile's S waves to arrive sums the partials in split order (which wave that is does not enter the result)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    int old = 0;
    if (lane == 0) old = atomicAdd(a.ctr + t, 1);
    old = __shfl(old, 0);
    if (old != a.S - 1) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int row = rt * 32 + mfma_row(i, h);
        if (row < a.rows && cv) {
            const int64_t o = (int64_t)row * a.N + col;
            float v = __builtin_nontemporal_load(a.part + o);
            for (int q = 1; q < a.S; ++q) v += __builtin_nontemporal_load(a.part + q * plane + o);
            v += bias;
            a.y[o] = a.relu ? fmaxf(v, 0.f) : v;
        }
    }
    if (lane == 0) atomicExch(a.ctr + t, 0);
}

static void fwd_split(int rows, int K, int N, int* S_out, int* kc_out) {
    const int tiles = ((rows + 31) / 32) * ((N + 31) / 32);
    int S = (K >= 8192 ? 2048 : 1024) / tiles;
    S = std::min(S, K / 128);
    while (S > 1 && (int64_t)S * rows * N > MLP_PART_FLOATS) --S;
    if (S < 1 || tiles > MLP_FWD_COUNTERS) S = 1;
    int kc = (K + S - 1) / S;
    kc = (kc + 7) & ~7;
    *S_out = (K + kc - 1) / kc;
    *kc_out = kc;
}
int mlp_fwd_splits(int rows, int K, int N) {
    int S, kc;
    fwd_split(rows, K, N, &S, &kc);
    return S;
}

void mlp_dense_fwd_members(const float* x, const int* idx, int64_t ldx, const float* w, const float* b, float* y, int rows, int K,
                           int N, int relu, float* part, int* ctr, const MlpMembers& mem, const MlpFwdStride& stride, hipStream_t s) {
    MlpFwdArgs a{x, idx, ldx, w, b, y, part, ctr, rows, K, N, 1, K, relu, 0, mem, stride};
    fwd_split(rows, K, N, &a.S, &a.kc);
    // a member's rows start a multiple of its stride after x: 16-byte aligned like x when the stride is a multiple of 4 floats
    a.vec = (ldx % 4 == 0 && a.kc % 4 == 0 && stride.x % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0) ? 1 : 0;
    const int waves = ((rows + 31) / 32) * ((N + 31) / 32) * a.S;
    hipLaunchKernelGGL(mlp_fwd_kernel, dim3((waves + 3) / 4, mem.n), dim3(256), 0, s, a);
}
void mlp_dense_fwd(const float* x, const int* idx, int64_t ldx, const float* w, const float* b, float* y, int rows, int K, int N,
                   int relu, float* part, int* ctr, hipStream_t s) {
    mlp_dense_fwd_members(x, idx, ldx, w, b, y, rows, K, N, relu, part, ctr, MLP_ONE_MEMBER, MlpFwdStride{}, s);
}

// ---- data gradient: dX = (dY W^T) [h > 0] -------------------------------------------------------------------------------------
// One wave per 32x32 tile of dX (rows x K); the sum runs over N: lane (r, h) holds A = dY[row r][n0 + 4h + j], B = W[k r][n0 + 4h + j].
__global__ __launch_bounds__(256) void mlp_bwd_x_kernel(const float* dy, const float* w, const float* hm, float* dx, int rows, int K,
                                                        int N, MlpMembers mem, MlpBwdStride m) {
    const int64_t mb = mlp_member(mem, blockIdx.y);
    dy += mb * m.dy, w += mb * m.w, dx += mb * m.dx;
    if (hm) hm += mb * m.h;
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int kt_n = (K + 31) >> 5;
    const int wv = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wv >= ((rows + 31) >> 5) * kt_n) return;
    const int rt = wv / kt_n, kt = wv - rt * kt_n;
    const int arow = rt * 32 + r, kcol = kt * 32 + r;
    const bool rv = arow < rows, kv = kcol < K;
    const float* dr = dy + (rv ? (int64_t)arow * N : 0);
    const float* wr = w + (kv ? (int64_t)kcol * N : 0);
    f32x16 acc = {};
    for (int n0 = 0; n0 < N; n0 += 8) {
        const int n = n0 + 4 * h;
        float av[4], bv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            av[j] = (rv && n + j < N) ? dr[n + j] : 0.f;
            bv[j] = (kv && n + j < N) ? wr[n + j] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j], bv[j], acc, 0, 0, 0);
    }
    if (!kv) return;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int row = rt * 32 + mfma_row(i, h);
        if (row < rows) {
            const int64_t o = (int64_t)row * K + kcol;
            dx[o] = (hm == nullptr || hm[o] > 0.f) ? acc[i] : 0.f;
        }
    }
}
void mlp_dense_bwd_x_members(const float* dy, const float* w, const float* h, float* dx, int rows, int K, int N,
                             const MlpMembers& mem, const MlpBwdStride& stride, hipStream_t s) {
    const int waves = ((rows + 31) / 32) * ((K + 31) / 32);
    hipLaunchKernelGGL(mlp_bwd_x_kernel, dim3((waves + 3) / 4, mem.n), dim3(256), 0, s, dy, w, h, dx, rows, K, N, mem, stride);
}
void mlp_dense_bwd_x(const float* dy, const float* w, const float* h, float* dx, int rows, int K, int N, hipStream_t s) {
    mlp_dense_bwd_x_members(dy, w, h, dx, rows, K, N, MLP_ONE_MEMBER, MlpBwdStride{}, s);
}

// ---- softmax + categorical cross-entropy (keras 2.0.9 / TF 1.4) -----------------------------------------------------------------
// softmax_ce_kernel (elementwise.hip, C = 2) for any C <= 64: p = softmax(z); q = p / sum(p); c = clip(q, 1e-7, 1 - 1e-7);
// loss = -sum t log c; the gradient flows through the normalisation and through the clip where q lies inside it.
__global__ __launch_bounds__(256) void mlp_softmax_ce_kernel(const float* z, const int* labels, const int* idx, int rows, int C,
                                                             float gscale, float* probs, float* dz, float* ce, float* correct,
                                                             MlpMembers mem, MlpCeStride m) {
    const int64_t mb = mlp_member(mem, blockIdx.y);          // the labels and idx are the group's, the rest the member's
    z += mb * m.z;
    if (probs) probs += mb * m.probs;
    if (dz) dz += mb * m.dz;
    if (ce) ce += mb * m.ce;
    if (correct) correct += mb * m.ce;
    const int c = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float eps = 1e-7f;
    const bool cv = c < C;
    const int64_t o = (int64_t)row * C + c;
    const float zc = cv ? z[o] : -INFINITY;
    const float mx = wave_max(zc);
    const float e = cv ? expf(zc - mx) : 0.f;
    const float inv = 1.f / wave_sum(e);
    const float p = e * inv;
    if (probs && cv) probs[o] = p;
    const float sm = wave_sum(p);
    const float q = p / sm;
    const float cl = fminf(fmaxf(q, eps), 1.f - eps);
    const int lab = labels[idx ? idx[row] : row];
    const float t = c == lab ? 1.f : 0.f;
    // argmax, first maximum (K.argmax)
    float bv = cv ? p : -INFINITY;
    int bi = c;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(bv, off);
        const int oi = __shfl_xor(bi, off);
        if (ov > bv || (ov == bv && oi < bi)) bv = ov, bi = oi;
    }
    const float lc = __shfl(logf(cl), lab);
    if (c == 0) {
        if (ce) ce[row] = -lc;
        if (correct) correct[row] = bi == lab ? 1.f : 0.f;
    }
    if (dz) {
        const float dq = (cv && q >= eps && q <= 1.f - eps) ? -(t / cl) * gscale : 0.f;
        const float dot = wave_sum(dq * p) / (sm * sm);
        const float dp = dq / sm - dot;
        const float pd = wave_sum(cv ? dp * p : 0.f);
        if (cv) dz[o] = p * (dp - pd);
    }
}
void mlp_softmax_ce_members(const float* z, const int* labels, const int* idx, int rows, int C, float gscale, float* probs, float* dz,
                            float* ce, float* correct, const MlpMembers& mem, const MlpCeStride& stride, hipStream_t s) {
    hipLaunchKernelGGL(mlp_softmax_ce_kernel, dim3((rows + 3) / 4, mem.n), dim3(256), 0, s, z, labels, idx, rows, C, gscale, probs, dz,
                       ce, correct, mem, stride);
}
void mlp_softmax_ce(const float* z, const int* labels, const int* idx, int rows, int C, float gscale, float* probs, float* dz,
                    float* ce, float* correct, hipStream_t s) {
    mlp_softmax_ce_members(z, labels, idx, rows, C, gscale, probs, dz, ce, correct, MLP_ONE_MEMBER, MlpCeStride{}, s);
}

// ---- per-file mean of the rows' probabilities and its arg-max (classifier._file_predictions) ---------------------------------------
// NumPy's probs[s:e].mean(axis=0).argmax() on float32 rows: one wave per file, lane c owns class c and adds its column in row order
// (eight loads in flight, the additions in order), divides once by fl32(e - s), and the wave takes the first maximum.  A long file
// stays on its one wave: the order of the sum is the contract.  Consecutive lanes read consecutive floats of a row.
__global__ __launch_bounds__(256) void mlp_file_mean_kernel(const float* __restrict__ probs, int C, const int64_t* __restrict__ files,
                                                            int64_t n_files, float* __restrict__ file_mean, int* __restrict__ file_pred) {
    const int c = threadIdx.x & 63;
    const int64_t f = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (f >= n_files) return;          // the whole wave
    const int64_t s = files[2 * f], F = files[2 * f + 1] - s;
    const bool cv = c < C;
    const float* p = probs + s * C + (cv ? c : 0);          // a lane without a class reads class 0's column and drops it
    float sum = 0.f;
    int64_t r = 0;
    for (; r + 8 <= F; r += 8) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = p[(r + j) * C];
#pragma unroll
        for (int j = 0; j < 8; ++j) sum = __fadd_rn(sum, v[j]);
    }
    for (; r < F; ++r) sum = __fadd_rn(sum, p[r * C]);
    const float mean = __fdiv_rn(sum, (float)F);
    if (file_mean && cv) file_mean[f * C + c] = mean;
    float bv = cv ? mean : -INFINITY;
    int bi = c;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(bv, off);
        const int oi = __shfl_xor(bi, off);
        if (ov > bv || (ov == bv && oi < bi)) bv = ov, bi = oi;
    }
    if (file_pred && c == 0) file_pred[f] = bi;
}
void mlp_file_mean(const float* probs, int C, const int64_t* files, int64_t n_files, float* file_mean, int* file_pred, hipStream_t s) {
    hipLaunchKernelGGL(mlp_file_mean_kernel, dim3((unsigned)((n_files + 3) / 4)), dim3(256), 0, s, probs, C, files, n_files, file_mean,
                       file_pred);
}
std::string mlp_file_ranges_error(const int64_t* files, int64_t n_files, int64_t n) {
    if (n_files < 1 || n_files > INT32_MAX) return "need 1 <= n_files <= 2^31 - 1";
    for (int64_t i = 0; i < n_files; ++i) {
        const int64_t s = files[2 * i], e = files[2 * i + 1];
        if (s < 0 || e <= s || e > n)
            return "file " + std::to_string(i) + " = [" + std::to_string(s) + ", " + std::to_string(e) + ") is empty or outside [0, " +
                   std::to_string(n) + ")";
    }
    return std::string();
}

// ---- weight gradient + L2 + Adam ------------------------------------------------------------------------------------------------
// Layer l's waves: ceil(K/32) * ceil(N/32) weight tiles, then ceil(N/64) bias tiles.  Weight tile (kt, nt): the sum runs over the
// batch, lane (r, h) holding A = X[idx[b0 + 4h + j]][kt*32 + r] and B = dY[b0 + 4h + j][nt*32 + r].  Bias tile: lane n sums its
// column of dY in row order.
__device__ __forceinline__ int wg_tiles_w(const MlpWgLayer& L) { return ((L.K + 31) >> 5) * ((L.N + 31) >> 5); }
__device__ __forceinline__ int wg_tiles_b(const MlpWgLayer& L) { return (L.N + 63) >> 6; }

// adam_kernel's update of one element, in its order of operations (gscale 1: exact)
__device__ __forceinline__ float adam_one(float w, float g, float* mp, float* vp, bool l2, const MlpWgrad& a, float l2x2, float lr_t) {
    float gi = g * 1.f;
    if (l2) gi = fmaf(l2x2, w, gi);
    const float mi = a.b1 * *mp + (1.f - a.b1) * gi;
    const float vi = a.b2 * *vp + (1.f - a.b2) * gi * gi;
    *mp = mi;
    *vp = vi;
    return w - lr_t * mi / (sqrtf(vi) + a.eps);
}

__global__ __launch_bounds__(256) void mlp_wgrad_kernel(MlpWgrad a, float* w2part, int* ctr, int total, MlpMembers mem, MlpWgStride m) {
    // the block row's member: its own parameters and moments, activations, gradients, w2part, counter, accumulators and, from
    // m.par, its rate and weight decay (lr_t = lr * the step's bias correction: one float32 product, as the host forms it)
    const int64_t mb = mlp_member(mem, blockIdx.y);
    w2part += mb * m.w2part, ctr += mb * m.ctr;
    // The table is read as constant memory, which it is for the length of a launch: scalar loads, one per wave.  Through a plain
    // pointer the compiler merged each of these loads with the load of the kernel argument it replaces into one flat load from a
    // selected address, and a vector load from the argument segment made every launch of the single model 29 % slower.
    typedef __attribute__((address_space(4))) const float cfloat;
    cfloat* par = (cfloat*)(m.par + mb * MLP_MEMBER_PARS);
    float lr_t = a.lr_t, wd = a.wd, l2x2 = a.l2x2;
    if (m.par) lr_t = par[0] * m.lr_scale, wd = par[1], l2x2 = par[2];
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int wv = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wv >= total) return;
    // the wave's layer, picked with selects (a dynamic index into the kernel arguments would copy them to scratch)
    int t = wv;
    const int n0 = wg_tiles_w(a.L[0]) + wg_tiles_b(a.L[0]), n1 = wg_tiles_w(a.L[1]) + wg_tiles_b(a.L[1]);
    const int l = (a.nl > 1 && t >= n0) ? ((a.nl > 2 && t >= n0 + n1) ? 2 : 1) : 0;
    t -= l == 0 ? 0 : l == 1 ? n0 : n0 + n1;
    MlpWgLayer L = l == 0 ? a.L[0] : l == 1 ? a.L[1] : a.L[2];
    L.x += mb * (l == 0 ? m.x[0] : l == 1 ? m.x[1] : m.x[2]), L.dy += mb * (l == 0 ? m.dy[0] : l == 1 ? m.dy[1] : m.dy[2]);
    if (a.adam) L.w += mb * m.p, L.b += mb * m.p, L.mw += mb * m.p, L.vw += mb * m.p, L.mb += mb * m.p, L.vb += mb * m.p;
    float w2 = 0.f;
    if (t < wg_tiles_w(L)) {
        const int nt_n = (L.N + 31) >> 5;
        const int kt = t / nt_n, nt = t - kt * nt_n;
        const int kin = kt * 32 + r, col = nt * 32 + r;
        const bool kv = kin < L.K, cv = col < L.N;
        f32x16 acc = {};
        for (int b0 = 0; b0 < a.rows; b0 += 8) {
            float av[4], bv[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int b = b0 + 4 * h + j;
                const bool bok = b < a.rows;
                av[j] = (bok && kv) ? L.x[(int64_t)(L.idx ? L.idx[b] : b) * L.ldx + kin] : 0.f;
                bv[j] = (bok && cv) ? L.dy[(int64_t)b * L.N + col] : 0.f;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j], bv[j], acc, 0, 0, 0);
        }
        if (cv) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int k = kt * 32 + mfma_row(i, h);
                if (k < L.K) {
                    const int64_t o = (int64_t)k * L.N + col;
                    if (a.adam) {
                        const float w = L.w[o];
                        w2 = fmaf(w, w, w2);
                        L.w[o] = adam_one(w, acc[i], L.mw + o, L.vw + o, true, a, l2x2, lr_t);
                    } else {
                        L.dw[o] = acc[i];
                    }
                }
            }
        }
    } else {
        const int n = (t - wg_tiles_w(L)) * 64 + lane;
        if (n < L.N) {
            float g = 0.f;
            for (int b = 0; b < a.rows; ++b) g += L.dy[(int64_t)b * L.N + n];
            if (a.adam)
                L.b[n] = adam_one(L.b[n], g, L.mb + n, L.vb + n, false, a, l2x2, lr_t);
            else
                L.db[n] = g;
        }
    }
    if (!a.adam) return;
    w2 = wave_sum(w2);
    if (lane == 0) w2part[wv] = w2;
    // the last wave of the launch closes the step: sum of the pre-update W^2 in tile order, the batch's loss and correct count
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    int old = 0;
    if (lane == 0) old = atomicAdd(ctr, 1);
    old = __shfl(old, 0);
    if (old != total - 1) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    double sw = 0.0;
    for (int i = lane; i < total; i += 64) sw += (double)__builtin_nontemporal_load(w2part + i);
    sw = wave_sum_d(sw);
    if (a.ce) {
        const float *ce = a.ce + mb * m.ce, *correct = a.correct + mb * m.ce;
        double* macc = a.acc + mb * 2;
        double sc = 0.0, sk = 0.0;
        for (int i = lane; i < a.rows; i += 64) {
            sc += (double)__builtin_nontemporal_load(ce + i);
            sk += (double)__builtin_nontemporal_load(correct + i);
        }
        sc = wave_sum_d(sc);
        sk = wave_sum_d(sk);
        if (lane == 0) {
            const float loss = (float)(sc / a.rows) + wd * (float)sw;     // keras: mean ce + wd * sum W^2, in float32
            macc[0] += (double)loss * a.rows;
            macc[1] += sk;
        }
    }
    if (lane == 0) {
        if (a.w2out) *a.w2out = (float)sw;
        atomicExch(ctr, 0);
    }
}

int mlp_wgrad_tiles(const MlpWgrad& a) {
    int total = 0;
    for (int l = 0; l < a.nl; ++l)
        total += ((a.L[l].K + 31) / 32) * ((a.L[l].N + 31) / 32) + (a.L[l].N + 63) / 64;
    return total;
}
void mlp_wgrad_members(const MlpWgrad& a, float* w2part, int* ctr, const MlpMembers& mem, const MlpWgStride& stride, hipStream_t s) {
    const int total = mlp_wgrad_tiles(a);
    hipLaunchKernelGGL(mlp_wgrad_kernel, dim3((total + 3) / 4, mem.n), dim3(256), 0, s, a, w2part, ctr, total, mem, stride);
}
void mlp_wgrad(const MlpWgrad& a, float* w2part, int* ctr, hipStream_t s) {
    mlp_wgrad_members(a, w2part, ctr, MLP_ONE_MEMBER, MlpWgStride{}, s);
}

}  // namespace l3

// ================================================================================================================================
// l3_mlp: the classifier's training state on one device (include/l3hip.h)
// ================================================================================================================================
using namespace l3;

namespace {
constexpr float MLP_B1 = 0.9f, MLP_B2 = 0.999f, MLP_EPS = 1e-8f;     // keras.optimizers.Adam defaults (2.0.9)
constexpr int MLP_EVAL_ROWS = 4096;                                  // rows per forward of evaluation / prediction
constexpr int64_t MLP_PREDICT_FLOATS = 16 << 20;                     // host rows staged per l3_mlp_predict block
constexpr int64_t MLP_MAX_DATA_BYTES = (int64_t)64 << 30;            // features resident per l3_mlp_set_data call

uint64_t splitmix64(uint64_t& s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
}  // namespace

// A group of G models of one shape (D, C, batch) on one device, trained on one resident data set in the same launches.  Member i's
// buffers lie i strides after member 0's: the parameter and moment arenas (nparam floats), the activations (`rows` rows), the
// split-K partials, the counters, w2part, ce / correct, the two accumulators, its {lr, wd, 2 wd}.  The features, labels, permutation
// and the staging block of predict are the group's.  l3_mlp is a group of one.
struct l3_mlp_group {
    int device = 0, D = 0, C = 0, B = 0, G = 0, rows = 0, total_wg = 0;
    float wd[MLP_MAX_MEMBERS] = {}, hpar[MLP_MAX_MEMBERS * MLP_MEMBER_PARS] = {};
    hipStream_t s = nullptr;
    int64_t off[6] = {}, len[6] = {}, nparam = 0;       // W1 b1 W2 b2 W3 b3 in a member's arena (keras order)
    float *p = nullptr, *m = nullptr, *v = nullptr, *best = nullptr;     // best: the keep_best slots, allocated by the first call
    bool kept[MLP_MAX_MEMBERS] = {};
    float *h1 = nullptr, *h2 = nullptr, *z = nullptr, *dz = nullptr, *dh1 = nullptr, *dh2 = nullptr, *xin = nullptr;
    float *part = nullptr, *w2part = nullptr, *ce = nullptr, *correct = nullptr, *sq = nullptr, *sq_scratch = nullptr, *par = nullptr;
    int *ctr = nullptr, *perm = nullptr, *ytr = nullptr, *yva = nullptr, *yzero = nullptr;
    double* acc = nullptr;
    float *xtr = nullptr, *xva = nullptr;
    int64_t ntr = 0, nva = 0, xin_rows = 0;
    DeviceBufs bufs;
};
struct l3_mlp {
    l3_mlp_group* g = nullptr;
};

namespace {
constexpr int MLP_CTRS = MLP_FWD_COUNTERS + 1;       // a member's counters: the forward's tiles, then the weight gradient's one

float* W(l3_mlp_group* g, int i) { return g->p + g->off[i]; }

MlpMembers all_members(const l3_mlp_group* g) {
    MlpMembers mem{0, g->G};
    for (int i = 0; i < g->G; ++i) mem.ids |= (uint64_t)i << (4 * i);
    return mem;
}

void forward(l3_mlp_group* g, const MlpMembers& mem, const float* x, const int* idx, int rows) {
    const int64_t P = g->nparam, R = g->rows;
    mlp_dense_fwd_members(x, idx, g->D, W(g, 0), W(g, 1), g->h1, rows, g->D, MLP_H1, 1, g->part, g->ctr, mem,
                          MlpFwdStride{0, P, P, R * MLP_H1, MLP_PART_FLOATS, MLP_CTRS}, g->s);
    mlp_dense_fwd_members(g->h1, nullptr, MLP_H1, W(g, 2), W(g, 3), g->h2, rows, MLP_H1, MLP_H2, 1, g->part, g->ctr, mem,
                          MlpFwdStride{R * MLP_H1, P, P, R * MLP_H2, MLP_PART_FLOATS, MLP_CTRS}, g->s);
    mlp_dense_fwd_members(g->h2, nullptr, MLP_H2, W(g, 4), W(g, 5), g->z, rows, MLP_H2, g->C, 0, g->part, g->ctr, mem,
                          MlpFwdStride{R * MLP_H2, P, P, R * g->C, MLP_PART_FLOATS, MLP_CTRS}, g->s);
}

// Rows [0, n) of x (on the device, labels y or none) through the members `mem`, `block` rows per forward.  sums (may be null):
// 2 doubles per member of the group, the sums of ce and of correct in row order.  probs_host (may be null): member i's (n, C)
// probabilities go to probs_host + i * probs_stride -- host memory, or with probs_kind = hipMemcpyDeviceToDevice a device buffer.
int evaluate(l3_mlp_group* g, const char* fn, const MlpMembers& mem, const float* x, const int* y, int64_t n, int64_t block,
             double* sums, float* probs_host, int64_t probs_stride, hipMemcpyKind probs_kind = hipMemcpyDeviceToHost) {
    std::vector<float> ce(sums ? block : 0), cor(sums ? block : 0);
    const MlpCeStride stride{(int64_t)g->rows * g->C, (int64_t)g->rows * g->C, 0, g->rows};
    for (int k = 0; sums && k < mem.n; ++k) sums[2 * mlp_member(mem, k)] = sums[2 * mlp_member(mem, k) + 1] = 0.0;
    for (int64_t r0 = 0; r0 < n; r0 += block) {
        const int rows = (int)std::min<int64_t>(block, n - r0);
        forward(g, mem, x + r0 * g->D, nullptr, rows);
        mlp_softmax_ce_members(g->z, y ? y + r0 : g->yzero, nullptr, rows, g->C, 1.f, probs_host ? g->dz : nullptr, nullptr, g->ce,
                               g->correct, mem, stride, g->s);
        for (int k = 0; k < mem.n; ++k) {
            const int i = mlp_member(mem, k);
            if (sums && (hipMemcpyAsync(ce.data(), g->ce + (int64_t)i * g->rows, rows * sizeof(float), hipMemcpyDeviceToHost, g->s) !=
                             hipSuccess ||
                         hipMemcpyAsync(cor.data(), g->correct + (int64_t)i * g->rows, rows * sizeof(float), hipMemcpyDeviceToHost,
                                        g->s) != hipSuccess))
                return fail(L3_EHIP, std::string(fn) + ": HIP error during evaluation");
            if (probs_host && hipMemcpyAsync(probs_host + i * probs_stride + r0 * g->C, g->dz + (int64_t)i * g->rows * g->C,
                                             (size_t)rows * g->C * sizeof(float), probs_kind, g->s) != hipSuccess)
                return fail(L3_EHIP, std::string(fn) + ": HIP error during evaluation");
            if (hipStreamSynchronize(g->s) != hipSuccess) return fail(L3_EHIP, std::string(fn) + ": HIP error during evaluation");
            for (int r = 0; sums && r < rows; ++r) sums[2 * i] += ce[r], sums[2 * i + 1] += cor[r];
        }
    }
    return L3_OK;
}

// keras categorical_crossentropy's L2 term of the members `mem`: weight_decay * sum of the squared kernels; out: one per member of
// the group.  SUMSQ_MAX_SEGS / 3 members per pair of launches.
int l2_term(l3_mlp_group* g, const char* fn, const MlpMembers& mem, double* out) {
    constexpr int PER = SUMSQ_MAX_SEGS / 3;
    float sq[3 * MLP_MAX_MEMBERS];
    for (int k0 = 0; k0 < mem.n; k0 += PER) {
        const int nk = std::min(PER, mem.n - k0);
        SumsqSegs segs{};
        segs.count = 3 * nk;
        for (int k = 0; k < nk; ++k)
            for (int i = 0; i < 3; ++i)
                segs.off[3 * k + i] = mlp_member(mem, k0 + k) * g->nparam + g->off[2 * i], segs.n[3 * k + i] = g->len[2 * i];
        sumsq_multi(g->p, segs, g->sq + 3 * k0, g->sq_scratch, g->s);
    }
    if (hipMemcpyAsync(sq, g->sq, 3 * mem.n * sizeof(float), hipMemcpyDeviceToHost, g->s) != hipSuccess ||
        hipStreamSynchronize(g->s) != hipSuccess)
        return fail(L3_EHIP, std::string(fn) + ": HIP error in the L2 term");
    for (int k = 0; k < mem.n; ++k) {
        const int i = mlp_member(mem, k);
        out[i] = (double)(g->wd[i] * ((sq[3 * k] + sq[3 * k + 1]) + sq[3 * k + 2]));
    }
    return L3_OK;
}

int group_create(const char* fn, int device, int D, int C, int batch, int n_members, const float* weight_decay, const uint64_t* seed,
                 l3_mlp_group** out) {
    const std::string name(fn);
    if (!out) return fail(L3_EINVAL, name + ": out is NULL");
    *out = nullptr;
    if (D <= 0 || D > (1 << 24)) return fail(L3_EINVAL, name + ": feature width D must be in [1, 2^24]");
    if (C < 2 || C > MLP_MAX_CLASSES) return fail(L3_EINVAL, name + ": class count must be in [2, 64]");
    if (batch <= 0 || batch > MLP_MAX_BATCH) return fail(L3_EINVAL, name + ": batch must be in [1, 4096]");
    if (n_members < 1 || n_members > MLP_MAX_MEMBERS) return fail(L3_EINVAL, name + ": n_members must be in [1, 16]");
    if (!weight_decay || !seed) return fail(L3_EINVAL, name + ": weight_decay or seed is NULL");
    for (int i = 0; i < n_members; ++i)
        if (!(weight_decay[i] >= 0.f)) return fail(L3_EINVAL, name + ": weight_decay must be >= 0");
    if (!device_ok(device)) return fail(L3_EHIP, no_gpu_message(fn, device));
    l3_mlp_group* g = new l3_mlp_group();
    g->device = device, g->D = D, g->C = C, g->B = batch, g->G = n_members;
    for (int i = 0; i < n_members; ++i) g->wd[i] = weight_decay[i];
    const int64_t shape[6][2] = {{D, MLP_H1}, {MLP_H1, 1}, {MLP_H1, MLP_H2}, {MLP_H2, 1}, {MLP_H2, C}, {C, 1}};
    for (int i = 0; i < 6; ++i) {
        g->off[i] = g->nparam;
        g->len[i] = shape[i][0] * shape[i][1];
        g->nparam += (g->len[i] + 63) & ~63;       // 256-byte aligned tensors
    }
    const int rows = g->rows = std::max(batch, MLP_EVAL_ROWS);
    {
        MlpWgrad a{};
        a.nl = 3;
        a.L[0].K = D, a.L[0].N = MLP_H1, a.L[1].K = MLP_H1, a.L[1].N = MLP_H2, a.L[2].K = MLP_H2, a.L[2].N = C;
        g->total_wg = mlp_wgrad_tiles(a);
    }
    g->xin_rows = std::max<int64_t>(32, std::min<int64_t>(MLP_EVAL_ROWS, MLP_PREDICT_FLOATS / D) & ~31);
    DeviceBufs& b = g->bufs;
    const size_t G = (size_t)n_members, np = G * (size_t)g->nparam;
    g->p = b.alloc<float>(np), g->m = b.alloc<float>(np), g->v = b.alloc<float>(np);
    g->h1 = b.alloc<float>(G * rows * MLP_H1), g->h2 = b.alloc<float>(G * rows * MLP_H2);
    g->z = b.alloc<float>(G * rows * C), g->dz = b.alloc<float>(G * rows * C);
    g->dh1 = b.alloc<float>(G * batch * MLP_H1), g->dh2 = b.alloc<float>(G * batch * MLP_H2);
    g->part = b.alloc<float>(G * MLP_PART_FLOATS), g->w2part = b.alloc<float>(G * g->total_wg);
    g->ce = b.alloc<float>(G * rows), g->correct = b.alloc<float>(G * rows);
    g->sq = b.alloc<float>(3 * MLP_MAX_MEMBERS), g->sq_scratch = b.alloc<float>(SUMSQ_MAX_SEGS * SUMSQ_BLOCKS);
    g->par = b.alloc<float>(MLP_MAX_MEMBERS * MLP_MEMBER_PARS);
    g->ctr = b.alloc<int>(G * MLP_CTRS), g->yzero = b.alloc<int>(rows), g->acc = b.alloc<double>(G * 2);
    g->xin = b.alloc<float>((size_t)(g->xin_rows * D));
    const bool ok = b.ok() && hipStreamCreateWithFlags(&g->s, hipStreamNonBlocking) == hipSuccess;
    if (!ok) {
        l3_mlp_group_destroy(g);
        return fail(L3_ENOMEM, name + ": device allocation failed");
    }
    // keras glorot_uniform kernels (limit sqrt(6 / (fan_in + fan_out))) from a host generator seeded per member; zero biases
    std::vector<float> host(np, 0.f);
    for (int mb = 0; mb < n_members; ++mb) {
        uint64_t st = seed[mb];
        for (int i = 0; i < 6; i += 2) {
            const double limit = std::sqrt(6.0 / (double)(shape[i][0] + shape[i][1]));
            for (int64_t j = 0; j < g->len[i]; ++j) {
                const double u = (double)(splitmix64(st) >> 11) * (1.0 / 9007199254740992.0);     // [0, 1)
                host[mb * g->nparam + g->off[i] + j] = (float)((2.0 * u - 1.0) * limit);
            }
        }
    }
    // every fill on the handle's own stream (non-blocking: it does not order against the null stream), finished before return
    if (hipMemcpyAsync(g->p, host.data(), np * sizeof(float), hipMemcpyHostToDevice, g->s) != hipSuccess ||
        hipMemsetAsync(g->m, 0, np * sizeof(float), g->s) != hipSuccess ||
        hipMemsetAsync(g->v, 0, np * sizeof(float), g->s) != hipSuccess ||
        hipMemsetAsync(g->ctr, 0, G * MLP_CTRS * sizeof(int), g->s) != hipSuccess ||
        hipMemsetAsync(g->yzero, 0, rows * sizeof(int), g->s) != hipSuccess || hipStreamSynchronize(g->s) != hipSuccess) {
        l3_mlp_group_destroy(g);
        return fail(L3_EHIP, name + ": HIP error while initialising");
    }
    *out = g;
    return L3_OK;
}

// set_data / set_data_dev: the features come from host memory or from another buffer of this device (`kind`)
int set_data(l3_mlp_group* m, const char* fn, const float* X_train, const int32_t* y_train, int64_t n_train, const float* X_valid,
             const int32_t* y_valid, int64_t n_valid, hipMemcpyKind kind) {
    const std::string name(fn);
    if (!m) return fail(L3_EINVAL, name + ": NULL handle");
    if (n_train <= 0 || !X_train || !y_train) return fail(L3_EINVAL, name + ": need n_train > 0 rows and their labels");
    if (n_valid < 0 || (n_valid > 0 && (!X_valid || !y_valid))) return fail(L3_EINVAL, name + ": bad validation set");
    if (n_train > INT32_MAX || n_valid > INT32_MAX) return fail(L3_EINVAL, name + ": more than 2^31 - 1 rows");
    const int64_t bytes = (n_train + n_valid) * (int64_t)m->D * 4;
    if ((n_train + n_valid) > MLP_MAX_DATA_BYTES / ((int64_t)m->D * 4))
        return fail(L3_ENOMEM, name + ": " + std::to_string(bytes) + " bytes of features exceed the 64 GiB cap");
    for (int64_t i = 0; i < n_train; ++i)
        if (y_train[i] < 0 || y_train[i] >= m->C)
            return fail(L3_EINVAL, name + ": y_train[" + std::to_string(i) + "] = " + std::to_string(y_train[i]) +
                                       " outside [0, " + std::to_string(m->C) + ")");
    for (int64_t i = 0; i < n_valid; ++i)
        if (y_valid[i] < 0 || y_valid[i] >= m->C)
            return fail(L3_EINVAL, name + ": y_valid[" + std::to_string(i) + "] = " + std::to_string(y_valid[i]) +
                                       " outside [0, " + std::to_string(m->C) + ")");
    (void)hipSetDevice(m->device);
    (void)hipStreamSynchronize(m->s);
    for (void* q : {(void*)m->xtr, (void*)m->xva, (void*)m->ytr, (void*)m->yva, (void*)m->perm}) m->bufs.release(q);
    m->xtr = m->xva = nullptr, m->ytr = m->yva = m->perm = nullptr, m->ntr = m->nva = 0;
    const size_t nva = (size_t)std::max<int64_t>(1, n_valid);
    m->xtr = m->bufs.alloc<float>((size_t)(n_train * m->D)), m->ytr = m->bufs.alloc<int>((size_t)n_train);
    m->perm = m->bufs.alloc<int>((size_t)n_train);
    m->xva = m->bufs.alloc<float>(nva * m->D), m->yva = m->bufs.alloc<int>(nva);
    if (!m->xtr || !m->ytr || !m->perm || !m->xva || !m->yva)
        return fail(L3_ENOMEM, name + ": device allocation of " + std::to_string(bytes) + " bytes failed");
    if (hipMemcpyAsync(m->xtr, X_train, n_train * m->D * sizeof(float), kind, m->s) != hipSuccess ||
        hipMemcpyAsync(m->ytr, y_train, n_train * sizeof(int32_t), hipMemcpyHostToDevice, m->s) != hipSuccess ||
        (n_valid > 0 &&
         (hipMemcpyAsync(m->xva, X_valid, n_valid * m->D * sizeof(float), kind, m->s) != hipSuccess ||
          hipMemcpyAsync(m->yva, y_valid, n_valid * sizeof(int32_t), hipMemcpyHostToDevice, m->s) != hipSuccess)) ||
        hipStreamSynchronize(m->s) != hipSuccess)
        return fail(L3_EHIP, name + ": copy to the device failed");
    m->ntr = n_train, m->nva = n_valid;
    return L3_OK;
}

int set_data_dev(l3_mlp_group* m, const char* fn, const l3_feat* train, int64_t lo, int64_t hi, const int32_t* y, const l3_feat* valid,
                 int64_t vlo, int64_t vhi, const int32_t* yv) {
    const std::string name(fn);
    if (!m || !train) return fail(L3_EINVAL, name + ": NULL handle");
    if (vhi == vlo) valid = nullptr;
    for (const l3_feat* f : {train, valid})
        if (f && (f->device != m->device || f->D != m->D))
            return fail(L3_EINVAL, name + ": the feature matrix is on another device or not " + std::to_string(m->D) + " columns wide");
    if (lo < 0 || hi < lo || hi > train->n || (valid && (vlo < 0 || vhi < vlo || vhi > valid->n)))
        return fail(L3_EINVAL, name + ": a row range lies outside its matrix");
    return set_data(m, fn, train->x + lo * m->D, y, hi - lo, valid ? valid->x + vlo * m->D : nullptr, yv, valid ? vhi - vlo : 0,
                    hipMemcpyDeviceToDevice);
}

// One epoch of the live members (live null: all): the steps, seven launches each whatever the number of members, then the
// validation rows.  stats_out: 4 doubles per member of the group, NaN for a member that is not live.
int group_epoch(l3_mlp_group* m, const char* fn, const int32_t* perm, const float* lr, const int32_t* live, int64_t t0,
                double* stats_out) {
    const std::string name(fn);
    if (!m || !perm || !lr || !stats_out || t0 < 0) return fail(L3_EINVAL, name + ": NULL argument or t0 < 0");
    if (m->ntr <= 0) return fail(L3_ESTATE, name + ": no training data (" + (m->G > 1 ? "l3_mlp_group_set_data" : "l3_mlp_set_data") + ")");
    for (int64_t i = 0; i < m->ntr; ++i)
        if (perm[i] < 0 || perm[i] >= m->ntr) return fail(L3_EINVAL, name + ": perm[" + std::to_string(i) + "] outside [0, n_train)");
    MlpMembers mem{0, 0};
    for (int i = 0; i < m->G; ++i) {
        for (int k = 0; k < 4; ++k) stats_out[4 * i + k] = NAN;
        if (live && !live[i]) continue;
        mem.ids |= (uint64_t)i << (4 * mem.n++);
        m->hpar[MLP_MEMBER_PARS * i] = lr[i], m->hpar[MLP_MEMBER_PARS * i + 1] = m->wd[i], m->hpar[MLP_MEMBER_PARS * i + 2] = 2.f * m->wd[i];
    }
    if (mem.n == 0) return L3_OK;
    (void)hipSetDevice(m->device);
    if (hipMemcpyAsync(m->perm, perm, m->ntr * sizeof(int32_t), hipMemcpyHostToDevice, m->s) != hipSuccess ||
        hipMemcpyAsync(m->par, m->hpar, sizeof(m->hpar), hipMemcpyHostToDevice, m->s) != hipSuccess ||
        hipMemsetAsync(m->acc, 0, m->G * 2 * sizeof(double), m->s) != hipSuccess)
        return fail(L3_EHIP, name + ": HIP error");
    const int64_t P = m->nparam, R = m->rows;
    MlpWgrad a{};
    a.nl = 3, a.adam = 1, a.b1 = MLP_B1, a.b2 = MLP_B2, a.eps = MLP_EPS;          // lr_t, wd, l2x2: the member's, from par
    a.ce = m->ce, a.correct = m->correct, a.acc = m->acc;
    MlpWgStride ws{{0, R * MLP_H1, R * MLP_H2}, {(int64_t)m->B * MLP_H1, (int64_t)m->B * MLP_H2, R * m->C}, P, m->total_wg, MLP_CTRS, R,
                   m->par, 0.f};
    const float* xs[3] = {m->xtr, m->h1, m->h2};
    const float* dys[3] = {m->dh1, m->dh2, m->dz};
    const int Ks[3] = {m->D, MLP_H1, MLP_H2}, Ns[3] = {MLP_H1, MLP_H2, m->C};
    for (int l = 0; l < 3; ++l) {
        MlpWgLayer& L = a.L[l];
        L.x = xs[l], L.ldx = Ks[l], L.dy = dys[l], L.K = Ks[l], L.N = Ns[l];
        L.w = W(m, 2 * l), L.b = W(m, 2 * l + 1);
        L.mw = m->m + m->off[2 * l], L.mb = m->m + m->off[2 * l + 1];
        L.vw = m->v + m->off[2 * l], L.vb = m->v + m->off[2 * l + 1];
    }
    const int64_t steps = (m->ntr + m->B - 1) / m->B;
    for (int64_t st = 0; st < steps; ++st) {
        const int nb = (int)std::min<int64_t>(m->B, m->ntr - st * m->B);
        const int* idx = m->perm + st * m->B;
        const float t = (float)(t0 + st + 1);
        // keras computes lr_t = lr * this in float32 (as do_update, engine.hip); the product is the kernel's, one per member
        ws.lr_scale = sqrtf(1.f - powf(MLP_B2, t)) / (1.f - powf(MLP_B1, t));
        a.rows = nb, a.L[0].idx = idx;
        forward(m, mem, m->xtr, idx, nb);
        mlp_softmax_ce_members(m->z, m->ytr, idx, nb, m->C, 1.f / nb, nullptr, m->dz, m->ce, m->correct, mem,
                               MlpCeStride{R * m->C, 0, R * m->C, R}, m->s);
        mlp_dense_bwd_x_members(m->dz, W(m, 4), m->h2, m->dh2, nb, MLP_H2, m->C, mem,
                                MlpBwdStride{R * m->C, P, R * MLP_H2, (int64_t)m->B * MLP_H2}, m->s);
        mlp_dense_bwd_x_members(m->dh2, W(m, 2), m->h1, m->dh1, nb, MLP_H1, MLP_H2, mem,
                                MlpBwdStride{(int64_t)m->B * MLP_H2, P, R * MLP_H1, (int64_t)m->B * MLP_H1}, m->s);
        mlp_wgrad_members(a, m->w2part, m->ctr + MLP_FWD_COUNTERS, mem, ws, m->s);
    }
    std::vector<double> acc(2 * m->G), sums(2 * m->G), l2(m->G);
    if (hipMemcpyAsync(acc.data(), m->acc, acc.size() * sizeof(double), hipMemcpyDeviceToHost, m->s) != hipSuccess ||
        hipStreamSynchronize(m->s) != hipSuccess)
        return fail(L3_EHIP, name + ": HIP error during the epoch");
    for (int k = 0; k < mem.n; ++k) {
        const int i = mlp_member(mem, k);
        stats_out[4 * i] = acc[2 * i] / (double)m->ntr;
        stats_out[4 * i + 1] = acc[2 * i + 1] / (double)m->ntr;
    }
    if (m->nva > 0) {
        int rc = evaluate(m, fn, mem, m->xva, m->yva, m->nva, MLP_EVAL_ROWS, sums.data(), nullptr, 0);
        if (rc == L3_OK) rc = l2_term(m, fn, mem, l2.data());
        if (rc != L3_OK) return rc;
        for (int k = 0; k < mem.n; ++k) {
            const int i = mlp_member(mem, k);
            stats_out[4 * i + 2] = sums[2 * i] / (double)m->nva + l2[i];
            stats_out[4 * i + 3] = sums[2 * i + 1] / (double)m->nva;
        }
    }
    return L3_OK;
}

// softmax probabilities of n rows through every member, member i's (n, C) at probs_out + i * n * C.  The rows are host rows X,
// staged block by block, or device rows xd; either way in blocks of xin_rows, so that every forward launch has the same shape
// (and split-K order) whichever way the rows come.  probs_kind: where probs_out is (evaluate).
int group_predict(l3_mlp_group* m, const char* fn, const float* X, const float* xd, int64_t n, float* probs_out,
                  hipMemcpyKind probs_kind = hipMemcpyDeviceToHost) {
    (void)hipSetDevice(m->device);
    const MlpMembers mem = all_members(m);
    for (int64_t r0 = 0; r0 < n; r0 += m->xin_rows) {
        const int64_t rows = std::min(m->xin_rows, n - r0);
        if (X && hipMemcpyAsync(m->xin, X + r0 * m->D, rows * m->D * sizeof(float), hipMemcpyHostToDevice, m->s) != hipSuccess)
            return fail(L3_EHIP, std::string(fn) + ": copy to the device failed");
        const int rc = evaluate(m, fn, mem, X ? m->xin : xd + r0 * m->D, nullptr, rows, rows, nullptr, probs_out + r0 * m->C, n * m->C,
                                probs_kind);
        if (rc != L3_OK) return rc;
    }
    return L3_OK;
}

int group_predict_dev(l3_mlp_group* m, const char* fn, const l3_feat* x, int64_t lo, int64_t hi, float* probs_out) {
    const std::string name(fn);
    if (!m || !x || !probs_out || hi <= lo) return fail(L3_EINVAL, name + ": NULL argument or no rows");
    if (x->device != m->device || x->D != m->D)
        return fail(L3_EINVAL, name + ": the feature matrix is on another device or not " + std::to_string(m->D) + " columns wide");
    if (lo < 0 || hi > x->n) return fail(L3_EINVAL, name + ": rows [lo, hi) outside the matrix");
    return group_predict(m, fn, nullptr, x->x + lo * m->D, hi - lo, probs_out);
}

int64_t param_count(const l3_mlp_group* m) {
    int64_t n = 0;
    for (int i = 0; i < 6; ++i) n += m->len[i];
    return n;
}

// a member's six tensors, keras order, between its arena and host memory
int copy_weights(l3_mlp_group* m, const char* fn, int member, float* host, int64_t n, bool to_host) {
    const std::string name(fn);
    if (!m || !host || member < 0 || member >= m->G || n != param_count(m))
        return fail(L3_EINVAL, name + ": NULL, no such member or wrong element count");
    (void)hipSetDevice(m->device);
    if (hipStreamSynchronize(m->s) != hipSuccess) return fail(L3_EHIP, name + ": HIP error");
    for (int i = 0; i < 6; ++i) {
        float* dev = m->p + member * m->nparam + m->off[i];
        if (hipMemcpyAsync(to_host ? host : dev, to_host ? dev : host, m->len[i] * sizeof(float),
                           to_host ? hipMemcpyDeviceToHost : hipMemcpyHostToDevice, m->s) != hipSuccess ||
            hipStreamSynchronize(m->s) != hipSuccess)
            return fail(L3_EHIP, name + ": copy failed");
        host += m->len[i];
    }
    return L3_OK;
}
}  // namespace

extern "C" {

// ---- l3_mlp_group ----------------------------------------------------------------------------------------------------------------
int l3_mlp_group_create(int device, int D, int C, int batch, int n_members, const float* weight_decay, const uint64_t* seed,
                        l3_mlp_group** out) {
    return group_create("l3_mlp_group_create", device, D, C, batch, n_members, weight_decay, seed, out);
}

void l3_mlp_group_destroy(l3_mlp_group* g) {
    if (!g) return;
    (void)hipSetDevice(g->device);
    if (g->s) (void)hipStreamSynchronize(g->s);
    if (g->s) (void)hipStreamDestroy(g->s);
    delete g;
}

int64_t l3_mlp_group_param_count(const l3_mlp_group* g) { return g ? param_count(g) : L3_EINVAL; }

int l3_mlp_group_set_data(l3_mlp_group* g, const float* X_train, const int32_t* y_train, int64_t n_train, const float* X_valid,
                          const int32_t* y_valid, int64_t n_valid) {
    return set_data(g, "l3_mlp_group_set_data", X_train, y_train, n_train, X_valid, y_valid, n_valid, hipMemcpyHostToDevice);
}

int l3_mlp_group_set_data_dev(l3_mlp_group* g, const l3_feat* train, int64_t lo, int64_t hi, const int32_t* y, const l3_feat* valid,
                              int64_t vlo, int64_t vhi, const int32_t* yv) {
    return set_data_dev(g, "l3_mlp_group_set_data_dev", train, lo, hi, y, valid, vlo, vhi, yv);
}

int l3_mlp_group_epoch(l3_mlp_group* g, const int32_t* perm, const float* lr, const int32_t* live, int64_t t0, double* stats_out) {
    if (!live) return fail(L3_EINVAL, "l3_mlp_group_epoch: NULL argument or t0 < 0");
    return group_epoch(g, "l3_mlp_group_epoch", perm, lr, live, t0, stats_out);
}

int l3_mlp_group_keep_best(l3_mlp_group* g, uint32_t mask) {
    if (!g || (mask >> g->G) != 0) return fail(L3_EINVAL, "l3_mlp_group_keep_best: NULL handle or a mask bit past the last member");
    (void)hipSetDevice(g->device);
    if (!g->best && mask) g->best = g->bufs.alloc<float>((size_t)g->G * g->nparam);
    if (!g->best && mask) return fail(L3_ENOMEM, "l3_mlp_group_keep_best: device allocation failed");
    for (int i = 0; i < g->G; ++i) {
        if (!(mask >> i & 1)) continue;
        if (hipMemcpyAsync(g->best + i * g->nparam, g->p + i * g->nparam, g->nparam * sizeof(float), hipMemcpyDeviceToDevice, g->s) !=
            hipSuccess)
            return fail(L3_EHIP, "l3_mlp_group_keep_best: copy failed");
        g->kept[i] = true;
    }
    if (hipStreamSynchronize(g->s) != hipSuccess) return fail(L3_EHIP, "l3_mlp_group_keep_best: copy failed");
    return L3_OK;
}

int l3_mlp_group_restore_best(l3_mlp_group* g, uint32_t mask) {
    if (!g || (mask >> g->G) != 0) return fail(L3_EINVAL, "l3_mlp_group_restore_best: NULL handle or a mask bit past the last member");
    for (int i = 0; i < g->G; ++i)
        if ((mask >> i & 1) && !g->kept[i])
            return fail(L3_ESTATE, "l3_mlp_group_restore_best: member " + std::to_string(i) + " has no kept weights (l3_mlp_group_keep_best)");
    (void)hipSetDevice(g->device);
    for (int i = 0; i < g->G; ++i)
        if ((mask >> i & 1) && hipMemcpyAsync(g->p + i * g->nparam, g->best + i * g->nparam, g->nparam * sizeof(float),
                                              hipMemcpyDeviceToDevice, g->s) != hipSuccess)
            return fail(L3_EHIP, "l3_mlp_group_restore_best: copy failed");
    if (hipStreamSynchronize(g->s) != hipSuccess) return fail(L3_EHIP, "l3_mlp_group_restore_best: copy failed");
    return L3_OK;
}

int l3_mlp_group_predict(l3_mlp_group* g, const float* X, int64_t n, float* probs_out) {
    if (!g || !X || !probs_out || n <= 0) return fail(L3_EINVAL, "l3_mlp_group_predict: NULL argument or n <= 0");
    return group_predict(g, "l3_mlp_group_predict", X, nullptr, n, probs_out);
}

int l3_mlp_group_predict_dev(l3_mlp_group* g, const l3_feat* x, int64_t lo, int64_t hi, float* probs_out) {
    return group_predict_dev(g, "l3_mlp_group_predict_dev", x, lo, hi, probs_out);
}

int l3_mlp_group_predict_resident(l3_mlp_group* g, int valid, float* probs_out) {
    if (!g || !probs_out || (valid != 0 && valid != 1))
        return fail(L3_EINVAL, "l3_mlp_group_predict_resident: NULL argument, or valid is neither 0 nor 1");
    const int64_t n = valid ? g->nva : g->ntr;
    if (n <= 0) return fail(L3_ESTATE, "l3_mlp_group_predict_resident: no such rows (l3_mlp_group_set_data)");
    return group_predict(g, "l3_mlp_group_predict_resident", nullptr, valid ? g->xva : g->xtr, n, probs_out);
}

int l3_mlp_group_get_weights(l3_mlp_group* g, int member, float* dst, int64_t n) {
    return copy_weights(g, "l3_mlp_group_get_weights", member, dst, n, true);
}

int l3_mlp_group_set_weights(l3_mlp_group* g, int member, const float* src, int64_t n) {
    return copy_weights(g, "l3_mlp_group_set_weights", member, const_cast<float*>(src), n, false);
}

// ---- l3_mlp: a group of one ------------------------------------------------------------------------------------------------------
int l3_mlp_create(int device, int D, int C, int batch, float weight_decay, uint64_t seed, l3_mlp** out) {
    if (!out) return fail(L3_EINVAL, "l3_mlp_create: out is NULL");
    *out = nullptr;
    l3_mlp_group* g = nullptr;
    const int rc = group_create("l3_mlp_create", device, D, C, batch, 1, &weight_decay, &seed, &g);
    if (rc != L3_OK) return rc;
    *out = new l3_mlp{g};
    return L3_OK;
}

void l3_mlp_destroy(l3_mlp* m) {
    if (!m) return;
    l3_mlp_group_destroy(m->g);
    delete m;
}

int64_t l3_mlp_param_count(const l3_mlp* m) { return m ? param_count(m->g) : L3_EINVAL; }

int l3_mlp_set_data(l3_mlp* m, const float* X_train, const int32_t* y_train, int64_t n_train, const float* X_valid,
                    const int32_t* y_valid, int64_t n_valid) {
    return set_data(m ? m->g : nullptr, "l3_mlp_set_data", X_train, y_train, n_train, X_valid, y_valid, n_valid, hipMemcpyHostToDevice);
}

int l3_mlp_set_data_dev(l3_mlp* m, const l3_feat* train, int64_t lo, int64_t hi, const int32_t* y, const l3_feat* valid, int64_t vlo,
                        int64_t vhi, const int32_t* yv) {
    return set_data_dev(m ? m->g : nullptr, "l3_mlp_set_data_dev", train, lo, hi, y, valid, vlo, vhi, yv);
}

int l3_mlp_epoch(l3_mlp* m, const int32_t* perm, float lr, int64_t t0, double* stats_out) {
    return group_epoch(m ? m->g : nullptr, "l3_mlp_epoch", perm, &lr, nullptr, t0, stats_out);
}

int l3_mlp_predict(l3_mlp* m, const float* X, int64_t n, float* probs_out) {
    if (!m || !X || !probs_out || n <= 0) return fail(L3_EINVAL, "l3_mlp_predict: NULL argument or n <= 0");
    return group_predict(m->g, "l3_mlp_predict", X, nullptr, n, probs_out);
}

int l3_mlp_predict_dev(l3_mlp* m, const l3_feat* x, int64_t lo, int64_t hi, float* probs_out) {
    return group_predict_dev(m ? m->g : nullptr, "l3_mlp_predict_dev", x, lo, hi, probs_out);
}

int l3_mlp_predict_files_dev(l3_mlp* m, const l3_feat* x, const int64_t* file_idxs, int64_t n_files, float* file_mean,
                             int32_t* file_pred) {
    const std::string name("l3_mlp_predict_files_dev");
    if (!m || !x || !file_idxs) return fail(L3_EINVAL, name + ": NULL argument");
    l3_mlp_group* g = m->g;
    if (x->device != g->device || x->D != g->D)
        return fail(L3_EINVAL, name + ": the feature matrix is on another device or not " + std::to_string(g->D) + " columns wide");
    const std::string bad = mlp_file_ranges_error(file_idxs, n_files, x->n);
    if (!bad.empty()) return fail(L3_EINVAL, name + ": " + bad);
    (void)hipSetDevice(g->device);
    const int C = g->C;
    float* probs = g->bufs.alloc<float>((size_t)(x->n * C));
    int64_t* files = g->bufs.put(file_idxs, (size_t)(2 * n_files), g->s);
    float* mean = g->bufs.alloc<float>((size_t)(n_files * C));
    int* pred = g->bufs.alloc<int>((size_t)n_files);
    int rc = probs && files && mean && pred ? L3_OK : fail(L3_ENOMEM, name + ": device allocation failed");
    if (rc == L3_OK) rc = group_predict(g, "l3_mlp_predict_files_dev", nullptr, x->x, x->n, probs, hipMemcpyDeviceToDevice);
    if (rc == L3_OK) {
        mlp_file_mean(probs, C, files, n_files, mean, pred, g->s);
        if ((file_mean && hipMemcpyAsync(file_mean, mean, (size_t)(n_files * C) * sizeof(float), hipMemcpyDeviceToHost, g->s) != hipSuccess) ||
            (file_pred && hipMemcpyAsync(file_pred, pred, (size_t)n_files * sizeof(int), hipMemcpyDeviceToHost, g->s) != hipSuccess))
            rc = fail(L3_EHIP, name + ": copy from the device failed");
    }
    // also after a failure: the stream has let go of the host table and of the buffers
    if ((hipStreamSynchronize(g->s) != hipSuccess || hipGetLastError() != hipSuccess) && rc == L3_OK) rc = fail(L3_EHIP, name + ": HIP error");
    g->bufs.release(probs), g->bufs.release(files), g->bufs.release(mean), g->bufs.release(pred);
    return rc;
}

int l3_mlp_get_weights(l3_mlp* m, float* dst, int64_t n) { return copy_weights(m ? m->g : nullptr, "l3_mlp_get_weights", 0, dst, n, true); }

int l3_mlp_set_weights(l3_mlp* m, const float* src, int64_t n) {
    return copy_weights(m ? m->g : nullptr, "l3_mlp_set_weights", 0, const_cast<float*>(src), n, false);
}

}  // extern "C"
