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
};
__global__ __launch_bounds__(256) void mlp_fwd_kernel(MlpFwdArgs a) {
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

void mlp_dense_fwd(const float* x, const int* idx, int64_t ldx, const float* w, const float* b, float* y, int rows, int K, int N,
                   int relu, float* part, int* ctr, hipStream_t s) {
    MlpFwdArgs a{x, idx, ldx, w, b, y, part, ctr, rows, K, N, 1, K, relu, 0};
    fwd_split(rows, K, N, &a.S, &a.kc);
    a.vec = (ldx % 4 == 0 && a.kc % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0) ? 1 : 0;
    const int waves = ((rows + 31) / 32) * ((N + 31) / 32) * a.S;
    hipLaunchKernelGGL(mlp_fwd_kernel, dim3((waves + 3) / 4), dim3(256), 0, s, a);
}

// ---- data gradient: dX = (dY W^T) [h > 0] -------------------------------------------------------------------------------------
// One wave per 32x32 tile of dX (rows x K); the sum runs over N: lane (r, h) holds A = dY[row r][n0 + 4h + j], B = W[k r][n0 + 4h + j].
__global__ __launch_bounds__(256) void mlp_bwd_x_kernel(const float* dy, const float* w, const float* hm, float* dx, int rows, int K,
                                                        int N) {
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
void mlp_dense_bwd_x(const float* dy, const float* w, const float* h, float* dx, int rows, int K, int N, hipStream_t s) {
    const int waves = ((rows + 31) / 32) * ((K + 31) / 32);
    hipLaunchKernelGGL(mlp_bwd_x_kernel, dim3((waves + 3) / 4), dim3(256), 0, s, dy, w, h, dx, rows, K, N);
}

// ---- softmax + categorical cross-entropy (keras 2.0.9 / TF 1.4) -----------------------------------------------------------------
// softmax_ce_kernel (elementwise.hip, C = 2) for any C <= 64: p = softmax(z); q = p / sum(p); c = clip(q, 1e-7, 1 - 1e-7);
// loss = -sum t log c; the gradient flows through the normalisation and through the clip where q lies inside it.
__global__ __launch_bounds__(256) void mlp_softmax_ce_kernel(const float* z, const int* labels, const int* idx, int rows, int C,
                                                             float gscale, float* probs, float* dz, float* ce, float* correct) {
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
void mlp_softmax_ce(const float* z, const int* labels, const int* idx, int rows, int C, float gscale, float* probs, float* dz,
                    float* ce, float* correct, hipStream_t s) {
    hipLaunchKernelGGL(mlp_softmax_ce_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, z, labels, idx, rows, C, gscale, probs, dz, ce,
                       correct);
}

// ---- weight gradient + L2 + Adam ------------------------------------------------------------------------------------------------
// Layer l's waves: ceil(K/32) * ceil(N/32) weight tiles, then ceil(N/64) bias tiles.  Weight tile (kt, nt): the sum runs over the
// batch, lane (r, h) holding A = X[idx[b0 + 4h + j]][kt*32 + r] and B = dY[b0 + 4h + j][nt*32 + r].  Bias tile: lane n sums its
// column of dY in row order.
__device__ __forceinline__ int wg_tiles_w(const MlpWgLayer& L) { return ((L.K + 31) >> 5) * ((L.N + 31) >> 5); }
__device__ __forceinline__ int wg_tiles_b(const MlpWgLayer& L) { return (L.N + 63) >> 6; }

// adam_kernel's update of one element, in its order of operations (gscale 1: exact)
__device__ __forceinline__ float adam_one(float w, float g, float* mp, float* vp, bool l2, const MlpWgrad& a) {
    float gi = g * 1.f;
    if (l2) gi = fmaf(a.l2x2, w, gi);
    const float mi = a.b1 * *mp + (1.f - a.b1) * gi;
    const float vi = a.b2 * *vp + (1.f - a.b2) * gi * gi;
    *mp = mi;
    *vp = vi;
    return w - a.lr_t * mi / (sqrtf(vi) + a.eps);
}

__global__ __launch_bounds__(256) void mlp_wgrad_kernel(MlpWgrad a, float* w2part, int* ctr, int total) {
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int wv = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wv >= total) return;
    // the wave's layer, picked with selects (a dynamic index into the kernel arguments would copy them to scratch)
    int t = wv;
    const int n0 = wg_tiles_w(a.L[0]) + wg_tiles_b(a.L[0]), n1 = wg_tiles_w(a.L[1]) + wg_tiles_b(a.L[1]);
    const int l = (a.nl > 1 && t >= n0) ? ((a.nl > 2 && t >= n0 + n1) ? 2 : 1) : 0;
    t -= l == 0 ? 0 : l == 1 ? n0 : n0 + n1;
    const MlpWgLayer L = l == 0 ? a.L[0] : l == 1 ? a.L[1] : a.L[2];
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
                        L.w[o] = adam_one(w, acc[i], L.mw + o, L.vw + o, true, a);
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
                L.b[n] = adam_one(L.b[n], g, L.mb + n, L.vb + n, false, a);
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
        double sc = 0.0, sk = 0.0;
        for (int i = lane; i < a.rows; i += 64) {
            sc += (double)__builtin_nontemporal_load(a.ce + i);
            sk += (double)__builtin_nontemporal_load(a.correct + i);
        }
        sc = wave_sum_d(sc);
        sk = wave_sum_d(sk);
        if (lane == 0) {
            const float loss = (float)(sc / a.rows) + a.wd * (float)sw;     // keras: mean ce + wd * sum W^2, in float32
            a.acc[0] += (double)loss * a.rows;
            a.acc[1] += sk;
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
void mlp_wgrad(const MlpWgrad& a, float* w2part, int* ctr, hipStream_t s) {
    const int total = mlp_wgrad_tiles(a);
    hipLaunchKernelGGL(mlp_wgrad_kernel, dim3((total + 3) / 4), dim3(256), 0, s, a, w2part, ctr, total);
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

struct l3_mlp {
    int device = 0, D = 0, C = 0, B = 0;
    float wd = 0.f;
    hipStream_t s = nullptr;
    int64_t off[6] = {}, len[6] = {}, nparam = 0;       // W1 b1 W2 b2 W3 b3 in the arenas (keras order)
    float *p = nullptr, *m = nullptr, *v = nullptr;
    float *h1 = nullptr, *h2 = nullptr, *z = nullptr, *dz = nullptr, *dh1 = nullptr, *dh2 = nullptr, *xin = nullptr;
    float *part = nullptr, *w2part = nullptr, *ce = nullptr, *correct = nullptr, *sq = nullptr, *sq_scratch = nullptr;
    int *ctr = nullptr, *perm = nullptr, *ytr = nullptr, *yva = nullptr, *yzero = nullptr;
    double* acc = nullptr;
    float *xtr = nullptr, *xva = nullptr;
    int64_t ntr = 0, nva = 0, perm_cap = 0, xin_rows = 0;
    DeviceBufs bufs;
};

namespace {
float* W(l3_mlp* m, int i) { return m->p + m->off[i]; }

void forward(l3_mlp* m, const float* x, const int* idx, int rows) {
    mlp_dense_fwd(x, idx, m->D, W(m, 0), W(m, 1), m->h1, rows, m->D, MLP_H1, 1, m->part, m->ctr, m->s);
    mlp_dense_fwd(m->h1, nullptr, MLP_H1, W(m, 2), W(m, 3), m->h2, rows, MLP_H1, MLP_H2, 1, m->part, m->ctr, m->s);
    mlp_dense_fwd(m->h2, nullptr, MLP_H2, W(m, 4), W(m, 5), m->z, rows, MLP_H2, m->C, 0, m->part, m->ctr, m->s);
}

// sum of ce and of correct over rows [0, n) of x (resident, labels y), MLP_EVAL_ROWS at a time; probs_host (n, C) when given
int evaluate(l3_mlp* m, const float* x, const int* y, int64_t n, double* ce_sum, double* correct_sum, float* probs_host) {
    std::vector<float> ce(MLP_EVAL_ROWS), cor(MLP_EVAL_ROWS);
    double sc = 0.0, sk = 0.0;
    for (int64_t r0 = 0; r0 < n; r0 += MLP_EVAL_ROWS) {
        const int rows = (int)std::min<int64_t>(MLP_EVAL_ROWS, n - r0);
        forward(m, x + r0 * m->D, nullptr, rows);
        mlp_softmax_ce(m->z, y ? y + r0 : m->yzero, nullptr, rows, m->C, 1.f, probs_host ? m->dz : nullptr, nullptr, m->ce,
                       m->correct, m->s);
        if (hipMemcpyAsync(ce.data(), m->ce, rows * sizeof(float), hipMemcpyDeviceToHost, m->s) != hipSuccess ||
            hipMemcpyAsync(cor.data(), m->correct, rows * sizeof(float), hipMemcpyDeviceToHost, m->s) != hipSuccess ||
            (probs_host && hipMemcpyAsync(probs_host + r0 * m->C, m->dz, (size_t)rows * m->C * sizeof(float),
                                          hipMemcpyDeviceToHost, m->s) != hipSuccess) ||
            hipStreamSynchronize(m->s) != hipSuccess)
            return fail(L3_EHIP, "l3_mlp: HIP error during evaluation");
        for (int i = 0; i < rows; ++i) sc += ce[i], sk += cor[i];
    }
    *ce_sum = sc;
    *correct_sum = sk;
    return L3_OK;
}

// keras categorical_crossentropy's L2 term: weight_decay * sum of the squared kernels
int l2_term(l3_mlp* m, double* out) {
    SumsqSegs segs{};
    segs.count = 3;
    for (int i = 0; i < 3; ++i) segs.off[i] = m->off[2 * i], segs.n[i] = m->len[2 * i];
    sumsq_multi(m->p, segs, m->sq, m->sq_scratch, m->s);
    float sq[3];
    if (hipMemcpyAsync(sq, m->sq, sizeof(sq), hipMemcpyDeviceToHost, m->s) != hipSuccess || hipStreamSynchronize(m->s) != hipSuccess)
        return fail(L3_EHIP, "l3_mlp: HIP error in the L2 term");
    *out = (double)(m->wd * ((sq[0] + sq[1]) + sq[2]));
    return L3_OK;
}

// l3_mlp_set_data / l3_mlp_set_data_dev: the features come from host memory or from another buffer of this device (`kind`)
int set_data(l3_mlp* m, const char* fn, const float* X_train, const int32_t* y_train, int64_t n_train, const float* X_valid,
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
}  // namespace

extern "C" {

int l3_mlp_create(int device, int D, int C, int batch, float weight_decay, uint64_t seed, l3_mlp** out) {
    if (!out) return fail(L3_EINVAL, "l3_mlp_create: out is NULL");
    *out = nullptr;
    if (D <= 0 || D > (1 << 24)) return fail(L3_EINVAL, "l3_mlp_create: feature width D must be in [1, 2^24]");
    if (C < 2 || C > MLP_MAX_CLASSES) return fail(L3_EINVAL, "l3_mlp_create: class count must be in [2, 64]");
    if (batch <= 0 || batch > MLP_MAX_BATCH) return fail(L3_EINVAL, "l3_mlp_create: batch must be in [1, 4096]");
    if (!(weight_decay >= 0.f)) return fail(L3_EINVAL, "l3_mlp_create: weight_decay must be >= 0");
    if (!device_ok(device)) return fail(L3_EHIP, no_gpu_message("l3_mlp_create", device));
    l3_mlp* m = new l3_mlp();
    m->device = device, m->D = D, m->C = C, m->B = batch, m->wd = weight_decay;
    const int64_t shape[6][2] = {{D, MLP_H1}, {MLP_H1, 1}, {MLP_H1, MLP_H2}, {MLP_H2, 1}, {MLP_H2, C}, {C, 1}};
    for (int i = 0; i < 6; ++i) {
        m->off[i] = m->nparam;
        m->len[i] = shape[i][0] * shape[i][1];
        m->nparam += (m->len[i] + 63) & ~63;       // 256-byte aligned tensors
    }
    const int rows = std::max(batch, MLP_EVAL_ROWS);
    int total_wg = 0;
    {
        MlpWgrad a{};
        a.nl = 3;
        a.L[0].K = D, a.L[0].N = MLP_H1, a.L[1].K = MLP_H1, a.L[1].N = MLP_H2, a.L[2].K = MLP_H2, a.L[2].N = C;
        total_wg = mlp_wgrad_tiles(a);
    }
    m->xin_rows = std::max<int64_t>(32, std::min<int64_t>(MLP_EVAL_ROWS, MLP_PREDICT_FLOATS / D) & ~31);
    DeviceBufs& b = m->bufs;
    const size_t np = (size_t)m->nparam;
    m->p = b.alloc<float>(np), m->m = b.alloc<float>(np), m->v = b.alloc<float>(np);
    m->h1 = b.alloc<float>((size_t)rows * MLP_H1), m->h2 = b.alloc<float>((size_t)rows * MLP_H2);
    m->z = b.alloc<float>((size_t)rows * C), m->dz = b.alloc<float>((size_t)rows * C);
    m->dh1 = b.alloc<float>((size_t)batch * MLP_H1), m->dh2 = b.alloc<float>((size_t)batch * MLP_H2);
    m->part = b.alloc<float>(MLP_PART_FLOATS), m->w2part = b.alloc<float>(total_wg);
    m->ce = b.alloc<float>(rows), m->correct = b.alloc<float>(rows);
    m->sq = b.alloc<float>(4), m->sq_scratch = b.alloc<float>(SUMSQ_MAX_SEGS * SUMSQ_BLOCKS);
    m->ctr = b.alloc<int>(MLP_FWD_COUNTERS + 1), m->yzero = b.alloc<int>(rows), m->acc = b.alloc<double>(2);
    m->xin = b.alloc<float>((size_t)(m->xin_rows * D));
    const bool ok = b.ok() && hipStreamCreateWithFlags(&m->s, hipStreamNonBlocking) == hipSuccess;
    if (!ok) {
        l3_mlp_destroy(m);
        return fail(L3_ENOMEM, "l3_mlp_create: device allocation failed");
    }
    // keras glorot_uniform kernels (limit sqrt(6 / (fan_in + fan_out))) from a seeded host generator; zero biases
    std::vector<float> host(m->nparam, 0.f);
    uint64_t st = seed;
    for (int i = 0; i < 6; i += 2) {
        const double limit = std::sqrt(6.0 / (double)(shape[i][0] + shape[i][1]));
        for (int64_t j = 0; j < m->len[i]; ++j) {
            const double u = (double)(splitmix64(st) >> 11) * (1.0 / 9007199254740992.0);     // [0, 1)
            host[m->off[i] + j] = (float)((2.0 * u - 1.0) * limit);
        }
    }
    // every fill on the handle's own stream (non-blocking: it does not order against the null stream), finished before return
    if (hipMemcpyAsync(m->p, host.data(), m->nparam * sizeof(float), hipMemcpyHostToDevice, m->s) != hipSuccess ||
        hipMemsetAsync(m->m, 0, m->nparam * sizeof(float), m->s) != hipSuccess ||
        hipMemsetAsync(m->v, 0, m->nparam * sizeof(float), m->s) != hipSuccess ||
        hipMemsetAsync(m->ctr, 0, (MLP_FWD_COUNTERS + 1) * sizeof(int), m->s) != hipSuccess ||
        hipMemsetAsync(m->yzero, 0, rows * sizeof(int), m->s) != hipSuccess || hipStreamSynchronize(m->s) != hipSuccess) {
        l3_mlp_destroy(m);
        return fail(L3_EHIP, "l3_mlp_create: HIP error while initialising");
    }
    *out = m;
    return L3_OK;
}

void l3_mlp_destroy(l3_mlp* m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    if (m->s) (void)hipStreamSynchronize(m->s);
    if (m->s) (void)hipStreamDestroy(m->s);
    delete m;
}

int64_t l3_mlp_param_count(const l3_mlp* m) {
    if (!m) return L3_EINVAL;
    int64_t n = 0;
    for (int i = 0; i < 6; ++i) n += m->len[i];
    return n;
}

int l3_mlp_set_data(l3_mlp* m, const float* X_train, const int32_t* y_train, int64_t n_train, const float* X_valid,
                    const int32_t* y_valid, int64_t n_valid) {
    return set_data(m, "l3_mlp_set_data", X_train, y_train, n_train, X_valid, y_valid, n_valid, hipMemcpyHostToDevice);
}

int l3_mlp_set_data_dev(l3_mlp* m, const l3_feat* train, int64_t lo, int64_t hi, const int32_t* y, const l3_feat* valid, int64_t vlo,
                        int64_t vhi, const int32_t* yv) {
    if (!m || !train) return fail(L3_EINVAL, "l3_mlp_set_data_dev: NULL handle");
    if (vhi == vlo) valid = nullptr;
    for (const l3_feat* f : {train, valid})
        if (f && (f->device != m->device || f->D != m->D))
            return fail(L3_EINVAL, "l3_mlp_set_data_dev: the feature matrix is on another device or not " + std::to_string(m->D) +
                                       " columns wide");
    if (lo < 0 || hi < lo || hi > train->n || (valid && (vlo < 0 || vhi < vlo || vhi > valid->n)))
        return fail(L3_EINVAL, "l3_mlp_set_data_dev: a row range lies outside its matrix");
    return set_data(m, "l3_mlp_set_data_dev", train->x + lo * m->D, y, hi - lo, valid ? valid->x + vlo * m->D : nullptr, yv,
                    valid ? vhi - vlo : 0, hipMemcpyDeviceToDevice);
}

int l3_mlp_epoch(l3_mlp* m, const int32_t* perm, float lr, int64_t t0, double* stats_out) {
    if (!m || !perm || !stats_out || t0 < 0) return fail(L3_EINVAL, "l3_mlp_epoch: NULL argument or t0 < 0");
    if (m->ntr <= 0) return fail(L3_ESTATE, "l3_mlp_epoch: no training data (l3_mlp_set_data)");
    for (int64_t i = 0; i < m->ntr; ++i)
        if (perm[i] < 0 || perm[i] >= m->ntr)
            return fail(L3_EINVAL, "l3_mlp_epoch: perm[" + std::to_string(i) + "] outside [0, n_train)");
    (void)hipSetDevice(m->device);
    if (hipMemcpyAsync(m->perm, perm, m->ntr * sizeof(int32_t), hipMemcpyHostToDevice, m->s) != hipSuccess ||
        hipMemsetAsync(m->acc, 0, 2 * sizeof(double), m->s) != hipSuccess)
        return fail(L3_EHIP, "l3_mlp_epoch: HIP error");
    MlpWgrad a{};
    a.nl = 3, a.adam = 1, a.l2x2 = 2.f * m->wd, a.b1 = MLP_B1, a.b2 = MLP_B2, a.eps = MLP_EPS, a.wd = m->wd;
    a.ce = m->ce, a.correct = m->correct, a.acc = m->acc;
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
        // keras computes lr_t in float32 (as do_update, engine.hip)
        a.lr_t = lr * (sqrtf(1.f - powf(MLP_B2, t)) / (1.f - powf(MLP_B1, t)));
        a.rows = nb, a.L[0].idx = idx;
        forward(m, m->xtr, idx, nb);
        mlp_softmax_ce(m->z, m->ytr, idx, nb, m->C, 1.f / nb, nullptr, m->dz, m->ce, m->correct, m->s);
        mlp_dense_bwd_x(m->dz, W(m, 4), m->h2, m->dh2, nb, MLP_H2, m->C, m->s);
        mlp_dense_bwd_x(m->dh2, W(m, 2), m->h1, m->dh1, nb, MLP_H1, MLP_H2, m->s);
        mlp_wgrad(a, m->w2part, m->ctr + MLP_FWD_COUNTERS, m->s);
    }
    double acc[2];
    if (hipMemcpyAsync(acc, m->acc, sizeof(acc), hipMemcpyDeviceToHost, m->s) != hipSuccess || hipStreamSynchronize(m->s) != hipSuccess)
        return fail(L3_EHIP, "l3_mlp_epoch: HIP error during the epoch");
    stats_out[0] = acc[0] / (double)m->ntr;
    stats_out[1] = acc[1] / (double)m->ntr;
    stats_out[2] = stats_out[3] = NAN;
    if (m->nva > 0) {
        double sc = 0.0, sk = 0.0, l2 = 0.0;
        int rc = evaluate(m, m->xva, m->yva, m->nva, &sc, &sk, nullptr);
        if (rc == L3_OK) rc = l2_term(m, &l2);
        if (rc != L3_OK) return rc;
        stats_out[2] = sc / (double)m->nva + l2;
        stats_out[3] = sk / (double)m->nva;
    }
    return L3_OK;
}

int l3_mlp_predict(l3_mlp* m, const float* X, int64_t n, float* probs_out) {
    if (!m || !X || !probs_out || n <= 0) return fail(L3_EINVAL, "l3_mlp_predict: NULL argument or n <= 0");
    (void)hipSetDevice(m->device);
    for (int64_t r0 = 0; r0 < n; r0 += m->xin_rows) {
        const int64_t rows = std::min(m->xin_rows, n - r0);
        double sc, sk;
        if (hipMemcpyAsync(m->xin, X + r0 * m->D, rows * m->D * sizeof(float), hipMemcpyHostToDevice, m->s) != hipSuccess)
            return fail(L3_EHIP, "l3_mlp_predict: copy to the device failed");
        const int rc = evaluate(m, m->xin, nullptr, rows, &sc, &sk, probs_out + r0 * m->C);
        if (rc != L3_OK) return rc;
    }
    return L3_OK;
}

int l3_mlp_predict_dev(l3_mlp* m, const l3_feat* x, int64_t lo, int64_t hi, float* probs_out) {
    if (!m || !x || !probs_out || hi <= lo) return fail(L3_EINVAL, "l3_mlp_predict_dev: NULL argument or no rows");
    if (x->device != m->device || x->D != m->D)
        return fail(L3_EINVAL, "l3_mlp_predict_dev: the feature matrix is on another device or not " + std::to_string(m->D) +
                                   " columns wide");
    if (lo < 0 || hi > x->n) return fail(L3_EINVAL, "l3_mlp_predict_dev: rows [lo, hi) outside the matrix");
    (void)hipSetDevice(m->device);
    const int64_t n = hi - lo;
    // l3_mlp_predict's row blocks, so that every forward launch has its shape (and its split-K order)
    for (int64_t r0 = 0; r0 < n; r0 += m->xin_rows) {
        const int64_t rows = std::min(m->xin_rows, n - r0);
        double sc, sk;
        const int rc = evaluate(m, x->x + (lo + r0) * m->D, nullptr, rows, &sc, &sk, probs_out + r0 * m->C);
        if (rc != L3_OK) return rc;
    }
    return L3_OK;
}

int l3_mlp_get_weights(l3_mlp* m, float* dst, int64_t n) {
    if (!m || !dst || n != l3_mlp_param_count(m)) return fail(L3_EINVAL, "l3_mlp_get_weights: NULL or wrong element count");
    (void)hipSetDevice(m->device);
    if (hipStreamSynchronize(m->s) != hipSuccess) return fail(L3_EHIP, "l3_mlp_get_weights: HIP error");
    for (int i = 0; i < 6; ++i) {
        if (hipMemcpyAsync(dst, m->p + m->off[i], m->len[i] * sizeof(float), hipMemcpyDeviceToHost, m->s) != hipSuccess ||
            hipStreamSynchronize(m->s) != hipSuccess)
            return fail(L3_EHIP, "l3_mlp_get_weights: copy failed");
        dst += m->len[i];
    }
    return L3_OK;
}

int l3_mlp_set_weights(l3_mlp* m, const float* src, int64_t n) {
    if (!m || !src || n != l3_mlp_param_count(m)) return fail(L3_EINVAL, "l3_mlp_set_weights: NULL or wrong element count");
    (void)hipSetDevice(m->device);
    if (hipStreamSynchronize(m->s) != hipSuccess) return fail(L3_EHIP, "l3_mlp_set_weights: HIP error");
    for (int i = 0; i < 6; ++i) {
        if (hipMemcpyAsync(m->p + m->off[i], src, m->len[i] * sizeof(float), hipMemcpyHostToDevice, m->s) != hipSuccess ||
            hipStreamSynchronize(m->s) != hipSuccess)
            return fail(L3_EHIP, "l3_mlp_set_weights: copy failed");
        src += m->len[i];
    }
    return L3_OK;
}

}  // extern "C"
