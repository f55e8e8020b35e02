// svm.hip -- the reference's SVM sound classifier (classifier/train.py:79-166: sklearn.svm.SVC, i.e. libsvm's C-SVC) trained and
// evaluated on the GPU, and the l3_svm handle of the C ABI.
//
// Training is decomposition in the ThunderSVM style, batched over every binary problem of a fit (one-vs-one pairs and the
// cross-validation sub-problems of probability estimates).  One outer iteration is four launches on one stream:
//   svm_select   one workgroup per problem: m(alpha) - M(alpha) for the stopping test; q / 2 violators from the top of I_up and
//                q / 2 from the bottom of I_low by -y grad (the working set)
//   svm_rows     K[w, t] = k(x[ws_w], x[idx_t]) for every working-set row against the problem's rows: gathered fp32 rows on the
//                fp32 matrix cores (v_mfma_f32_32x32x2_f32), the kernel function applied in the epilogue
//   svm_smo      one workgroup per problem solves the q-variable sub-problem with libsvm's second-order pair selection (WSS3)
//                on the q x q block held in LDS; alpha and grad in float64
//   svm_grad     grad_t += sum_s dalpha_s y_s y_t K[s, t] in float64 from the rows svm_rows wrote
// then one host synchronisation for all problems (which are still active).  Prediction is one fused launch per class block:
// K(X_test, SV) tiles in registers times the class's dual coefficients, the n_test x n_SV kernel matrix never reaching HBM.
// Every problem carries its own box bound C (l3_svm_fit_costs), so the grid of a parameter search over C is one batch.  The held-out
// decision values of probability estimates come from one launch for all cross-validation sub-problems (svm_cv_decision_kernel: one
// wave per sub-problem and 32 held-out rows, the arithmetic of the prediction launch at two classes).
// No float atomics anywhere: the same inputs give bit-identical results.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/l3hip.h"
#include "device_common.h"
#include "featprep.h"
#include "kernels.h"
#include "svm_eval.h"

namespace l3 {
namespace {

constexpr int SVM_QMAX = 128;          // working-set cap: the q x q fp32 block is 64 KiB of LDS
constexpr int SVM_MAX_CLASSES = 64;
constexpr double SVM_TAU = 1e-12;      // libsvm's TAU: the curvature used where K_ii + K_jj - 2 K_ij <= 0 (sigmoid is not PSD)


struct SvmKern {
    int kind, degree;
    float gamma, coef0;
};

// libsvm's powi: repeated squaring (the same products for an integer degree)
__device__ __forceinline__ float powi_f(float base, int times) {
    float tmp = base, ret = 1.f;
    for (int t = times; t > 0; t /= 2) {
        if (t % 2 == 1) ret *= tmp;
        tmp = tmp * tmp;
    }
    return ret;
}

__device__ __forceinline__ float kfun(const SvmKern& k, float dot, float xx, float yy) {
    switch (k.kind) {
        case L3_SVM_POLY: return powi_f(k.gamma * dot + k.coef0, k.degree);
        case L3_SVM_RBF: return expf(-k.gamma * fmaxf(xx + yy - 2.f * dot, 0.f));
        case L3_SVM_SIGMOID: return tanhf(k.gamma * dot + k.coef0);
        default: return dot;
    }
}

// ---- squared row norms (rbf), summed in float64 ------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void svm_norms_kernel(const float* x, int64_t n, int D, float* xx) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const float* xr = x + row * D;
    double s = 0.0;
    for (int k = lane; k < D; k += 64) s += (double)xr[k] * (double)xr[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) xx[row] = (float)s;
}

// ---- kernel rows ---------------------------------------------------------------------------------------------------------------
// One wave per (problem, 32-column tile); the wave runs the problem's rows in groups of four 32-row tiles, so every column row
// it loads feeds up to 128 rows.  Step of 8 k: lane (r, h) holds x[row r][k0 + 4h + j] (one float4 of each row) and MFMA j sums
// k0 + j and k0 + 4 + j, as mlp_fwd_kernel does.
struct SvmRowsArgs {
    const float* x;              // resident rows (n_x, D)
    const float* xx;             // their squared norms
    const int* ridx;             // problem p's rows: ridx + p * rstride, nrows[p] of them (or nrows_all when nrows is NULL)
    const int* nrows;
    const int* cidx;             // problem p's columns: cidx[col_off[p] .. col_off[p + 1])
    const int64_t* col_off;
    const int64_t* tile_off;     // prefix of ceil(columns / 32) per problem
    const int* active;           // may be NULL
    float* out;                  // problem p: out + rstride * col_off[p], row w at w * columns + t
    int P, rstride, nrows_all, D, vec;
    SvmKern k;
};

__global__ __launch_bounds__(256) void svm_rows_kernel(SvmRowsArgs a) {
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int64_t wv = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wv >= a.tile_off[a.P]) return;
    int lo = 0, hi = a.P - 1;                 // the problem whose tiles hold wv
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.tile_off[mid] <= wv) lo = mid; else hi = mid - 1;
    }
    const int p = lo;
    if (a.active && !a.active[p]) return;
    const int nr = a.nrows ? a.nrows[p] : a.nrows_all;
    if (nr <= 0) return;
    const int64_t c0 = a.col_off[p];
    const int ncol = (int)(a.col_off[p + 1] - c0);
    const int col = (int)(wv - a.tile_off[p]) * 32 + r;
    const bool cv = col < ncol;
    const int cg = cv ? a.cidx[c0 + col] : 0;
    const float* xc = a.x + (int64_t)cg * a.D;
    const float ycn = cv ? a.xx[cg] : 0.f;
    const int* rows = a.ridx + (int64_t)p * a.rstride;
    float* out = a.out + (int64_t)a.rstride * c0;
    for (int g0 = 0; g0 < nr; g0 += 128) {
        const int nt = min(4, (nr - g0 + 31) >> 5);
        const float* xr[4];
        bool rv[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int w = g0 + t * 32 + r;
            rv[t] = t < nt && w < nr;
            xr[t] = a.x + (rv[t] ? (int64_t)rows[w] * a.D : 0);
        }
        f32x16 acc[4] = {};
        for (int k0 = 0; k0 < a.D; k0 += 8) {
            const int kk = k0 + 4 * h;
            float bv[4];
            if (a.vec && kk + 4 <= a.D) {
                const float4 qv = cv ? *reinterpret_cast<const float4*>(xc + kk) : make_float4(0.f, 0.f, 0.f, 0.f);
                bv[0] = qv.x, bv[1] = qv.y, bv[2] = qv.z, bv[3] = qv.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) bv[j] = (cv && kk + j < a.D) ? xc[kk + j] : 0.f;
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (t >= nt) break;
                float av[4];
                if (a.vec && kk + 4 <= a.D) {
                    const float4 qv = rv[t] ? *reinterpret_cast<const float4*>(xr[t] + kk) : make_float4(0.f, 0.f, 0.f, 0.f);
                    av[0] = qv.x, av[1] = qv.y, av[2] = qv.z, av[3] = qv.w;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) av[j] = (rv[t] && kk + j < a.D) ? xr[t][kk + j] : 0.f;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j], bv[j], acc[t], 0, 0, 0);
            }
        }
        if (!cv) continue;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (t >= nt) break;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int w = g0 + t * 32 + mfma_row(i, h);
                if (w < nr) out[(int64_t)w * ncol + col] = kfun(a.k, acc[t][i], a.xx[rows[w]], ycn);
            }
        }
    }
}

// ---- block reductions (argmax with a deterministic tie rule) -------------------------------------------------------------
// (v, i) beats (w, j) when v > w, or v == w and i > j (libsvm's ">=" scans keep the LAST index of a tie)
__device__ __forceinline__ void argmax_pair(double& v, int& i, double w, int j) {
    if (w > v || (w == v && j > i)) v = w, i = j;
}
template <int NT>
__device__ void block_argmax(double& v, int& i, double* sv, int* si) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double w = __shfl_xor(v, o);
        const int j = __shfl_xor(i, o);
        argmax_pair(v, i, w, j);
    }
    const int wid = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sv[wid] = v, si[wid] = i;
    __syncthreads();
    v = sv[0], i = si[0];
    for (int k = 1; k < NT / 64; ++k) argmax_pair(v, i, sv[k], si[k]);
}

// ---- working-set selection -------------------------------------------------------------------------------------------------
struct SvmState {
    const float* x;
    const int64_t* off;          // problem p's entries: [off[p], off[p + 1])
    const int* idx;              // global row of each entry
    const signed char* y;        // +1 / -1
    double *alpha, *grad;
    int *wsl, *wsg, *nws;        // per problem: q local / global working-set rows, their count
    double* dal;                 // per problem: q alpha changes of the last local solve
    int* active;
    long long* updates;          // local SMO updates so far
    int* outer;
    double *gap, *rho;
    float* krow;                 // problem p: q * off[p], row w at w * n_p + t
    const int64_t *tile32, *tile256;
    const double* C;             // the box bound of each problem
    double tol, local_rel;
    long long max_updates;       // per problem (-1: libsvm's cap, resolved on the host)
    int P, q, outer_cap;
};

__device__ __forceinline__ bool in_up(signed char y, double a, double C) { return y > 0 ? a < C : a > 0.0; }
__device__ __forceinline__ bool in_low(signed char y, double a, double C) { return y > 0 ? a > 0.0 : a < C; }

constexpr int SEL_NT = 512;
__global__ __launch_bounds__(SEL_NT) void svm_select_kernel(SvmState s) {
    __shared__ double sv[SEL_NT / 64];
    __shared__ int si[SEL_NT / 64];
    __shared__ int ups[SVM_QMAX / 2], lows[SVM_QMAX / 2];
    const int p = blockIdx.x;
    if (!s.active[p]) return;
    const int64_t off = s.off[p];
    const int n = (int)(s.off[p + 1] - off);
    const double* G = s.grad + off;
    const double* A = s.alpha + off;
    const signed char* Y = s.y + off;
    const int half = s.q / 2;
    // picks leave in the order (key desc, index asc) for I_up and (key asc, index asc) for I_low; the previous pick bounds the next
    double pu = INFINITY, pl = -INFINITY;
    int pui = -1, pli = -1, nu = 0, nl = 0;
    const double Cp = s.C[p];
    for (int rnd = 0; rnd < half; ++rnd) {
        double bu = -INFINITY, bl = -INFINITY;       // bl holds -key so that both sides reduce as argmax
        int bui = -1, bli = -1;
        for (int t = threadIdx.x; t < n; t += SEL_NT) {
            const signed char yt = Y[t];
            const double a = A[t], key = -(double)yt * G[t];
            if (pui != -2 && in_up(yt, a, Cp) && (key < pu || (key == pu && t > pui)))
                if (bui < 0 || key > bu || (key == bu && t < bui)) bu = key, bui = t;
            if (pli != -2 && in_low(yt, a, Cp) && (key > pl || (key == pl && t > pli)))
                if (bli < 0 || -key > bl || (-key == bl && t < bli)) bl = -key, bli = t;
        }
        // argmax_pair prefers the larger index on equal keys; the scan above kept the smaller, so reduce on -index
        int nbu = bui < 0 ? INT_MIN : -bui, nbl = bli < 0 ? INT_MIN : -bli;
        if (bui < 0) bu = -INFINITY;
        if (bli < 0) bl = -INFINITY;
        block_argmax<SEL_NT>(bu, nbu, sv, si);
        block_argmax<SEL_NT>(bl, nbl, sv, si);
        bui = nbu == INT_MIN ? -1 : -nbu;
        bli = nbl == INT_MIN ? -1 : -nbl;
        if (rnd == 0) {
            const double gap = (bui < 0 || bli < 0) ? -INFINITY : bu + bl;     // m(alpha) - M(alpha)
            const bool capped = s.updates[p] >= s.max_updates || s.outer[p] >= s.outer_cap;
            if (gap < s.tol || capped) {
                if (threadIdx.x == 0) s.active[p] = 0, s.gap[p] = gap, s.nws[p] = 0;
                return;
            }
            if (threadIdx.x == 0) s.gap[p] = gap;
        }
        if (threadIdx.x == 0) {
            if (bui >= 0) ups[nu] = bui;
            if (bli >= 0) lows[nl] = bli;
        }
        nu += bui >= 0, nl += bli >= 0;
        if (bui >= 0) pu = bu, pui = bui; else pui = -2;        // -2: that side is exhausted
        if (bli >= 0) pl = -bl, pli = bli; else pli = -2;
        if (pui == -2 && pli == -2) break;
        __syncthreads();
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        // the union of both lists (a free variable may sit in both)
        int* wl = s.wsl + (int64_t)p * s.q;
        int* wg = s.wsg + (int64_t)p * s.q;
        int c = 0;
        for (int i = 0; i < nu; ++i) wl[c++] = ups[i];
        for (int i = 0; i < nl; ++i) {
            bool dup = false;
            for (int j = 0; j < nu; ++j) dup |= ups[j] == lows[i];
            if (!dup) wl[c++] = lows[i];
        }
        for (int i = 0; i < c; ++i) wg[i] = s.idx[off + wl[i]];
        s.nws[p] = c;
        s.outer[p] += 1;
    }
}

// ---- local SMO: one workgroup per problem, one thread per working-set variable --------------------------------------------------
// libsvm's Solver::select_working_set (WSS3) and its two-variable update, on the q x q block in LDS.  The solve stops when the
// local gap falls below max(eps, local_rel * first local gap), when no pair can move, or at the update cap.
struct SvmSmoArgs {
    const float* K;               // problem p's rows: K + koff, ld n_p (or the q x q block itself for the operator)
    const int64_t* off;
    const int* wsl;
    const int* nws;
    const signed char* y;
    double *alpha;                // in / out
    const double* grad;
    double* dal;                  // out: alpha change per variable
    long long* updates;           // in / out, per problem
    int* active;                  // may be NULL (operator)
    const double* C;              // the box bound of each problem
    double eps, local_rel;
    long long max_updates;
    int q, ldk_is_n;
};

constexpr int SMO_NT = SVM_QMAX;
__global__ __launch_bounds__(SMO_NT) void svm_smo_kernel(SvmSmoArgs a) {
    __shared__ float Kb[SVM_QMAX * SVM_QMAX];
    __shared__ double sv[SMO_NT / 64], Av[SVM_QMAX];
    __shared__ int si[SMO_NT / 64];
    __shared__ double upd_a[2], gij[2];
    const int p = blockIdx.x;
    if (a.active && !a.active[p]) return;
    const int nw = a.nws[p];
    if (nw <= 0) return;
    const int64_t off = a.off[p];
    const int n = (int)(a.off[p + 1] - off);
    const int ld = a.ldk_is_n ? n : nw;
    const float* Kp = a.K + (int64_t)a.q * off;
    const int* wl = a.wsl + (int64_t)p * a.q;
    for (int e = threadIdx.x; e < nw * nw; e += SMO_NT) {
        const int w = e / nw, v = e - w * nw;
        Kb[w * SVM_QMAX + v] = Kp[(int64_t)w * ld + wl[v]];
    }
    const int k = threadIdx.x;
    const bool kv = k < nw;
    const int lk = kv ? wl[k] : 0;
    const signed char yk = kv ? a.y[off + lk] : 1;
    const double a0 = kv ? a.alpha[off + lk] : 0.0;
    double ak = a0, gk = kv ? a.grad[off + lk] : 0.0;
    if (kv) Av[k] = ak;
    __syncthreads();
    const double Ckk = kv ? (double)Kb[k * SVM_QMAX + k] : 0.0;
    const double Cp = a.C[p];
    const long long cap = a.max_updates - a.updates[p];
    long long upd = 0;
    double local_eps = a.eps;
    for (int it = 0;; ++it) {
        // i = argmax over I_up of -y G
        double vi = (kv && in_up(yk, ak, Cp)) ? -(double)yk * gk : -INFINITY;
        int ii = (kv && in_up(yk, ak, Cp)) ? k : -1;
        block_argmax<SMO_NT>(vi, ii, sv, si);
        const double Gmax = vi;
        // j: Gmax2 = max over I_low of y G; the second-order choice among I_low with grad_diff > 0
        double g2 = (kv && in_low(yk, ak, Cp)) ? (double)yk * gk : -INFINITY;
        int g2i = (kv && in_low(yk, ak, Cp)) ? k : -1;
        double ob = -INFINITY;      // -obj_diff, as argmax
        int oj = -1;
        if (ii >= 0 && kv && in_low(yk, ak, Cp)) {
            const double gd = Gmax + (double)yk * gk;
            if (gd > 0.0) {
                double quad = (double)Kb[ii * SVM_QMAX + ii] + Ckk - 2.0 * (double)Kb[ii * SVM_QMAX + k];
                if (!(quad > 0.0)) quad = SVM_TAU;
                ob = gd * gd / quad, oj = k;
            }
        }
        block_argmax<SMO_NT>(g2, g2i, sv, si);
        block_argmax<SMO_NT>(ob, oj, sv, si);
        const double gap = (ii < 0 || g2i < 0) ? -INFINITY : Gmax + g2;
        if (it == 0) local_eps = fmax(a.eps, a.local_rel * gap);
        if (ii < 0 || oj < 0 || gap < local_eps || upd >= cap) break;
        const int i = ii, j = oj;
        // the two gradients the update reads, from their owners; then libsvm's two-variable update (Solver::Solve) by thread 0
        if (k == i) gij[0] = gk;
        if (k == j) gij[1] = gk;
        __syncthreads();
        if (k == 0) {
            const double Kii = Kb[i * SVM_QMAX + i], Kjj = Kb[j * SVM_QMAX + j], Kij = Kb[i * SVM_QMAX + j];
            const signed char yi = a.y[off + wl[i]], yj = a.y[off + wl[j]];
            const double Gi = gij[0], Gj = gij[1];
            double ai = Av[i], aj = Av[j];
            const double C = Cp;
            if (yi != yj) {
                double quad = Kii + Kjj + 2.0 * (-(Kij));       // QD_i + QD_j + 2 Q_ij, Q_ij = y_i y_j K_ij = -K_ij
                if (quad <= 0.0) quad = SVM_TAU;
                const double delta = (-Gi - Gj) / quad;
                const double diff = ai - aj;
                ai += delta;
                aj += delta;
                if (diff > 0) {
                    if (aj < 0) aj = 0, ai = diff;
                } else {
                    if (ai < 0) ai = 0, aj = -diff;
                }
                if (diff > 0.0) {        // C_i - C_j = 0
                    if (ai > C) ai = C, aj = C - diff;
                } else {
                    if (aj > C) aj = C, ai = C + diff;
                }
            } else {
                double quad = Kii + Kjj - 2.0 * Kij;
                if (quad <= 0.0) quad = SVM_TAU;
                const double delta = (Gi - Gj) / quad;
                const double sum = ai + aj;
                ai -= delta;
                aj += delta;
                if (sum > C) {
                    if (ai > C) ai = C, aj = sum - C;
                } else {
                    if (aj < 0) aj = 0, ai = sum;
                }
                if (sum > C) {
                    if (aj > C) aj = C, ai = sum - C;
                } else {
                    if (ai < 0) ai = 0, aj = sum;
                }
            }
            upd_a[0] = ai - Av[i];
            upd_a[1] = aj - Av[j];
            Av[i] = ai, Av[j] = aj;
        }
        __syncthreads();
        if (kv) {
            const double di = upd_a[0], dj = upd_a[1];
            const signed char yi = a.y[off + wl[i]], yj = a.y[off + wl[j]];
            const double qki = (double)(yk * yi) * (double)Kb[k * SVM_QMAX + i];
            const double qkj = (double)(yk * yj) * (double)Kb[k * SVM_QMAX + j];
            gk += qki * di + qkj * dj;
            ak = Av[k];
        }
        ++upd;
        __syncthreads();
    }
    if (kv) {
        a.alpha[off + lk] = ak;
        a.dal[(int64_t)p * a.q + k] = ak - a0;
    }
    if (k == 0) {
        a.updates[p] += upd;
        if (upd == 0 && a.active) a.active[p] = 0;      // no pair can move: the problem stalls (its gap stays >= tol)
    }
}

// ---- gradient update: grad_t += y_t sum_s dalpha_s y_s K[s, t] --------------------------------------------------------------------
__global__ __launch_bounds__(256) void svm_grad_kernel(SvmState s) {
    __shared__ double dy[SVM_QMAX];
    const int64_t b = blockIdx.x;
    if (b >= s.tile256[s.P]) return;
    int lo = 0, hi = s.P - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (s.tile256[mid] <= b) lo = mid; else hi = mid - 1;
    }
    const int p = lo;
    if (!s.active[p]) return;
    const int nw = s.nws[p];
    const int64_t off = s.off[p];
    const int n = (int)(s.off[p + 1] - off);
    if (threadIdx.x < nw)
        dy[threadIdx.x] = s.dal[(int64_t)p * s.q + threadIdx.x] * (double)s.y[off + s.wsl[(int64_t)p * s.q + threadIdx.x]];
    __syncthreads();
    const int t = (int)(b - s.tile256[p]) * 256 + threadIdx.x;
    if (t >= n) return;
    const float* Kp = s.krow + (int64_t)s.q * off;
    double acc = 0.0;
    for (int w = 0; w < nw; ++w) {
        const double d = dy[w];
        if (d != 0.0) acc += d * (double)Kp[(int64_t)w * n + t];
    }
    s.grad[off + t] += (double)s.y[off + t] * acc;
}

// ---- start state and libsvm's rho -----------------------------------------------------------------------------------------------
__global__ void svm_init_kernel(SvmState s, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) s.alpha[i] = 0.0, s.grad[i] = -1.0;
    if (i < s.P) s.active[i] = 1, s.updates[i] = 0, s.outer[i] = 0, s.nws[i] = 0, s.gap[i] = INFINITY;
}

// Solver::calculate_rho: the mean of y G over free variables, else the middle of [lb, ub]
__global__ __launch_bounds__(256) void svm_rho_kernel(SvmState s) {
    __shared__ double red[3][4];
    __shared__ long long cnt[4];
    const int p = blockIdx.x;
    const int64_t off = s.off[p];
    const int n = (int)(s.off[p + 1] - off);
    const double Cp = s.C[p];
    double ub = INFINITY, lb = -INFINITY, sum = 0.0;
    long long nf = 0;
    for (int t = threadIdx.x; t < n; t += 256) {
        const signed char yt = s.y[off + t];
        const double a = s.alpha[off + t], yG = (double)yt * s.grad[off + t];
        if (a >= Cp) {
            if (yt < 0) ub = fmin(ub, yG); else lb = fmax(lb, yG);
        } else if (a <= 0.0) {
            if (yt > 0) ub = fmin(ub, yG); else lb = fmax(lb, yG);
        } else {
            ++nf;
            sum += yG;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ub = fmin(ub, __shfl_xor(ub, o));
        lb = fmax(lb, __shfl_xor(lb, o));
        sum += __shfl_xor(sum, o);
        nf += __shfl_xor(nf, o);
    }
    const int wid = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) red[0][wid] = ub, red[1][wid] = lb, red[2][wid] = sum, cnt[wid] = nf;
    __syncthreads();
    if (threadIdx.x == 0) {
        ub = red[0][0], lb = red[1][0], sum = red[2][0], nf = cnt[0];
        for (int w = 1; w < 4; ++w) ub = fmin(ub, red[0][w]), lb = fmax(lb, red[1][w]), sum += red[2][w], nf += cnt[w];
        s.rho[p] = nf > 0 ? sum / (double)nf : (ub + lb) / 2.0;
    }
}

// ---- fused decision values --------------------------------------------------------------------------------------------------
// One single-wave workgroup per (32 test rows, class c): K(x_test, SV) tiles of class c's support vectors on the matrix cores, the kernel function
// in registers, then S[m, c, r] = sum over the class's SVs of K * coef[r, sv] (float64) for r < R = n_class - 1.  The tile goes
// through LDS to meet the coefficients; the kernel matrix is never written out.
struct SvmDecArgs {
    const float *xt, *xtn;         // test rows / their squared norms, indexed through xidx (NULL: identity)
    const int* xidx;
    const float *sv, *svn;         // support vectors / norms, through svidx (NULL: identity)
    const int* svidx;
    const int64_t* cs;             // class c's SVs: [cs[c], cs[c + 1])
    const double* coef;            // (R, n_sv)
    double* S;                     // (n, n_class, R)
    int64_t n, n_sv;
    int D, ncls, vec;
    SvmKern k;
};

__global__ __launch_bounds__(64) void svm_decision_kernel(SvmDecArgs a) {
    extern __shared__ unsigned char smem[];
    const int R = a.ncls - 1;
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    float* T = reinterpret_cast<float*>(smem);
    double* Sacc = reinterpret_cast<double*>(smem + 32 * 33 * sizeof(float));
    const int64_t row_tiles = (a.n + 31) >> 5;
    const int64_t wv = blockIdx.x;
    if (wv >= row_tiles * a.ncls) return;
    const int c = (int)(wv % a.ncls);
    const int64_t rt = wv / a.ncls;
    const int64_t m = rt * 32 + r;
    const bool mv = m < a.n;
    const int64_t mg = mv ? (a.xidx ? a.xidx[m] : m) : 0;
    const float* xr = a.xt + mg * a.D;
    for (int e = lane; e < 32 * R; e += 64) Sacc[e] = 0.0;
    const int64_t s0 = a.cs[c], s1 = a.cs[c + 1];
    for (int64_t sb = s0; sb < s1; sb += 32) {
        const int64_t sidx = sb + r;
        const bool sv_ok = sidx < s1;
        const int64_t sg = sv_ok ? (a.svidx ? a.svidx[sidx] : sidx) : 0;
        const float* svr = a.sv + sg * a.D;
        f32x16 acc = {};
        for (int k0 = 0; k0 < a.D; k0 += 8) {
            const int kk = k0 + 4 * h;
            float av[4], bv[4];
            if (a.vec && kk + 4 <= a.D) {
                const float4 qa = mv ? *reinterpret_cast<const float4*>(xr + kk) : make_float4(0.f, 0.f, 0.f, 0.f);
                const float4 qb = sv_ok ? *reinterpret_cast<const float4*>(svr + kk) : make_float4(0.f, 0.f, 0.f, 0.f);
                av[0] = qa.x, av[1] = qa.y, av[2] = qa.z, av[3] = qa.w;
                bv[0] = qb.x, bv[1] = qb.y, bv[2] = qb.z, bv[3] = qb.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    av[j] = (mv && kk + j < a.D) ? xr[kk + j] : 0.f;
                    bv[j] = (sv_ok && kk + j < a.D) ? svr[kk + j] : 0.f;
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j], bv[j], acc, 0, 0, 0);
        }
        // lane (r, h) holds column r (an SV) of rows mfma_row(i, h): kernel function, then the tile to LDS as T[row][sv]
        const float ysn = sv_ok ? a.svn[sg] : 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int row = mfma_row(i, h);
            const int64_t mr = rt * 32 + row;
            float kvv = 0.f;
            if (sv_ok && mr < a.n) kvv = kfun(a.k, acc[i], a.xtn[a.xidx ? a.xidx[mr] : mr], ysn);
            T[row * 33 + r] = kvv;
        }
        __syncthreads();
        const int ns = (int)min<int64_t>(32, s1 - sb);
        for (int e = lane; e < 32 * R; e += 64) {
            const int rr = e >> 5, row = e & 31;
            const double* cf = a.coef + (int64_t)rr * a.n_sv + sb;
            double s = Sacc[e];
            for (int j = 0; j < ns; ++j) s += (double)T[row * 33 + j] * cf[j];
            Sacc[e] = s;
        }
        __syncthreads();
    }
    for (int e = lane; e < 32 * R; e += 64) {
        const int rr = e >> 5, row = e & 31;
        const int64_t mr = rt * 32 + row;
        if (mr < a.n) a.S[(mr * a.ncls + c) * R + rr] = Sacc[e];
    }
}

// pair (i, j), i < j: S[m, i, j - 1] + S[m, j, i] - rho_ij (libsvm's svm_predict_values)
__global__ void svm_pairs_kernel(const double* S, const double* rho, int64_t n, int ncls, double* dec) {
    const int P = ncls * (ncls - 1) / 2, R = ncls - 1;
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * P) return;
    const int64_t m = e / P;
    int p = (int)(e - m * P), i = 0;
    while (p >= ncls - 1 - i) p -= ncls - 1 - i, ++i;
    const int j = i + 1 + p;
    const int pp = (int)(e - m * P);
    dec[e] = S[(m * ncls + i) * R + (j - 1)] + S[(m * ncls + j) * R + i] - rho[pp];
}

// ---- held-out decision values of many binary models in one launch -------------------------------------------------------------
// Job j is one binary model (a cross-validation sub-problem of probability estimates) scored on its held-out rows.  One wave per
// (job, 32 held-out rows), found through the prefix of tiles as svm_rows_kernel finds its problem.  The arithmetic is
// svm_decision_kernel followed by svm_pairs_kernel at two classes: the same 32 x 32 tiles and k-steps, the same kfun, the positives'
// and the negatives' sums each in float64 in support-vector order (tiles start at each side's first support vector), then
// S_pos + S_neg - rho.  Every row is an index into the resident matrix.
struct SvmCvArgs {
    const float *x, *xx;           // the resident rows and their squared norms
    const int64_t* held_off;       // job j's held-out rows: held[held_off[j] .. held_off[j + 1])
    const int* held;
    const int64_t* sv_off;         // its support vectors: sv[sv_off[j] .. sv_off[j + 1]), the negatives from sv_off[j] + sv_neg[j]
    const int64_t* sv_neg;
    const int* sv;
    const double* coef;            // one per support vector
    const double* rho;             // one per job
    const int64_t* tile_off;       // prefix of ceil(held-out rows / 32) per job
    double* dec;                   // one per held-out row
    int64_t tile0;                 // the first tile of this launch
    int J, D, vec;
    SvmKern k;
};

__global__ __launch_bounds__(64) void svm_cv_decision_kernel(SvmCvArgs a) {
    __shared__ float T[32 * 33];
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    const int64_t wv = a.tile0 + blockIdx.x;
    if (wv >= a.tile_off[a.J]) return;
    int lo = 0, hi = a.J - 1;                 // the job whose tiles hold wv (a job without held-out rows owns none)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.tile_off[mid] <= wv) lo = mid; else hi = mid - 1;
    }
    const int j = lo;
    const int64_t h0 = a.held_off[j];
    const int64_t n = a.held_off[j + 1] - h0;
    const int64_t rt = wv - a.tile_off[j];
    const int* held = a.held + h0;
    const int64_t m = rt * 32 + r;
    const bool mv = m < n;
    const int64_t mg = mv ? held[m] : 0;
    const float* xr = a.x + mg * a.D;
    double side[2] = {0.0, 0.0};              // lanes 0 .. 31: row `lane` of the tile
    for (int c = 0; c < 2; ++c) {
        const int64_t s0 = c == 0 ? a.sv_off[j] : a.sv_off[j] + a.sv_neg[j];
        const int64_t s1 = c == 0 ? a.sv_off[j] + a.sv_neg[j] : a.sv_off[j + 1];
        double acc64 = 0.0;
        for (int64_t sb = s0; sb < s1; sb += 32) {
            const int64_t sidx = sb + r;
            const bool sv_ok = sidx < s1;
            const int64_t sg = sv_ok ? a.sv[sidx] : 0;
            const float* svr = a.x + sg * a.D;
            f32x16 acc = {};
            for (int k0 = 0; k0 < a.D; k0 += 8) {
                const int kk = k0 + 4 * h;
                float av[4], bv[4];
                if (a.vec && kk + 4 <= a.D) {
                    const float4 qa = mv ? *reinterpret_cast<const float4*>(xr + kk) : make_float4(0.f, 0.f, 0.f, 0.f);
                    const float4 qb = sv_ok ? *reinterpret_cast<const float4*>(svr + kk) : make_float4(0.f, 0.f, 0.f, 0.f);
                    av[0] = qa.x, av[1] = qa.y, av[2] = qa.z, av[3] = qa.w;
                    bv[0] = qb.x, bv[1] = qb.y, bv[2] = qb.z, bv[3] = qb.w;
                } else {
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        av[t] = (mv && kk + t < a.D) ? xr[kk + t] : 0.f;
                        bv[t] = (sv_ok && kk + t < a.D) ? svr[kk + t] : 0.f;
                    }
                }
#pragma unroll
                for (int t = 0; t < 4; ++t) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t], bv[t], acc, 0, 0, 0);
            }
            const float ysn = sv_ok ? a.xx[sg] : 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int row = mfma_row(i, h);
                const int64_t mr = rt * 32 + row;
                float kvv = 0.f;
                if (sv_ok && mr < n) kvv = kfun(a.k, acc[i], a.xx[held[mr]], ysn);
                T[row * 33 + r] = kvv;
            }
            __syncthreads();
            const int ns = (int)min<int64_t>(32, s1 - sb);
            if (lane < 32) {
                const double* cf = a.coef + sb;
                double s = acc64;
                for (int t = 0; t < ns; ++t) s += (double)T[lane * 33 + t] * cf[t];
                acc64 = s;
            }
            __syncthreads();
        }
        side[c] = acc64;
    }
    if (lane < 32 && rt * 32 + lane < n) a.dec[h0 + rt * 32 + lane] = side[0] + side[1] - a.rho[j];
}

// out (n, D) = x[idx]: the support vectors of a resident model, and the rows l3_svm_get_rows downloads
__global__ void svm_gather_rows_kernel(const float* x, const int* idx, int64_t n, int D, float* out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * D) return;
    const int64_t r = e / D;
    out[e] = x[(int64_t)idx[r] * D + (e - r * D)];
}

}  // namespace
}  // namespace l3

// ================================================================================================================================
// l3_svm: the resident training matrix and the batched solver (include/l3hip.h)
// ================================================================================================================================
using namespace l3;

struct l3_svm {
    int device = 0;
    hipStream_t s = nullptr;
    DeviceBufs bufs;          // owns x and xx
    float *x = nullptr, *xx = nullptr;
    int64_t n = 0;
    int D = 0;
    // the resident model of l3_svm_set_model (mbufs owns it): support vectors with their norms, grouped by class
    DeviceBufs mbufs;
    bool has_model = false, has_prob = false;
    SvmKern mk{};
    float *msv = nullptr, *msvn = nullptr;
    int64_t* mcs = nullptr;
    double *mcoef = nullptr, *mrho = nullptr, *mA = nullptr, *mB = nullptr;
    int64_t m_nsv = 0;
    int m_ncls = 0, mD = 0;
};

namespace {
bool kern_ok(const l3_svm_kernel* kp, std::string* why) {
    if (!kp) return *why = "kernel parameters are NULL", false;
    if (kp->kind < L3_SVM_LINEAR || kp->kind > L3_SVM_SIGMOID) return *why = "unknown kernel", false;
    if (kp->kind == L3_SVM_POLY && (kp->degree < 0 || kp->degree > 64)) return *why = "poly degree must be in [0, 64]", false;
    if (!std::isfinite(kp->gamma) || !std::isfinite(kp->coef0)) return *why = "gamma and coef0 must be finite", false;
    return true;
}
SvmKern to_kern(const l3_svm_kernel* kp) { return SvmKern{kp->kind, kp->degree, (float)kp->gamma, (float)kp->coef0}; }

void launch_norms(const float* x, int64_t n, int D, float* xx, hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(svm_norms_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, x, n, D, xx);
}

int vec_ok(const float* x, int D) { return (D % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0) ? 1 : 0; }

// the decision values of n rows (given on the device) in blocks bounded by the S scratch
int decision_dev(hipStream_t s, const float* xt, const float* xtn, const int* xidx, int64_t n, const float* sv, const float* svn,
                 const int* svidx, int64_t n_sv, int D, int ncls, const int64_t* cs_d, const double* coef_d, const double* rho_d,
                 const SvmKern& k, double* S, int64_t rows_blk, double* dec_d) {
    const int R = ncls - 1, P = ncls * R / 2;
    const size_t lds = 32 * 33 * sizeof(float) + (size_t)32 * R * sizeof(double);
    for (int64_t r0 = 0; r0 < n; r0 += rows_blk) {
        const int64_t rows = std::min(rows_blk, n - r0);
        SvmDecArgs a{};
        a.xt = xidx ? xt : xt + r0 * D, a.xtn = xidx ? xtn : xtn + r0, a.xidx = xidx ? xidx + r0 : nullptr;
        a.sv = sv, a.svn = svn, a.svidx = svidx, a.cs = cs_d, a.coef = coef_d, a.S = S, a.n = rows, a.n_sv = n_sv;
        a.D = D, a.ncls = ncls, a.k = k;
        a.vec = vec_ok(sv, D) & vec_ok(xt, D);
        const int64_t waves = ((rows + 31) / 32) * ncls;
        hipLaunchKernelGGL(svm_decision_kernel, dim3((unsigned)waves), dim3(64), lds, s, a);
        const int64_t e = rows * P;
        hipLaunchKernelGGL(svm_pairs_kernel, dim3((unsigned)((e + 255) / 256)), dim3(256), 0, s, S, rho_d, rows, ncls, dec_d + r0 * P);
    }
    return hipGetLastError() == hipSuccess ? L3_OK : fail(L3_EHIP, "l3_svm: decision launch failed");
}

int64_t prefix_tiles(const std::vector<int64_t>& off, int per, std::vector<int64_t>* tiles) {
    const size_t P = off.size() - 1;
    tiles->assign(P + 1, 0);
    for (size_t p = 0; p < P; ++p) (*tiles)[p + 1] = (*tiles)[p] + (off[p + 1] - off[p] + per - 1) / per;
    return (*tiles)[P];
}
}  // namespace

extern "C" {

int l3_svm_create(int device, l3_svm** out) {
    if (!out) return fail(L3_EINVAL, "l3_svm_create: out is NULL");
    *out = nullptr;
    if (!device_ok(device))
        return fail(L3_EHIP, no_gpu_message("l3_svm_create", device));
    l3_svm* m = new l3_svm();
    m->device = device;
    if (hipStreamCreateWithFlags(&m->s, hipStreamNonBlocking) != hipSuccess) {
        delete m;
        return fail(L3_EHIP, "l3_svm_create: stream creation failed");
    }
    *out = m;
    return L3_OK;
}

void l3_svm_destroy(l3_svm* m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    if (m->s) (void)hipStreamSynchronize(m->s);
    if (m->s) (void)hipStreamDestroy(m->s);
    delete m;
}

int l3_svm_set_data(l3_svm* m, const float* X, int64_t n, int D) {
    if (!m || !X) return fail(L3_EINVAL, "l3_svm_set_data: NULL argument");
    if (n <= 0 || n > INT32_MAX || D <= 0 || D > (1 << 24)) return fail(L3_EINVAL, "l3_svm_set_data: need 1 <= n < 2^31, 1 <= D <= 2^24");
    (void)hipSetDevice(m->device);
    (void)hipStreamSynchronize(m->s);
    m->bufs.release(m->x), m->bufs.release(m->xx);
    m->x = m->xx = nullptr, m->n = 0;
    if (!(m->x = m->bufs.alloc<float>((size_t)n * D)) || !(m->xx = m->bufs.alloc<float>((size_t)n)))
        return fail(L3_ENOMEM, "l3_svm_set_data: device allocation of " + std::to_string(n * D * 4) + " bytes failed");
    if (hipMemcpyAsync(m->x, X, (size_t)n * D * sizeof(float), hipMemcpyHostToDevice, m->s) != hipSuccess)
        return fail(L3_EHIP, "l3_svm_set_data: copy to the device failed");
    launch_norms(m->x, n, D, m->xx, m->s);
    if (hipStreamSynchronize(m->s) != hipSuccess) return fail(L3_EHIP, "l3_svm_set_data: HIP error");
    m->n = n, m->D = D;
    return L3_OK;
}

int l3_svm_fit(l3_svm* m, const l3_svm_kernel* kp, double C, double tol, int64_t max_iter, int n_prob, const int64_t* prob_off,
               const int32_t* rows, const int8_t* signs, int q, double* alpha_out, double* rho_out, int64_t* updates_out,
               int32_t* outer_out, double* gap_out) {
    if (n_prob <= 0) return fail(L3_EINVAL, "l3_svm_fit: no problems");
    const std::vector<double> costs((size_t)n_prob, C);
    return l3_svm_fit_costs(m, kp, costs.data(), tol, max_iter, n_prob, prob_off, rows, signs, q, alpha_out, rho_out, updates_out,
                            outer_out, gap_out);
}

int l3_svm_fit_costs(l3_svm* m, const l3_svm_kernel* kp, const double* C, double tol, int64_t max_iter, int n_prob,
                     const int64_t* prob_off, const int32_t* rows, const int8_t* signs, int q, double* alpha_out, double* rho_out,
                     int64_t* updates_out, int32_t* outer_out, double* gap_out) {
    std::string why;
    if (!m || !C || !prob_off || !rows || !signs || !alpha_out || !rho_out) return fail(L3_EINVAL, "l3_svm_fit: NULL argument");
    if (!kern_ok(kp, &why)) return fail(L3_EINVAL, "l3_svm_fit: " + why);
    if (m->n <= 0) return fail(L3_ESTATE, "l3_svm_fit: no training data (l3_svm_set_data)");
    if (n_prob <= 0) return fail(L3_EINVAL, "l3_svm_fit: no problems");
    if (!(tol > 0.0)) return fail(L3_EINVAL, "l3_svm_fit: need C > 0 and tol > 0");
    for (int p = 0; p < n_prob; ++p)
        if (!(C[p] > 0.0) || !std::isfinite(C[p])) return fail(L3_EINVAL, "l3_svm_fit: need C > 0 and tol > 0");
    if (q == 0) q = L3_SVM_DEFAULT_WS;
    if (q < 2 || q > SVM_QMAX || (q & 1)) return fail(L3_EINVAL, "l3_svm_fit: working-set size must be even, in [2, 128]");
    if (prob_off[0] != 0) return fail(L3_EINVAL, "l3_svm_fit: prob_off[0] must be 0");
    for (int p = 0; p < n_prob; ++p)
        if (prob_off[p + 1] - prob_off[p] < 2) return fail(L3_EINVAL, "l3_svm_fit: problem " + std::to_string(p) + " has < 2 rows");
    const int64_t total = prob_off[n_prob];
    for (int64_t i = 0; i < total; ++i) {
        if (rows[i] < 0 || rows[i] >= m->n) return fail(L3_EINVAL, "l3_svm_fit: rows[" + std::to_string(i) + "] outside [0, n)");
        if (signs[i] != 1 && signs[i] != -1) return fail(L3_EINVAL, "l3_svm_fit: signs must be +1 or -1");
    }
    (void)hipSetDevice(m->device);
    const std::vector<int64_t> off(prob_off, prob_off + n_prob + 1);
    std::vector<int64_t> t32, t256;
    const int64_t n32 = prefix_tiles(off, 32, &t32), n256 = prefix_tiles(off, 256, &t256);
    DeviceBufs b;
    SvmState st{};
    st.x = m->x;
    st.off = b.put(off.data(), n_prob + 1, m->s);
    st.idx = b.put(rows, total, m->s);
    st.y = reinterpret_cast<const signed char*>(b.put(signs, total, m->s));
    st.alpha = b.alloc<double>(total), st.grad = b.alloc<double>(total);
    st.wsl = b.alloc<int>((int64_t)n_prob * q), st.wsg = b.alloc<int>((int64_t)n_prob * q), st.nws = b.alloc<int>(n_prob);
    st.dal = b.alloc<double>((int64_t)n_prob * q);
    st.active = b.alloc<int>(n_prob), st.updates = b.alloc<long long>(n_prob), st.outer = b.alloc<int>(n_prob);
    st.gap = b.alloc<double>(n_prob), st.rho = b.alloc<double>(n_prob);
    st.krow = b.alloc<float>(total * q);
    st.tile32 = b.put(t32.data(), n_prob + 1, m->s), st.tile256 = b.put(t256.data(), n_prob + 1, m->s);
    st.C = b.put(C, n_prob, m->s);
    if (!b.ok()) return fail(L3_ENOMEM, "l3_svm_fit: device allocation failed (" + std::to_string(total * q * 4) + " bytes of kernel rows)");
    st.tol = tol, st.local_rel = L3_SVM_LOCAL_REL, st.P = n_prob, st.q = q;
    // libsvm's cap when max_iter is -1: max(10^7, 100 l) updates; the largest problem sets it for all
    int64_t nmax = 0;
    for (int p = 0; p < n_prob; ++p) nmax = std::max(nmax, off[p + 1] - off[p]);
    st.max_updates = max_iter > 0 ? max_iter : std::max<int64_t>(10000000, 100 * nmax);
    st.outer_cap = 1 << 24;
    hipLaunchKernelGGL(svm_init_kernel, dim3((unsigned)((std::max<int64_t>(total, n_prob) + 255) / 256)), dim3(256), 0, m->s, st,
                       total);
    SvmRowsArgs ra{};
    ra.x = m->x, ra.xx = m->xx, ra.ridx = st.wsg, ra.nrows = st.nws, ra.cidx = st.idx, ra.col_off = st.off, ra.tile_off = st.tile32;
    ra.active = st.active, ra.out = st.krow, ra.P = n_prob, ra.rstride = q, ra.D = m->D, ra.vec = vec_ok(m->x, m->D), ra.k = to_kern(kp);
    SvmSmoArgs sa{};
    sa.K = st.krow, sa.off = st.off, sa.wsl = st.wsl, sa.nws = st.nws, sa.y = st.y, sa.alpha = st.alpha, sa.grad = st.grad;
    sa.dal = st.dal, sa.updates = st.updates, sa.active = st.active, sa.C = st.C, sa.eps = tol, sa.local_rel = L3_SVM_LOCAL_REL;
    sa.max_updates = st.max_updates, sa.q = q, sa.ldk_is_n = 1;
    std::vector<int> act(n_prob);
    for (;;) {
        hipLaunchKernelGGL(svm_select_kernel, dim3(n_prob), dim3(SEL_NT), 0, m->s, st);
        hipLaunchKernelGGL(svm_rows_kernel, dim3((unsigned)((n32 + 3) / 4)), dim3(256), 0, m->s, ra);
        hipLaunchKernelGGL(svm_smo_kernel, dim3(n_prob), dim3(SMO_NT), 0, m->s, sa);
        hipLaunchKernelGGL(svm_grad_kernel, dim3((unsigned)n256), dim3(256), 0, m->s, st);
        if (hipGetLastError() != hipSuccess) return fail(L3_EHIP, "l3_svm_fit: launch failed");
        // the one synchronisation of the outer iteration, for all problems
        if (hipMemcpyAsync(act.data(), st.active, n_prob * sizeof(int), hipMemcpyDeviceToHost, m->s) != hipSuccess ||
            hipStreamSynchronize(m->s) != hipSuccess)
            return fail(L3_EHIP, "l3_svm_fit: HIP error in the solver");
        bool any = false;
        for (int p = 0; p < n_prob; ++p) any |= act[p] != 0;
        if (!any) break;
    }
    hipLaunchKernelGGL(svm_rho_kernel, dim3(n_prob), dim3(256), 0, m->s, st);
    std::vector<long long> upd(n_prob);
    if (hipMemcpyAsync(alpha_out, st.alpha, total * sizeof(double), hipMemcpyDeviceToHost, m->s) != hipSuccess ||
        hipMemcpyAsync(rho_out, st.rho, n_prob * sizeof(double), hipMemcpyDeviceToHost, m->s) != hipSuccess ||
        hipMemcpyAsync(upd.data(), st.updates, n_prob * sizeof(long long), hipMemcpyDeviceToHost, m->s) != hipSuccess ||
        (outer_out && hipMemcpyAsync(outer_out, st.outer, n_prob * sizeof(int), hipMemcpyDeviceToHost, m->s) != hipSuccess) ||
        (gap_out && hipMemcpyAsync(gap_out, st.gap, n_prob * sizeof(double), hipMemcpyDeviceToHost, m->s) != hipSuccess) ||
        hipStreamSynchronize(m->s) != hipSuccess)
        return fail(L3_EHIP, "l3_svm_fit: copy from the device failed");
    if (updates_out)
        for (int p = 0; p < n_prob; ++p) updates_out[p] = upd[p];
    return L3_OK;
}

int l3_svm_decision(l3_svm* m, const l3_svm_kernel* kp, const float* X, const int32_t* x_idx, int64_t n, int D, const float* SV,
                    const int32_t* sv_idx, int64_t n_sv, int n_class, const int64_t* sv_start, const double* coef, const double* rho,
                    double* dec_out) {
    std::string why;
    if (!m || !sv_start || !coef || !rho || !dec_out || n <= 0) return fail(L3_EINVAL, "l3_svm_decision: NULL argument or n <= 0");
    if (!kern_ok(kp, &why)) return fail(L3_EINVAL, "l3_svm_decision: " + why);
    if (n_class < 2 || n_class > SVM_MAX_CLASSES) return fail(L3_EINVAL, "l3_svm_decision: class count must be in [2, 64]");
    if ((!X) == (!x_idx) || (!SV) == (!sv_idx)) return fail(L3_EINVAL, "l3_svm_decision: give rows either as a matrix or as indices");
    if ((x_idx || sv_idx) && (m->n <= 0 || D != m->D)) return fail(L3_ESTATE, "l3_svm_decision: indices need the resident matrix of D columns");
    if (D <= 0 || D > (1 << 24) || n_sv < 0 || n > INT32_MAX) return fail(L3_EINVAL, "l3_svm_decision: bad sizes");
    if (sv_start[0] != 0 || sv_start[n_class] != n_sv) return fail(L3_EINVAL, "l3_svm_decision: sv_start must run from 0 to n_sv");
    for (int c = 0; c < n_class; ++c)
        if (sv_start[c + 1] < sv_start[c]) return fail(L3_EINVAL, "l3_svm_decision: sv_start must not decrease");
    if (x_idx)
        for (int64_t i = 0; i < n; ++i)
            if (x_idx[i] < 0 || x_idx[i] >= m->n) return fail(L3_EINVAL, "l3_svm_decision: x_idx outside [0, n)");
    if (sv_idx)
        for (int64_t i = 0; i < n_sv; ++i)
            if (sv_idx[i] < 0 || sv_idx[i] >= m->n) return fail(L3_EINVAL, "l3_svm_decision: sv_idx outside [0, n)");
    (void)hipSetDevice(m->device);
    const int R = n_class - 1, P = n_class * R / 2;
    int64_t rows_blk = std::min<int64_t>({65536, (int64_t(64) << 20) / D, (int64_t(32) << 20) / ((int64_t)n_class * R)});
    rows_blk = std::max<int64_t>(32, rows_blk & ~int64_t(31));
    DeviceBufs b;
    const float *sv = m->x, *svn = m->xx;
    const int* svi = nullptr;
    if (SV) {
        float* d = b.put(SV, n_sv * D, m->s);
        float* dn = b.alloc<float>(n_sv);
        if (b.ok()) launch_norms(d, n_sv, D, dn, m->s);
        sv = d, svn = dn;
    } else {
        svi = b.put(sv_idx, n_sv, m->s);
    }
    const int64_t* cs = b.put(sv_start, n_class + 1, m->s);
    const double* cf = b.put(coef, (int64_t)R * n_sv, m->s);
    const double* rh = b.put(rho, P, m->s);
    double* S = b.alloc<double>(std::min(rows_blk, n) * n_class * R);
    double* dec = b.alloc<double>(n * P);
    if (!b.ok()) return fail(L3_ENOMEM, "l3_svm_decision: device allocation failed");
    const SvmKern k = to_kern(kp);
    int rc = L3_OK;
    if (x_idx) {
        const int* xi = b.put(x_idx, n, m->s);
        if (!b.ok()) return fail(L3_ENOMEM, "l3_svm_decision: device allocation failed");
        rc = decision_dev(m->s, m->x, m->xx, xi, n, sv, svn, svi, n_sv, D, n_class, cs, cf, rh, k, S, rows_blk, dec);
    } else {
        // host rows staged in blocks
        const int64_t blk = std::min(rows_blk, n);
        float* xt = b.alloc<float>(blk * D);
        float* xtn = b.alloc<float>(blk);
        if (!b.ok()) return fail(L3_ENOMEM, "l3_svm_decision: device allocation failed");
        for (int64_t r0 = 0; r0 < n && rc == L3_OK; r0 += blk) {
            const int64_t rows = std::min(blk, n - r0);
            if (hipMemcpyAsync(xt, X + r0 * D, (size_t)rows * D * sizeof(float), hipMemcpyHostToDevice, m->s) != hipSuccess)
                return fail(L3_EHIP, "l3_svm_decision: copy to the device failed");
            launch_norms(xt, rows, D, xtn, m->s);
            rc = decision_dev(m->s, xt, xtn, nullptr, rows, sv, svn, svi, n_sv, D, n_class, cs, cf, rh, k, S, rows_blk, dec + r0 * P);
        }
    }
    if (rc != L3_OK) return rc;
    if (hipMemcpyAsync(dec_out, dec, (size_t)n * P * sizeof(double), hipMemcpyDeviceToHost, m->s) != hipSuccess ||
        hipStreamSynchronize(m->s) != hipSuccess)
        return fail(L3_EHIP, "l3_svm_decision: HIP error");
    return L3_OK;
}

int l3_svm_cv_decision(l3_svm* m, const l3_svm_kernel* kp, int n_jobs, const int64_t* held_off, const int32_t* held_rows,
                       const int64_t* sv_off, const int64_t* sv_neg, const int32_t* sv_rows, const double* coef, const double* rho,
                       double* dec_out) {
    std::string why;
    if (!m || !held_off || !held_rows || !sv_off || !sv_neg || !sv_rows || !coef || !rho || !dec_out)
        return fail(L3_EINVAL, "l3_svm_cv_decision: NULL argument");
    if (!kern_ok(kp, &why)) return fail(L3_EINVAL, "l3_svm_cv_decision: " + why);
    if (m->n <= 0) return fail(L3_ESTATE, "l3_svm_cv_decision: no resident matrix (l3_svm_set_data)");
    if (n_jobs <= 0) return fail(L3_EINVAL, "l3_svm_cv_decision: no jobs");
    if (held_off[0] != 0 || sv_off[0] != 0) return fail(L3_EINVAL, "l3_svm_cv_decision: held_off[0] and sv_off[0] must be 0");
    for (int j = 0; j < n_jobs; ++j) {
        if (held_off[j + 1] < held_off[j] || sv_off[j + 1] < sv_off[j])
            return fail(L3_EINVAL, "l3_svm_cv_decision: offsets of job " + std::to_string(j) + " decrease");
        if (sv_neg[j] < 0 || sv_neg[j] > sv_off[j + 1] - sv_off[j])
            return fail(L3_EINVAL, "l3_svm_cv_decision: sv_neg of job " + std::to_string(j) + " lies outside its support vectors");
    }
    const int64_t n_held = held_off[n_jobs], n_sv = sv_off[n_jobs];
    for (int64_t i = 0; i < n_held; ++i)
        if (held_rows[i] < 0 || held_rows[i] >= m->n)
            return fail(L3_EINVAL, "l3_svm_cv_decision: held_rows[" + std::to_string(i) + "] outside [0, n)");
    for (int64_t i = 0; i < n_sv; ++i)
        if (sv_rows[i] < 0 || sv_rows[i] >= m->n)
            return fail(L3_EINVAL, "l3_svm_cv_decision: sv_rows[" + std::to_string(i) + "] outside [0, n)");
    if (n_held == 0) return L3_OK;
    (void)hipSetDevice(m->device);
    const std::vector<int64_t> hoff(held_off, held_off + n_jobs + 1);
    std::vector<int64_t> tiles;
    const int64_t n_tiles = prefix_tiles(hoff, 32, &tiles);
    DeviceBufs b;
    SvmCvArgs a{};
    a.x = m->x, a.xx = m->xx;
    a.held_off = b.put(held_off, n_jobs + 1, m->s), a.held = b.put(held_rows, n_held, m->s);
    a.sv_off = b.put(sv_off, n_jobs + 1, m->s), a.sv_neg = b.put(sv_neg, n_jobs, m->s), a.sv = b.put(sv_rows, n_sv, m->s);
    a.coef = b.put(coef, n_sv, m->s), a.rho = b.put(rho, n_jobs, m->s);
    a.tile_off = b.put(tiles.data(), n_jobs + 1, m->s);
    a.dec = b.alloc<double>(n_held);
    if (!b.ok()) {
        (void)hipStreamSynchronize(m->s);       // copies from the caller's buffers may still be queued
        return fail(L3_ENOMEM, "l3_svm_cv_decision: device allocation failed");
    }
    a.J = n_jobs, a.D = m->D, a.vec = vec_ok(m->x, m->D), a.k = to_kern(kp);
    // one launch; more only where the tiles outnumber a grid dimension
    const int64_t grid_max = 0x7fffffff;
    for (int64_t t0 = 0; t0 < n_tiles; t0 += grid_max) {
        a.tile0 = t0;
        hipLaunchKernelGGL(svm_cv_decision_kernel, dim3((unsigned)std::min(grid_max, n_tiles - t0)), dim3(64), 0, m->s, a);
    }
    const bool ok = hipGetLastError() == hipSuccess &&
                    hipMemcpyAsync(dec_out, a.dec, (size_t)n_held * sizeof(double), hipMemcpyDeviceToHost, m->s) == hipSuccess;
    // the one host wait of the call
    const bool done = hipStreamSynchronize(m->s) == hipSuccess;
    if (!ok || !done) return fail(L3_EHIP, "l3_svm_cv_decision: HIP error");
    return L3_OK;
}

int l3_svm_set_data_dev(l3_svm* m, const l3_feat* f, int64_t lo, int64_t hi) {
    if (!m || !f) return fail(L3_EINVAL, "l3_svm_set_data_dev: NULL handle");
    if (f->device != m->device) return fail(L3_EINVAL, "l3_svm_set_data_dev: the feature matrix is on another device");
    if (lo < 0 || hi <= lo || hi > f->n) return fail(L3_EINVAL, "l3_svm_set_data_dev: rows [lo, hi) lie outside the matrix or are none");
    const int64_t n = hi - lo;
    if (n > INT32_MAX || f->D <= 0 || f->D > (1 << 24)) return fail(L3_EINVAL, "l3_svm_set_data_dev: need 1 <= n < 2^31, 1 <= D <= 2^24");
    const int D = (int)f->D;
    (void)hipSetDevice(m->device);
    (void)hipStreamSynchronize(m->s);
    m->bufs.release(m->x), m->bufs.release(m->xx);
    m->x = m->xx = nullptr, m->n = 0;
    if (!(m->x = m->bufs.alloc<float>((size_t)n * D)) || !(m->xx = m->bufs.alloc<float>((size_t)n)))
        return fail(L3_ENOMEM, "l3_svm_set_data_dev: device allocation of " + std::to_string(n * D * 4) + " bytes failed");
    if (hipMemcpyAsync(m->x, f->x + lo * D, (size_t)n * D * sizeof(float), hipMemcpyDeviceToDevice, m->s) != hipSuccess)
        return fail(L3_EHIP, "l3_svm_set_data_dev: copy on the device failed");
    launch_norms(m->x, n, D, m->xx, m->s);
    if (hipStreamSynchronize(m->s) != hipSuccess) return fail(L3_EHIP, "l3_svm_set_data_dev: HIP error");
    m->n = n, m->D = D;
    return L3_OK;
}

int l3_svm_get_rows(l3_svm* m, const int32_t* idx, int64_t n, float* out) {
    if (!m || !idx || !out || n <= 0) return fail(L3_EINVAL, "l3_svm_get_rows: NULL argument or n <= 0");
    if (m->n <= 0) return fail(L3_ESTATE, "l3_svm_get_rows: no resident matrix (l3_svm_set_data)");
    for (int64_t i = 0; i < n; ++i)
        if (idx[i] < 0 || idx[i] >= m->n) return fail(L3_EINVAL, "l3_svm_get_rows: idx[" + std::to_string(i) + "] outside [0, n)");
    (void)hipSetDevice(m->device);
    DeviceBufs b;
    const int* di = b.put(idx, n, m->s);
    float* d = b.alloc<float>((size_t)n * m->D);
    if (!b.ok()) return fail(L3_ENOMEM, "l3_svm_get_rows: device allocation failed");
    const int64_t e = n * m->D;
    hipLaunchKernelGGL(svm_gather_rows_kernel, dim3((unsigned)((e + 255) / 256)), dim3(256), 0, m->s, m->x, di, n, m->D, d);
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(out, d, (size_t)e * sizeof(float), hipMemcpyDeviceToHost, m->s) != hipSuccess ||
        hipStreamSynchronize(m->s) != hipSuccess)
        return fail(L3_EHIP, "l3_svm_get_rows: HIP error");
    return L3_OK;
}

int l3_svm_set_model(l3_svm* m, const l3_svm_kernel* kp, const float* SV, const int32_t* sv_idx, int64_t n_sv, int D, int n_class,
                     const int64_t* sv_start, const double* coef, const double* rho, const double* probA, const double* probB) {
    std::string why;
    if (!m || !sv_start || !coef || !rho) return fail(L3_EINVAL, "l3_svm_set_model: NULL argument");
    if (!kern_ok(kp, &why)) return fail(L3_EINVAL, "l3_svm_set_model: " + why);
    if (n_class < 2 || n_class > SVM_MAX_CLASSES) return fail(L3_EINVAL, "l3_svm_set_model: class count must be in [2, 64]");
    if ((!SV) == (!sv_idx)) return fail(L3_EINVAL, "l3_svm_set_model: give support vectors either as a matrix or as indices");
    if ((!probA) != (!probB)) return fail(L3_EINVAL, "l3_svm_set_model: probA and probB come together");
    if (sv_idx && (m->n <= 0 || D != m->D)) return fail(L3_ESTATE, "l3_svm_set_model: indices need the resident matrix of D columns");
    if (D <= 0 || D > (1 << 24) || n_sv < 0 || n_sv > INT32_MAX) return fail(L3_EINVAL, "l3_svm_set_model: bad sizes");
    if (sv_start[0] != 0 || sv_start[n_class] != n_sv) return fail(L3_EINVAL, "l3_svm_set_model: sv_start must run from 0 to n_sv");
    for (int c = 0; c < n_class; ++c)
        if (sv_start[c + 1] < sv_start[c]) return fail(L3_EINVAL, "l3_svm_set_model: sv_start must not decrease");
    if (sv_idx)
        for (int64_t i = 0; i < n_sv; ++i)
            if (sv_idx[i] < 0 || sv_idx[i] >= m->n) return fail(L3_EINVAL, "l3_svm_set_model: sv_idx outside [0, n)");
    (void)hipSetDevice(m->device);
    (void)hipStreamSynchronize(m->s);
    m->mbufs.clear();
    m->has_model = m->has_prob = false;
    DeviceBufs& b = m->mbufs;
    const int R = n_class - 1, P = n_class * R / 2;
    DeviceBufs tmp;
    if (SV) {
        m->msv = b.put(SV, (size_t)n_sv * D, m->s);
    } else {
        m->msv = b.alloc<float>((size_t)n_sv * D);
        const int* di = tmp.put(sv_idx, n_sv, m->s);
        const int64_t e = n_sv * D;
        if (b.ok() && tmp.ok() && e > 0)
            hipLaunchKernelGGL(svm_gather_rows_kernel, dim3((unsigned)((e + 255) / 256)), dim3(256), 0, m->s, m->x, di, n_sv, D, m->msv);
    }
    m->msvn = b.alloc<float>((size_t)n_sv);
    m->mcs = b.put(sv_start, n_class + 1, m->s);
    m->mcoef = b.put(coef, (size_t)R * n_sv, m->s);
    m->mrho = b.put(rho, P, m->s);
    m->mA = probA ? b.put(probA, P, m->s) : nullptr;
    m->mB = probB ? b.put(probB, P, m->s) : nullptr;
    // the pointers, not b.ok(): mbufs lives as long as the handle, and a failure it once met must not fail every later model
    if (!m->msv || !m->msvn || !m->mcs || !m->mcoef || !m->mrho || (probA && (!m->mA || !m->mB)) || !tmp.ok()) {
        (void)hipStreamSynchronize(m->s);
        b.clear();
        return fail(L3_ENOMEM, "l3_svm_set_model: device allocation failed");
    }
    launch_norms(m->msv, n_sv, D, m->msvn, m->s);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(m->s) != hipSuccess) {
        b.clear();
        return fail(L3_EHIP, "l3_svm_set_model: HIP error");
    }
    m->mk = to_kern(kp), m->m_nsv = n_sv, m->m_ncls = n_class, m->mD = D;
    m->has_model = true, m->has_prob = probA != nullptr;
    return L3_OK;
}

int l3_svm_score(l3_svm* m, const float* X, const int32_t* x_idx, const l3_feat* feat, int64_t lo, int64_t hi, int64_t n, int D,
                 const int32_t* labels, const int64_t* files, int64_t n_files, int32_t* pred_out, double* ovr_out,
                 double* hinge_sum_out, double* proba_out, double* file_proba_out, int32_t* file_pred_out) {
    if (!m) return fail(L3_EINVAL, "l3_svm_score: NULL handle");
    if ((X != nullptr) + (x_idx != nullptr) + (feat != nullptr) != 1)
        return fail(L3_EINVAL, "l3_svm_score: give rows as exactly one of a matrix, indices or a device matrix");
    if (!m->has_model) return fail(L3_ESTATE, "l3_svm_score: no model (l3_svm_set_model)");
    const bool want_files = file_proba_out || file_pred_out;
    const bool want_prob = proba_out || want_files;
    if (want_prob && !m->has_prob) return fail(L3_ESTATE, "l3_svm_score: the model was set without probA / probB");
    if (feat) {
        if (feat->device != m->device || feat->D != m->mD)
            return fail(L3_EINVAL, "l3_svm_score: the feature matrix is on another device or not " + std::to_string(m->mD) +
                                       " columns wide");
        if (lo < 0 || hi <= lo || hi > feat->n || n != hi - lo)
            return fail(L3_EINVAL, "l3_svm_score: rows [lo, hi) lie outside the matrix, are none, or are not n");
        D = m->mD;
    }
    if (n <= 0 || n > INT32_MAX || D != m->mD) return fail(L3_EINVAL, "l3_svm_score: need 1 <= n < 2^31 rows of the model's width");
    if (x_idx) {
        if (m->n <= 0 || m->D != D) return fail(L3_ESTATE, "l3_svm_score: indices need the resident matrix of D columns");
        for (int64_t i = 0; i < n; ++i)
            if (x_idx[i] < 0 || x_idx[i] >= m->n) return fail(L3_EINVAL, "l3_svm_score: x_idx outside [0, n)");
    }
    const int C = m->m_ncls, R = C - 1, P = C * R / 2;
    if (hinge_sum_out && !labels) return fail(L3_EINVAL, "l3_svm_score: the hinge loss needs labels");
    if (labels)
        for (int64_t i = 0; i < n; ++i)
            if (labels[i] < 0 || labels[i] >= C) return fail(L3_EINVAL, "l3_svm_score: labels[" + std::to_string(i) + "] outside [0, C)");
    if (want_files) {
        if (!files || n_files <= 0) return fail(L3_EINVAL, "l3_svm_score: file outputs need file ranges");
        for (int64_t f = 0; f < n_files; ++f)
            if (files[2 * f] < 0 || files[2 * f] >= files[2 * f + 1] || files[2 * f + 1] > n)
                return fail(L3_EINVAL, "l3_svm_score: file " + std::to_string(f) + " is empty or outside [0, n)");
    }
    (void)hipSetDevice(m->device);
    // l3_svm_decision's row blocks, so that every decision launch has its shape
    int64_t rows_blk = std::min<int64_t>({65536, (int64_t(64) << 20) / D, (int64_t(32) << 20) / ((int64_t)C * R)});
    rows_blk = std::max<int64_t>(32, rows_blk & ~int64_t(31));
    const int64_t blk = std::min(rows_blk, n);
    const int ovr_w = C == 2 ? 1 : C;
    const int64_t chunks = (n + SVM_HINGE_CHUNK - 1) / SVM_HINGE_CHUNK;
    DeviceBufs b;
    hipStream_t s = m->s;
    double* S = b.alloc<double>((size_t)blk * C * R);
    double* dec = b.alloc<double>((size_t)blk * P);
    float* xt = X ? b.alloc<float>((size_t)blk * D) : nullptr;
    float* xtn = x_idx ? nullptr : b.alloc<float>((size_t)blk);
    const int* xi = x_idx ? b.put(x_idx, n, s) : nullptr;
    const int* d_lab = hinge_sum_out ? b.put(labels, n, s) : nullptr;
    const int64_t* d_files = want_files ? b.put(files, 2 * n_files, s) : nullptr;
    int* d_pred = pred_out ? b.alloc<int>(n) : nullptr;
    double* d_ovr = ovr_out ? b.alloc<double>((size_t)n * ovr_w) : nullptr;
    double* d_hinge = hinge_sum_out ? b.alloc<double>(n) : nullptr;
    double* d_part = hinge_sum_out ? b.alloc<double>(chunks + 1) : nullptr;
    double* d_pp = want_prob ? b.alloc<double>((size_t)blk * P) : nullptr;
    double* d_proba = want_prob ? b.alloc<double>((size_t)n * C) : nullptr;
    double* d_fp = file_proba_out ? b.alloc<double>((size_t)n_files * C) : nullptr;
    int* d_fpred = file_pred_out ? b.alloc<int>(n_files) : nullptr;
    if (!b.ok()) return fail(L3_ENOMEM, "l3_svm_score: device allocation failed");
    for (int64_t r0 = 0; r0 < n; r0 += blk) {
        const int64_t rows = std::min(blk, n - r0);
        int rc;
        if (x_idx) {
            rc = decision_dev(s, m->x, m->xx, xi + r0, rows, m->msv, m->msvn, nullptr, m->m_nsv, D, C, m->mcs, m->mcoef, m->mrho, m->mk,
                              S, rows_blk, dec);
        } else {
            const float* xb = feat ? feat->x + (lo + r0) * D : xt;
            if (X && hipMemcpyAsync(xt, X + r0 * D, (size_t)rows * D * sizeof(float), hipMemcpyHostToDevice, s) != hipSuccess) {
                (void)hipStreamSynchronize(s);          // copies from the caller's buffers are still queued
                return fail(L3_EHIP, "l3_svm_score: copy to the device failed");
            }
            launch_norms(xb, rows, D, xtn, s);
            rc = decision_dev(s, xb, xtn, nullptr, rows, m->msv, m->msvn, nullptr, m->m_nsv, D, C, m->mcs, m->mcoef, m->mrho, m->mk, S,
                              rows_blk, dec);
        }
        if (rc != L3_OK) {
            (void)hipStreamSynchronize(s);
            return rc;
        }
        svm_tail(s, dec, rows, C, want_prob ? m->mA : nullptr, want_prob ? m->mB : nullptr, d_lab ? d_lab + r0 : nullptr,
                 d_pred ? d_pred + r0 : nullptr, d_ovr ? d_ovr + r0 * ovr_w : nullptr, d_hinge ? d_hinge + r0 : nullptr, d_pp);
        if (want_prob) svm_coupling(s, d_pp, rows, C, d_proba + r0 * C, nullptr);
    }
    if (want_files) svm_file_mean(s, d_proba, C, d_files, n_files, d_fp, d_fpred);
    if (hinge_sum_out) svm_hinge_sum(s, d_hinge, n, d_part, d_part + chunks);
    bool ok = hipGetLastError() == hipSuccess;
    auto get = [&](void* dst, const void* src, size_t bytes) {
        if (dst && ok) ok = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s) == hipSuccess;
    };
    get(pred_out, d_pred, (size_t)n * sizeof(int));
    get(ovr_out, d_ovr, (size_t)n * ovr_w * sizeof(double));
    get(hinge_sum_out, d_part ? d_part + chunks : nullptr, sizeof(double));
    get(proba_out, d_proba, (size_t)n * C * sizeof(double));
    get(file_proba_out, d_fp, (size_t)n_files * C * sizeof(double));
    get(file_pred_out, d_fpred, (size_t)n_files * sizeof(int));
    // the one host wait of the call
    const bool done = hipStreamSynchronize(s) == hipSuccess;
    if (!ok || !done) return fail(L3_EHIP, "l3_svm_score: HIP error");
    return L3_OK;
}

int l3_op_svm_kernel_rows(int device, const l3_svm_kernel* kp, const float* x, int64_t n_x, int D, const int32_t* a_idx, int na,
                          const int32_t* b_idx, int nb, float* out) {
    std::string why;
    if (!x || !a_idx || !b_idx || !out || n_x <= 0 || na <= 0 || nb <= 0 || D <= 0 || D > (1 << 24))
        return fail(L3_EINVAL, "l3_op_svm_kernel_rows: NULL pointer or non-positive size");
    if (!kern_ok(kp, &why)) return fail(L3_EINVAL, "l3_op_svm_kernel_rows: " + why);
    for (int i = 0; i < na; ++i)
        if (a_idx[i] < 0 || a_idx[i] >= n_x) return fail(L3_EINVAL, "l3_op_svm_kernel_rows: a_idx outside [0, n_x)");
    for (int i = 0; i < nb; ++i)
        if (b_idx[i] < 0 || b_idx[i] >= n_x) return fail(L3_EINVAL, "l3_op_svm_kernel_rows: b_idx outside [0, n_x)");
    if (!device_ok(device)) return fail(L3_EHIP, "l3_op_svm_kernel_rows: HIP device not available (libl3hip needs an AMD GPU)");
    DeviceBufs b;
    hipStream_t s = nullptr;
    const float* dx = b.put(x, n_x * D, s);
    float* dxx = b.alloc<float>(n_x);
    const int* da = b.put(a_idx, na, s);
    const int* db = b.put(b_idx, nb, s);
    const int64_t off[2] = {0, nb}, tiles[2] = {0, (nb + 31) / 32};
    const int64_t* doff = b.put(off, 2, s);
    const int64_t* dt = b.put(tiles, 2, s);
    float* dout = b.alloc<float>((int64_t)na * nb);
    if (!b.ok()) return fail(L3_ENOMEM, "l3_op_svm_kernel_rows: device allocation failed");
    launch_norms(dx, n_x, D, dxx, s);
    SvmRowsArgs ra{};
    ra.x = dx, ra.xx = dxx, ra.ridx = da, ra.nrows = nullptr, ra.nrows_all = na, ra.cidx = db, ra.col_off = doff, ra.tile_off = dt;
    ra.active = nullptr, ra.out = dout, ra.P = 1, ra.rstride = na, ra.D = D, ra.vec = vec_ok(dx, D), ra.k = to_kern(kp);
    hipLaunchKernelGGL(svm_rows_kernel, dim3((unsigned)((tiles[1] + 3) / 4)), dim3(256), 0, s, ra);
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(out, dout, (size_t)na * nb * sizeof(float), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return fail(L3_EHIP, "l3_op_svm_kernel_rows: HIP error");
    return L3_OK;
}

int l3_op_svm_smo(int device, const float* K, const int8_t* y, int q, double C, double eps, double local_rel, int64_t max_updates,
                  double* alpha, const double* grad, int64_t* updates_out) {
    if (!K || !y || !alpha || !grad || q < 2 || q > SVM_QMAX) return fail(L3_EINVAL, "l3_op_svm_smo: NULL pointer or q outside [2, 128]");
    if (!(C > 0.0) || !(eps > 0.0) || !(local_rel >= 0.0)) return fail(L3_EINVAL, "l3_op_svm_smo: need C > 0, eps > 0, local_rel >= 0");
    for (int i = 0; i < q; ++i) {
        if (y[i] != 1 && y[i] != -1) return fail(L3_EINVAL, "l3_op_svm_smo: y must be +1 or -1");
        if (!(alpha[i] >= 0.0 && alpha[i] <= C)) return fail(L3_EINVAL, "l3_op_svm_smo: alpha outside [0, C]");
    }
    if (!device_ok(device)) return fail(L3_EHIP, "l3_op_svm_smo: HIP device not available (libl3hip needs an AMD GPU)");
    DeviceBufs b;
    hipStream_t s = nullptr;
    std::vector<int> wl(q);
    for (int i = 0; i < q; ++i) wl[i] = i;
    const int64_t off[2] = {0, q};
    const long long zero = 0;
    SvmSmoArgs sa{};
    sa.K = b.put(K, (int64_t)q * q, s);
    sa.off = b.put(off, 2, s);
    sa.wsl = b.put(wl.data(), q, s);
    sa.nws = b.put(&q, 1, s);
    sa.y = reinterpret_cast<const signed char*>(b.put(y, q, s));
    double* da = b.put(alpha, q, s);
    sa.alpha = da;
    sa.grad = b.put(grad, q, s);
    sa.dal = b.alloc<double>(q);
    long long* du = b.put(&zero, 1, s);
    sa.updates = du;
    sa.C = b.put(&C, 1, s);
    if (!b.ok()) return fail(L3_ENOMEM, "l3_op_svm_smo: device allocation failed");
    sa.active = nullptr, sa.eps = eps, sa.local_rel = local_rel;
    sa.max_updates = max_updates > 0 ? max_updates : (long long)1 << 62;
    sa.q = q, sa.ldk_is_n = 1;
    hipLaunchKernelGGL(svm_smo_kernel, dim3(1), dim3(SMO_NT), 0, s, sa);
    long long u = 0;
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(alpha, da, q * sizeof(double), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(&u, du, sizeof(u), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        return fail(L3_EHIP, "l3_op_svm_smo: HIP error");
    if (updates_out) *updates_out = u;
    return L3_OK;
}

}  // extern "C"
