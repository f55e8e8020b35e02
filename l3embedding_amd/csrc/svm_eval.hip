// svm_eval.hip -- what train_svm reports about a fitted SVC (classifier/train.py:134-166), computed from the pair decisions where
// svm.hip's decision launch leaves them: libsvm's one-vs-one vote, sklearn's ovr decision values and hinge loss, Platt's pair
// probabilities, libsvm's multiclass_probability per row and the per-file mean of the frame probabilities with its argmax.
//   svm_tail_kernel        one wave per row, lane c = class c: the row's P decisions go to LDS once; vote, ovr value, hinge term,
//                          and (lanes striding the pairs) sigmoid_predict clipped to [1e-7, 1 - 1e-7] into a (rows, P) scratch
//   svm_coupling_kernel    one wave per row, lane t = class t: the symmetric Q (k, k) in LDS, the scalar loop of svm.cpp
//                          multiclass_probability operation for operation (tests/svm_ref.multiclass_probability is its restatement)
//   svm_file_mean_kernel   one wave per file: the row-order float64 sum of its rows' probabilities / count, argmax to the lower class
//   svm_chunk_sum_kernel   the hinge terms of a call in chunks of 256 rows in row order, then the chunk sums in chunk order
//   svm_sigmoid_train_kernel   svm.cpp sigmoid_train (Platt's A, B) of every pair of a fit at once, one workgroup per pair
// Everything is float64 and rounded operation by operation (no contraction), no float atomics: the same inputs give the same bits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/l3hip.h"
#include "host_common.h"
#include "svm_eval.h"

// every float64 operation below is rounded on its own, as numpy rounds it
#pragma clang fp contract(off)

namespace l3 {
namespace {

constexpr int SVM_EVAL_MAX_CLASSES = 64;
constexpr double SVM_MIN_PROB = 1e-7;

// libsvm's pair order (0, 1), (0, 2), ..., (1, 2), ...: the column of pair (i, j), i < j
__device__ __forceinline__ int pair_col(int i, int j, int C) { return i * C - i * (i + 1) / 2 + (j - i - 1); }

// lane l's value (l is the same in every lane)
__device__ __forceinline__ double bcast(double v, int l) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

struct SvmTailArgs {
    const double* dec;           // (rows, P)
    const double *A, *B;         // Platt's parameters per pair, or NULL
    const int* labels;           // class indices per row, or NULL
    int* pred;
    double *ovr, *hinge, *pp;
    int64_t rows;
    int C, P;
};

__global__ __launch_bounds__(64) void svm_tail_kernel(SvmTailArgs a) {
    extern __shared__ double sdec[];
    const int64_t row = blockIdx.x;
    const int lane = threadIdx.x, C = a.C;
    const double* d = a.dec + row * a.P;
    for (int k = lane; k < a.P; k += 64) {
        const double v = d[k];
        sdec[k] = v;
        if (a.pp) {
            // svm.cpp sigmoid_predict in the branch that keeps exp's argument <= 0, then svm_predict_probability's clip
            const double f = v * a.A[k] + a.B[k];
            const double e = exp(-fabs(f));
            const double p = f >= 0.0 ? e / (1.0 + e) : 1.0 / (1.0 + e);
            a.pp[row * a.P + k] = fmin(fmax(p, SVM_MIN_PROB), 1.0 - SVM_MIN_PROB);
        }
    }
    __syncthreads();
    const int c = lane;
    const bool cv = c < C;
    // class c's pairs in global pair order: (0, c) ... (c - 1, c), then (c, c + 1) ...  libsvm's vote gives a pair to its first
    // class when dec > 0; sklearn's ovr votes are of (dec < 0), so a decision of exactly 0 counts for the other side there
    int votes = 0, votes_ovr = 0;
    double conf = 0.0;
    if (cv) {
        for (int i = 0; i < c; ++i) {
            const double v = sdec[pair_col(i, c, C)];
            conf = conf - v;
            votes += !(v > 0.0);
            votes_ovr += v < 0.0;
        }
        for (int j = c + 1; j < C; ++j) {
            const double v = sdec[pair_col(c, j, C)];
            conf = conf + v;
            votes += v > 0.0;
            votes_ovr += !(v < 0.0);
        }
    }
    if (a.pred) {
        int key = cv ? votes * 64 + (63 - c) : -1;       // most votes, then the lower class
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) key = max(key, __shfl_xor(key, o));
        if (lane == 0) a.pred[row] = 63 - (key & 63);
    }
    if (C == 2) {
        // sklearn's flipped single column, and y in {-1, +1} (the larger label +1) times it
        const double v = -sdec[0];
        if (lane == 0) {
            if (a.ovr) a.ovr[row] = v;
            if (a.hinge) {
                const double y = a.labels[row] == 1 ? 1.0 : -1.0;
                const double loss = 1.0 - y * v;
                a.hinge[row] = loss <= 0.0 ? 0.0 : loss;
            }
        }
        return;
    }
    const double val = (double)votes_ovr + conf / (3.0 * (fabs(conf) + 1.0));
    if (a.ovr && cv) a.ovr[row * C + c] = val;
    if (a.hinge) {
        // Crammer-Singer: the true class's value minus the largest other one
        const int y = a.labels[row];
        const double own = __shfl(val, y);
        double other = (cv && c != y) ? val : -INFINITY;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) other = fmax(other, __shfl_xor(other, o));
        const double loss = 1.0 - (own - other);
        if (lane == 0) a.hinge[row] = loss <= 0.0 ? 0.0 : loss;
    }
}

// svm.cpp multiclass_probability.  Q is symmetric in its bits (a product commutes), so lane t reads Q[t][j] as Q[j][t]: 64 lanes on
// 64 consecutive doubles, free of bank conflicts whatever k is, where its own row would put every lane on one bank at k = 64.
__global__ __launch_bounds__(64) void svm_coupling_kernel(const double* pp, int64_t rows, int k, double* proba, int* iters) {
    extern __shared__ double Q[];
    const int64_t row = blockIdx.x;
    const int lane = threadIdx.x;
    const int P = k * (k - 1) / 2;
    const double* pr = pp + row * P;
    // r[i][j] = P(i | i or j) from the upper triangle, r[j][i] = 1 - r[i][j]
    for (int e = lane; e < k * k; e += 64) {
        const int i = e / k, j = e - i * k;
        if (i < j) {
            const double p = pr[pair_col(i, j, k)];
            Q[i * k + j] = p;
            Q[j * k + i] = 1.0 - p;
        }
    }
    __syncthreads();
    const int tc = min(lane, k - 1);       // lanes past the last class shadow it, so that every lane stays in every step
    double qtt = 0.0;                      // Q[t][t] = sum over j != t of r[j][t]^2, in increasing j
    for (int j = 0; j < k; ++j) {
        if (j != tc) {
            const double r = Q[j * k + tc];
            qtt += r * r;
        }
    }
    __syncthreads();
    for (int e = lane; e < k * k; e += 64) {
        const int i = e / k, j = e - i * k;
        if (i < j) {
            const double q = -(Q[j * k + i] * Q[i * k + j]);
            Q[i * k + j] = q;
            Q[j * k + i] = q;
        }
    }
    __syncthreads();
    if (lane < k) Q[lane * k + lane] = qtt;
    __syncthreads();
    double p = 1.0 / (double)k;
    const double eps = 0.005 / (double)k;
    const int max_iter = max(100, k);
    int it = 0;
    for (; it < max_iter; ++it) {
        double Qp = 0.0;
        for (int j = 0; j < k; ++j) Qp += Q[j * k + tc] * bcast(p, j);
        const double prod = p * Qp;
        double pQp = 0.0;
        for (int t = 0; t < k; ++t) pQp += bcast(prod, t);
        double err = lane < k ? fabs(Qp - pQp) : 0.0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) err = fmax(err, __shfl_xor(err, o));
        if (err < eps) break;
        for (int t = 0; t < k; ++t) {
            const double Qtt = Q[t * k + t], Qpt = bcast(Qp, t);
            const double diff = (-Qpt + pQp) / Qtt;
            if (tc == t) p += diff;
            pQp = (pQp + diff * (diff * Qtt + 2.0 * Qpt)) / (1.0 + diff) / (1.0 + diff);
            Qp = (Qp + diff * Q[t * k + tc]) / (1.0 + diff);
            p /= (1.0 + diff);
        }
    }
    if (lane < k) proba[row * k + lane] = p;
    if (iters && lane == 0) iters[row] = it;
}

__global__ __launch_bounds__(64) void svm_file_mean_kernel(const double* proba, int C, const int64_t* files, int64_t n_files,
                                                           double* file_proba, int* file_pred) {
    const int64_t f = blockIdx.x;
    const int lane = threadIdx.x;
    const int64_t s = files[2 * f], e = files[2 * f + 1];
    const bool cv = lane < C;
    double sum = 0.0;
    if (cv)
        for (int64_t r = s; r < e; ++r) sum += proba[r * C + lane];
    const double mean = sum / (double)(e - s);
    if (file_proba && cv) file_proba[f * C + lane] = mean;
    if (file_pred) {
        double v = cv ? mean : -INFINITY;
        int i = lane;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double w = __shfl_xor(v, o);
            const int j = __shfl_xor(i, o);
            if (w > v || (w == v && j < i)) v = w, i = j;
        }
        if (lane == 0) file_pred[f] = i;
    }
}

// out[b] = in[b * chunk] + ... in row order (one thread per chunk)
__global__ void svm_chunk_sum_kernel(const double* in, int64_t n, int64_t chunk, double* out) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t r0 = b * chunk;
    if (r0 >= n) return;
    const int64_t r1 = min(n, r0 + chunk);
    double sum = 0.0;
    for (int64_t r = r0; r < r1; ++r) sum += in[r];
    out[b] = sum;
}

// ---- svm.cpp sigmoid_train for many pairs at once -------------------------------------------------------------------------------
// One workgroup per job (a pair's cross-validation decision values and its +1 / -1 labels).  Every sum over the rows (the five of
// the Newton step, the objective of the line search, the count of positives) is taken as thread t's partial over rows t, t + NT, ...
// in row order and then a tree over the NT partials in LDS: a fixed order, so a job's result does not depend on the batch around it.
// The scalar part (priors, targets, the start point, sigma = 1e-12, the |g| < 1e-5 stop, the backtracking down to 1e-10, 100
// iterations at most) is svm.cpp's, evaluated by every thread on the same reduced values.
constexpr int SIG_NT = 256;

// sums of v[0 .. N) over the workgroup -> every thread; red holds N * SIG_NT doubles
template <int N>
__device__ __forceinline__ void sig_block_sum(double (&v)[N], double* red) {
    const int t = threadIdx.x;
#pragma unroll
    for (int i = 0; i < N; ++i) red[i * SIG_NT + t] = v[i];
    __syncthreads();
    for (int o = SIG_NT / 2; o > 0; o >>= 1) {
        if (t < o) {
#pragma unroll
            for (int i = 0; i < N; ++i) red[i * SIG_NT + t] = red[i * SIG_NT + t] + red[i * SIG_NT + t + o];
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = red[i * SIG_NT];
    __syncthreads();
}

// svm.cpp sigmoid_train's objective at (A, B)
__device__ __forceinline__ double sig_objective(const double* dec, const signed char* y, int l, double hi, double lo, double A,
                                                double B, double* red) {
    double f[1] = {0.0};
    for (int i = threadIdx.x; i < l; i += SIG_NT) {
        const double t = y[i] > 0 ? hi : lo;
        const double fApB = dec[i] * A + B;
        if (fApB >= 0.0)
            f[0] += t * fApB + log(1.0 + exp(-fApB));
        else
            f[0] += (t - 1.0) * fApB + log(1.0 + exp(fApB));
    }
    sig_block_sum<1>(f, red);
    return f[0];
}

__global__ __launch_bounds__(SIG_NT) void svm_sigmoid_train_kernel(const int64_t* off, const double* dec_all, const signed char* y_all,
                                                                   double* A_out, double* B_out, int* iters_out) {
    __shared__ double red[5 * SIG_NT];
    const int job = blockIdx.x;
    const int64_t o = off[job];
    const int l = (int)(off[job + 1] - o);
    const double* dec = dec_all + o;
    const signed char* y = y_all + o;
    const int max_iter = 100;
    const double min_step = 1e-10, sigma = 1e-12, eps = 1e-5;
    double cnt[1] = {0.0};
    for (int i = threadIdx.x; i < l; i += SIG_NT) cnt[0] += y[i] > 0 ? 1.0 : 0.0;
    sig_block_sum<1>(cnt, red);
    const double prior1 = cnt[0], prior0 = (double)l - prior1;
    const double hi = (prior1 + 1.0) / (prior1 + 2.0), lo = 1.0 / (prior0 + 2.0);
    double A = 0.0, B = log((prior0 + 1.0) / (prior1 + 1.0));
    double fval = sig_objective(dec, y, l, hi, lo, A, B, red);
    int iter = 0;
    for (; iter < max_iter; ++iter) {
        double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};        // h11, h22, h21, g1, g2
        for (int i = threadIdx.x; i < l; i += SIG_NT) {
            const double d = dec[i];
            const double fApB = d * A + B;
            double p, q;
            if (fApB >= 0.0) {
                p = exp(-fApB) / (1.0 + exp(-fApB));
                q = 1.0 / (1.0 + exp(-fApB));
            } else {
                p = 1.0 / (1.0 + exp(fApB));
                q = exp(fApB) / (1.0 + exp(fApB));
            }
            const double d2 = p * q;
            v[0] += d * d * d2;
            v[1] += d2;
            v[2] += d * d2;
            const double d1 = (y[i] > 0 ? hi : lo) - p;
            v[3] += d * d1;
            v[4] += d1;
        }
        sig_block_sum<5>(v, red);
        const double h11 = sigma + v[0], h22 = sigma + v[1], h21 = v[2], g1 = v[3], g2 = v[4];
        if (fabs(g1) < eps && fabs(g2) < eps) break;
        const double det = h11 * h22 - h21 * h21;
        const double dA = -(h22 * g1 - h21 * g2) / det;
        const double dB = -(-h21 * g1 + h11 * g2) / det;
        const double gd = g1 * dA + g2 * dB;
        double step = 1.0;
        while (step >= min_step) {
            const double nA = A + step * dA, nB = B + step * dB;
            const double nf = sig_objective(dec, y, l, hi, lo, nA, nB, red);
            if (nf < fval + 0.0001 * step * gd) {
                A = nA, B = nB, fval = nf;
                break;
            }
            step = step / 2.0;
        }
        if (step < min_step) break;        // the line search failed
    }
    if (threadIdx.x == 0) {
        A_out[job] = A, B_out[job] = B;
        if (iters_out) iters_out[job] = iter;
    }
}

}  // namespace

void svm_tail(hipStream_t s, const double* dec, int64_t rows, int C, const double* A, const double* B, const int* labels, int* pred,
              double* ovr, double* hinge, double* pairprob) {
    if (rows <= 0) return;
    SvmTailArgs a{};
    a.dec = dec, a.A = A, a.B = B, a.labels = labels, a.pred = pred, a.ovr = ovr, a.hinge = labels ? hinge : nullptr;
    a.pp = (A && B) ? pairprob : nullptr, a.rows = rows, a.C = C, a.P = C * (C - 1) / 2;
    hipLaunchKernelGGL(svm_tail_kernel, dim3((unsigned)rows), dim3(64), (size_t)a.P * sizeof(double), s, a);
}

void svm_coupling(hipStream_t s, const double* pairprob, int64_t rows, int C, double* proba, int* iters) {
    if (rows <= 0) return;
    hipLaunchKernelGGL(svm_coupling_kernel, dim3((unsigned)rows), dim3(64), (size_t)C * C * sizeof(double), s, pairprob, rows, C, proba,
                       iters);
}

void svm_file_mean(hipStream_t s, const double* proba, int C, const int64_t* files, int64_t n_files, double* file_proba,
                   int* file_pred) {
    if (n_files <= 0) return;
    hipLaunchKernelGGL(svm_file_mean_kernel, dim3((unsigned)n_files), dim3(64), 0, s, proba, C, files, n_files, file_proba, file_pred);
}

void svm_hinge_sum(hipStream_t s, const double* terms, int64_t n, double* partial, double* out) {
    const int64_t chunks = (n + SVM_HINGE_CHUNK - 1) / SVM_HINGE_CHUNK;
    hipLaunchKernelGGL(svm_chunk_sum_kernel, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, s, terms, n, (int64_t)SVM_HINGE_CHUNK,
                       partial);
    hipLaunchKernelGGL(svm_chunk_sum_kernel, dim3(1), dim3(64), 0, s, partial, chunks, chunks, out);
}

}  // namespace l3

using namespace l3;

extern "C" int l3_op_svm_tail(int device, const double* dec, int64_t n, int n_class, const double* probA, const double* probB,
                              const int32_t* labels, const int64_t* files, int64_t n_files, int32_t* pred_out, double* ovr_out,
                              double* hinge_sum_out, double* pair_proba_out, double* proba_out, double* file_proba_out,
                              int32_t* file_pred_out, int32_t* iters_out) {
    if (!dec || n <= 0 || n > INT32_MAX) return fail(L3_EINVAL, "l3_op_svm_tail: need decisions of 1 <= n < 2^31 rows");
    if (n_class < 2 || n_class > SVM_EVAL_MAX_CLASSES) return fail(L3_EINVAL, "l3_op_svm_tail: class count must be in [2, 64]");
    const int C = n_class, P = C * (C - 1) / 2;
    const bool want_prob = pair_proba_out || proba_out || file_proba_out || file_pred_out || iters_out;
    const bool want_files = file_proba_out || file_pred_out;
    if ((!probA) != (!probB)) return fail(L3_EINVAL, "l3_op_svm_tail: probA and probB come together");
    if (want_prob && !probA) return fail(L3_EINVAL, "l3_op_svm_tail: probabilities need probA and probB");
    if (hinge_sum_out && !labels) return fail(L3_EINVAL, "l3_op_svm_tail: the hinge loss needs labels");
    if (want_files && (!files || n_files <= 0)) return fail(L3_EINVAL, "l3_op_svm_tail: file outputs need file ranges");
    if (labels)
        for (int64_t i = 0; i < n; ++i)
            if (labels[i] < 0 || labels[i] >= C) return fail(L3_EINVAL, "l3_op_svm_tail: labels[" + std::to_string(i) + "] outside [0, C)");
    if (want_files)
        for (int64_t f = 0; f < n_files; ++f)
            if (files[2 * f] < 0 || files[2 * f] >= files[2 * f + 1] || files[2 * f + 1] > n)
                return fail(L3_EINVAL, "l3_op_svm_tail: file " + std::to_string(f) + " is empty or outside [0, n)");
    if (!device_ok(device)) return fail(L3_EHIP, no_gpu_message("l3_op_svm_tail", device));
    DeviceBufs b;
    hipStream_t s = nullptr;
    const int ovr_w = C == 2 ? 1 : C;
    const int64_t chunks = (n + SVM_HINGE_CHUNK - 1) / SVM_HINGE_CHUNK;
    const double* d_dec = b.put(dec, (size_t)n * P, s);
    const double* d_A = want_prob ? b.put(probA, P, s) : nullptr;
    const double* d_B = want_prob ? b.put(probB, P, s) : nullptr;
    const int* d_lab = hinge_sum_out ? b.put(labels, n, s) : nullptr;
    const int64_t* d_files = want_files ? b.put(files, 2 * n_files, s) : nullptr;
    int* d_pred = pred_out ? b.alloc<int>(n) : nullptr;
    double* d_ovr = ovr_out ? b.alloc<double>((size_t)n * ovr_w) : nullptr;
    double* d_hinge = hinge_sum_out ? b.alloc<double>(n) : nullptr;
    double* d_part = hinge_sum_out ? b.alloc<double>(chunks + 1) : nullptr;
    double* d_pp = want_prob ? b.alloc<double>((size_t)n * P) : nullptr;
    double* d_proba = want_prob ? b.alloc<double>((size_t)n * C) : nullptr;
    int* d_it = want_prob ? b.alloc<int>(n) : nullptr;
    double* d_fp = file_proba_out ? b.alloc<double>((size_t)n_files * C) : nullptr;
    int* d_fpred = file_pred_out ? b.alloc<int>(n_files) : nullptr;
    if (!b.ok()) return fail(L3_ENOMEM, "l3_op_svm_tail: device allocation failed");
    svm_tail(s, d_dec, n, C, d_A, d_B, d_lab, d_pred, d_ovr, d_hinge, d_pp);
    if (want_prob) svm_coupling(s, d_pp, n, C, d_proba, d_it);
    if (want_files) svm_file_mean(s, d_proba, C, d_files, n_files, d_fp, d_fpred);
    if (hinge_sum_out) svm_hinge_sum(s, d_hinge, n, d_part, d_part + chunks);
    bool ok = hipGetLastError() == hipSuccess;
    auto get = [&](void* dst, const void* src, size_t bytes) {
        if (dst && ok) ok = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s) == hipSuccess;
    };
    get(pred_out, d_pred, (size_t)n * sizeof(int));
    get(ovr_out, d_ovr, (size_t)n * ovr_w * sizeof(double));
    get(hinge_sum_out, d_part ? d_part + chunks : nullptr, sizeof(double));
    get(pair_proba_out, d_pp, (size_t)n * P * sizeof(double));
    get(proba_out, d_proba, (size_t)n * C * sizeof(double));
    get(iters_out, d_it, (size_t)n * sizeof(int));
    get(file_proba_out, d_fp, (size_t)n_files * C * sizeof(double));
    get(file_pred_out, d_fpred, (size_t)n_files * sizeof(int));
    // the wait also covers the copies still queued from the caller's buffers when something above failed
    const bool done = hipStreamSynchronize(s) == hipSuccess;
    if (!ok || !done) return fail(L3_EHIP, "l3_op_svm_tail: HIP error");
    return L3_OK;
}

extern "C" int l3_op_svm_sigmoid_train(int device, int n_jobs, const int64_t* off, const double* dec, const int8_t* signs,
                                       double* A_out, double* B_out, int32_t* iters_out) {
    if (!off || !dec || !signs || !A_out || !B_out || n_jobs <= 0)
        return fail(L3_EINVAL, "l3_op_svm_sigmoid_train: NULL argument or no jobs");
    if (off[0] != 0) return fail(L3_EINVAL, "l3_op_svm_sigmoid_train: off[0] must be 0");
    for (int j = 0; j < n_jobs; ++j)
        if (off[j + 1] <= off[j] || off[j + 1] - off[j] > INT32_MAX)
            return fail(L3_EINVAL, "l3_op_svm_sigmoid_train: job " + std::to_string(j) + " needs 1 <= rows < 2^31");
    const int64_t total = off[n_jobs];
    for (int64_t i = 0; i < total; ++i) {
        if (signs[i] != 1 && signs[i] != -1) return fail(L3_EINVAL, "l3_op_svm_sigmoid_train: signs must be +1 or -1");
        if (!std::isfinite(dec[i])) return fail(L3_EINVAL, "l3_op_svm_sigmoid_train: decision values must be finite");
    }
    if (!device_ok(device)) return fail(L3_EHIP, no_gpu_message("l3_op_svm_sigmoid_train", device));
    DeviceBufs b;
    hipStream_t s = nullptr;
    const int64_t* d_off = b.put(off, n_jobs + 1, s);
    const double* d_dec = b.put(dec, total, s);
    const signed char* d_y = reinterpret_cast<const signed char*>(b.put(signs, total, s));
    double* d_A = b.alloc<double>(n_jobs);
    double* d_B = b.alloc<double>(n_jobs);
    int* d_it = b.alloc<int>(n_jobs);
    if (!b.ok()) {
        (void)hipStreamSynchronize(s);
        return fail(L3_ENOMEM, "l3_op_svm_sigmoid_train: device allocation failed");
    }
    hipLaunchKernelGGL(svm_sigmoid_train_kernel, dim3((unsigned)n_jobs), dim3(SIG_NT), 0, s, d_off, d_dec, d_y, d_A, d_B, d_it);
    bool ok = hipGetLastError() == hipSuccess;
    auto get = [&](void* dst, const void* src, size_t bytes) {
        if (dst && ok) ok = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s) == hipSuccess;
    };
    get(A_out, d_A, n_jobs * sizeof(double));
    get(B_out, d_B, n_jobs * sizeof(double));
    get(iters_out, d_it, n_jobs * sizeof(int));
    const bool done = hipStreamSynchronize(s) == hipSuccess;
    if (!ok || !done) return fail(L3_EHIP, "l3_op_svm_sigmoid_train: HIP error");
    return L3_OK;
}
