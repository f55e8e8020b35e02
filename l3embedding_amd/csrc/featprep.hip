// featprep.hip -- fold preprocessing of the downstream classifier on the GPU (data/usc/features.py:52-150,243-253): the l3_feat
// handle of the C ABI and its kernels.  Every kernel streams the (n, D) matrix with columns across lanes (consecutive lanes read
// consecutive floats, four per lane when D % 4 == 0) and rows along the loop; all of them are bound by HBM.
//
//   feat_gather        X[rows] -> a new matrix            (remove_data_overlap :60-73, the shuffle :143-148)
//   feat_colreduce     per chunk of L3_FEAT_CHUNK_ROWS rows: column min / max, float64 sum, float64 sum of (x - mean)^2
//   feat_combine       the chunks' partial results, in chunk order
//   feat_affine32      x * scale + shift, two float32 roundings             (MinMaxScaler.transform)
//   feat_standardize   (x - mean) / scale through float64, two float32 roundings (StandardScaler.transform)
//   feat_file_stats    compute_stats_features of every file (:243-253)
//   feat_assemble      row ranges of other matrices -> a new matrix  (the np.vstack of data/usc/folds.py:24-112)
//   feat_split         X[rows_a], X[rows_b] -> two new matrices, X kept  (train_param_search's cut, classifier/train.py:416-423)
//
// The arithmetic whose roundings are part of the contract is written with the __f*_rn / __d*_rn intrinsics, which the compiler
// never contracts into a fused multiply-add; the file is also built with -ffp-contract=off (_build.py).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/l3hip.h"
#include "feat_assemble.h"
#include "feat_split.h"
#include "featprep.h"

namespace l3 {
namespace {

constexpr int CHUNK = L3_FEAT_CHUNK_ROWS;
constexpr int LDS_ROWS = L3_FEAT_STATS_LDS_ROWS;
constexpr int ELEM_BLOCK = 256;          // threads of an elementwise block
constexpr int ELEM_VECS = 4096;          // lane-sized pieces one elementwise block handles (whole rows)

// V floats of one lane: one dword, or four when the row length allows it
template <int V>
struct Vec;
template <>
struct Vec<1> {
    float v[1];
    __device__ static Vec load(const float* p) { return Vec{{*p}}; }
    __device__ void store(float* p) const { *p = v[0]; }
};
template <>
struct Vec<4> {
    float v[4];
    __device__ static Vec load(const float* p) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        return Vec{{q.x, q.y, q.z, q.w}};
    }
    __device__ void store(float* p) const { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
};

// ---- elementwise: a block owns `rows_per_block` whole rows, a contiguous span of the matrix ---------------------------------------
// op 0: gather (src row rows[r]); op 1: affine32 (a = scale, b = shift, float32); op 2: standardize (ma = mean, mb = scale, float64)
template <int V, int OP>
__global__ __launch_bounds__(ELEM_BLOCK) void feat_elementwise_kernel(const float* x, float* y, int64_t n,
                                                                     int Dv, int rows_per_block, const int64_t* __restrict__ rows,
                                                                     const float* __restrict__ a, const float* __restrict__ b,
                                                                     const double* __restrict__ ma, const double* __restrict__ mb) {
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
    const int nr = (int)min((int64_t)rows_per_block, n - r0);
    const int span = nr * Dv;
    const int64_t D = (int64_t)Dv * V;
    for (int e = threadIdx.x; e < span; e += ELEM_BLOCK) {
        const int r = e / Dv, cv = e - r * Dv;
        const int c = cv * V;
        const int64_t dst = (r0 + r) * D + c;
        if (OP == 0) {
            Vec<V>::load(x + rows[r0 + r] * D + c).store(y + dst);
        } else {
            Vec<V> q = Vec<V>::load(x + dst);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                if (OP == 1) {
                    q.v[j] = __fadd_rn(__fmul_rn(q.v[j], a[c + j]), b[c + j]);
                } else {
                    const float t = (float)__dsub_rn((double)q.v[j], ma[c + j]);
                    q.v[j] = (float)__ddiv_rn((double)t, mb[c + j]);
                }
            }
            q.store(y + dst);
        }
    }
}

// ---- column reductions over one chunk of rows: one wave per (chunk, 64 lanes of columns) ------------------------------------------
// MODE 0: p0 = min, p1 = max (float); MODE 1: d0 = float64 sum in row order; MODE 2: d0 = float64 sum of (fl64(x) - mean)^2
template <int V, int MODE>
__global__ __launch_bounds__(64) void feat_colreduce_kernel(const float* __restrict__ x, int64_t n, int64_t D, const double* __restrict__ mean,
                                                           float* __restrict__ p0, float* __restrict__ p1, double* __restrict__ d0) {
    const int64_t c = ((int64_t)blockIdx.y * 64 + threadIdx.x) * V;
    if (c >= D) return;
    const int64_t r0 = (int64_t)blockIdx.x * CHUNK;
    const int nr = (int)min((int64_t)CHUNK, n - r0);
    const float* p = x + r0 * D + c;
    float lo[V], hi[V];
    double acc[V], mu[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
        lo[j] = INFINITY, hi[j] = -INFINITY, acc[j] = 0.0;
        mu[j] = MODE == 2 ? mean[c + j] : 0.0;
    }
#pragma unroll 8
    for (int r = 0; r < nr; ++r) {
        const Vec<V> q = Vec<V>::load(p + (int64_t)r * D);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            if (MODE == 0) {
                lo[j] = fminf(lo[j], q.v[j]);
                hi[j] = fmaxf(hi[j], q.v[j]);
            } else if (MODE == 1) {
                acc[j] = __dadd_rn(acc[j], (double)q.v[j]);
            } else {
                const double d = __dsub_rn((double)q.v[j], mu[j]);
                acc[j] = __dadd_rn(acc[j], __dmul_rn(d, d));
            }
        }
    }
    const int64_t o = (int64_t)blockIdx.x * D + c;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        if (MODE == 0)
            p0[o + j] = lo[j], p1[o + j] = hi[j];
        else
            d0[o + j] = acc[j];
    }
}

// the chunks' partial results of one column, in chunk order.  MODE 0: min / max; else out = sum / n
template <int MODE>
__global__ __launch_bounds__(256) void feat_combine_kernel(int64_t chunks, int64_t D, int64_t n, const float* __restrict__ p0,
                                                          const float* __restrict__ p1, const double* __restrict__ d0,
                                                          float* __restrict__ out0, float* __restrict__ out1, double* __restrict__ dout) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= D) return;
    if (MODE == 0) {
        float lo = INFINITY, hi = -INFINITY;
        for (int64_t k = 0; k < chunks; ++k) {
            lo = fminf(lo, p0[k * D + c]);
            hi = fmaxf(hi, p1[k * D + c]);
        }
        out0[c] = lo, out1[c] = hi;
    } else {
        double s = 0.0;
        for (int64_t k = 0; k < chunks; ++k) s = __dadd_rn(s, d0[k * D + c]);
        dout[c] = __ddiv_rn(s, (double)n);
    }
}

// ---- compute_stats_features: one wave per (file, 64 columns), a lane per column ---------------------------------------------------
// order-preserving image of a float's bits (NaN out of contract)
__device__ __forceinline__ uint32_t ordered_bits(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float from_ordered_bits(uint32_t u) {
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

__global__ __launch_bounds__(64) void feat_file_stats_kernel(const float* __restrict__ x, int64_t D, const int64_t* __restrict__ files,
                                                            float* __restrict__ out) {
    __shared__ float slab[LDS_ROWS * 64];
    const int lane = threadIdx.x;
    const int64_t c = (int64_t)blockIdx.y * 64 + lane;
    if (c >= D) return;          // a lane touches its own LDS column only: no barrier anywhere in this kernel
    const int64_t s = files[2 * blockIdx.x], e = files[2 * blockIdx.x + 1];
    const int F = (int)(e - s);
    const bool in_lds = F <= LDS_ROWS;          // the same for the whole block
    const float* col = x + s * D + c;
    auto at = [&](int r) { return in_lds ? slab[r * 64 + lane] : col[(int64_t)r * D]; };

    // pass 1, in row order: extrema, the float32 and float64 sums; the file goes to LDS if it fits
    float lo = INFINITY, hi = -INFINITY, sum32 = 0.f;
    double sum64 = 0.0;
#pragma unroll 4
    for (int r = 0; r < F; ++r) {
        const float v = col[(int64_t)r * D];
        if (in_lds) slab[r * 64 + lane] = v;
        lo = fminf(lo, v), hi = fmaxf(hi, v);
        sum32 = __fadd_rn(sum32, v);
        sum64 = __dadd_rn(sum64, (double)v);
    }
    const float fF = (float)F;
    const float mean32 = __fdiv_rn(sum32, fF);
    const double mean64 = __ddiv_rn(sum64, (double)F);

    // pass 2, in row order: the float32 variance and the float64 central moments
    float v32 = 0.f;
    double s2 = 0.0, s3 = 0.0, s4 = 0.0;
    for (int r = 0; r < F; ++r) {
        const float v = at(r);
        const float t = __fsub_rn(v, mean32);
        v32 = __fadd_rn(v32, __fmul_rn(t, t));
        const double d = __dsub_rn((double)v, mean64);
        const double d2 = __dmul_rn(d, d);
        s2 = __dadd_rn(s2, d2);
        s3 = __dadd_rn(s3, __dmul_rn(d2, d));
        s4 = __dadd_rn(s4, __dmul_rn(d2, d2));
    }
    const float var32 = __fdiv_rn(v32, fF);
    const double m2 = __ddiv_rn(s2, (double)F), m3 = __ddiv_rn(s3, (double)F), m4 = __ddiv_rn(s4, (double)F);
    const double thr = __dmul_rn(1e-15, mean64);          // np.finfo(np.float64).resolution * mean
    const bool zero = m2 <= __dmul_rn(thr, thr);
    const float skew = zero ? 0.f : (float)__ddiv_rn(m3, __dmul_rn(m2, __dsqrt_rn(m2)));
    const float kurt = zero ? -3.f : (float)__dsub_rn(__ddiv_rn(m4, __dmul_rn(m2, m2)), 3.0);

    // median: the element of rank k = (F - 1) / 2 by a bitwise radix select (32 counting passes), then for even F the next one up
    const int k = (F - 1) >> 1;
    uint32_t prefix = 0, mask = 0;
    int rank = k;
    for (int bit = 31; bit >= 0; --bit) {
        const uint32_t b = 1u << bit;
        int zeros = 0;
        for (int r = 0; r < F; ++r) {
            const uint32_t u = ordered_bits(at(r));
            zeros += ((u & mask) == prefix && !(u & b)) ? 1 : 0;
        }
        if (rank >= zeros) rank -= zeros, prefix |= b;
        mask |= b;
    }
    float median = from_ordered_bits(prefix);
    if (!(F & 1)) {
        // rank k + 1: the same value if it occurs more than once past rank k, else the smallest value above it
        int not_above = 0;
        uint32_t next = 0xffffffffu;
        for (int r = 0; r < F; ++r) {
            const uint32_t u = ordered_bits(at(r));
            if (u <= prefix)
                ++not_above;
            else
                next = min(next, u);
        }
        const float upper = not_above >= k + 2 ? median : from_ordered_bits(next);
        median = __fdiv_rn(__fadd_rn(median, upper), 2.f);
    }

    float* o = out + (int64_t)blockIdx.x * 7 * D + c;
    o[0] = lo, o[D] = hi, o[2 * D] = median, o[3 * D] = mean32, o[4 * D] = var32, o[5 * D] = skew, o[6 * D] = kurt;
}

// ---- assembly: the output rows in spans of `rows_per_wave`, one wave per span ----------------------------------------------------------
// table[s] = {address of segment s's first source row, its first output row}, S entries and the sentinel {nullptr, n}: segment s
// owns the output rows [table[s].first, table[s + 1].first), none of them empty.  A wave finds the segment of its first row by
// bisection and walks on from there; inside a segment source and destination are both contiguous, so the piece of a segment that
// falls into the span is one flat copy: four floats per lane where both ends are 16-byte aligned (then a tail of fewer than
// four), one float per lane otherwise.  Everything is read once and written once: non-temporal.
typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int ASM_BLOCK = 256;           // four waves
constexpr int ASM_WAVE_FLOATS = 4096;    // what one wave moves when rows are shorter than that (16 KiB)

__global__ __launch_bounds__(ASM_BLOCK) void feat_assemble_kernel(const AssembleEntry* __restrict__ table, int64_t S, float* __restrict__ y,
                                                                 int64_t n, int64_t D, int rows_per_wave) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * (ASM_BLOCK / 64) + (threadIdx.x >> 6);
    const int64_t r0 = wave * rows_per_wave;
    if (r0 >= n) return;
    const int64_t r1 = min(n, r0 + rows_per_wave);
    // the last s in [0, S) with table[s].first <= r0 (table[0].first == 0)
    int64_t s = 0, hi = S;
    while (hi - s > 1) {
        const int64_t mid = (s + hi) >> 1;
        if (table[mid].first <= r0)
            s = mid;
        else
            hi = mid;
    }
    int64_t r = r0;
    while (r < r1) {
        const int64_t first = table[s].first, next = table[s + 1].first;          // s + 1 <= S: the sentinel
        const int64_t e = min(r1, next);
        const float* src = table[s].src + (r - first) * D;
        float* dst = y + r * D;
        const int len = (int)((e - r) * D);          // <= max(ASM_WAVE_FLOATS, D) <= 2^21
        if ((((uintptr_t)src | (uintptr_t)dst) & 15) == 0) {
            const int nv = len >> 2;
#pragma unroll 4
            for (int i = lane; i < nv; i += 64)
                __builtin_nontemporal_store(__builtin_nontemporal_load(reinterpret_cast<const f32x4*>(src) + i),
                                            reinterpret_cast<f32x4*>(dst) + i);
            const int t = (nv << 2) + lane;
            if (t < len) __builtin_nontemporal_store(__builtin_nontemporal_load(src + t), dst + t);
        } else {
#pragma unroll 4
            for (int i = lane; i < len; i += 64) __builtin_nontemporal_store(__builtin_nontemporal_load(src + i), dst + i);
        }
        r = e;
        ++s;
    }
}

// ---- split: the output rows of both new matrices, A's then B's, in spans of `rows_per_wave`, one wave per span -------------------------
// table = rows_a followed by rows_b (n_out entries): output row o copies source row table[o], into ya at row o when o < n_a and into yb
// at row o - n_a otherwise.  Dv pieces of V floats per row (V = 4: 16-byte accesses, x, ya and yb hipMalloc'ed and D % 4 == 0, so every
// row starts 16-byte aligned; V = 1: 4-byte accesses).  A row of 64 pieces or more is swept by the whole wave, its index wave-uniform;
// shorter rows are taken together as one flat run of pieces, each lane finding the row of its piece.  The source may be read more
// than once (repeated indices); every output float is written once: non-temporal.  No atomics, no order between waves.
static_assert(SPLIT_BLOCK == ASM_BLOCK && SPLIT_WAVE_FLOATS == ASM_WAVE_FLOATS, "feat_split.h plans for the assembly kernel's shape");
template <int V>
struct Piece;
template <>
struct Piece<1> { typedef float type; };
template <>
struct Piece<4> { typedef f32x4 type; };

template <int V>
__global__ __launch_bounds__(SPLIT_BLOCK) void feat_split_kernel(const float* __restrict__ x, const int64_t* __restrict__ table,
                                                                float* __restrict__ ya, float* __restrict__ yb, int64_t n_a, int64_t n_out,
                                                                int Dv, int rows_per_wave) {
    typedef typename Piece<V>::type P;
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * (SPLIT_BLOCK / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t r0 = wave * rows_per_wave;
    if (r0 >= n_out) return;
    const int nr = (int)min((int64_t)rows_per_wave, n_out - r0);
    const int64_t D = (int64_t)Dv * V;
    if (Dv >= 64) {
        for (int r = 0; r < nr; ++r) {
            const int64_t o = r0 + r;
            const P* src = reinterpret_cast<const P*>(x + table[o] * D);
            P* dst = reinterpret_cast<P*>(o < n_a ? ya + o * D : yb + (o - n_a) * D);
#pragma unroll 4
            for (int i = lane; i < Dv; i += 64) __builtin_nontemporal_store(__builtin_nontemporal_load(src + i), dst + i);
        }
    } else {
        const int span = nr * Dv;          // < 64 * rows_per_wave <= SPLIT_WAVE_FLOATS
#pragma unroll 4
        for (int e = lane; e < span; e += 64) {
            const int r = e / Dv, i = e - r * Dv;
            const int64_t o = r0 + r;
            const P* src = reinterpret_cast<const P*>(x + table[o] * D);
            P* dst = reinterpret_cast<P*>(o < n_a ? ya + o * D : yb + (o - n_a) * D);
            __builtin_nontemporal_store(__builtin_nontemporal_load(src + i), dst + i);
        }
    }
}

// ---- launchers ------------------------------------------------------------------------------------------------------------------
bool vec4(const l3_feat* f) { return f->D % 4 == 0; }          // hipMalloc'ed base, rows of a multiple of 16 bytes

template <int OP>
void launch_elementwise(const l3_feat* f, const float* x, float* y, int64_t n_rows, const int64_t* rows, const float* a, const float* b,
                        const double* ma, const double* mb) {
    const int V = vec4(f) ? 4 : 1;
    const int Dv = (int)(f->D / V);
    const int rpb = std::max(1, ELEM_VECS / Dv);
    const dim3 grid((unsigned)((n_rows + rpb - 1) / rpb));
    if (V == 4)
        hipLaunchKernelGGL((feat_elementwise_kernel<4, OP>), grid, dim3(ELEM_BLOCK), 0, f->s, x, y, n_rows, Dv, rpb, rows, a, b, ma, mb);
    else
        hipLaunchKernelGGL((feat_elementwise_kernel<1, OP>), grid, dim3(ELEM_BLOCK), 0, f->s, x, y, n_rows, Dv, rpb, rows, a, b, ma, mb);
}

int64_t chunks_of(const l3_feat* f) { return (f->n + CHUNK - 1) / CHUNK; }

template <int MODE>
void launch_colreduce(const l3_feat* f, const double* mean, float* p0, float* p1, double* d0) {
    const int V = vec4(f) ? 4 : 1;
    const dim3 grid((unsigned)chunks_of(f), (unsigned)((f->D / V + 63) / 64));
    if (V == 4)
        hipLaunchKernelGGL((feat_colreduce_kernel<4, MODE>), grid, dim3(64), 0, f->s, f->x, f->n, f->D, mean, p0, p1, d0);
    else
        hipLaunchKernelGGL((feat_colreduce_kernel<1, MODE>), grid, dim3(64), 0, f->s, f->x, f->n, f->D, mean, p0, p1, d0);
}

template <int MODE>
void launch_combine(const l3_feat* f, const float* p0, const float* p1, const double* d0, float* out0, float* out1, double* dout) {
    hipLaunchKernelGGL((feat_combine_kernel<MODE>), dim3((unsigned)((f->D + 255) / 256)), dim3(256), 0, f->s, chunks_of(f), f->D, f->n, p0,
                       p1, d0, out0, out1, dout);
}

// the stream has finished and no launch failed
bool finished(l3_feat* f) { return hipStreamSynchronize(f->s) == hipSuccess && hipGetLastError() == hipSuccess; }

// the handle's matrix becomes `y` of n rows of D floats
void adopt(l3_feat* f, float* y, int64_t n, int64_t D) {
    f->bufs.release(f->x);
    f->x = y, f->n = n, f->D = D;
}

int enter(l3_feat* f, bool args_ok, const char* fn) {
    if (!f || !args_ok) return fail(L3_EINVAL, std::string(fn) + ": NULL argument");
    if (hipSetDevice(f->device) != hipSuccess) return fail(L3_EHIP, no_gpu_message(fn, f->device));
    return L3_OK;
}

}  // namespace
}  // namespace l3

using namespace l3;

extern "C" {

int l3_feat_create(int device, const float* X, int64_t n, int64_t D, l3_feat** out) {
    if (!out) return fail(L3_EINVAL, "l3_feat_create: out is NULL");
    *out = nullptr;
    if (!X || n < 1 || n > INT32_MAX || D < 1 || D > (1 << 21))
        return fail(L3_EINVAL, "l3_feat_create: need X, 1 <= n <= 2^31 - 1 rows and 1 <= D <= 2^21 columns");
    if (!device_ok(device)) return fail(L3_EHIP, no_gpu_message("l3_feat_create", device));
    l3_feat* f = new l3_feat();
    f->device = device, f->n = n, f->D = D;
    f->x = f->bufs.alloc<float>((size_t)(n * D));
    if (!f->x || hipStreamCreateWithFlags(&f->s, hipStreamNonBlocking) != hipSuccess) {
        l3_feat_destroy(f);
        return fail(L3_ENOMEM, "l3_feat_create: device allocation of " + std::to_string(n * D * 4) + " bytes failed");
    }
    if (hipMemcpyAsync(f->x, X, (size_t)(n * D) * sizeof(float), hipMemcpyHostToDevice, f->s) != hipSuccess || !finished(f)) {
        l3_feat_destroy(f);
        return fail(L3_EHIP, "l3_feat_create: copy to the device failed");
    }
    *out = f;
    return L3_OK;
}

int l3_feat_alloc(int device, int64_t n, int64_t D, l3_feat** out) {
    if (!out) return fail(L3_EINVAL, "l3_feat_alloc: out is NULL");
    *out = nullptr;
    if (n < 1 || n > INT32_MAX || D < 1 || D > (1 << 21))
        return fail(L3_EINVAL, "l3_feat_alloc: need 1 <= n <= 2^31 - 1 rows and 1 <= D <= 2^21 columns");
    if (!device_ok(device)) return fail(L3_EHIP, no_gpu_message("l3_feat_alloc", device));
    l3_feat* f = new l3_feat();
    f->device = device, f->n = n, f->D = D;
    f->x = f->bufs.alloc<float>((size_t)(n * D));
    if (!f->x || hipStreamCreateWithFlags(&f->s, hipStreamNonBlocking) != hipSuccess) {
        l3_feat_destroy(f);
        return fail(L3_ENOMEM, "l3_feat_alloc: device allocation of " + std::to_string(n * D * 4) + " bytes failed");
    }
    if (hipMemsetAsync(f->x, 0, (size_t)(n * D) * sizeof(float), f->s) != hipSuccess || !finished(f)) {
        l3_feat_destroy(f);
        return fail(L3_EHIP, "l3_feat_alloc: zero fill on the device failed");
    }
    *out = f;
    return L3_OK;
}

void l3_feat_destroy(l3_feat* f) {
    if (!f) return;
    (void)hipSetDevice(f->device);
    if (f->s) (void)hipStreamSynchronize(f->s);
    if (f->s) (void)hipStreamDestroy(f->s);
    delete f;
}

int l3_feat_shape(const l3_feat* f, int64_t* n, int64_t* D) {
    if (!f || !n || !D) return fail(L3_EINVAL, "l3_feat_shape: NULL argument");
    *n = f->n, *D = f->D;
    return L3_OK;
}

int l3_feat_download(l3_feat* f, int64_t lo, int64_t hi, float* dst) {
    const int rc = enter(f, dst != nullptr, "l3_feat_download");
    if (rc != L3_OK) return rc;
    if (lo < 0 || hi < lo || hi > f->n) return fail(L3_EINVAL, "l3_feat_download: rows [lo, hi) outside the matrix");
    if (hi == lo) return L3_OK;
    if (hipMemcpyAsync(dst, f->x + lo * f->D, (size_t)((hi - lo) * f->D) * sizeof(float), hipMemcpyDeviceToHost, f->s) != hipSuccess ||
        !finished(f))
        return fail(L3_EHIP, "l3_feat_download: copy from the device failed");
    return L3_OK;
}

int l3_feat_assemble(int device, const l3_feat_segment* segs, int64_t n_segs, l3_feat** out) {
    if (!out) return fail(L3_EINVAL, "l3_feat_assemble: out is NULL");
    std::vector<FeatSegView> views;
    for (int64_t i = 0; segs && i < n_segs; ++i) {
        const l3_feat* g = segs[i].src;
        views.push_back(g ? FeatSegView{true, g->device, g->n, g->D, g->x, segs[i].lo, segs[i].hi}
                          : FeatSegView{false, 0, 0, 0, nullptr, segs[i].lo, segs[i].hi});
    }
    AssemblePlan plan;
    std::string err;
    if (!plan_assemble(device, views.data(), segs ? n_segs : 0, &plan, &err)) return fail(L3_EINVAL, err);
    if (!device_ok(device)) return fail(L3_EHIP, no_gpu_message("l3_feat_assemble", device));
    // whatever a source's stream still holds comes first (every l3_feat call has finished when it returns, so this waits for nothing
    // unless the caller runs a call on a source from another thread, which the handle's contract forbids anyway)
    const l3_feat* seen = nullptr;
    for (int64_t i = 0; i < n_segs; ++i)
        if (segs[i].src != seen) {
            seen = segs[i].src;
            if (hipStreamSynchronize(seen->s) != hipSuccess) return fail(L3_EHIP, "l3_feat_assemble: a source's stream failed");
        }
    l3_feat* f = new l3_feat();
    f->device = device, f->n = plan.rows, f->D = plan.D;
    f->x = f->bufs.alloc<float>((size_t)(plan.rows * plan.D));
    AssembleEntry* table = nullptr;
    if (f->x && hipStreamCreateWithFlags(&f->s, hipStreamNonBlocking) == hipSuccess) table = f->bufs.put(plan.table.data(), plan.table.size(), f->s);
    if (!table) {
        l3_feat_destroy(f);
        return fail(L3_ENOMEM, "l3_feat_assemble: device allocation of " + std::to_string(plan.rows * plan.D * 4) + " bytes failed");
    }
    const int rpw = (int)std::max<int64_t>(1, ASM_WAVE_FLOATS / plan.D);
    const int64_t waves = (plan.rows + rpw - 1) / rpw, per_block = ASM_BLOCK / 64;
    hipLaunchKernelGGL(feat_assemble_kernel, dim3((unsigned)((waves + per_block - 1) / per_block)), dim3(ASM_BLOCK), 0, f->s, table,
                       (int64_t)plan.table.size() - 1, f->x, plan.rows, plan.D, rpw);
    const bool ok = finished(f);
    f->bufs.release(table);
    if (!ok) {
        l3_feat_destroy(f);
        return fail(L3_EHIP, "l3_feat_assemble: HIP error");
    }
    *out = f;
    return L3_OK;
}

int l3_feat_split(const l3_feat* src, const int64_t* rows_a, int64_t n_a, const int64_t* rows_b, int64_t n_b, l3_feat** out_a,
                  l3_feat** out_b) {
    SplitPlan plan;
    std::string err;
    if (!plan_split(src != nullptr, src ? src->n : 0, src ? src->D : 0, rows_a, n_a, rows_b, n_b, out_a != nullptr, out_b != nullptr, &plan,
                    &err))
        return fail(L3_EINVAL, err);
    if (hipSetDevice(src->device) != hipSuccess) return fail(L3_EHIP, no_gpu_message("l3_feat_split", src->device));
    // as in l3_feat_assemble: the source holds its final values at entry, and its stream is synchronised all the same
    if (hipStreamSynchronize(src->s) != hipSuccess) return fail(L3_EHIP, "l3_feat_split: the source's stream failed");
    l3_feat* parts[2] = {new l3_feat(), n_b ? new l3_feat() : nullptr};
    const int64_t counts[2] = {n_a, n_b};
    bool ok = true;
    for (int k = 0; k < 2 && ok; ++k) {
        l3_feat* f = parts[k];
        if (!f) continue;
        f->device = src->device, f->n = counts[k], f->D = src->D;
        f->x = f->bufs.alloc<float>((size_t)(counts[k] * src->D));
        ok = f->x && hipStreamCreateWithFlags(&f->s, hipStreamNonBlocking) == hipSuccess;
    }
    // both tables in one buffer, A's entries then B's; the launch runs on A's stream and writes both matrices
    l3_feat* a = parts[0];
    int64_t* table = ok ? a->bufs.alloc<int64_t>((size_t)(n_a + n_b)) : nullptr;
    if (!table) {
        l3_feat_destroy(parts[0]), l3_feat_destroy(parts[1]);
        return fail(L3_ENOMEM, "l3_feat_split: device allocation of " + std::to_string((n_a + n_b) * (src->D * 4 + 8)) + " bytes failed");
    }
    ok = hipMemcpyAsync(table, rows_a, (size_t)n_a * sizeof(int64_t), hipMemcpyHostToDevice, a->s) == hipSuccess &&
         (!n_b || hipMemcpyAsync(table + n_a, rows_b, (size_t)n_b * sizeof(int64_t), hipMemcpyHostToDevice, a->s) == hipSuccess);
    if (ok) {
        float* yb = parts[1] ? parts[1]->x : nullptr;
        const int Dv = (int)(src->D / plan.vec);
        if (plan.vec == 4)
            hipLaunchKernelGGL(feat_split_kernel<4>, dim3(plan.blocks), dim3(SPLIT_BLOCK), 0, a->s, src->x, table, a->x, yb, n_a, n_a + n_b, Dv,
                               plan.rows_per_wave);
        else
            hipLaunchKernelGGL(feat_split_kernel<1>, dim3(plan.blocks), dim3(SPLIT_BLOCK), 0, a->s, src->x, table, a->x, yb, n_a, n_a + n_b, Dv,
                               plan.rows_per_wave);
    }
    ok = finished(a) && ok;          // also after a failed copy: the stream has let go of the host tables
    a->bufs.release(table);
    if (!ok) {
        l3_feat_destroy(parts[0]), l3_feat_destroy(parts[1]);
        return fail(L3_EHIP, "l3_feat_split: HIP error");
    }
    *out_a = parts[0];
    if (n_b) *out_b = parts[1];
    return L3_OK;
}

int l3_feat_gather(l3_feat* f, const int64_t* rows, int64_t n_out) {
    const int rc = enter(f, rows != nullptr, "l3_feat_gather");
    if (rc != L3_OK) return rc;
    if (n_out < 1 || n_out > INT32_MAX) return fail(L3_EINVAL, "l3_feat_gather: need 1 <= n_out <= 2^31 - 1 rows");
    for (int64_t i = 0; i < n_out; ++i)
        if (rows[i] < 0 || rows[i] >= f->n)
            return fail(L3_EINVAL, "l3_feat_gather: rows[" + std::to_string(i) + "] = " + std::to_string(rows[i]) + " outside [0, " +
                                       std::to_string(f->n) + ")");
    float* y = f->bufs.alloc<float>((size_t)(n_out * f->D));
    int64_t* drows = f->bufs.put(rows, (size_t)n_out, f->s);
    if (!y || !drows) {
        f->bufs.release(y), f->bufs.release(drows);
        return fail(L3_ENOMEM, "l3_feat_gather: device allocation failed");
    }
    launch_elementwise<0>(f, f->x, y, n_out, drows, nullptr, nullptr, nullptr, nullptr);
    const bool ok = finished(f);
    f->bufs.release(drows);
    if (!ok) {
        f->bufs.release(y);
        return fail(L3_EHIP, "l3_feat_gather: HIP error");
    }
    adopt(f, y, n_out, f->D);
    return L3_OK;
}

int l3_feat_minmax(l3_feat* f, float* min_out, float* max_out) {
    const int rc = enter(f, min_out && max_out, "l3_feat_minmax");
    if (rc != L3_OK) return rc;
    const size_t part = (size_t)(chunks_of(f) * f->D);
    float *p0 = f->bufs.alloc<float>(part), *p1 = f->bufs.alloc<float>(part), *o = f->bufs.alloc<float>((size_t)(2 * f->D));
    int out = L3_OK;
    if (!p0 || !p1 || !o) {
        out = fail(L3_ENOMEM, "l3_feat_minmax: device allocation failed");
    } else {
        launch_colreduce<0>(f, nullptr, p0, p1, nullptr);
        launch_combine<0>(f, p0, p1, nullptr, o, o + f->D, nullptr);
        if (hipMemcpyAsync(min_out, o, f->D * sizeof(float), hipMemcpyDeviceToHost, f->s) != hipSuccess ||
            hipMemcpyAsync(max_out, o + f->D, f->D * sizeof(float), hipMemcpyDeviceToHost, f->s) != hipSuccess || !finished(f))
            out = fail(L3_EHIP, "l3_feat_minmax: HIP error");
    }
    f->bufs.release(p0), f->bufs.release(p1), f->bufs.release(o);
    return out;
}

int l3_feat_affine32(l3_feat* f, const float* scale, const float* shift) {
    const int rc = enter(f, scale && shift, "l3_feat_affine32");
    if (rc != L3_OK) return rc;
    float *a = f->bufs.put(scale, (size_t)f->D, f->s), *b = f->bufs.put(shift, (size_t)f->D, f->s);
    int out = L3_OK;
    if (!a || !b) {
        out = fail(L3_ENOMEM, "l3_feat_affine32: device allocation failed");
    } else {
        launch_elementwise<1>(f, f->x, f->x, f->n, nullptr, a, b, nullptr, nullptr);
        if (!finished(f)) out = fail(L3_EHIP, "l3_feat_affine32: HIP error");
    }
    f->bufs.release(a), f->bufs.release(b);
    return out;
}

int l3_feat_moments(l3_feat* f, double* mean_out, double* var_out) {
    const int rc = enter(f, mean_out && var_out, "l3_feat_moments");
    if (rc != L3_OK) return rc;
    double *part = f->bufs.alloc<double>((size_t)(chunks_of(f) * f->D)), *o = f->bufs.alloc<double>((size_t)(2 * f->D));
    int out = L3_OK;
    if (!part || !o) {
        out = fail(L3_ENOMEM, "l3_feat_moments: device allocation failed");
    } else {
        launch_colreduce<1>(f, nullptr, nullptr, nullptr, part);
        launch_combine<1>(f, nullptr, nullptr, part, nullptr, nullptr, o);
        launch_colreduce<2>(f, o, nullptr, nullptr, part);
        launch_combine<2>(f, nullptr, nullptr, part, nullptr, nullptr, o + f->D);
        if (hipMemcpyAsync(mean_out, o, f->D * sizeof(double), hipMemcpyDeviceToHost, f->s) != hipSuccess ||
            hipMemcpyAsync(var_out, o + f->D, f->D * sizeof(double), hipMemcpyDeviceToHost, f->s) != hipSuccess || !finished(f))
            out = fail(L3_EHIP, "l3_feat_moments: HIP error");
    }
    f->bufs.release(part), f->bufs.release(o);
    return out;
}

int l3_feat_standardize(l3_feat* f, const double* mean, const double* scale) {
    const int rc = enter(f, mean && scale, "l3_feat_standardize");
    if (rc != L3_OK) return rc;
    double *a = f->bufs.put(mean, (size_t)f->D, f->s), *b = f->bufs.put(scale, (size_t)f->D, f->s);
    int out = L3_OK;
    if (!a || !b) {
        out = fail(L3_ENOMEM, "l3_feat_standardize: device allocation failed");
    } else {
        launch_elementwise<2>(f, f->x, f->x, f->n, nullptr, nullptr, nullptr, a, b);
        if (!finished(f)) out = fail(L3_EHIP, "l3_feat_standardize: HIP error");
    }
    f->bufs.release(a), f->bufs.release(b);
    return out;
}

int l3_feat_file_stats(l3_feat* f, const int64_t* file_idxs, int64_t n_files) {
    const int rc = enter(f, file_idxs != nullptr, "l3_feat_file_stats");
    if (rc != L3_OK) return rc;
    if (n_files < 1 || n_files > INT32_MAX) return fail(L3_EINVAL, "l3_feat_file_stats: need 1 <= n_files <= 2^31 - 1");
    if (7 * f->D > (1 << 21)) return fail(L3_EINVAL, "l3_feat_file_stats: 7 D exceeds the 2^21 columns of a matrix");
    for (int64_t i = 0; i < n_files; ++i) {
        const int64_t s = file_idxs[2 * i], e = file_idxs[2 * i + 1];
        if (s < 0 || e <= s || e > f->n)
            return fail(L3_EINVAL, "l3_feat_file_stats: file " + std::to_string(i) + " = [" + std::to_string(s) + ", " +
                                       std::to_string(e) + ") is empty or outside [0, " + std::to_string(f->n) + ")");
    }
    float* y = f->bufs.alloc<float>((size_t)(n_files * 7 * f->D));
    int64_t* files = f->bufs.put(file_idxs, (size_t)(2 * n_files), f->s);
    if (!y || !files) {
        f->bufs.release(y), f->bufs.release(files);
        return fail(L3_ENOMEM, "l3_feat_file_stats: device allocation failed");
    }
    hipLaunchKernelGGL(feat_file_stats_kernel, dim3((unsigned)n_files, (unsigned)((f->D + 63) / 64)), dim3(64), 0, f->s, f->x, f->D, files,
                       y);
    const bool ok = finished(f);
    f->bufs.release(files);
    if (!ok) {
        f->bufs.release(y);
        return fail(L3_EHIP, "l3_feat_file_stats: HIP error");
    }
    adopt(f, y, n_files, 7 * f->D);
    return L3_OK;
}

}  // extern "C"
