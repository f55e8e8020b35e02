// eig.hip -- the device side of a top-k eigensolver of a symmetric float64 matrix by block subspace iteration (include/l3hip.h, "Symmetric
// top-k problems"; DESIGN.md section 8v, "The subspace solver").  A handle holds S (D, D) and two blocks of m vectors, V and W, the
// rows of (m, D) row-major float64 matrices, as PCA.components_ is.  The iteration itself, its Rayleigh-Ritz steps and its
// orthonormalisation are the caller's (l3embedding_amd/eigen.py): the m x m problems go to LAPACK on the host, everything that is
// D long stays here.
//
// The contract is the arithmetic, and this file is compiled with -ffp-contract=off (_build.py):
//   apply / gram / mix   every output entry is ONE float64 accumulator of v_mfma_f64_16x16x4_f64 that takes its reduction index in
//             ascending steps of 4 from 0, the steps past the end padded with zeros.  Nothing splits a reduction over waves, workgroups
//             or a second pass, so the order is a function of (D, m) alone and two calls give the same bits.  The order of the four
//             products inside one instruction is the hardware's: the claim is the bound |c - exact| <= gamma_(K + 1) sum |a b|, gamma_n
//             = n u / (1 - n u), u = 2^-53, K the reduction length, and not equality with an ascending chain.
//   gram      with a == b only the entries i <= j are computed, and each is written to (i, j) and (j, i).
//   mix       always into a third block, which then takes the place of dst: dst may be src.
//   residual  r = fl(w - fl(theta v)) entry by entry; a row's sum of r^2 is 256 sequential partial sums (lane t takes the entries t,
//             t + 256, ... in ascending order, each square rounded once and added) folded by a fixed binary tree; one correctly rounded
//             square root.
//   trace     the diagonal is copied and summed on the host in ascending order.
//
// The tile.  One kernel serves the three products: C (M, N) = A (M, K) . B, with A row major along K and B either (N, K) row major
// along K (apply: B = S, which equals its transpose; gram: B = the other block) or (K, N) row major along N (mix: B = the source
// block).  A workgroup of 4 waves owns a 64 x 64 tile of C; wave w the 32 x 32 quarter (w >> 1, w & 1) as 2 x 2 accumulators of 16 x
// 16.  A chunk of 16 reduction indices of both panels is staged in LDS, double buffered with one barrier a chunk: the next chunk's
// global loads are issued before this chunk's 16 matrix instructions a wave, which take 64 cycles each and hide them.  A panel along
// K is staged as [row][18]: lane (r = l & 15, k = l >> 4) of a k-step reads [r][4 s + k], and 36 r + 2 k (in 4-byte banks) is distinct
// over each half wave.  A panel along N is staged as [k][80]: the two k of a half wave are 32 banks apart.  The workgroups are numbered
// so that the tiles which share a panel of B (the M tiles of one N tile) follow each other on one XCD and share its L2
// (device_common.h xcd_remap): S is D^2 float64 and is read ceil(m / 64) times a product.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/l3hip.h"
#include "device_common.h"
#include "host_common.h"
#include "pca.h"

namespace l3 {
namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int BLOCK = 256;
constexpr int TM = 64, TN = 64;          // the tile of C
constexpr int KC = 16;                   // reduction indices of a staged chunk
constexpr int LDK = KC + 2;              // doubles of a staged row of a panel along K
constexpr int LDN = TN + 16;             // doubles of a staged row of a panel along N
constexpr int A_STAGE = TM * LDK;
constexpr int B_STAGE = TN * LDK > KC * LDN ? TN * LDK : KC * LDN;
constexpr int NA = TM * KC / 2 / BLOCK;          // pairs of doubles a lane stages per chunk and panel
static_assert(NA * 2 * BLOCK == TM * KC && TM == TN, "a chunk of a panel is NA pairs a lane");

// a pair of consecutive doubles p[0], p[1] of a row that ends at p[left - 1]: zeros past the end; one 16-byte load when `vec`
__device__ __forceinline__ double2 load_pair(const double* __restrict__ p, int left, bool vec) {
    double2 v = make_double2(0.0, 0.0);
    if (left >= 2 && vec) return *reinterpret_cast<const double2*>(p);
    if (left >= 1) v.x = p[0];
    if (left >= 2) v.y = p[1];
    return v;
}

// a panel along K: rows r0 .. r0 + 63 of X (rows, ld), reduction indices k0 .. k0 + 15.  Lane tid stages the pairs (row tid >> 3 + 32 i,
// k 2 (tid & 7)): eight lanes read 128 consecutive bytes of a row.
__device__ __forceinline__ void fetch_k(double2 (&pre)[NA], const double* __restrict__ X, int ld, int rows, int K, int r0, int k0, int tid, bool vec) {
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        const int r = r0 + (tid >> 3) + 32 * i, k = k0 + 2 * (tid & 7);
        pre[i] = r < rows && k < K ? load_pair(X + (int64_t)r * ld + k, K - k, vec) : make_double2(0.0, 0.0);
    }
}

__device__ __forceinline__ void store_k(double* st, const double2 (&pre)[NA], int tid) {
#pragma unroll
    for (int i = 0; i < NA; ++i) *reinterpret_cast<double2*>(st + ((tid >> 3) + 32 * i) * LDK + 2 * (tid & 7)) = pre[i];
}

// a panel along N: reduction indices (rows of X) k0 .. k0 + 15, columns c0 .. c0 + 63.  Lane tid stages the pairs (k tid >> 5 + 8 i,
// column 2 (tid & 31)).
__device__ __forceinline__ void fetch_n(double2 (&pre)[NA], const double* __restrict__ X, int ld, int K, int cols, int k0, int c0, int tid, bool vec) {
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        const int k = k0 + (tid >> 5) + 8 * i, c = c0 + 2 * (tid & 31);
        pre[i] = k < K && c < cols ? load_pair(X + (int64_t)k * ld + c, cols - c, vec) : make_double2(0.0, 0.0);
    }
}

__device__ __forceinline__ void store_n(double* st, const double2 (&pre)[NA], int tid) {
#pragma unroll
    for (int i = 0; i < NA; ++i) *reinterpret_cast<double2*>(st + ((tid >> 5) + 8 * i) * LDN + 2 * (tid & 31)) = pre[i];
}

// C[i][j] = sum over k of A[i][k] B(k, j) for i < M, j < N: B(k, j) = B[j][k] (BN false) or B[k][j] (BN true).  sym: A and B are one
// block and C is M x M: the tiles below the diagonal are left out, and an entry i <= j is written to (i, j) and to (j, i).
// Workgroup b: the tile (b' % MT, b' / MT) of the MT x NT tiles, b' = xcd_remap(b).
template <bool BN>
__global__ __launch_bounds__(BLOCK) void eig_product_kernel(const double* __restrict__ A, int lda, const double* __restrict__ B, int ldb,
                                                            double* __restrict__ C, int ldc, int M, int N, int K, int MT, int sym) {
    __shared__ __attribute__((aligned(16))) double stage[2 * (A_STAGE + B_STAGE)];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, q = lane >> 4;
    const int t = xcd_remap((int)blockIdx.x, (int)gridDim.x);
    const int i0 = (t % MT) * TM, j0 = (t / MT) * TN;
    if (sym && i0 > j0) return;          // (the whole workgroup: no barrier is left behind)
    const bool vec_a = (lda & 1) == 0, vec_b = (ldb & 1) == 0;
    const int chunks = (K + KC - 1) / KC;

    f64x4 acc[2][2] = {};
    double2 pa[NA], pb[NA];
    fetch_k(pa, A, lda, M, K, i0, 0, tid, vec_a);
    if (BN) fetch_n(pb, B, ldb, K, N, 0, j0, tid, vec_b);
    else fetch_k(pb, B, ldb, N, K, j0, 0, tid, vec_b);
    for (int c = 0; c < chunks; ++c) {
        double* sa = stage + (c & 1) * (A_STAGE + B_STAGE);
        double* sb = sa + A_STAGE;
        // (this buffer was last read two chunks ago, and every wave has passed the barrier of the chunk between)
        store_k(sa, pa, tid);
        if (BN) store_n(sb, pb, tid);
        else store_k(sb, pb, tid);
        __syncthreads();
        if (c + 1 < chunks) {
            fetch_k(pa, A, lda, M, K, i0, (c + 1) * KC, tid, vec_a);
            if (BN) fetch_n(pb, B, ldb, K, N, (c + 1) * KC, j0, tid, vec_b);
            else fetch_k(pb, B, ldb, N, K, j0, (c + 1) * KC, tid, vec_b);
        }
        const double* ar = sa + (32 * (w >> 1) + r) * LDK + q;
        const double* br = BN ? sb + q * LDN + 32 * (w & 1) + r : sb + (32 * (w & 1) + r) * LDK + q;
#pragma unroll
        for (int s = 0; s < KC / 4; ++s) {          // k-step s: lane (r, q) holds A[r][4 s + q] and B(4 s + q, r)
            const double a0 = ar[4 * s], a1 = ar[16 * LDK + 4 * s];
            const double b0 = BN ? br[4 * s * LDN] : br[4 * s];
            const double b1 = BN ? br[4 * s * LDN + 16] : br[16 * LDK + 4 * s];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
    // register g of lane (r, q) is row q + 4 g, column r of its 16 x 16 result
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int i = i0 + 32 * (w >> 1) + 16 * u + q + 4 * g, j = j0 + 32 * (w & 1) + 16 * v + r;
                if (i >= M || j >= N) continue;
                if (!sym) {
                    C[(int64_t)i * ldc + j] = acc[u][v][g];
                } else if (i <= j) {
                    C[(int64_t)i * ldc + j] = acc[u][v][g];
                    C[(int64_t)j * ldc + i] = acc[u][v][g];
                }
            }
}

// res[j] = sqrt(sum over d of fl(w[j][d] - fl(theta[j] v[j][d]))^2): workgroup j, lane t the entries t, t + 256, ... in ascending order,
// then a binary tree over the 256 partial sums in a fixed order
__global__ __launch_bounds__(BLOCK) void eig_residual_kernel(const double* __restrict__ V, const double* __restrict__ W, const double* __restrict__ theta,
                                                             int D, double* __restrict__ res) {
    __shared__ double part[BLOCK];
    const int j = blockIdx.x, tid = threadIdx.x;
    const double th = theta[j];
    const double *v = V + (int64_t)j * D, *wr = W + (int64_t)j * D;
    double acc = 0.0;
    for (int d = tid; d < D; d += BLOCK) {
        const double e = wr[d] - th * v[d];
        acc += e * e;
    }
    part[tid] = acc;
    __syncthreads();
    for (int half = BLOCK / 2; half > 0; half >>= 1) {
        if (tid < half) part[tid] += part[tid + half];
        __syncthreads();
    }
    if (tid == 0) res[j] = sqrt(part[0]);
}

__global__ __launch_bounds__(BLOCK) void eig_diagonal_kernel(const double* __restrict__ S, int D, double* __restrict__ diag) {
    const int d = blockIdx.x * BLOCK + threadIdx.x;
    if (d < D) diag[d] = S[(int64_t)d * D + d];
}

}  // namespace
}  // namespace l3

struct l3_eig {
    int device = 0, D = 0, m = 0;
    hipStream_t s = nullptr;
    l3::DeviceBufs bufs;
    double* S = nullptr;                    // (D, D)
    double* block[3] = {};                  // V, W and the block a mix writes, which then changes places with its dst: (m, D) each
    double *Mx = nullptr, *G = nullptr;     // (m, m): the matrix of a mix, the result of a gram
    double *theta = nullptr, *res = nullptr, *diag = nullptr;
    bool has_S = false;
};

namespace l3 {
namespace {

bool finished(hipStream_t s) { return hipStreamSynchronize(s) == hipSuccess && hipGetLastError() == hipSuccess; }

unsigned tiles_of(int n, int per) { return (unsigned)((n + per - 1) / per); }

int enter(l3_eig* h, const char* fn) {
    if (!h) return fail(L3_EINVAL, std::string(fn) + ": NULL handle");
    if (hipSetDevice(h->device) != hipSuccess) return fail(L3_EHIP, no_gpu_message(fn, h->device));
    return L3_OK;
}

int need_matrix(const l3_eig* h, const char* fn) {
    if (!h->has_S) return fail(L3_ESTATE, std::string(fn) + ": the matrix comes first (l3_eig_set_matrix or l3_eig_set_matrix_pca)");
    return L3_OK;
}

int check_which(int which, const char* name, const char* fn) {
    if (which != L3_EIG_V && which != L3_EIG_W)
        return fail(L3_EINVAL, std::string(fn) + ": " + name + " must be L3_EIG_V or L3_EIG_W, not " + std::to_string(which));
    return L3_OK;
}

template <bool BN>
void launch_product(l3_eig* h, const double* A, int lda, const double* B, int ldb, double* C, int ldc, int M, int N, int K, bool sym) {
    const unsigned MT = tiles_of(M, TM), NT = tiles_of(N, TN);
    hipLaunchKernelGGL((eig_product_kernel<BN>), dim3(MT * NT), dim3(BLOCK), 0, h->s, A, lda, B, ldb, C, ldc, M, N, K, (int)MT, sym ? 1 : 0);
}

// W = V S^T, and S^T = S
void launch_apply(l3_eig* h) { launch_product<false>(h, h->block[L3_EIG_V], h->D, h->S, h->D, h->block[L3_EIG_W], h->D, h->m, h->D, h->D, false); }

void launch_gram(l3_eig* h, int a, int b) {
    launch_product<false>(h, h->block[a], h->D, h->block[b], h->D, h->G, h->m, h->m, h->m, h->D, a == b);
}

// block[2] = Mx block[src]
void launch_mix(l3_eig* h, int src) { launch_product<true>(h, h->Mx, h->m, h->block[src], h->D, h->block[2], h->D, h->m, h->D, h->m, false); }

void launch_residual(l3_eig* h) {
    hipLaunchKernelGGL(eig_residual_kernel, dim3((unsigned)h->m), dim3(BLOCK), 0, h->s, h->block[L3_EIG_V], h->block[L3_EIG_W], h->theta, h->D, h->res);
}

}  // namespace
}  // namespace l3

using namespace l3;

extern "C" {

int l3_eig_create(int device, int D, int m, l3_eig** out) {
    const char* fn = "l3_eig_create";
    if (!out) return fail(L3_EINVAL, std::string(fn) + ": out is NULL");
    *out = nullptr;
    if (D < 1 || D > L3_PCA_MAX_D) return fail(L3_EINVAL, std::string(fn) + ": need 1 <= D <= " + std::to_string(L3_PCA_MAX_D) + ", not " + std::to_string(D));
    if (m < 1 || m > std::min(D, L3_EIG_MAX_M))
        return fail(L3_EINVAL, std::string(fn) + ": need 1 <= m <= min(D, " + std::to_string(L3_EIG_MAX_M) + ") vectors, not " + std::to_string(m));
    if (!device_ok(device)) return fail(L3_EHIP, no_gpu_message(fn, device));
    l3_eig* h = new l3_eig();
    h->device = device, h->D = D, h->m = m;
    if (hipStreamCreateWithFlags(&h->s, hipStreamNonBlocking) != hipSuccess) {
        h->s = nullptr;
        l3_eig_destroy(h);
        return fail(L3_EHIP, std::string(fn) + ": hipStreamCreate failed");
    }
    const size_t DD = (size_t)D * D, mD = (size_t)m * D, mm = (size_t)m * m;
    h->S = h->bufs.alloc<double>(DD);
    for (double*& b : h->block) b = h->bufs.alloc<double>(mD);
    h->Mx = h->bufs.alloc<double>(mm);
    h->G = h->bufs.alloc<double>(mm);
    h->theta = h->bufs.alloc<double>((size_t)m);
    h->res = h->bufs.alloc<double>((size_t)m);
    h->diag = h->bufs.alloc<double>((size_t)D);
    bool ok = h->bufs.ok();
    // blocks that were never set are zeros, not whatever the allocation held
    for (int b = 0; ok && b < 3; ++b) ok = hipMemsetAsync(h->block[b], 0, mD * sizeof(double), h->s) == hipSuccess;
    ok = ok && hipMemsetAsync(h->Mx, 0, mm * sizeof(double), h->s) == hipSuccess;
    ok = ok && hipMemsetAsync(h->theta, 0, (size_t)m * sizeof(double), h->s) == hipSuccess && finished(h->s);
    if (!ok) {
        l3_eig_destroy(h);
        return fail(L3_ENOMEM, std::string(fn) + ": device allocation of " + std::to_string((DD + 3 * mD + 2 * mm) * sizeof(double)) + " bytes failed");
    }
    *out = h;
    return L3_OK;
}

void l3_eig_destroy(l3_eig* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->s) (void)hipStreamSynchronize(h->s);
    if (h->s) (void)hipStreamDestroy(h->s);
    delete h;
}

int l3_eig_set_matrix(l3_eig* h, const double* S) {
    const char* fn = "l3_eig_set_matrix";
    if (int rc = enter(h, fn)) return rc;
    if (!S) return fail(L3_EINVAL, std::string(fn) + ": S is NULL");
    h->has_S = false;
    // the lowest (i, j) in row-major order that is not finite or differs from (j, i) in its bits.  Entries i <= j suffice: an offender
    // below the diagonal has its mirror image, which comes first, either equal to it (and then not finite) or different from it.
    const int D = h->D, FB = 64;
    int64_t bad = -1;
    for (int bi = 0; bi < D; bi += FB)
        for (int bj = bi; bj < D; bj += FB)
            for (int i = bi; i < std::min(D, bi + FB); ++i)
                for (int j = std::max(i, bj); j < std::min(D, bj + FB); ++j) {
                    const double x = S[(size_t)i * D + j], y = S[(size_t)j * D + i];
                    if (std::isfinite(x) && memcmp(&x, &y, sizeof(double)) == 0) continue;
                    const int64_t at = (int64_t)i * D + j;
                    if (bad < 0 || at < bad) bad = at;
                }
    if (bad >= 0) {
        const int i = (int)(bad / D), j = (int)(bad % D);
        const std::string where = "entry (" + std::to_string(i) + ", " + std::to_string(j) + ")";
        if (!std::isfinite(S[bad])) return fail(L3_EINVAL, std::string(fn) + ": " + where + " is not finite");
        return fail(L3_EINVAL, std::string(fn) + ": " + where + " differs from entry (" + std::to_string(j) + ", " + std::to_string(i) + "): the matrix is not symmetric");
    }
    if (hipMemcpyAsync(h->S, S, (size_t)D * D * sizeof(double), hipMemcpyHostToDevice, h->s) != hipSuccess || !finished(h->s))
        return fail(L3_EHIP, std::string(fn) + ": copy to the device failed");
    h->has_S = true;
    return L3_OK;
}

int l3_eig_set_matrix_pca(l3_eig* h, const l3_pca* pca) {
    const char* fn = "l3_eig_set_matrix_pca";
    if (int rc = enter(h, fn)) return rc;
    if (!pca) return fail(L3_EINVAL, std::string(fn) + ": the l3_pca handle is NULL");
    if (pca->device != h->device)
        return fail(L3_EINVAL, std::string(fn) + ": the l3_pca is on device " + std::to_string(pca->device) + ", the handle on device " + std::to_string(h->device));
    if (pca->D != h->D) return fail(L3_EINVAL, std::string(fn) + ": the l3_pca has " + std::to_string(pca->D) + " features, the handle " + std::to_string(h->D));
    const double* S = pca_resident_scatter(pca);
    if (!S) return fail(L3_ESTATE, std::string(fn) + ": the l3_pca holds no scatter matrix (l3_pca_scatter comes first)");
    h->has_S = false;
    // (every l3_pca call has finished on its stream when it returns: S holds its final values, finite and equal to its transpose)
    if (hipMemcpyAsync(h->S, S, (size_t)h->D * h->D * sizeof(double), hipMemcpyDeviceToDevice, h->s) != hipSuccess || !finished(h->s))
        return fail(L3_EHIP, std::string(fn) + ": the copy on the device failed");
    h->has_S = true;
    return L3_OK;
}

int l3_eig_trace(l3_eig* h, double* trace) {
    const char* fn = "l3_eig_trace";
    if (int rc = enter(h, fn)) return rc;
    if (!trace) return fail(L3_EINVAL, std::string(fn) + ": trace is NULL");
    if (int rc = need_matrix(h, fn)) return rc;
    std::vector<double> diag((size_t)h->D);
    hipLaunchKernelGGL(eig_diagonal_kernel, dim3(tiles_of(h->D, BLOCK)), dim3(BLOCK), 0, h->s, h->S, h->D, h->diag);
    if (hipMemcpyAsync(diag.data(), h->diag, diag.size() * sizeof(double), hipMemcpyDeviceToHost, h->s) != hipSuccess || !finished(h->s))
        return fail(L3_EHIP, std::string(fn) + ": the kernel or the copy from the device failed");
    double t = 0.0;
    for (double d : diag) t += d;
    *trace = t;
    return L3_OK;
}

int l3_eig_set_block(l3_eig* h, int which, const double* B) {
    const char* fn = "l3_eig_set_block";
    if (int rc = enter(h, fn)) return rc;
    if (!B) return fail(L3_EINVAL, std::string(fn) + ": B is NULL");
    if (int rc = check_which(which, "which", fn)) return rc;
    if (hipMemcpyAsync(h->block[which], B, (size_t)h->m * h->D * sizeof(double), hipMemcpyHostToDevice, h->s) != hipSuccess || !finished(h->s))
        return fail(L3_EHIP, std::string(fn) + ": copy to the device failed");
    return L3_OK;
}

int l3_eig_get_block(l3_eig* h, int which, double* B) {
    const char* fn = "l3_eig_get_block";
    if (int rc = enter(h, fn)) return rc;
    if (!B) return fail(L3_EINVAL, std::string(fn) + ": B is NULL");
    if (int rc = check_which(which, "which", fn)) return rc;
    if (hipMemcpyAsync(B, h->block[which], (size_t)h->m * h->D * sizeof(double), hipMemcpyDeviceToHost, h->s) != hipSuccess || !finished(h->s))
        return fail(L3_EHIP, std::string(fn) + ": copy from the device failed");
    return L3_OK;
}

int l3_eig_apply(l3_eig* h) {
    const char* fn = "l3_eig_apply";
    if (int rc = enter(h, fn)) return rc;
    if (int rc = need_matrix(h, fn)) return rc;
    launch_apply(h);
    if (!finished(h->s)) return fail(L3_EHIP, std::string(fn) + ": the kernel failed");
    return L3_OK;
}

int l3_eig_gram(l3_eig* h, int a, int b, double* G) {
    const char* fn = "l3_eig_gram";
    if (int rc = enter(h, fn)) return rc;
    if (!G) return fail(L3_EINVAL, std::string(fn) + ": G is NULL");
    if (int rc = check_which(a, "a", fn)) return rc;
    if (int rc = check_which(b, "b", fn)) return rc;
    launch_gram(h, a, b);
    if (hipMemcpyAsync(G, h->G, (size_t)h->m * h->m * sizeof(double), hipMemcpyDeviceToHost, h->s) != hipSuccess || !finished(h->s))
        return fail(L3_EHIP, std::string(fn) + ": the kernel or the copy from the device failed");
    return L3_OK;
}

int l3_eig_mix(l3_eig* h, int src, const double* M, int dst) {
    const char* fn = "l3_eig_mix";
    if (int rc = enter(h, fn)) return rc;
    if (!M) return fail(L3_EINVAL, std::string(fn) + ": M is NULL");
    if (int rc = check_which(src, "src", fn)) return rc;
    if (int rc = check_which(dst, "dst", fn)) return rc;
    if (hipMemcpyAsync(h->Mx, M, (size_t)h->m * h->m * sizeof(double), hipMemcpyHostToDevice, h->s) != hipSuccess)
        return fail(L3_EHIP, std::string(fn) + ": copy to the device failed");
    launch_mix(h, src);
    if (!finished(h->s)) return fail(L3_EHIP, std::string(fn) + ": the kernel failed");
    std::swap(h->block[dst], h->block[2]);
    return L3_OK;
}

int l3_eig_residual(l3_eig* h, const double* theta, double* res) {
    const char* fn = "l3_eig_residual";
    if (int rc = enter(h, fn)) return rc;
    if (!theta || !res) return fail(L3_EINVAL, std::string(fn) + ": theta and res must not be NULL");
    if (hipMemcpyAsync(h->theta, theta, (size_t)h->m * sizeof(double), hipMemcpyHostToDevice, h->s) != hipSuccess)
        return fail(L3_EHIP, std::string(fn) + ": copy to the device failed");
    launch_residual(h);
    if (hipMemcpyAsync(res, h->res, (size_t)h->m * sizeof(double), hipMemcpyDeviceToHost, h->s) != hipSuccess || !finished(h->s))
        return fail(L3_EHIP, std::string(fn) + ": the kernel or the copy from the device failed");
    return L3_OK;
}

// Device time of `reps` rounds on the resident matrix and blocks, in ms per round (hipEvents; one untimed round first).  what 0:
// apply; 1: gram(V, W); 2: the product of a mix of V by the resident m x m matrix, into the third block (no block changes places); 3:
// residual with the resident theta.  For profiles/ records; no test asserts a time.
int l3_eig_time(l3_eig* h, int what, int reps, double* ms) {
    const char* fn = "l3_eig_time";
    if (int rc = enter(h, fn)) return rc;
    if (!ms || reps < 1 || what < 0 || what > 3) return fail(L3_EINVAL, std::string(fn) + ": need ms, reps >= 1 and what in [0, 3]");
    if (what == 0)
        if (int rc = need_matrix(h, fn)) return rc;
    hipEvent_t a, b;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return fail(L3_EHIP, std::string(fn) + ": hipEventCreate failed");
    auto run = [&](int count) {
        for (int r = 0; r < count; ++r) {
            if (what == 0) launch_apply(h);
            else if (what == 1) launch_gram(h, L3_EIG_V, L3_EIG_W);
            else if (what == 2) launch_mix(h, L3_EIG_V);
            else launch_residual(h);
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

}  // extern "C"
