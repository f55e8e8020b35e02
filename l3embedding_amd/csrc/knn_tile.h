// knn_tile.h -- the distance arithmetic that csrc/knn.hip and csrc/kmeans.hip share: the epilogue of one pair and the 128 x 128 tile of
// dot products on the fp32 matrix cores.  A pair's bits are this chain's and nothing else's (include/l3hip.h, "Nearest neighbours"
// and "K-means"): v_mfma_f32_32x32x2_f32 with one accumulator taking the k-steps in ascending order is the ascending fmaf chain, D is
// never split over waves or accumulators, and a k past D is a zero in both operands.  A file that includes this is compiled with
// -ffp-contract=off (_build.py): the epilogue's multiplications and subtractions stay separate roundings.  csrc/pca.hip projects with
// the same tile (rows against components) and centres the rows as it fetches them (PRE below).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/l3hip.h"
#include "device_common.h"

namespace l3 {
namespace knn_tile {

constexpr int BLOCK = 256;
constexpr int TQ = 128, TC = 128;           // queries and candidates of a workgroup's tile
constexpr int KC = 32, LDK = KC + 1;        // features of a staged chunk; LDS row of 32 + 1

__device__ __forceinline__ float distance_of(int metric, float dot, float sq, float sc) {
    if (metric == L3_KNN_COSINE) return __fsub_rn(1.0f, __fmul_rn(__fmul_rn(dot, sq), sc));
    const float x = __fsub_rn(__fadd_rn(sq, sc), __fmul_rn(2.0f, dot));
    return x < 0.0f ? 0.0f : x;          // (fmaxf would turn a NaN into 0)
}

// ---- the tile's dot products ------------------------------------------------------------------------------------------------------
// A chunk is 256 rows (128 queries, then 128 candidates) of 32 features: 2048 float4, 8 a lane; slot e = tid + 256 i is row e >> 3,
// features 4 (e & 7) .. + 3, so i < 4 are query rows and i >= 4 candidate rows.
// PRE (csrc/pca.hip): one float32 operation on a query row's feature k as it is fetched, with qp[k]: PRE_SUB fl(q[k] - qp[k]), PRE_DIV
// fl(q[k] / qp[k]).  A k past D stays the zero it is.  PRE_NONE (knn.hip, kmeans.hip) fetches the rows as they are.
enum { PRE_NONE = 0, PRE_SUB = 1, PRE_DIV = 2 };
template <int PRE>
__device__ __forceinline__ float fetched(float x, float p) {
    return PRE == PRE_SUB ? __fsub_rn(x, p) : __fdiv_rn(x, p);
}

template <int PRE = PRE_NONE>
__device__ __forceinline__ void fetch_chunk(float4 (&pre)[8], const float* __restrict__ Q, const float* __restrict__ Cd, int D, bool vec,
                                            int64_t i0, int64_t nq, int64_t j0, int64_t nc, int k0, int tid,
                                            const float* __restrict__ qp = nullptr) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int e = tid + BLOCK * i, row = e >> 3, k = k0 + (e & 7) * 4;
        const bool isq = i < 4;
        const int64_t g = isq ? i0 + row : j0 + (row - TQ);
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (g < (isq ? nq : nc) && k < D) {
            const float* p = (isq ? Q : Cd) + g * D + k;
            if (vec) {          // D % 4 == 0: the four features are inside the row together
                v = *reinterpret_cast<const float4*>(p);
            } else {
                v.x = p[0];
                if (k + 1 < D) v.y = p[1];
                if (k + 2 < D) v.z = p[2];
                if (k + 3 < D) v.w = p[3];
            }
            if constexpr (PRE != PRE_NONE) {
                if (isq) {
                    v.x = fetched<PRE>(v.x, qp[k]);
                    if (k + 1 < D) v.y = fetched<PRE>(v.y, qp[k + 1]);
                    if (k + 2 < D) v.z = fetched<PRE>(v.z, qp[k + 2]);
                    if (k + 3 < D) v.w = fetched<PRE>(v.w, qp[k + 3]);
                }
            }
        }
        pre[i] = v;
    }
}

__device__ __forceinline__ void store_chunk(const float4 (&pre)[8], float* stage, int tid) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int e = tid + BLOCK * i;
        float* s = stage + (e >> 3) * LDK + (e & 7) * 4;
        s[0] = pre[i].x, s[1] = pre[i].y, s[2] = pre[i].z, s[3] = pre[i].w;
    }
}

// acc[t][i] += dot of query row i0 + 32 w + mfma_row(i, h) and candidate j0 + 32 t + r, lane = (r, h).  Every lane of the workgroup
// comes here (barriers); stage holds (TQ + TC) x LDK floats.  The last chunk's reads of the stage may still be going on in other
// waves when a wave returns.
template <int PRE = PRE_NONE>
__device__ __forceinline__ void accumulate_tile(f32x16 (&acc)[4], float* stage, const float* __restrict__ Q, const float* __restrict__ Cd,
                                                int D, int64_t i0, int64_t nq, int64_t j0, int64_t nc, int tid,
                                                const float* __restrict__ qp = nullptr) {
    const int lane = tid & 63, r = lane & 31, h = lane >> 5, w = tid >> 6;
    const bool vec = (D & 3) == 0;
    float4 pre[8];
    fetch_chunk<PRE>(pre, Q, Cd, D, vec, i0, nq, j0, nc, 0, tid, qp);
    const float* qrow = stage + (32 * w + r) * LDK + h;
    const float* crow = stage + (TQ + r) * LDK + h;
    for (int k0 = 0; k0 < D; k0 += KC) {
        __syncthreads();          // the chunk before has been read
        store_chunk(pre, stage, tid);
        __syncthreads();
        if (k0 + KC < D) fetch_chunk<PRE>(pre, Q, Cd, D, vec, i0, nq, j0, nc, k0 + KC, tid, qp);
#pragma unroll 4
        for (int s = 0; s < KC / 2; ++s) {          // k-step s: features k0 + 2 s (lanes h = 0) and k0 + 2 s + 1 (h = 1), in that order
            const float a = qrow[2 * s];
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, crow[t * 32 * LDK + 2 * s], acc[t], 0, 0, 0);
        }
    }
}

// The distances of the tile, from the accumulators to M[query][candidate] (TQ x TC floats): wave w writes the rows 32 w .. 32 w + 31.
__device__ __forceinline__ void tile_distances(const f32x16 (&acc)[4], float* M, const float* qs, const float* cs, int metric, int tid) {
    const int lane = tid & 63, r = lane & 31, h = lane >> 5, w = tid >> 6;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const float sc = cs[32 * t + r];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int row = 32 * w + mfma_row(i, h);
            M[row * TC + 32 * t + r] = distance_of(metric, acc[t][i], qs[row], sc);
        }
    }
}

}  // namespace knn_tile
}  // namespace l3
