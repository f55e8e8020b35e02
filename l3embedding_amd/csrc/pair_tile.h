// pair_tile.h -- the arithmetic every pair kernel shares (csrc/pairs.hip, csrc/locmap.hip): one step of the head's chain and the
// 64 x 64 tile's accumulation.  A pair's bits are this chain's and nothing else's (include/l3hip.h, "The head over pairs").
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/l3hip.h"

namespace l3 {

constexpr int TILE = L3_PAIRS_TILE;          // frames and seconds of a workgroup's tile
constexpr int KC = 32;                       // columns of U / T per LDS pass
constexpr int BLOCK = 256;

__device__ __forceinline__ float pair_step(float acc, float u, float t, float w) {
    return __fmaf_rn(fmaxf(__fadd_rn(u, t), 0.0f), w, acc);
}

// The 4 x 4 accumulators of lane (ty, tx) over a tile of 64 rows of U and 64 rows of T: the one inner loop of every tiled mode.
// row_u(r) / row_t(r), r = 0 .. 63, give the row of U / T that stands at place r of the tile, or a negative number for a place past
// the tile's edge, which is staged as zeros.  Every lane of the workgroup calls it; it ends on a barrier, after which Us and Ts are
// free.
template <class RowU, class RowT>
__device__ __forceinline__ void accumulate_rows(float (&acc)[4][4], float (*Us)[TILE], float (*Ts)[TILE], const float* __restrict__ U,
                                                const float* __restrict__ T, const float* __restrict__ wd, int H, RowU row_u, RowT row_t,
                                                int tid, int tx, int ty) {
    for (int k0 = 0; k0 < H; k0 += KC) {
        for (int q = tid; q < TILE * KC / 4; q += BLOCK) {
            const int r = q & (TILE - 1), k = (q / TILE) * 4;
            float4 u = make_float4(0.0f, 0.0f, 0.0f, 0.0f), t = u;
            const int64_t ru = row_u(r), rt = row_t(r);
            if (ru >= 0) u = *reinterpret_cast<const float4*>(U + ru * H + k0 + k);
            if (rt >= 0) t = *reinterpret_cast<const float4*>(T + rt * H + k0 + k);
            Us[k][r] = u.x, Us[k + 1][r] = u.y, Us[k + 2][r] = u.z, Us[k + 3][r] = u.w;
            Ts[k][r] = t.x, Ts[k + 1][r] = t.y, Ts[k + 2][r] = t.z, Ts[k + 3][r] = t.w;
        }
        __syncthreads();
#pragma unroll 8
        for (int k = 0; k < KC; ++k) {
            const float4 uv = *reinterpret_cast<const float4*>(&Us[k][ty * 4]);
            const float4 tv = *reinterpret_cast<const float4*>(&Ts[k][tx * 4]);
            const float w = wd[k0 + k];
            const float ur[4] = {uv.x, uv.y, uv.z, uv.w}, tc[4] = {tv.x, tv.y, tv.z, tv.w};
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[a][c] = pair_step(acc[a][c], ur[a], tc[c], w);
        }
        __syncthreads();
    }
}

// The tile of frames i0 .. i0 + 63 and seconds j0 .. j0 + 63; rows at or past v1 / a1 are staged as zeros.
__device__ __forceinline__ void accumulate_tile(float (&acc)[4][4], float (*Us)[TILE], float (*Ts)[TILE], const float* __restrict__ U,
                                                const float* __restrict__ T, const float* __restrict__ wd, int H, int i0, int v1, int j0,
                                                int a1, int tid, int tx, int ty) {
    accumulate_rows(
        acc, Us, Ts, U, T, wd, H, [=](int r) { return i0 + r < v1 ? (int64_t)(i0 + r) : (int64_t)-1; },
        [=](int r) { return j0 + r < a1 ? (int64_t)(j0 + r) : (int64_t)-1; }, tid, tx, ty);
}

}  // namespace l3
