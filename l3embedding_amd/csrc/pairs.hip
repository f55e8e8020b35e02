// pairs.hip -- cross-modal retrieval: the AVC head scored over every (frame, second) pair.
//
// The head (model.py:25-31) is dense_2(relu(dense_1(concatenate(v, a)))).  dense_1 splits over the concatenation, W1 = [W1v; W1a],
// and of the two logits only their difference matters, so with
//     u_i = v_i W1v                     (Nv, H)
//     t_j = a_j W1a + b1                (Na, H)
//     wd  = fl32(W2[:, 1] - W2[:, 0]),  bd = fl32(b2[1] - b2[0])
// the pair (i, j) costs H x (add, max, fma):   margin_ij = sum_k relu(u_ik + t_jk) wd_k + bd = logit(corresponding) - logit(not).
//
//   project_kernel     rows (n, K) x W (K, H) [+ b] -> (n, H), fp32 VALU.  Every output element is ONE fma chain over k = 0 .. K-1 in
//                      that order, started at 0, the bias added last: a row's bits depend on the row and the weights alone, not on
//                      how many rows go with it or where it sits (a split-K GEMM whose split count follows the row count would not
//                      give that).  0.5 GFMA for 8192 rows of 512: not worth a matrix-core form.
//   pair_tile_kernel   a 64 x 64 tile of pairs per workgroup of 256 lanes, a 4 x 4 register block per lane.  U and T tiles go through
//                      LDS 32 columns at a time, transposed ([k][row]), so that per k a lane reads its 4 frames and its 4 seconds as
//                      one ds_read_b128 each (the frames' read is a broadcast within 16 lanes, the seconds' covers 64 consecutive
//                      floats) and feeds 16 pairs = 48 VALU operations from 8 LDS values.  wd is read through scalar loads.
//                      MODE 0 / 1 store margins / probabilities of a block; MODE 2 stores nothing and counts, per frame and per
//                      second, the pairs that beat the truth pair's score: in registers, then across lanes (shuffles; LDS integer
//                      adds for the columns), then one integer atomic add per (row, tile): exact and the same from run to run.
//   pair_list_kernel   listed pairs, a lane per pair, the same chain.
//   pair_topk_kernel   for 64 queries a workgroup, the k <= 64 best candidates of a segment of the other side in a strict order
//                      (margin, then index), the tile's accumulation shared with pair_tile_kernel (accumulate_tile); nothing but the
//                      lists is stored.  topk_merge_kernel joins the segments' lists, a wave per query.
// Every mode runs pair_step() (pair_tile.h, shared with locmap.hip) over k = 0 .. H-1 in that order from acc = 0 and adds bd last,
// with explicit single-rounding intrinsics: the same pair gives the same bits in every mode, block and position.  Rows past a
// tile's edge are loaded as zeros and are neither stored nor counted.  No float atomics.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/l3hip.h"
#include "featprep.h"
#include "host_common.h"
#include "pair_tile.h"
#include "pairs.h"

namespace l3 {
namespace {

constexpr int64_t MAX_ITEMS = (int64_t)65535 * TILE;          // gridDim.y
constexpr int PROJ_ROWS = 32, PROJ_COLS = 128, PROJ_PAD = 36; // project_kernel: tile of rows x panel of outputs; LDS row of 32 + 4

// 1 / (1 + exp(-m)): expf (1 ulp), one addition, one correctly rounded division
__device__ __forceinline__ float sigmoid_of(float m) { return __fdiv_rn(1.0f, __fadd_rn(1.0f, expf(-m))); }

// y (n, H) = x (n, K; row stride ldx) W (K, H) [+ b]
__global__ __launch_bounds__(BLOCK) void project_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ w,
                                                        const float* __restrict__ b, float* __restrict__ y, int64_t n, int K, int H) {
    __shared__ __attribute__((aligned(16))) float xs[KC][PROJ_PAD];
    __shared__ __attribute__((aligned(16))) float ws[KC][PROJ_COLS];
    const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
    const int64_t r0 = (int64_t)blockIdx.x * PROJ_ROWS;
    const int c0 = blockIdx.y * PROJ_COLS;
    float acc[4][4] = {};
    for (int k0 = 0; k0 < K; k0 += KC) {
        for (int q = tid; q < PROJ_ROWS * KC; q += BLOCK) {
            const int r = q >> 5, k = q & 31;
            xs[k][r] = (r0 + r < n && k0 + k < K) ? x[(r0 + r) * ldx + k0 + k] : 0.0f;
        }
        for (int q = tid; q < KC * PROJ_COLS / 4; q += BLOCK) {
            const int k = q >> 5, c = (q & 31) * 4;
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (k0 + k < K && c0 + c < H) v = *reinterpret_cast<const float4*>(w + (int64_t)(k0 + k) * H + c0 + c);   // H % 4 == 0
            *reinterpret_cast<float4*>(&ws[k][c]) = v;
        }
        __syncthreads();
#pragma unroll 8
        for (int k = 0; k < KC; ++k) {
            const float4 xv = *reinterpret_cast<const float4*>(&xs[k][ty * 4]);
            const float4 wv = *reinterpret_cast<const float4*>(&ws[k][tx * 4]);
            const float xr[4] = {xv.x, xv.y, xv.z, xv.w}, wc[4] = {wv.x, wv.y, wv.z, wv.w};
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[a][c] = __fmaf_rn(xr[a], wc[c], acc[a][c]);
        }
        __syncthreads();
    }
    const int c = c0 + tx * 4;
    if (c >= H) return;
    float4 bias = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (b) bias = *reinterpret_cast<const float4*>(b + c);
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int64_t r = r0 + ty * 4 + a;
        if (r >= n) continue;
        float4 o = make_float4(acc[a][0], acc[a][1], acc[a][2], acc[a][3]);
        if (b) o = make_float4(__fadd_rn(o.x, bias.x), __fadd_rn(o.y, bias.y), __fadd_rn(o.z, bias.z), __fadd_rn(o.w, bias.w));
        *reinterpret_cast<float4*>(y + r * H + c) = o;
    }
}

enum { MODE_MARGIN = 0, MODE_PROB = 1, MODE_RANK = 2 };

// The pairs [v0, v1) x [a0, a1).  MODE 0 / 1: out[(i - v0) * ldo + (j - a0)].  MODE 2: rv[i] += #{j: m_ij > sv[i], gv[i] != ga[j]} and
// ra[j] += #{i: m_ij > sa[j], gv[i] != ga[j]}; sv / rv or sa / ra may be null (that direction is not counted), gv and ga are null
// together (nothing is excluded).
template <int MODE>
__global__ __launch_bounds__(BLOCK) void pair_tile_kernel(const float* __restrict__ U, const float* __restrict__ T,
                                                          const float* __restrict__ wd, float bd, int H, int v0, int v1, int a0, int a1,
                                                          float* __restrict__ out, int64_t ldo, const float* __restrict__ sv,
                                                          const float* __restrict__ sa, const int32_t* __restrict__ gv,
                                                          const int32_t* __restrict__ ga, int32_t* __restrict__ rv, int32_t* __restrict__ ra) {
    __shared__ __attribute__((aligned(16))) float Us[KC][TILE];
    __shared__ __attribute__((aligned(16))) float Ts[KC][TILE];
    __shared__ int colcnt[TILE];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int i0 = v0 + blockIdx.y * TILE, j0 = a0 + blockIdx.x * TILE;
    if (MODE == MODE_RANK && tid < TILE) colcnt[tid] = 0;          // (ordered before its first use by the barriers of the loop: H >= KC)
    float acc[4][4] = {};
    accumulate_tile(acc, Us, Ts, U, T, wd, H, i0, v1, j0, a1, tid, tx, ty);
    const int j = j0 + tx * 4;
    if (MODE != MODE_RANK) {
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int i = i0 + ty * 4 + a;
            if (i >= v1) continue;
            float m[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                m[c] = __fadd_rn(acc[a][c], bd);
                if (MODE == MODE_PROB) m[c] = sigmoid_of(m[c]);
            }
            float* o = out + (int64_t)(i - v0) * ldo + (j - a0);
            if (j + 3 < a1 && (ldo & 3) == 0) {
                *reinterpret_cast<float4*>(o) = make_float4(m[0], m[1], m[2], m[3]);
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (j + c < a1) o[c] = m[c];
            }
        }
        return;
    }
    // every lane stays to the end: the shuffles below are over whole waves
    int cc[4] = {0, 0, 0, 0};
    float sj[4];
    int gj[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const bool vj = j + c < a1;
        sj[c] = (sa && vj) ? sa[j + c] : 0.0f;
        gj[c] = (ga && vj) ? ga[j + c] : 0;
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int i = i0 + ty * 4 + a;
        const bool vi = i < v1;
        const float si = (sv && vi) ? sv[i] : 0.0f;
        const int gi = (gv && vi) ? gv[i] : 0;
        int rc = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float m = __fadd_rn(acc[a][c], bd);
            const bool neg = vi && j + c < a1 && (!gv || gi != gj[c]);
            rc += (neg && sv && m > si) ? 1 : 0;
            cc[c] += (neg && sa && m > sj[c]) ? 1 : 0;
        }
        rc += __shfl_xor(rc, 1);          // the 16 lanes that share a frame are neighbours in a wave
        rc += __shfl_xor(rc, 2);
        rc += __shfl_xor(rc, 4);
        rc += __shfl_xor(rc, 8);
        if (tx == 0 && vi && rv && rc) atomicAdd(&rv[i], rc);
    }
    if (!sa) return;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        cc[c] += __shfl_xor(cc[c], 16);     // the 4 lanes of a wave that share a second
        cc[c] += __shfl_xor(cc[c], 32);
        if ((tid & 63) < 16 && cc[c]) atomicAdd(&colcnt[tx * 4 + c], cc[c]);
    }
    __syncthreads();
    if (tid < TILE && j0 + tid < a1 && colcnt[tid]) atomicAdd(&ra[j0 + tid], colcnt[tid]);
}

__global__ __launch_bounds__(BLOCK) void pair_list_kernel(const float* __restrict__ U, const float* __restrict__ T,
                                                          const float* __restrict__ wd, float bd, int H, const int32_t* __restrict__ iv,
                                                          const int32_t* __restrict__ ia, int64_t n, float* __restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    const float4* u = reinterpret_cast<const float4*>(U + (int64_t)iv[p] * H);
    const float4* t = reinterpret_cast<const float4*>(T + (int64_t)ia[p] * H);
    float acc = 0.0f;
    for (int k = 0; k < H / 4; ++k) {
        const float4 a = u[k], b = t[k];
        acc = pair_step(acc, a.x, b.x, wd[4 * k]);
        acc = pair_step(acc, a.y, b.y, wd[4 * k + 1]);
        acc = pair_step(acc, a.z, b.z, wd[4 * k + 2]);
        acc = pair_step(acc, a.w, b.w, wd[4 * k + 3]);
    }
    out[p] = __fadd_rn(acc, bd);
}

// ---- top-k lists (l3hip.h: "The order of a list") ----------------------------------------------------------------------------------
// A list is k (margin, index) entries in the strict order `ahead`, one entry per lane of a wave (k <= 64 = the wave); an empty slot
// is (-inf, EMPTY), which every candidate is ahead of: a real index is below 2^22.
constexpr int TOPK_MAX = L3_PAIRS_TOPK_MAX;
constexpr int EMPTY = INT32_MAX;
constexpr int TOPK_MAX_SEGMENTS = 256;
// The segment count aims at four workgroups to each of the 256 CUs for k <= 16 and at two above: every segment more keeps more waves
// on a SIMD, and costs every query the insertions of one more list that starts empty, which grow with k.  Measured at 8192 x 8192,
// k = 10 and 64, segments 2 .. 32 (profiles/r33_pair_topk.txt).  A segment is no shorter than TOPK_MIN_TILES tiles.
constexpr int TOPK_WORKGROUPS_SHORT = 1024, TOPK_WORKGROUPS_LONG = 512, TOPK_SHORT_K = 16;
constexpr int TOPK_MIN_TILES = 4;

__device__ __forceinline__ bool ahead(float m, int j, float m2, int j2) { return (m > m2) | ((m == m2) & (j < j2)); }   // (no branches)

__device__ __forceinline__ float lane_value(float x, int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), lane)); }
__device__ __forceinline__ int lane_value(int x, int lane) { return __builtin_amdgcn_readlane(x, lane); }

// lane l reads lane l - 1 (DPP wave_shr:1, a VALU move); lane 0 keeps its own
__device__ __forceinline__ int lane_above(int x) { return __builtin_amdgcn_update_dpp(x, x, 0x138, 0xf, 0xf, false); }

// The candidate (cm, cj), the same in every lane, into the sorted list whose entry l is lane l's (em, ej): the entries ahead of it
// are a prefix, its place is their number, the rest move down by one lane and the k-th falls off.  Whole waves only.
__device__ __forceinline__ void list_insert(float& em, int& ej, float cm, int cj, int lane, int k) {
    const int pos = __popcll(__ballot((lane < k) & ahead(em, ej, cm, cj)));
    const float pm = __int_as_float(lane_above(__float_as_int(em)));
    const int pj = lane_above(ej);
    em = lane == pos ? cm : lane > pos ? pm : em;
    ej = lane == pos ? cj : lane > pos ? pj : ej;
}

// Workgroup (x, y): the queries Q[64 x, 64 x + 64) against the candidate tiles [y tiles_per_seg, (y + 1) tiles_per_seg) of C, 64
// candidates at a time.  After a tile's accumulation the staging area holds its 64 x 64 margins; wave w then owns the queries
// 16 w .. 16 w + 15 (the rows its own lanes wrote), a lane per candidate.  Lane qq of the wave keeps query 16 w + qq's group, truth
// and k-th entry -- its threshold -- in registers: what is a candidate and ahead of the threshold is found by one ballot a query,
// and only then is the query's list (LDS, k entries) loaded, inserted into (a candidate that the threshold has overtaken meanwhile
// is skipped) and stored.  A segment's first tile meets empty lists and fills them by counting instead: a candidate's place is the
// number of the tile's candidates ahead of it.  The lists go to pm / pj[(y nq + i) k + l]; topk_merge_kernel joins the segments.  truth, and gq / gc
// together, may be null.
__global__ __launch_bounds__(BLOCK) void pair_topk_kernel(const float* __restrict__ Q, const float* __restrict__ Cd,
                                                          const float* __restrict__ wd, float bd, int H, int nq, int nc, int k,
                                                          int tiles_per_seg, const int32_t* __restrict__ truth,
                                                          const int32_t* __restrict__ gq, const int32_t* __restrict__ gc,
                                                          float* __restrict__ pm, int32_t* __restrict__ pj) {
    constexpr int QW = TILE / (BLOCK / 64);                                    // queries of a wave
    __shared__ __attribute__((aligned(16))) float stage[2][KC][TILE];          // U / T staging, then the tile's margins [query][candidate]
    extern __shared__ __attribute__((aligned(16))) unsigned char lists[];      // TILE x k margins, then TILE x k indices
    float* lm = reinterpret_cast<float*>(lists);
    int* lj = reinterpret_cast<int*>(lm + TILE * k);
    float* M = &stage[0][0][0];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i0 = blockIdx.x * TILE;
    const int ntiles = (nc + TILE - 1) / TILE;
    const int t0 = blockIdx.y * tiles_per_seg, t1 = min(ntiles, t0 + tiles_per_seg);
    for (int q = tid; q < TILE * k; q += BLOCK) lm[q] = -INFINITY, lj[q] = EMPTY;
    const int iq = i0 + w * QW + lane;          // lanes 0 .. QW-1: the wave's queries
    const bool viq = lane < QW && iq < nq;
    const int qgroup = (gq && viq) ? gq[iq] : 0, qtruth = (truth && viq) ? truth[iq] : -1;
    float thm = -INFINITY;
    int thj = EMPTY;
    __syncthreads();
    for (int tile = t0; tile < t1; ++tile) {
        const int j0 = tile * TILE;
        float acc[4][4] = {};
        accumulate_tile(acc, stage[0], stage[1], Q, Cd, wd, H, i0, nq, j0, nc, tid, tx, ty);
#pragma unroll
        for (int a = 0; a < 4; ++a)
            *reinterpret_cast<float4*>(&M[(ty * 4 + a) * TILE + tx * 4]) =
                make_float4(__fadd_rn(acc[a][0], bd), __fadd_rn(acc[a][1], bd), __fadd_rn(acc[a][2], bd), __fadd_rn(acc[a][3], bd));
        __syncthreads();
        const int j = j0 + lane;
        const bool vj = j < nc;
        const int gj = (gc && vj) ? gc[j] : 0;
        float mq[QW];
#pragma unroll
        for (int qq = 0; qq < QW; ++qq) mq[qq] = M[(w * QW + qq) * TILE + lane];
#pragma unroll
        for (int qq = 0; qq < QW; ++qq) {
            const int q = w * QW + qq;
            const float m = mq[qq];
            const bool cand = vj && i0 + q < nq && m == m && (!gc || gj != lane_value(qgroup, qq) || j == lane_value(qtruth, qq));
            if (tile == t0) {          // the lists are empty: a candidate's place is the number of candidates ahead of it
                int place = 0;
                for (unsigned long long rest = __ballot(cand); rest; rest &= rest - 1) {
                    const int b = __ffsll((long long)rest) - 1;
                    place += ahead(lane_value(m, b), j0 + b, m, j) ? 1 : 0;
                }
                if (cand && place < k) lm[q * k + place] = m, lj[q * k + place] = j;
                const float nm = lm[q * k + k - 1];          // (the wave's own LDS writes are in order before these reads)
                const int nj = lj[q * k + k - 1];
                if (lane == qq) thm = nm, thj = nj;
                continue;
            }
            unsigned long long pass = __ballot(cand && ahead(m, j, lane_value(thm, qq), lane_value(thj, qq)));
            if (!pass) continue;
            float em = lane < k ? lm[q * k + lane] : -INFINITY;
            int ej = lane < k ? lj[q * k + lane] : EMPTY;
            while (pass) {
                const int b = __ffsll((long long)pass) - 1;
                pass &= pass - 1;
                const float cm = lane_value(m, b);
                if (ahead(cm, j0 + b, lane_value(em, k - 1), lane_value(ej, k - 1))) list_insert(em, ej, cm, j0 + b, lane, k);
            }
            if (lane < k) lm[q * k + lane] = em, lj[q * k + lane] = ej;
            const float nm = lane_value(em, k - 1);
            const int nj = lane_value(ej, k - 1);
            if (lane == qq) thm = nm, thj = nj;
        }
        __syncthreads();
    }
    for (int q = tid; q < TILE * k; q += BLOCK) {
        const int i = i0 + q / k;
        if (i >= nq) continue;
        const int64_t o = ((int64_t)blockIdx.y * nq + i) * k + q % k;
        pm[o] = lm[q], pj[o] = lj[q];
    }
}

// A wave per query: the `segments` sorted lists of pair_topk_kernel into the first k of their union, in the same order; empty slots
// leave as index -1 and margin -inf.
__global__ __launch_bounds__(BLOCK) void topk_merge_kernel(const float* __restrict__ pm, const int32_t* __restrict__ pj, int nq, int k,
                                                           int segments, int32_t* __restrict__ idx, float* __restrict__ margin) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * (BLOCK / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (q >= nq) return;          // whole waves leave
    float em = -INFINITY;
    int ej = EMPTY;
    for (int s = 0; s < segments; ++s) {
        const int64_t base = ((int64_t)s * nq + q) * k;
        const float sm = lane < k ? pm[base + lane] : -INFINITY;
        const int sj = lane < k ? pj[base + lane] : EMPTY;
        if (s == 0) {
            em = sm, ej = sj;
            continue;
        }
        for (int l = 0; l < k; ++l) {          // a segment's entries come in order: the first that is not ahead of the k-th ends it
            const float cm = lane_value(sm, l);
            const int cj = lane_value(sj, l);
            if (cj == EMPTY || !ahead(cm, cj, lane_value(em, k - 1), lane_value(ej, k - 1))) break;
            list_insert(em, ej, cm, cj, lane, k);
        }
    }
    if (lane < k) {
        idx[(int64_t)q * k + lane] = ej == EMPTY ? -1 : ej;
        margin[(int64_t)q * k + lane] = em;
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
bool finished(hipStream_t s) { return hipStreamSynchronize(s) == hipSuccess && hipGetLastError() == hipSuccess; }

void launch_project(const float* x, int64_t ldx, const float* w, const float* b, float* y, int64_t n, int K, int H, hipStream_t s) {
    const dim3 grid((unsigned)((n + PROJ_ROWS - 1) / PROJ_ROWS), (unsigned)((H + PROJ_COLS - 1) / PROJ_COLS));
    hipLaunchKernelGGL(project_kernel, grid, dim3(BLOCK), 0, s, x, ldx, w, b, y, n, K, H);
}

void launch_tile(int mode, const float* U, const float* T, const float* wd, float bd, int H, int v0, int v1, int a0, int a1, float* out,
                 const float* sv, const float* sa, const int32_t* gv, const int32_t* ga, int32_t* rv, int32_t* ra, hipStream_t s) {
    const dim3 grid((unsigned)((a1 - a0 + TILE - 1) / TILE), (unsigned)((v1 - v0 + TILE - 1) / TILE));
    const int64_t ldo = a1 - a0;
    if (mode == MODE_MARGIN)
        hipLaunchKernelGGL(pair_tile_kernel<MODE_MARGIN>, grid, dim3(BLOCK), 0, s, U, T, wd, bd, H, v0, v1, a0, a1, out, ldo, sv, sa, gv, ga, rv, ra);
    else if (mode == MODE_PROB)
        hipLaunchKernelGGL(pair_tile_kernel<MODE_PROB>, grid, dim3(BLOCK), 0, s, U, T, wd, bd, H, v0, v1, a0, a1, out, ldo, sv, sa, gv, ga, rv, ra);
    else
        hipLaunchKernelGGL(pair_tile_kernel<MODE_RANK>, grid, dim3(BLOCK), 0, s, U, T, wd, bd, H, v0, v1, a0, a1, out, ldo, sv, sa, gv, ga, rv, ra);
}

void launch_list(const float* U, const float* T, const float* wd, float bd, int H, const int32_t* iv, const int32_t* ia, int64_t n,
                 float* out, hipStream_t s) {
    hipLaunchKernelGGL(pair_list_kernel, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, U, T, wd, bd, H, iv, ia, n, out);
}

// Segments of the candidate side for nq queries against nc candidates: `asked` clamped to the number of tiles, or, for 0, enough
// to fill the chip without making the segments shorter than TOPK_MIN_TILES tiles.
int topk_segments(int64_t nq, int64_t nc, int k, int asked) {
    const int64_t qt = (nq + TILE - 1) / TILE, ct = (nc + TILE - 1) / TILE;
    int64_t s = asked;
    const int64_t aim = k <= TOPK_SHORT_K ? TOPK_WORKGROUPS_SHORT : TOPK_WORKGROUPS_LONG;
    if (asked == 0) s = std::min<int64_t>((aim + qt - 1) / qt, ct / TOPK_MIN_TILES);
    return (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(s, ct), TOPK_MAX_SEGMENTS));
}

size_t topk_partial_count(int64_t nq, int k, int segments) { return (size_t)segments * (size_t)nq * (size_t)k; }

void launch_topk_lists(const float* Q, const float* Cd, const float* wd, float bd, int H, int64_t nq, int64_t nc, int k, int segments,
                       const int32_t* truth, const int32_t* gq, const int32_t* gc, float* pm, int32_t* pj, hipStream_t s) {
    const int ct = (int)((nc + TILE - 1) / TILE);
    const dim3 grid((unsigned)((nq + TILE - 1) / TILE), (unsigned)segments);
    hipLaunchKernelGGL(pair_topk_kernel, grid, dim3(BLOCK), (size_t)TILE * k * 8, s, Q, Cd, wd, bd, H, (int)nq, (int)nc, k,
                       (ct + segments - 1) / segments, truth, gq, gc, pm, pj);
}

void launch_topk_merge(const float* pm, const int32_t* pj, int64_t nq, int k, int segments, int32_t* idx, float* margin, hipStream_t s) {
    hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)((nq + BLOCK / 64 - 1) / (BLOCK / 64))), dim3(BLOCK), 0, s, pm, pj, (int)nq, k,
                       segments, idx, margin);
}

bool head_ok(int H) { return H >= KC && H % KC == 0 && H <= 4096; }

template <class T>
int grow(l3_pairs* p, T** buf, size_t* cap, size_t count, const char* fn) {
    if (*buf && count <= *cap) return L3_OK;
    // whatever read the old buffer has finished: every call on the handle waits for its stream before it returns
    p->bufs.grow(buf, cap, count);
    if (*buf) return L3_OK;
    return fail(L3_ENOMEM, std::string(fn) + ": device allocation of " + std::to_string(DeviceBufs::bytes_of<T>(count)) + " bytes failed");
}

int enter(l3_pairs* p, const char* fn) {
    if (!p) return fail(L3_EINVAL, std::string(fn) + ": NULL handle");
    if (hipSetDevice(p->device) != hipSuccess) return fail(L3_EHIP, no_gpu_message(fn, p->device));
    return L3_OK;
}

int need_sets(const l3_pairs* p, const char* fn) {
    if (!p->head_set) return fail(L3_ESTATE, std::string(fn) + ": l3_pairs_set_head has not been called");
    if (p->Nv < 1 || p->Na < 1) return fail(L3_ESTATE, std::string(fn) + ": l3_pairs_set_vision and l3_pairs_set_audio come first");
    return L3_OK;
}

// rows (n, K) on the device -> the projected set of one side
int project_side(l3_pairs* p, bool vision, const float* x_dev, int64_t n, const char* fn) {
    const int K = vision ? p->nv : p->na;
    float** dst = vision ? &p->U : &p->T;
    size_t* cap = vision ? &p->cap_U : &p->cap_T;
    (vision ? p->Nv : p->Na) = 0;
    if (int rc = grow(p, dst, cap, (size_t)n * p->head, fn)) return rc;
    launch_project(x_dev, K, p->w1 + (vision ? 0 : (size_t)p->nv * p->head), vision ? nullptr : p->b1, *dst, n, K, p->head, p->s);
    if (!finished(p->s)) return fail(L3_EHIP, std::string(fn) + ": the projection failed on the device");
    (vision ? p->Nv : p->Na) = n;
    return L3_OK;
}

int set_side_host(l3_pairs* p, bool vision, const float* rows, int64_t n, const char* fn) {
    if (int rc = enter(p, fn)) return rc;
    if (!rows) return fail(L3_EINVAL, std::string(fn) + ": rows is NULL");
    if (n < 1 || n > MAX_ITEMS) return fail(L3_EINVAL, std::string(fn) + ": need 1 <= n <= " + std::to_string(MAX_ITEMS) + " rows, not " + std::to_string(n));
    if (!p->head_set) return fail(L3_ESTATE, std::string(fn) + ": l3_pairs_set_head has not been called");
    const int K = vision ? p->nv : p->na;
    if (int rc = grow(p, &p->rows, &p->cap_rows, (size_t)n * K, fn)) return rc;
    if (hipMemcpyAsync(p->rows, rows, (size_t)n * K * sizeof(float), hipMemcpyHostToDevice, p->s) != hipSuccess)
        return fail(L3_EHIP, std::string(fn) + ": copy to the device failed");
    return project_side(p, vision, p->rows, n, fn);
}

int set_side_dev(l3_pairs* p, bool vision, const l3_feat* f, int64_t lo, int64_t hi, const char* fn) {
    if (int rc = enter(p, fn)) return rc;
    if (!f) return fail(L3_EINVAL, std::string(fn) + ": the feature matrix is NULL");
    const int K = vision ? p->nv : p->na;
    if (f->device != p->device)
        return fail(L3_EINVAL, std::string(fn) + ": the features are on device " + std::to_string(f->device) + ", the scorer on device " + std::to_string(p->device));
    if (f->D != K)
        return fail(L3_EINVAL, std::string(fn) + ": the features have " + std::to_string(f->D) + " columns, the tower's output " + std::to_string(K));
    if (lo < 0 || hi > f->n || lo >= hi)
        return fail(L3_EINVAL, std::string(fn) + ": rows [" + std::to_string(lo) + ", " + std::to_string(hi) + ") are empty or outside the " +
                                   std::to_string(f->n) + " rows of the features");
    if (hi - lo > MAX_ITEMS) return fail(L3_EINVAL, std::string(fn) + ": at most " + std::to_string(MAX_ITEMS) + " rows");
    if (!p->head_set) return fail(L3_ESTATE, std::string(fn) + ": l3_pairs_set_head has not been called");
    // (every l3_feat call has finished on its handle's stream when it returns: the rows hold their final values)
    return project_side(p, vision, f->x + lo * f->D, hi - lo, fn);
}

}  // namespace

// what csrc/locmap.hip shares with this file: the projection's launch and the handle's conventions
void pairs_project(const float* x, int64_t ldx, const float* w, const float* b, float* y, int64_t n, int K, int H, hipStream_t s) {
    launch_project(x, ldx, w, b, y, n, K, H, s);
}
bool pairs_head_ok(int H) { return head_ok(H); }
bool pairs_finished(hipStream_t s) { return finished(s); }
int pairs_enter(l3_pairs* p, const char* fn) { return enter(p, fn); }
int pairs_grow(l3_pairs* p, float** buf, size_t* cap, size_t count, const char* fn) { return grow(p, buf, cap, count, fn); }
int pairs_grow(l3_pairs* p, int32_t** buf, size_t* cap, size_t count, const char* fn) { return grow(p, buf, cap, count, fn); }
}  // namespace l3

using namespace l3;

extern "C" {

int l3_pairs_create(int device, int nv, int na, int head, l3_pairs** out) {
    if (!out) return fail(L3_EINVAL, "l3_pairs_create: out is NULL");
    *out = nullptr;
    if (nv < 1 || na < 1 || nv > (1 << 20) || na > (1 << 20) || !head_ok(head))
        return fail(L3_EINVAL, "l3_pairs_create: need tower widths in [1, 2^20] and a head width that is a multiple of 32 in [32, 4096]; got nv " +
                                   std::to_string(nv) + ", na " + std::to_string(na) + ", head " + std::to_string(head));
    if (!device_ok(device)) return fail(L3_EHIP, no_gpu_message("l3_pairs_create", device));
    l3_pairs* p = new l3_pairs();
    p->device = device, p->nv = nv, p->na = na, p->head = head;
    p->w1 = p->bufs.alloc<float>((size_t)(nv + na) * head);
    p->b1 = p->bufs.alloc<float>((size_t)head);
    p->wd = p->bufs.alloc<float>((size_t)head);
    if (!p->bufs.ok() || hipStreamCreateWithFlags(&p->s, hipStreamNonBlocking) != hipSuccess) {
        l3_pairs_destroy(p);
        return fail(L3_ENOMEM, "l3_pairs_create: device allocation failed");
    }
    *out = p;
    return L3_OK;
}

void l3_pairs_destroy(l3_pairs* p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    if (p->s) (void)hipStreamSynchronize(p->s);
    if (p->s) (void)hipStreamDestroy(p->s);
    delete p;
}

int l3_pairs_set_head(l3_pairs* p, const float* w1, const float* b1, const float* w2, const float* b2) {
    if (int rc = enter(p, "l3_pairs_set_head")) return rc;
    if (!w1 || !b1 || !w2 || !b2) return fail(L3_EINVAL, "l3_pairs_set_head: w1, b1, w2 and b2 must not be NULL");
    const int H = p->head;
    std::vector<float> wd((size_t)H);
    for (int k = 0; k < H; ++k) wd[k] = w2[2 * k + 1] - w2[2 * k];          // one float32 rounding each
    p->head_set = false, p->Nv = p->Na = 0;                                // sets projected with another head are void
    p->map_put.assign(p->map_put.size(), 0), p->map_done = 0;              // ... and so is the location map
    if (hipMemcpyAsync(p->w1, w1, (size_t)(p->nv + p->na) * H * sizeof(float), hipMemcpyHostToDevice, p->s) != hipSuccess ||
        hipMemcpyAsync(p->b1, b1, (size_t)H * sizeof(float), hipMemcpyHostToDevice, p->s) != hipSuccess ||
        hipMemcpyAsync(p->wd, wd.data(), (size_t)H * sizeof(float), hipMemcpyHostToDevice, p->s) != hipSuccess || !finished(p->s))
        return fail(L3_EHIP, "l3_pairs_set_head: copy to the device failed");
    p->bd = b2[1] - b2[0];
    p->head_set = true;
    return L3_OK;
}

int l3_pairs_set_vision(l3_pairs* p, const float* rows, int64_t n) { return set_side_host(p, true, rows, n, "l3_pairs_set_vision"); }
int l3_pairs_set_audio(l3_pairs* p, const float* rows, int64_t n) { return set_side_host(p, false, rows, n, "l3_pairs_set_audio"); }
int l3_pairs_set_vision_dev(l3_pairs* p, const l3_feat* f, int64_t lo, int64_t hi) { return set_side_dev(p, true, f, lo, hi, "l3_pairs_set_vision_dev"); }
int l3_pairs_set_audio_dev(l3_pairs* p, const l3_feat* f, int64_t lo, int64_t hi) { return set_side_dev(p, false, f, lo, hi, "l3_pairs_set_audio_dev"); }

int l3_pairs_matrix(l3_pairs* p, int64_t v0, int64_t v1, int64_t a0, int64_t a1, int prob, float* out) {
    if (int rc = enter(p, "l3_pairs_matrix")) return rc;
    if (!out) return fail(L3_EINVAL, "l3_pairs_matrix: out is NULL");
    if (int rc = need_sets(p, "l3_pairs_matrix")) return rc;
    if (v0 < 0 || v1 > p->Nv || v0 >= v1 || a0 < 0 || a1 > p->Na || a0 >= a1)
        return fail(L3_EINVAL, "l3_pairs_matrix: the block [" + std::to_string(v0) + ", " + std::to_string(v1) + ") x [" + std::to_string(a0) + ", " +
                                   std::to_string(a1) + ") is empty or outside the " + std::to_string(p->Nv) + " x " + std::to_string(p->Na) + " pairs");
    const size_t count = (size_t)(v1 - v0) * (size_t)(a1 - a0);
    if (int rc = grow(p, &p->out, &p->cap_out, count, "l3_pairs_matrix")) return rc;
    launch_tile(prob ? MODE_PROB : MODE_MARGIN, p->U, p->T, p->wd, p->bd, p->head, (int)v0, (int)v1, (int)a0, (int)a1, p->out, nullptr, nullptr,
                nullptr, nullptr, nullptr, nullptr, p->s);
    if (hipMemcpyAsync(out, p->out, count * sizeof(float), hipMemcpyDeviceToHost, p->s) != hipSuccess || !finished(p->s))
        return fail(L3_EHIP, "l3_pairs_matrix: the kernel or the copy from the device failed");
    return L3_OK;
}

int l3_pairs_list(l3_pairs* p, const int32_t* iv, const int32_t* ia, int64_t n, float* margin_out) {
    if (int rc = enter(p, "l3_pairs_list")) return rc;
    if (!iv || !ia || !margin_out) return fail(L3_EINVAL, "l3_pairs_list: iv, ia and margin_out must not be NULL");
    if (int rc = need_sets(p, "l3_pairs_list")) return rc;
    if (n < 1 || n > INT32_MAX) return fail(L3_EINVAL, "l3_pairs_list: need 1 <= n <= 2^31 - 1 pairs");
    for (int64_t q = 0; q < n; ++q)
        if (iv[q] < 0 || iv[q] >= p->Nv || ia[q] < 0 || ia[q] >= p->Na)
            return fail(L3_EINVAL, "l3_pairs_list: pair " + std::to_string(q) + " = (" + std::to_string(iv[q]) + ", " + std::to_string(ia[q]) +
                                       ") outside the " + std::to_string(p->Nv) + " x " + std::to_string(p->Na) + " pairs");
    if (int rc = grow(p, &p->idx, &p->cap_idx, (size_t)n * 2, "l3_pairs_list")) return rc;
    if (int rc = grow(p, &p->out, &p->cap_out, (size_t)n, "l3_pairs_list")) return rc;
    if (hipMemcpyAsync(p->idx, iv, (size_t)n * 4, hipMemcpyHostToDevice, p->s) != hipSuccess ||
        hipMemcpyAsync(p->idx + n, ia, (size_t)n * 4, hipMemcpyHostToDevice, p->s) != hipSuccess)
        return fail(L3_EHIP, "l3_pairs_list: copy to the device failed");
    launch_list(p->U, p->T, p->wd, p->bd, p->head, p->idx, p->idx + n, n, p->out, p->s);
    if (hipMemcpyAsync(margin_out, p->out, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, p->s) != hipSuccess || !finished(p->s))
        return fail(L3_EHIP, "l3_pairs_list: the kernel or the copy from the device failed");
    return L3_OK;
}

int l3_pairs_ranks(l3_pairs* p, const int32_t* truth_a, const int32_t* truth_v, const int32_t* group_v, const int32_t* group_a,
                   int32_t* rank_v2a, int32_t* rank_a2v) {
    const char* fn = "l3_pairs_ranks";
    if (int rc = enter(p, fn)) return rc;
    if ((truth_a == nullptr) != (rank_v2a == nullptr) || (truth_v == nullptr) != (rank_a2v == nullptr) || (!truth_a && !truth_v))
        return fail(L3_EINVAL, std::string(fn) + ": a direction needs both its truth and its rank vector, and one direction at least is needed");
    if ((group_v == nullptr) != (group_a == nullptr))
        return fail(L3_EINVAL, std::string(fn) + ": group_v and group_a are given together or both NULL");
    if (int rc = need_sets(p, fn)) return rc;
    const int64_t Nv = p->Nv, Na = p->Na;
    for (int64_t i = 0; truth_a && i < Nv; ++i)
        if (truth_a[i] < 0 || truth_a[i] >= Na)
            return fail(L3_EINVAL, std::string(fn) + ": truth_a[" + std::to_string(i) + "] = " + std::to_string(truth_a[i]) + " outside [0, " + std::to_string(Na) + ")");
    for (int64_t j = 0; truth_v && j < Na; ++j)
        if (truth_v[j] < 0 || truth_v[j] >= Nv)
            return fail(L3_EINVAL, std::string(fn) + ": truth_v[" + std::to_string(j) + "] = " + std::to_string(truth_v[j]) + " outside [0, " + std::to_string(Nv) + ")");
    // idx: {iv, ia} of the truth pairs (Nv + Na each), groups (Nv + Na), counts (Nv + Na); out: truth scores (Nv + Na)
    const int64_t N = Nv + Na;
    if (int rc = grow(p, &p->idx, &p->cap_idx, (size_t)N * 4, fn)) return rc;
    if (int rc = grow(p, &p->out, &p->cap_out, (size_t)N, fn)) return rc;
    std::vector<int32_t> host((size_t)N * 3, 0);
    int32_t *iv = host.data(), *ia = iv + N, *gr = ia + N;
    for (int64_t i = 0; i < Nv; ++i) iv[i] = (int32_t)i, ia[i] = truth_a ? truth_a[i] : 0;
    for (int64_t j = 0; j < Na; ++j) iv[Nv + j] = truth_v ? truth_v[j] : 0, ia[Nv + j] = (int32_t)j;
    if (group_v) {
        for (int64_t i = 0; i < Nv; ++i) gr[i] = group_v[i];
        for (int64_t j = 0; j < Na; ++j) gr[Nv + j] = group_a[j];
    }
    int32_t* d_cnt = p->idx + 3 * N;
    if (hipMemcpyAsync(p->idx, host.data(), (size_t)N * 3 * 4, hipMemcpyHostToDevice, p->s) != hipSuccess ||
        hipMemsetAsync(d_cnt, 0, (size_t)N * 4, p->s) != hipSuccess)
        return fail(L3_EHIP, std::string(fn) + ": copy to the device failed");
    launch_list(p->U, p->T, p->wd, p->bd, p->head, p->idx, p->idx + N, N, p->out, p->s);
    const int32_t* d_g = group_v ? p->idx + 2 * N : nullptr;
    launch_tile(MODE_RANK, p->U, p->T, p->wd, p->bd, p->head, 0, (int)Nv, 0, (int)Na, nullptr, truth_a ? p->out : nullptr,
                truth_v ? p->out + Nv : nullptr, d_g, d_g ? d_g + Nv : nullptr, truth_a ? d_cnt : nullptr, truth_v ? d_cnt + Nv : nullptr, p->s);
    bool ok = true;
    if (rank_v2a) ok = ok && hipMemcpyAsync(rank_v2a, d_cnt, (size_t)Nv * 4, hipMemcpyDeviceToHost, p->s) == hipSuccess;
    if (rank_a2v) ok = ok && hipMemcpyAsync(rank_a2v, d_cnt + Nv, (size_t)Na * 4, hipMemcpyDeviceToHost, p->s) == hipSuccess;
    if (!ok || !finished(p->s)) return fail(L3_EHIP, std::string(fn) + ": the kernels or the copy from the device failed");
    return L3_OK;
}

int l3_pairs_topk(l3_pairs* p, int k, const int32_t* truth_a, const int32_t* truth_v, const int32_t* group_v, const int32_t* group_a,
                  int32_t* idx_v2a, float* margin_v2a, int32_t* idx_a2v, float* margin_a2v) {
    const char* fn = "l3_pairs_topk";
    if (int rc = enter(p, fn)) return rc;
    if (k < 1 || k > TOPK_MAX) return fail(L3_EINVAL, std::string(fn) + ": need 1 <= k <= " + std::to_string(TOPK_MAX) + ", not " + std::to_string(k));
    if ((idx_v2a == nullptr) != (margin_v2a == nullptr) || (idx_a2v == nullptr) != (margin_a2v == nullptr) || (!idx_v2a && !idx_a2v))
        return fail(L3_EINVAL, std::string(fn) + ": a direction needs both its idx and its margin output, and one direction at least is needed");
    if ((group_v == nullptr) != (group_a == nullptr))
        return fail(L3_EINVAL, std::string(fn) + ": group_v and group_a are given together or both NULL");
    if ((truth_a || truth_v) && !group_v)
        return fail(L3_EINVAL, std::string(fn) + ": a truth without groups keeps nothing: nothing is excluded");
    if (int rc = need_sets(p, fn)) return rc;
    const int64_t Nv = p->Nv, Na = p->Na, N = Nv + Na;
    if (!idx_v2a) truth_a = nullptr;          // the truth of a direction that is not asked for is not read
    if (!idx_a2v) truth_v = nullptr;
    for (int64_t i = 0; truth_a && i < Nv; ++i)
        if (truth_a[i] < 0 || truth_a[i] >= Na)
            return fail(L3_EINVAL, std::string(fn) + ": truth_a[" + std::to_string(i) + "] = " + std::to_string(truth_a[i]) + " outside [0, " + std::to_string(Na) + ")");
    for (int64_t j = 0; truth_v && j < Na; ++j)
        if (truth_v[j] < 0 || truth_v[j] >= Nv)
            return fail(L3_EINVAL, std::string(fn) + ": truth_v[" + std::to_string(j) + "] = " + std::to_string(truth_v[j]) + " outside [0, " + std::to_string(Nv) + ")");
    // idx: truths (Nv + Na), groups (Nv + Na), a direction's partial indices, its final indices; out: its partial and final margins.
    // The two directions run one after the other through the same scratch.
    const int sv = topk_segments(Nv, Na, k, 0), sa = topk_segments(Na, Nv, k, 0);
    const size_t part = std::max(idx_v2a ? topk_partial_count(Nv, k, sv) : 0, idx_a2v ? topk_partial_count(Na, k, sa) : 0);
    const size_t fin = (size_t)std::max(Nv, Na) * k;
    if (int rc = grow(p, &p->idx, &p->cap_idx, (size_t)N * 2 + part + fin, fn)) return rc;
    if (int rc = grow(p, &p->out, &p->cap_out, part + fin, fn)) return rc;
    std::vector<int32_t> host((size_t)N * 2, 0);
    for (int64_t i = 0; truth_a && i < Nv; ++i) host[i] = truth_a[i];
    for (int64_t j = 0; truth_v && j < Na; ++j) host[Nv + j] = truth_v[j];
    for (int64_t i = 0; group_v && i < Nv; ++i) host[N + i] = group_v[i];
    for (int64_t j = 0; group_a && j < Na; ++j) host[N + Nv + j] = group_a[j];
    if (hipMemcpyAsync(p->idx, host.data(), (size_t)N * 2 * 4, hipMemcpyHostToDevice, p->s) != hipSuccess)
        return fail(L3_EHIP, std::string(fn) + ": copy to the device failed");
    const int32_t *d_ta = truth_a ? p->idx : nullptr, *d_tv = truth_v ? p->idx + Nv : nullptr;
    const int32_t *d_gv = group_v ? p->idx + N : nullptr, *d_ga = group_v ? p->idx + N + Nv : nullptr;
    int32_t *d_pj = p->idx + 2 * N, *d_idx = d_pj + part;
    float *d_pm = p->out, *d_m = p->out + part;
    bool ok = true;
    if (idx_v2a) {
        launch_topk_lists(p->U, p->T, p->wd, p->bd, p->head, Nv, Na, k, sv, d_ta, d_gv, d_ga, d_pm, d_pj, p->s);
        launch_topk_merge(d_pm, d_pj, Nv, k, sv, d_idx, d_m, p->s);
        ok = ok && hipMemcpyAsync(idx_v2a, d_idx, (size_t)Nv * k * 4, hipMemcpyDeviceToHost, p->s) == hipSuccess &&
             hipMemcpyAsync(margin_v2a, d_m, (size_t)Nv * k * 4, hipMemcpyDeviceToHost, p->s) == hipSuccess;
    }
    if (idx_a2v) {          // fl32(u + t) is commutative: the same kernel with the sets exchanged gives the same bits
        launch_topk_lists(p->T, p->U, p->wd, p->bd, p->head, Na, Nv, k, sa, d_tv, d_ga, d_gv, d_pm, d_pj, p->s);
        launch_topk_merge(d_pm, d_pj, Na, k, sa, d_idx, d_m, p->s);
        ok = ok && hipMemcpyAsync(idx_a2v, d_idx, (size_t)Na * k * 4, hipMemcpyDeviceToHost, p->s) == hipSuccess &&
             hipMemcpyAsync(margin_a2v, d_m, (size_t)Na * k * 4, hipMemcpyDeviceToHost, p->s) == hipSuccess;
    }
    if (!ok || !finished(p->s)) return fail(L3_EHIP, std::string(fn) + ": the kernels or the copy from the device failed");
    return L3_OK;
}

int l3_op_project(int device, const float* x, const float* w, const float* b, int64_t n, int K, int H, float* out) {
    if (!x || !w || !out) return fail(L3_EINVAL, "l3_op_project: x, w and out must not be NULL");
    if (n < 1 || n > MAX_ITEMS || K < 1 || K > (1 << 20) || !head_ok(H))
        return fail(L3_EINVAL, "l3_op_project: need 1 <= n, 1 <= K <= 2^20 and H a multiple of 32 in [32, 4096]");
    if (!device_ok(device)) return fail(L3_EHIP, no_gpu_message("l3_op_project", device));
    DeviceBufs bufs;
    float* dx = bufs.put(x, (size_t)n * K, nullptr);
    float* dw = bufs.put(w, (size_t)K * H, nullptr);
    float* db = b ? bufs.put(b, (size_t)H, nullptr) : nullptr;
    float* dy = bufs.alloc<float>((size_t)n * H);
    if (!bufs.ok()) return fail(L3_ENOMEM, "l3_op_project: device allocation or upload failed");
    launch_project(dx, K, dw, db, dy, n, K, H, nullptr);
    if (hipMemcpy(out, dy, (size_t)n * H * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess || hipGetLastError() != hipSuccess)
        return fail(L3_EHIP, "l3_op_project: the kernel or the copy from the device failed");
    return L3_OK;
}

int l3_op_pair_margins(int device, const float* u, const float* t, const float* wd, float bd, int64_t Nv, int64_t Na, int H, float* out) {
    if (!u || !t || !wd || !out) return fail(L3_EINVAL, "l3_op_pair_margins: u, t, wd and out must not be NULL");
    if (Nv < 1 || Na < 1 || Nv > MAX_ITEMS || Na > MAX_ITEMS || !head_ok(H))
        return fail(L3_EINVAL, "l3_op_pair_margins: need 1 <= Nv, Na and H a multiple of 32 in [32, 4096]");
    if (!device_ok(device)) return fail(L3_EHIP, no_gpu_message("l3_op_pair_margins", device));
    DeviceBufs bufs;
    float* du = bufs.put(u, (size_t)Nv * H, nullptr);
    float* dt = bufs.put(t, (size_t)Na * H, nullptr);
    float* dw = bufs.put(wd, (size_t)H, nullptr);
    float* dout = bufs.alloc<float>((size_t)Nv * Na);
    if (!bufs.ok()) return fail(L3_ENOMEM, "l3_op_pair_margins: device allocation or upload failed");
    launch_tile(MODE_MARGIN, du, dt, dw, bd, H, 0, (int)Nv, 0, (int)Na, dout, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    if (hipMemcpy(out, dout, (size_t)Nv * Na * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess || hipGetLastError() != hipSuccess)
        return fail(L3_EHIP, "l3_op_pair_margins: the kernel or the copy from the device failed");
    return L3_OK;
}

int l3_op_pair_topk(int device, const float* u, const float* t, const float* wd, float bd, int64_t Nv, int64_t Na, int H, int k,
                    const int32_t* truth, const int32_t* group_q, const int32_t* group_c, int segments, int32_t* idx, float* margin) {
    const char* fn = "l3_op_pair_topk";
    if (!u || !t || !wd || !idx || !margin) return fail(L3_EINVAL, std::string(fn) + ": u, t, wd, idx and margin must not be NULL");
    if (Nv < 1 || Na < 1 || Nv > MAX_ITEMS || Na > MAX_ITEMS || !head_ok(H))
        return fail(L3_EINVAL, std::string(fn) + ": need 1 <= Nv, Na and H a multiple of 32 in [32, 4096]");
    if (k < 1 || k > TOPK_MAX || segments < 0 || segments > TOPK_MAX_SEGMENTS)
        return fail(L3_EINVAL, std::string(fn) + ": need 1 <= k <= " + std::to_string(TOPK_MAX) + " and 0 <= segments <= " + std::to_string(TOPK_MAX_SEGMENTS));
    if ((group_q == nullptr) != (group_c == nullptr)) return fail(L3_EINVAL, std::string(fn) + ": group_q and group_c are given together or both NULL");
    if (truth && !group_q) return fail(L3_EINVAL, std::string(fn) + ": a truth without groups keeps nothing: nothing is excluded");
    for (int64_t i = 0; truth && i < Nv; ++i)
        if (truth[i] < 0 || truth[i] >= Na)
            return fail(L3_EINVAL, std::string(fn) + ": truth[" + std::to_string(i) + "] = " + std::to_string(truth[i]) + " outside [0, " + std::to_string(Na) + ")");
    if (!device_ok(device)) return fail(L3_EHIP, no_gpu_message(fn, device));
    const int S = topk_segments(Nv, Na, k, segments);
    DeviceBufs bufs;
    float* du = bufs.put(u, (size_t)Nv * H, nullptr);
    float* dt = bufs.put(t, (size_t)Na * H, nullptr);
    float* dw = bufs.put(wd, (size_t)H, nullptr);
    int32_t* dtr = truth ? bufs.put(truth, (size_t)Nv, nullptr) : nullptr;
    int32_t* dgq = group_q ? bufs.put(group_q, (size_t)Nv, nullptr) : nullptr;
    int32_t* dgc = group_c ? bufs.put(group_c, (size_t)Na, nullptr) : nullptr;
    float* dpm = bufs.alloc<float>(topk_partial_count(Nv, k, S));
    int32_t* dpj = bufs.alloc<int32_t>(topk_partial_count(Nv, k, S));
    float* dm = bufs.alloc<float>((size_t)Nv * k);
    int32_t* di = bufs.alloc<int32_t>((size_t)Nv * k);
    if (!bufs.ok()) return fail(L3_ENOMEM, std::string(fn) + ": device allocation or upload failed");
    launch_topk_lists(du, dt, dw, bd, H, Nv, Na, k, S, dtr, dgq, dgc, dpm, dpj, nullptr);
    launch_topk_merge(dpm, dpj, Nv, k, S, di, dm, nullptr);
    if (hipMemcpy(idx, di, (size_t)Nv * k * 4, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(margin, dm, (size_t)Nv * k * 4, hipMemcpyDeviceToHost) != hipSuccess || hipGetLastError() != hipSuccess)
        return fail(L3_EHIP, std::string(fn) + ": the kernels or the copy from the device failed");
    return L3_OK;
}

// Device time of `reps` launches of one kernel on resident operands, in ms per launch (hipEvents; one untimed launch first).
// what 0: the pair kernel storing margins of the whole matrix; 1: the rank mode with the diagonal as truth (Nv == Na); 2 / 3: the
// vision / audio projection of `n_rows` zero rows; 4: the top-k lists of both directions (both kernels of each) with the diagonal as
// truth and no groups (Nv == Na), k = n_rows or 10 for n_rows 0; 5: the merge kernel of the frames' lists alone, after one untimed
// pass that fills the segments' lists.  For profiles/ records; no test asserts a time.
int l3_pairs_time(l3_pairs* p, int what, int64_t n_rows, int reps, double* ms) {
    const char* fn = "l3_pairs_time";
    if (int rc = enter(p, fn)) return rc;
    if (!ms || reps < 1 || what < 0 || what > 5) return fail(L3_EINVAL, std::string(fn) + ": need ms, reps >= 1 and what in [0, 5]");
    const bool topk = what >= 4;
    const int k = (topk && n_rows) ? ((n_rows < 1 || n_rows > TOPK_MAX) ? 0 : (int)n_rows) : 10;
    if (topk && (k < 1 || k > TOPK_MAX)) return fail(L3_EINVAL, std::string(fn) + ": top-k is timed with k (n_rows) in [1, " + std::to_string(TOPK_MAX) + "], or 0 for 10");
    int seg = 1;
    size_t part = 0;
    if (!p->head_set) return fail(L3_ESTATE, std::string(fn) + ": l3_pairs_set_head has not been called");
    hipEvent_t a, b;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return fail(L3_EHIP, std::string(fn) + ": hipEventCreate failed");
    int rc = L3_OK;
    auto run = [&](int n) {
        for (int r = 0; r < n; ++r) {
            if (what == 0) {
                launch_tile(MODE_MARGIN, p->U, p->T, p->wd, p->bd, p->head, 0, (int)p->Nv, 0, (int)p->Na, p->out, nullptr, nullptr, nullptr, nullptr,
                            nullptr, nullptr, p->s);
            } else if (what == 1) {
                launch_tile(MODE_RANK, p->U, p->T, p->wd, p->bd, p->head, 0, (int)p->Nv, 0, (int)p->Na, nullptr, p->out, p->out + p->Nv, nullptr,
                            nullptr, p->idx, p->idx + p->Nv, p->s);
            } else if (topk) {          // idx: the diagonal (N), partial indices, final indices; out: partial and final margins
                int32_t *d_pj = p->idx + p->Nv, *d_idx = d_pj + part;
                float *d_pm = p->out, *d_m = p->out + part;
                if (what == 4) launch_topk_lists(p->U, p->T, p->wd, p->bd, p->head, p->Nv, p->Na, k, seg, p->idx, nullptr, nullptr, d_pm, d_pj, p->s);
                launch_topk_merge(d_pm, d_pj, p->Nv, k, seg, d_idx, d_m, p->s);
                if (what == 4) launch_topk_lists(p->T, p->U, p->wd, p->bd, p->head, p->Na, p->Nv, k, seg, p->idx, nullptr, nullptr, d_pm, d_pj, p->s);
                if (what == 4) launch_topk_merge(d_pm, d_pj, p->Na, k, seg, d_idx, d_m, p->s);
            } else {
                const bool vision = what == 2;
                launch_project(p->rows, vision ? p->nv : p->na, p->w1 + (vision ? 0 : (size_t)p->nv * p->head), vision ? nullptr : p->b1, p->out,
                               n_rows, vision ? p->nv : p->na, p->head, p->s);
            }
        }
    };
    if (topk) {
        if ((rc = need_sets(p, fn)) == L3_OK && p->Nv != p->Na) rc = fail(L3_EINVAL, std::string(fn) + ": top-k is timed with Nv == Na");
        if (rc == L3_OK) {
            seg = topk_segments(p->Nv, p->Na, k, 0);
            part = topk_partial_count(p->Nv, k, seg);
            const size_t fin = (size_t)p->Nv * k;
            std::vector<int32_t> d((size_t)p->Nv);
            for (int64_t i = 0; i < p->Nv; ++i) d[i] = (int32_t)i;
            if ((rc = grow(p, &p->idx, &p->cap_idx, (size_t)p->Nv + part + fin, fn)) == L3_OK &&
                (rc = grow(p, &p->out, &p->cap_out, part + fin, fn)) == L3_OK) {
                if (hipMemcpyAsync(p->idx, d.data(), (size_t)p->Nv * 4, hipMemcpyHostToDevice, p->s) != hipSuccess)
                    rc = fail(L3_EHIP, std::string(fn) + ": copy to the device failed");
                else if (what == 5)
                    launch_topk_lists(p->U, p->T, p->wd, p->bd, p->head, p->Nv, p->Na, k, seg, p->idx, nullptr, nullptr, p->out, p->idx + p->Nv, p->s);
                if (rc == L3_OK && !finished(p->s)) rc = fail(L3_EHIP, std::string(fn) + ": the set-up failed on the device");
            }
        }
    } else if (what <= 1) {
        if ((rc = need_sets(p, fn)) == L3_OK) {
            const int64_t N = p->Nv + p->Na;
            if (what == 0) rc = grow(p, &p->out, &p->cap_out, (size_t)p->Nv * (size_t)p->Na, fn);
            if (what == 1 && p->Nv != p->Na) rc = fail(L3_EINVAL, std::string(fn) + ": the rank mode is timed with Nv == Na");
            if (what == 1 && rc == L3_OK) rc = grow(p, &p->out, &p->cap_out, (size_t)N, fn);
            if (what == 1 && rc == L3_OK) rc = grow(p, &p->idx, &p->cap_idx, (size_t)N, fn);
            if (what == 1 && rc == L3_OK) {
                std::vector<int32_t> d((size_t)p->Nv);
                for (int64_t i = 0; i < p->Nv; ++i) d[i] = (int32_t)i;
                if (grow(p, &p->rows, &p->cap_rows, (size_t)N, fn) == L3_OK &&
                    hipMemcpyAsync(p->rows, d.data(), (size_t)p->Nv * 4, hipMemcpyHostToDevice, p->s) == hipSuccess) {
                    const int32_t* di = reinterpret_cast<const int32_t*>(p->rows);
                    launch_list(p->U, p->T, p->wd, p->bd, p->head, di, di, p->Nv, p->out, p->s);
                    launch_list(p->U, p->T, p->wd, p->bd, p->head, di, di, p->Nv, p->out + p->Nv, p->s);
                    if (!finished(p->s)) rc = fail(L3_EHIP, std::string(fn) + ": the truth scores failed on the device");
                } else {
                    rc = fail(L3_EHIP, std::string(fn) + ": copy to the device failed");
                }
            }
        }
    } else {
        if (n_rows < 1 || n_rows > MAX_ITEMS) rc = fail(L3_EINVAL, std::string(fn) + ": n_rows out of range");
        const int K = what == 2 ? p->nv : p->na;
        if (rc == L3_OK) rc = grow(p, &p->rows, &p->cap_rows, (size_t)n_rows * K, fn);
        if (rc == L3_OK) rc = grow(p, &p->out, &p->cap_out, (size_t)n_rows * p->head, fn);
        if (rc == L3_OK && hipMemsetAsync(p->rows, 0, (size_t)n_rows * K * 4, p->s) != hipSuccess) rc = fail(L3_EHIP, std::string(fn) + ": memset failed");
    }
    if (rc == L3_OK) {
        run(1);
        float t = 0.0f;
        if (hipEventRecord(a, p->s) != hipSuccess) rc = fail(L3_EHIP, std::string(fn) + ": hipEventRecord failed");
        run(reps);
        if (rc == L3_OK && (hipEventRecord(b, p->s) != hipSuccess || !finished(p->s) || hipEventElapsedTime(&t, a, b) != hipSuccess))
            rc = fail(L3_EHIP, std::string(fn) + ": the timed launches failed");
        *ms = (double)t / reps;
    }
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    return rc;
}

}  // extern "C"
