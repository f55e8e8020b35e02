// knn.hip -- nearest neighbours among embedding rows: distance blocks, listed pairs, top-k lists and votes.
//
// The arithmetic, which is the contract (include/l3hip.h, "Nearest neighbours"):
//     dot(q, c) = fmaf(q[D-1], c[D-1], ... fmaf(q[0], c[0], 0))          one fp32 chain in ascending feature order
//     nn(x)     = dot(x, x)                                              computed once per row when the rows are set
//     sqeuclidean  d = max(0, fl(fl(nn(q) + nn(c)) - 2 dot(q, c)))       (a NaN stays a NaN)
//     cosine       d = fl(1 - fl(fl(dot(q, c) r(q)) r(c))),  r(x) = 1 / sqrt(nn(x)) correctly rounded, 0 for nn(x) == 0
// v_mfma_f32_32x32x2_f32 gives exactly that chain when one accumulator takes the k-steps in ascending order, which is how every
// kernel here uses it: D is never split over waves or accumulators, and a k past D is a zero in both operands (fmaf(0, 0, acc) ==
// acc).  So a pair has the same bits in the matrix, in a list of pairs and in a top-k list, at every segment count and wherever it
// falls in a tile.  The file is compiled with -ffp-contract=off (_build.py): the epilogues' multiplications and subtractions stay
// separate roundings.
//
//   knn_side_kernel    a lane per row: nn(x) or r(x), the row's "side value"
//   knn_tile_kernel    a 128 x 128 block of distances per workgroup of 4 waves; wave w owns the query rows 32 w .. 32 w + 31 and all
//                      128 candidates: four independent 32 x 32 accumulators (the fp32 MFMA's issue rate needs no more).
//                      The tile's code is in knn_tile.h, which kmeans.hip shares.
//                      Query and candidate rows go through LDS 32 features at a time as [row][33]; the next chunk's global loads are
//                      issued into registers before the current chunk's MFMAs.  Rows past a set's end and features past D are zeros
//                      in the stage and are never read from memory.
//   knn_list_kernel    listed pairs, a lane per pair, the fmaf chain.
//   knn_topk_kernel    for 128 queries a workgroup, the k <= 64 nearest candidates of a segment of the database; the tile's
//                      distances go to LDS as [query][candidate] and through the threshold / ballot / list_insert scheme of
//                      pairs.hip's pair_topk_kernel (a copy with the order reversed: the smaller distance first; the two files
//                      share no code, so pairs.hip compiles as before).  knn_merge_kernel joins the segments, a wave per query.
//   knn_vote_kernel    neighbour indices + labels -> int32 votes per class at up to 8 list sizes and the predicted class, a wave per
//                      query; knn_file_vote_kernel sums a file's frames, a workgroup per file.  LDS integer adds only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/l3hip.h"
#include "device_common.h"
#include "featprep.h"
#include "host_common.h"
#include "knn.h"
#include "knn_tile.h"

namespace l3 {
namespace {

using namespace knn_tile;          // BLOCK, TQ, TC, KC, LDK, distance_of and the tile's dot products

constexpr int TOPK_MAX = L3_KNN_TOPK_MAX;
constexpr int EMPTY = INT32_MAX;            // a real index is at most 2^31 - 2
constexpr int MAX_SEGMENTS = L3_KNN_MAX_SEGMENTS;
// The segment count fills the chip evenly: a workgroup is one wave per SIMD and two fit a CU while their LDS does (k <= 15), so the
// chip has 256 or 512 places, and the count is the one whose workgroups fill whole rounds of those places best, a round lasting a
// segment's tiles (a last round that leaves most CUs idle cost a quarter of the time at 8 000 x 64 000 x 6144,
// profiles/r35_knn.txt), among counts that keep a
// segment MIN_TILES tiles long, so that the lists' start and the merge stay small beside the distances, and the workgroups within
// MAX_ROUNDS rounds.
constexpr int CUS = 256, CU_LDS_BYTES = 160 * 1024, STATIC_LDS_BYTES = (TQ * TC + TQ + TC) * 4;
constexpr int MIN_TILES = 4, MAX_ROUNDS = 8;
constexpr int VOTE_MAX_SIZES = L3_KNN_MAX_SIZES, VOTE_MAX_CLASSES = L3_KNN_MAX_CLASSES;
constexpr int64_t MAX_ROWS = INT32_MAX;     // indices 0 .. 2^31 - 2
constexpr int64_t TIME_BLOCK = 8192;        // l3_knn_time what 1: the block [0, 8192) x [0, 8192) at most

__global__ __launch_bounds__(BLOCK) void knn_side_kernel(const float* __restrict__ x, int64_t n, int D, int metric, float* __restrict__ out) {
    const int64_t r = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (r >= n) return;
    const float* p = x + r * D;
    float acc = 0.0f;
    int k = 0;
    if ((D & 3) == 0) {
        for (; k < D; k += 4) {
            const float4 v = *reinterpret_cast<const float4*>(p + k);
            acc = __fmaf_rn(v.x, v.x, acc);
            acc = __fmaf_rn(v.y, v.y, acc);
            acc = __fmaf_rn(v.z, v.z, acc);
            acc = __fmaf_rn(v.w, v.w, acc);
        }
    }
    for (; k < D; ++k) acc = __fmaf_rn(p[k], p[k], acc);
    out[r] = metric == L3_KNN_COSINE ? (acc == 0.0f ? 0.0f : __fdiv_rn(1.0f, __fsqrt_rn(acc))) : acc;
}

// ---- the tile (knn_tile.h: fetch_chunk, store_chunk, accumulate_tile, tile_distances) -----------------------------------------------
// The block [q0, q1) x [c0, c1) of distances: out[(i - q0) ldo + (j - c0)].  Workgroup (x, y): candidates from c0 + 128 x, queries
// from q0 + 128 y.
__global__ __launch_bounds__(BLOCK) void knn_tile_kernel(const float* __restrict__ Q, const float* __restrict__ Cd, const float* __restrict__ sq,
                                                         const float* __restrict__ sc, int D, int metric, int64_t q0, int64_t q1, int64_t c0,
                                                         int64_t c1, float* __restrict__ out, int64_t ldo) {
    __shared__ __attribute__((aligned(16))) float stage[TQ * TC];          // the staged chunks, then the tile's distances
    __shared__ float qs[TQ], cs[TC];
    const int tid = threadIdx.x;
    const int64_t i0 = q0 + (int64_t)blockIdx.y * TQ, j0 = c0 + (int64_t)blockIdx.x * TC;
    if (tid < TQ) qs[tid] = i0 + tid < q1 ? sq[i0 + tid] : 0.0f;
    if (tid < TC) cs[tid] = j0 + tid < c1 ? sc[j0 + tid] : 0.0f;
    f32x16 acc[4] = {};
    accumulate_tile(acc, stage, Q, Cd, D, i0, q1, j0, c1, tid);
    __syncthreads();          // every wave has read the last chunk: the stage becomes the distances
    tile_distances(acc, stage, qs, cs, metric, tid);
    __syncthreads();
    for (int e = tid; e < TQ * TC; e += BLOCK) {
        const int64_t i = i0 + e / TC, j = j0 + e % TC;
        if (i < q1 && j < c1) out[(i - q0) * ldo + (j - c0)] = stage[e];
    }
}

__global__ __launch_bounds__(BLOCK) void knn_list_kernel(const float* __restrict__ Q, const float* __restrict__ Cd, const float* __restrict__ sq,
                                                         const float* __restrict__ sc, int D, int metric, const int32_t* __restrict__ iq,
                                                         const int32_t* __restrict__ ic, int64_t n, float* __restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    const float* a = Q + (int64_t)iq[p] * D;
    const float* b = Cd + (int64_t)ic[p] * D;
    float acc = 0.0f;
    for (int k = 0; k < D; ++k) acc = __fmaf_rn(a[k], b[k], acc);
    out[p] = distance_of(metric, acc, sq[iq[p]], sc[ic[p]]);
}

// ---- top-k lists (l3hip.h: "The order of a neighbour list") ------------------------------------------------------------------------
// A list is k (distance, index) entries in the strict order `ahead`, one entry per lane of a wave (k <= 64 = the wave); an empty slot
// is (+inf, EMPTY), which every candidate is ahead of.
__device__ __forceinline__ bool ahead(float d, int j, float d2, int j2) { return (d < d2) | ((d == d2) & (j < j2)); }   // (no branches)

__device__ __forceinline__ float lane_value(float x, int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), lane)); }
__device__ __forceinline__ int lane_value(int x, int lane) { return __builtin_amdgcn_readlane(x, lane); }

// lane l reads lane l - 1 (DPP wave_shr:1, a VALU move); lane 0 keeps its own
__device__ __forceinline__ int lane_above(int x) { return __builtin_amdgcn_update_dpp(x, x, 0x138, 0xf, 0xf, false); }

// The candidate (cd, cj), the same in every lane, into the sorted list whose entry l is lane l's (ed, ej): the entries ahead of it
// are a prefix, its place is their number, the rest move down by one lane and the k-th falls off.  Whole waves only.
__device__ __forceinline__ void list_insert(float& ed, int& ej, float cd, int cj, int lane, int k) {
    const int pos = __popcll(__ballot((lane < k) & ahead(ed, ej, cd, cj)));
    const float pd = __int_as_float(lane_above(__float_as_int(ed)));
    const int pj = lane_above(ej);
    ed = lane == pos ? cd : lane > pos ? pd : ed;
    ej = lane == pos ? cj : lane > pos ? pj : ej;
}

// Workgroup (x, y): the queries [128 x, 128 x + 128) against the candidate tiles [y tiles_per_seg, (y + 1) tiles_per_seg), 128
// candidates at a time.  After a tile's accumulation the stage holds its 128 x 128 distances; wave w owns the queries 32 w .. 32 w + 31
// (the rows its own lanes wrote) and takes the tile's candidates in two halves of 64, a lane per candidate.  Lane qq < 32 of the wave
// keeps query 32 w + qq's group and k-th entry -- its threshold -- in registers: what is a candidate and ahead of the threshold is
// found by one ballot a query and half, and only then is the query's list (LDS, k entries) loaded, inserted into and stored.  The
// segment's first half tile meets empty lists and fills them by counting: a candidate's place is the number of candidates ahead of
// it.  The lists go to pd / pj[(y nq + i) k + l]; knn_merge_kernel joins the segments.  gq and gc are null together.
__global__ __launch_bounds__(BLOCK) void knn_topk_kernel(const float* __restrict__ Q, const float* __restrict__ Cd, const float* __restrict__ sq,
                                                         const float* __restrict__ sc, int D, int metric, int nq, int nc, int k,
                                                         int tiles_per_seg, const int32_t* __restrict__ gq, const int32_t* __restrict__ gc,
                                                         float* __restrict__ pd, int32_t* __restrict__ pj) {
    constexpr int QW = TQ / (BLOCK / 64);                                      // queries of a wave: 32
    __shared__ __attribute__((aligned(16))) float stage[TQ * TC];              // the staged chunks, then the tile's distances
    __shared__ float qs[TQ], cs[TC];
    extern __shared__ __attribute__((aligned(16))) unsigned char lists[];      // TQ x k distances, then TQ x k indices
    float* ld = reinterpret_cast<float*>(lists);
    int* lj = reinterpret_cast<int*>(ld + TQ * k);
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t i0 = (int64_t)blockIdx.x * TQ;
    const int64_t ntiles = ((int64_t)nc + TC - 1) / TC;
    const int64_t t0 = (int64_t)blockIdx.y * tiles_per_seg, t1 = min(ntiles, t0 + tiles_per_seg);
    for (int q = tid; q < TQ * k; q += BLOCK) ld[q] = INFINITY, lj[q] = EMPTY;
    if (tid < TQ) qs[tid] = i0 + tid < nq ? sq[i0 + tid] : 0.0f;
    const int64_t iq = i0 + w * QW + lane;          // lanes 0 .. QW-1: the wave's queries
    const bool viq = lane < QW && iq < nq;
    const int qgroup = (gq && viq) ? gq[iq] : 0;
    float thd = INFINITY;
    int thj = EMPTY;
    __syncthreads();
    for (int64_t tile = t0; tile < t1; ++tile) {
        const int64_t j0 = tile * TC;
        if (tid < TC) cs[tid] = j0 + tid < nc ? sc[j0 + tid] : 0.0f;          // (read after the barriers of the accumulation)
        f32x16 acc[4] = {};
        accumulate_tile(acc, stage, Q, Cd, D, i0, nq, j0, nc, tid);
        __syncthreads();          // every wave has read the last chunk: the stage becomes the distances
        tile_distances(acc, stage, qs, cs, metric, tid);
        for (int half = 0; half < TC / 64; ++half) {
            const int64_t jl = j0 + half * 64 + lane;
            const bool vj = jl < nc;
            const int j = (int)jl, jb = (int)(j0 + half * 64);          // (jb + b < nc wherever it is used)
            const int gj = (gc && vj) ? gc[jl] : 0;
            const bool first = tile == t0 && half == 0;
            for (int qq = 0; qq < QW; ++qq) {
                const int q = w * QW + qq;
                const float d = stage[q * TC + half * 64 + lane];          // (the wave's own LDS writes are in order before this read)
                const bool cand = vj && i0 + q < nq && d == d && (!gc || gj != lane_value(qgroup, qq));
                if (first) {          // the lists are empty: a candidate's place is the number of candidates ahead of it
                    int place = 0;
                    for (unsigned long long rest = __ballot(cand); rest; rest &= rest - 1) {
                        const int b = __ffsll((long long)rest) - 1;
                        place += ahead(lane_value(d, b), jb + b, d, j) ? 1 : 0;
                    }
                    if (cand && place < k) ld[q * k + place] = d, lj[q * k + place] = j;
                    const float nd = ld[q * k + k - 1];
                    const int nj = lj[q * k + k - 1];
                    if (lane == qq) thd = nd, thj = nj;
                    continue;
                }
                unsigned long long pass = __ballot(cand && ahead(d, j, lane_value(thd, qq), lane_value(thj, qq)));
                if (!pass) continue;
                float ed = lane < k ? ld[q * k + lane] : INFINITY;
                int ej = lane < k ? lj[q * k + lane] : EMPTY;
                while (pass) {
                    const int b = __ffsll((long long)pass) - 1;
                    pass &= pass - 1;
                    const float cd = lane_value(d, b);
                    if (ahead(cd, jb + b, lane_value(ed, k - 1), lane_value(ej, k - 1))) list_insert(ed, ej, cd, jb + b, lane, k);
                }
                if (lane < k) ld[q * k + lane] = ed, lj[q * k + lane] = ej;
                const float nd = lane_value(ed, k - 1);
                const int nj = lane_value(ej, k - 1);
                if (lane == qq) thd = nd, thj = nj;
            }
        }
        __syncthreads();          // the distances have been read: the next tile's chunks, and its cs, may come
    }
    for (int q = tid; q < TQ * k; q += BLOCK) {
        const int64_t i = i0 + q / k;
        if (i >= nq) continue;
        const int64_t o = ((int64_t)blockIdx.y * nq + i) * k + q % k;
        pd[o] = ld[q], pj[o] = lj[q];
    }
}

// A wave per query: the `segments` sorted lists of knn_topk_kernel into the first k of their union, in the same order; empty slots
// leave as index -1 and distance +inf.
__global__ __launch_bounds__(BLOCK) void knn_merge_kernel(const float* __restrict__ pd, const int32_t* __restrict__ pj, int nq, int k,
                                                          int segments, int32_t* __restrict__ idx, float* __restrict__ dist) {
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * (BLOCK / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (q >= nq) return;          // whole waves leave
    float ed = INFINITY;
    int ej = EMPTY;
    for (int s = 0; s < segments; ++s) {
        const int64_t base = ((int64_t)s * nq + q) * k;
        const float sd = lane < k ? pd[base + lane] : INFINITY;
        const int sj = lane < k ? pj[base + lane] : EMPTY;
        if (s == 0) {
            ed = sd, ej = sj;
            continue;
        }
        for (int l = 0; l < k; ++l) {          // a segment's entries come in order: the first that is not ahead of the k-th ends it
            const float cd = lane_value(sd, l);
            const int cj = lane_value(sj, l);
            if (cj == EMPTY || !ahead(cd, cj, lane_value(ed, k - 1), lane_value(ej, k - 1))) break;
            list_insert(ed, ej, cd, cj, lane, k);
        }
    }
    if (lane < k) {
        idx[q * k + lane] = ej == EMPTY ? -1 : ej;
        dist[q * k + lane] = ed;
    }
}

// ---- votes ------------------------------------------------------------------------------------------------------------------------
// The class of the most votes, the lowest class among equals, -1 when nobody voted: (bv, bc) of a lane's classes in ascending order
// (bv starts at 0, so a class without votes never leads), then across the wave.
__device__ __forceinline__ int wave_leader(int bv, int bc) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int ov = __shfl_xor(bv, o), oc = __shfl_xor(bc, o);
        if (ov > bv || (ov == bv && ov > 0 && oc < bc)) bv = ov, bc = oc;
    }
    return bc;
}

// A wave per query: entry l < k of its list votes for labels[idx[q k + l]] at every size ks[s] > l (ks ascending: the votes of size
// s are those of size s - 1 and the entries ks[s - 1] .. ks[s] - 1).  counts (n, S, C) and pred (n, S), each written when not null.
__global__ __launch_bounds__(BLOCK) void knn_vote_kernel(const int32_t* __restrict__ idx, const int32_t* __restrict__ labels, int64_t n, int k,
                                                         const int32_t* __restrict__ ks, int S, int C, int32_t* __restrict__ counts,
                                                         int32_t* __restrict__ pred) {
    __shared__ int cnt[BLOCK / 64][VOTE_MAX_CLASSES];
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t q = (int64_t)blockIdx.x * (BLOCK / 64) + w;
    if (q >= n) return;          // whole waves leave; no workgroup barrier below
    int* c = cnt[w];
    for (int e = lane; e < C; e += 64) c[e] = 0;
    const int j = lane < k ? idx[q * k + lane] : -1;
    const int lab = j >= 0 ? labels[j] : -1;
    int prev = 0;
    for (int s = 0; s < S; ++s) {
        const int ke = ks[s];
        if (lane >= prev && lane < ke && lab >= 0) atomicAdd(&c[lab], 1);          // (LDS, integers; a wave's LDS operations are in order)
        prev = ke;
        int bv = 0, bc = -1;
        for (int e = lane; e < C; e += 64) {
            const int v = c[e];
            if (counts) counts[(q * S + s) * C + e] = v;
            if (v > bv) bv = v, bc = e;
        }
        bc = wave_leader(bv, bc);
        if (lane == 0 && pred) pred[q * S + s] = bc;
    }
}

// A workgroup per file: the votes of the rows [files[2 f], files[2 f + 1]) summed per size and class, straight from the lists.
__global__ __launch_bounds__(BLOCK) void knn_file_vote_kernel(const int32_t* __restrict__ idx, const int32_t* __restrict__ labels, int k,
                                                              const int32_t* __restrict__ ks, int S, int C, const int64_t* __restrict__ files,
                                                              int32_t* __restrict__ fcounts, int32_t* __restrict__ fpred) {
    __shared__ int hist[VOTE_MAX_SIZES][VOTE_MAX_CLASSES];
    const int tid = threadIdx.x;
    const int64_t f = blockIdx.x, r0 = files[2 * f], r1 = files[2 * f + 1];
    for (int e = tid; e < VOTE_MAX_SIZES * VOTE_MAX_CLASSES; e += BLOCK) (&hist[0][0])[e] = 0;
    __syncthreads();
    const int64_t total = (r1 - r0) * k;
    for (int64_t e = tid; e < total; e += BLOCK) {
        const int l = (int)(e % k);
        const int j = idx[r0 * k + e];
        if (j < 0) continue;
        const int lab = labels[j];
        for (int s = 0; s < S; ++s)
            if (l < ks[s]) atomicAdd(&hist[s][lab], 1);
    }
    __syncthreads();
    if (fcounts)
        for (int e = tid; e < S * C; e += BLOCK) fcounts[f * S * C + e] = hist[e / C][e % C];
    if (tid < S && fpred) {
        int bv = 0, bc = -1;
        for (int e = 0; e < C; ++e)
            if (hist[tid][e] > bv) bv = hist[tid][e], bc = e;
        fpred[f * S + tid] = bc;
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
bool finished(hipStream_t s) { return hipStreamSynchronize(s) == hipSuccess && hipGetLastError() == hipSuccess; }

void launch_side(const float* x, int64_t n, int D, int metric, float* out, hipStream_t s) {
    hipLaunchKernelGGL(knn_side_kernel, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, x, n, D, metric, out);
}

void launch_tile(const l3_knn* h, int64_t q0, int64_t q1, int64_t c0, int64_t c1, float* out, hipStream_t s) {
    const dim3 grid((unsigned)((c1 - c0 + TC - 1) / TC), (unsigned)((q1 - q0 + TQ - 1) / TQ));
    hipLaunchKernelGGL(knn_tile_kernel, grid, dim3(BLOCK), 0, s, h->Q, h->X, h->sQ, h->sX, h->D, h->metric, q0, q1, c0, c1, out, c1 - c0);
}

// Segments of the database for nq queries against nc candidates at list size k: `asked` clamped to the number of tiles, or, for 0,
// the count described at MAX_ROUNDS above.
int topk_segments(int64_t nq, int64_t nc, int k, int asked) {
    const int64_t qt = (nq + TQ - 1) / TQ, ct = (nc + TC - 1) / TC;
    if (asked) return (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(asked, ct), MAX_SEGMENTS));
    const int64_t places = CUS * (2 * (STATIC_LDS_BYTES + TQ * k * 8) <= CU_LDS_BYTES ? 2 : 1);
    const int64_t most = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(ct / MIN_TILES, MAX_SEGMENTS), (MAX_ROUNDS * places + qt - 1) / qt));
    int64_t best = 1;
    double best_fill = 0.0;
    for (int64_t s = 1; s <= most; ++s) {          // a round takes a segment's tiles; the segments that hold tiles make the workgroups
        const int64_t per = (ct + s - 1) / s, held = (ct + per - 1) / per, rounds = (qt * held + places - 1) / places;
        const double fill = (double)(qt * ct) / (double)(rounds * places * per);
        if (fill > best_fill + 1e-9) best = s, best_fill = fill;          // the smaller count among equals
    }
    return (int)best;
}

void launch_topk(const l3_knn* h, int k, int segments, const int32_t* gq, const int32_t* gc, float* pd, int32_t* pj, int32_t* idx,
                 float* dist, hipStream_t s) {
    // (per device, so on every launch: the lists of k = 64 and the stage are 129 KiB of the CU's 160)
    (void)hipFuncSetAttribute((const void*)knn_topk_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, TQ * TOPK_MAX * 8);
    const int64_t ct = (h->nX + TC - 1) / TC;
    const dim3 grid((unsigned)((h->nQ + TQ - 1) / TQ), (unsigned)segments);
    hipLaunchKernelGGL(knn_topk_kernel, grid, dim3(BLOCK), (size_t)TQ * k * 8, s, h->Q, h->X, h->sQ, h->sX, h->D, h->metric, (int)h->nQ,
                       (int)h->nX, k, (int)((ct + segments - 1) / segments), gq, gc, pd, pj);
    hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)((h->nQ + BLOCK / 64 - 1) / (BLOCK / 64))), dim3(BLOCK), 0, s, pd, pj, (int)h->nQ, k,
                       segments, idx, dist);
}

template <class T>
int grow(l3_knn* h, T** buf, size_t* cap, size_t count, const char* fn) {
    if (*buf && count <= *cap) return L3_OK;
    // whatever read the old buffer has finished: every call on the handle waits for its stream before it returns
    h->bufs.grow(buf, cap, count);
    if (*buf) return L3_OK;
    return fail(L3_ENOMEM, std::string(fn) + ": device allocation of " + std::to_string(DeviceBufs::bytes_of<T>(count)) + " bytes failed");
}

int enter(l3_knn* h, const char* fn) {
    if (!h) return fail(L3_EINVAL, std::string(fn) + ": NULL handle");
    if (hipSetDevice(h->device) != hipSuccess) return fail(L3_EHIP, no_gpu_message(fn, h->device));
    return L3_OK;
}

int need_sets(const l3_knn* h, const char* fn) {
    if (h->nX < 1 || h->nQ < 1)
        return fail(L3_EINVAL, std::string(fn) + ": the database and the queries come first (l3_knn_set_database, then l3_knn_set_queries or l3_knn_query_self)");
    return L3_OK;
}

// the query side follows the database when it is the database
void follow_self(l3_knn* h) {
    if (h->self) h->Q = h->X, h->sQ = h->sX, h->nQ = h->nX;
}

// rows on their way into one side: x_host or x_dev (n, D) -> the side's own buffer and its side values
int set_side(l3_knn* h, bool database, const float* x_host, const float* x_dev, int64_t n, const char* fn) {
    float** dst = database ? &h->X : &h->Q;
    float** sv = database ? &h->sX : &h->sQ;
    size_t* cap = database ? &h->cap_X : &h->cap_Q;
    size_t* cap_sv = database ? &h->cap_sX : &h->cap_sQ;
    if (database) {
        h->nX = 0;
        if (h->self) h->nQ = 0;
    } else {
        if (h->self) h->Q = nullptr, h->sQ = nullptr, h->cap_Q = h->cap_sQ = 0;          // they were the database's
        h->self = false, h->nQ = 0;
    }
    if (int rc = grow(h, dst, cap, (size_t)n * h->D, fn)) return rc;
    if (int rc = grow(h, sv, cap_sv, (size_t)n, fn)) return rc;
    const hipMemcpyKind kind = x_host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
    if (hipMemcpyAsync(*dst, x_host ? x_host : x_dev, (size_t)n * h->D * sizeof(float), kind, h->s) != hipSuccess)
        return fail(L3_EHIP, std::string(fn) + ": copy to the handle's rows failed");
    launch_side(*dst, n, h->D, h->metric, *sv, h->s);
    if (!finished(h->s)) return fail(L3_EHIP, std::string(fn) + ": the norms failed on the device");
    (database ? h->nX : h->nQ) = n;
    follow_self(h);
    return L3_OK;
}

int set_labels(l3_knn* h, const int32_t* labels, int64_t n, const char* fn) {
    h->has_labels = false, h->label_max = -1;
    if (!labels) return L3_OK;
    int32_t hi = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (labels[i] < 0) return fail(L3_EINVAL, std::string(fn) + ": labels[" + std::to_string(i) + "] = " + std::to_string(labels[i]) + " is negative");
        hi = std::max(hi, labels[i]);
    }
    if (int rc = grow(h, &h->labels, &h->cap_labels, (size_t)n, fn)) return rc;
    if (hipMemcpyAsync(h->labels, labels, (size_t)n * 4, hipMemcpyHostToDevice, h->s) != hipSuccess || !finished(h->s))
        return fail(L3_EHIP, std::string(fn) + ": copy of the labels to the device failed");
    h->has_labels = true, h->label_max = hi;
    return L3_OK;
}

int check_rows(const float* rows, int64_t n, const char* fn) {
    if (!rows) return fail(L3_EINVAL, std::string(fn) + ": rows is NULL");
    if (n < 1 || n > MAX_ROWS) return fail(L3_EINVAL, std::string(fn) + ": need 1 <= n <= 2^31 - 1 rows, not " + std::to_string(n));
    return L3_OK;
}

int check_feat(const l3_knn* h, const l3_feat* f, int64_t lo, int64_t hi, const char* fn) {
    if (!f) return fail(L3_EINVAL, std::string(fn) + ": the feature matrix is NULL");
    if (f->device != h->device)
        return fail(L3_EINVAL, std::string(fn) + ": the features are on device " + std::to_string(f->device) + ", the handle on device " + std::to_string(h->device));
    if (f->D != h->D)
        return fail(L3_EINVAL, std::string(fn) + ": the features have " + std::to_string(f->D) + " columns, the handle's rows " + std::to_string(h->D));
    if (lo < 0 || hi > f->n || lo >= hi)
        return fail(L3_EINVAL, std::string(fn) + ": rows [" + std::to_string(lo) + ", " + std::to_string(hi) + ") are empty or outside the " +
                                   std::to_string(f->n) + " rows of the features");
    if (hi - lo > MAX_ROWS) return fail(L3_EINVAL, std::string(fn) + ": at most 2^31 - 1 rows");
    return L3_OK;
}

int check_k(int k, const char* fn) {
    if (k < 1 || k > TOPK_MAX) return fail(L3_EINVAL, std::string(fn) + ": need 1 <= k <= " + std::to_string(TOPK_MAX) + ", not " + std::to_string(k));
    return L3_OK;
}

int check_groups(const int32_t* gq, const int32_t* gc, const char* fn) {
    if ((gq == nullptr) != (gc == nullptr)) return fail(L3_EINVAL, std::string(fn) + ": group_q and group_c are given together or both NULL");
    return L3_OK;
}

// The lists of every query on the device.  Scratch: idx = groups (nQ + nX), partial indices, final indices (nQ k), then `extra`
// int32 of the caller's; out = partial distances, final distances.
struct Lists {
    int32_t *idx = nullptr, *extra = nullptr;
    float* dist = nullptr;
};

int run_topk(l3_knn* h, int k, int asked_segments, const int32_t* gq, const int32_t* gc, size_t extra, const char* fn, Lists* got) {
    const int64_t nQ = h->nQ, nX = h->nX;
    const int seg = topk_segments(nQ, nX, k, asked_segments);
    const size_t part = (size_t)seg * (size_t)nQ * (size_t)k, fin = (size_t)nQ * k, ng = gq ? (size_t)(nQ + nX) : 0;
    if (int rc = grow(h, &h->idx, &h->cap_idx, ng + part + fin + extra, fn)) return rc;
    if (int rc = grow(h, &h->out, &h->cap_out, part + fin, fn)) return rc;
    if (gq && (hipMemcpyAsync(h->idx, gq, (size_t)nQ * 4, hipMemcpyHostToDevice, h->s) != hipSuccess ||
               hipMemcpyAsync(h->idx + nQ, gc, (size_t)nX * 4, hipMemcpyHostToDevice, h->s) != hipSuccess))
        return fail(L3_EHIP, std::string(fn) + ": copy of the groups to the device failed");
    int32_t* d_pj = h->idx + ng;
    got->idx = d_pj + part, got->extra = got->idx + fin, got->dist = h->out + part;
    launch_topk(h, k, seg, gq ? h->idx : nullptr, gq ? h->idx + nQ : nullptr, h->out, d_pj, got->idx, got->dist, h->s);
    return L3_OK;
}

}  // namespace
}  // namespace l3

using namespace l3;

extern "C" {

int l3_knn_create(int device, int D, int metric, l3_knn** out) {
    if (!out) return fail(L3_EINVAL, "l3_knn_create: out is NULL");
    *out = nullptr;
    if (D < 1 || D > (1 << 20)) return fail(L3_EINVAL, "l3_knn_create: need 1 <= D <= 2^20 features, not " + std::to_string(D));
    if (metric != L3_KNN_SQEUCLIDEAN && metric != L3_KNN_COSINE)
        return fail(L3_EINVAL, "l3_knn_create: metric must be L3_KNN_SQEUCLIDEAN or L3_KNN_COSINE, not " + std::to_string(metric));
    if (!device_ok(device)) return fail(L3_EHIP, no_gpu_message("l3_knn_create", device));
    l3_knn* h = new l3_knn();
    h->device = device, h->D = D, h->metric = metric;
    if (hipStreamCreateWithFlags(&h->s, hipStreamNonBlocking) != hipSuccess) {
        h->s = nullptr;
        l3_knn_destroy(h);
        return fail(L3_EHIP, "l3_knn_create: hipStreamCreate failed");
    }
    *out = h;
    return L3_OK;
}

void l3_knn_destroy(l3_knn* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->s) (void)hipStreamSynchronize(h->s);
    if (h->s) (void)hipStreamDestroy(h->s);
    delete h;
}

int l3_knn_set_database(l3_knn* h, const float* rows, int64_t n, const int32_t* labels) {
    const char* fn = "l3_knn_set_database";
    if (int rc = enter(h, fn)) return rc;
    if (int rc = check_rows(rows, n, fn)) return rc;
    h->nX = 0;
    if (h->self) h->nQ = 0;
    if (int rc = set_labels(h, labels, n, fn)) return rc;
    return set_side(h, true, rows, nullptr, n, fn);
}

int l3_knn_set_database_dev(l3_knn* h, const l3_feat* f, int64_t lo, int64_t hi, const int32_t* labels) {
    const char* fn = "l3_knn_set_database_dev";
    if (int rc = enter(h, fn)) return rc;
    if (int rc = check_feat(h, f, lo, hi, fn)) return rc;
    h->nX = 0;
    if (h->self) h->nQ = 0;
    if (int rc = set_labels(h, labels, hi - lo, fn)) return rc;
    // (every l3_feat call has finished on its handle's stream when it returns: the rows hold their final values)
    return set_side(h, true, nullptr, f->x + lo * f->D, hi - lo, fn);
}

int l3_knn_set_queries(l3_knn* h, const float* rows, int64_t n) {
    const char* fn = "l3_knn_set_queries";
    if (int rc = enter(h, fn)) return rc;
    if (int rc = check_rows(rows, n, fn)) return rc;
    return set_side(h, false, rows, nullptr, n, fn);
}

int l3_knn_set_queries_dev(l3_knn* h, const l3_feat* f, int64_t lo, int64_t hi) {
    const char* fn = "l3_knn_set_queries_dev";
    if (int rc = enter(h, fn)) return rc;
    if (int rc = check_feat(h, f, lo, hi, fn)) return rc;
    return set_side(h, false, nullptr, f->x + lo * f->D, hi - lo, fn);
}

int l3_knn_query_self(l3_knn* h) {
    const char* fn = "l3_knn_query_self";
    if (int rc = enter(h, fn)) return rc;
    if (h->nX < 1) return fail(L3_EINVAL, std::string(fn) + ": l3_knn_set_database comes first");
    if (!h->self) {          // the queries' own rows go: the handle waits for its stream at the end of every call, nothing reads them
        h->bufs.release(h->Q);
        h->bufs.release(h->sQ);
        h->cap_Q = h->cap_sQ = 0;
    }
    h->self = true;
    follow_self(h);
    return L3_OK;
}

int l3_knn_matrix(l3_knn* h, int64_t q0, int64_t q1, int64_t c0, int64_t c1, float* out) {
    const char* fn = "l3_knn_matrix";
    if (int rc = enter(h, fn)) return rc;
    if (!out) return fail(L3_EINVAL, std::string(fn) + ": out is NULL");
    if (int rc = need_sets(h, fn)) return rc;
    if (q0 < 0 || q1 > h->nQ || q0 >= q1 || c0 < 0 || c1 > h->nX || c0 >= c1 || q1 - q0 > (int64_t)65535 * TQ)
        return fail(L3_EINVAL, std::string(fn) + ": the block [" + std::to_string(q0) + ", " + std::to_string(q1) + ") x [" + std::to_string(c0) + ", " +
                                   std::to_string(c1) + ") is empty, has more than 65535 * 128 queries or is outside the " + std::to_string(h->nQ) +
                                   " x " + std::to_string(h->nX) + " pairs");
    const size_t count = (size_t)(q1 - q0) * (size_t)(c1 - c0);
    if (int rc = grow(h, &h->out, &h->cap_out, count, fn)) return rc;
    launch_tile(h, q0, q1, c0, c1, h->out, h->s);
    if (hipMemcpyAsync(out, h->out, count * sizeof(float), hipMemcpyDeviceToHost, h->s) != hipSuccess || !finished(h->s))
        return fail(L3_EHIP, std::string(fn) + ": the kernel or the copy from the device failed");
    return L3_OK;
}

int l3_knn_list(l3_knn* h, const int32_t* iq, const int32_t* ic, int64_t n, float* out) {
    const char* fn = "l3_knn_list";
    if (int rc = enter(h, fn)) return rc;
    if (!iq || !ic || !out) return fail(L3_EINVAL, std::string(fn) + ": iq, ic and out must not be NULL");
    if (int rc = need_sets(h, fn)) return rc;
    if (n < 1 || n > INT32_MAX) return fail(L3_EINVAL, std::string(fn) + ": need 1 <= n <= 2^31 - 1 pairs");
    for (int64_t p = 0; p < n; ++p)
        if (iq[p] < 0 || iq[p] >= h->nQ || ic[p] < 0 || ic[p] >= h->nX)
            return fail(L3_EINVAL, std::string(fn) + ": pair " + std::to_string(p) + " = (" + std::to_string(iq[p]) + ", " + std::to_string(ic[p]) +
                                       ") outside the " + std::to_string(h->nQ) + " x " + std::to_string(h->nX) + " pairs");
    if (int rc = grow(h, &h->idx, &h->cap_idx, (size_t)n * 2, fn)) return rc;
    if (int rc = grow(h, &h->out, &h->cap_out, (size_t)n, fn)) return rc;
    if (hipMemcpyAsync(h->idx, iq, (size_t)n * 4, hipMemcpyHostToDevice, h->s) != hipSuccess ||
        hipMemcpyAsync(h->idx + n, ic, (size_t)n * 4, hipMemcpyHostToDevice, h->s) != hipSuccess)
        return fail(L3_EHIP, std::string(fn) + ": copy to the device failed");
    hipLaunchKernelGGL(knn_list_kernel, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, h->s, h->Q, h->X, h->sQ, h->sX, h->D, h->metric,
                       h->idx, h->idx + n, n, h->out);
    if (hipMemcpyAsync(out, h->out, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, h->s) != hipSuccess || !finished(h->s))
        return fail(L3_EHIP, std::string(fn) + ": the kernel or the copy from the device failed");
    return L3_OK;
}

static int topk_to_host(l3_knn* h, int k, int segments, const int32_t* gq, const int32_t* gc, int32_t* idx_out, float* dist_out, const char* fn) {
    Lists got;
    if (int rc = run_topk(h, k, segments, gq, gc, 0, fn, &got)) return rc;
    const size_t fin = (size_t)h->nQ * k;
    if (hipMemcpyAsync(idx_out, got.idx, fin * 4, hipMemcpyDeviceToHost, h->s) != hipSuccess ||
        hipMemcpyAsync(dist_out, got.dist, fin * 4, hipMemcpyDeviceToHost, h->s) != hipSuccess || !finished(h->s))
        return fail(L3_EHIP, std::string(fn) + ": the kernels or the copy from the device failed");
    return L3_OK;
}

int l3_knn_topk(l3_knn* h, int k, const int32_t* group_q, const int32_t* group_c, int32_t* idx_out, float* dist_out) {
    const char* fn = "l3_knn_topk";
    if (int rc = enter(h, fn)) return rc;
    if (!idx_out || !dist_out) return fail(L3_EINVAL, std::string(fn) + ": idx_out and dist_out must not be NULL");
    if (int rc = check_k(k, fn)) return rc;
    if (int rc = check_groups(group_q, group_c, fn)) return rc;
    if (int rc = need_sets(h, fn)) return rc;
    return topk_to_host(h, k, 0, group_q, group_c, idx_out, dist_out, fn);
}

int l3_knn_vote(l3_knn* h, int k, const int32_t* ks, int S, int n_classes, const int32_t* group_q, const int32_t* group_c,
                const int64_t* file_idxs, int64_t n_files, int32_t* counts, int32_t* pred, int32_t* file_counts, int32_t* file_pred) {
    const char* fn = "l3_knn_vote";
    if (int rc = enter(h, fn)) return rc;
    if (int rc = check_k(k, fn)) return rc;
    if (!ks || S < 1 || S > VOTE_MAX_SIZES) return fail(L3_EINVAL, std::string(fn) + ": need 1 <= S <= " + std::to_string(VOTE_MAX_SIZES) + " list sizes in ks");
    for (int s = 0; s < S; ++s)
        if (ks[s] < 1 || ks[s] > k || (s && ks[s] <= ks[s - 1]))
            return fail(L3_EINVAL, std::string(fn) + ": ks must ascend strictly within [1, k = " + std::to_string(k) + "]; ks[" + std::to_string(s) + "] = " + std::to_string(ks[s]));
    if (n_classes < 1 || n_classes > VOTE_MAX_CLASSES)
        return fail(L3_EINVAL, std::string(fn) + ": need 1 <= n_classes <= " + std::to_string(VOTE_MAX_CLASSES) + ", not " + std::to_string(n_classes));
    if (int rc = check_groups(group_q, group_c, fn)) return rc;
    if (int rc = need_sets(h, fn)) return rc;
    if (!h->has_labels) return fail(L3_EINVAL, std::string(fn) + ": the database was set without labels");
    if (h->label_max >= n_classes)
        return fail(L3_EINVAL, std::string(fn) + ": the database holds the label " + std::to_string(h->label_max) + ", outside [0, " + std::to_string(n_classes) + ")");
    if ((file_counts || file_pred) && !file_idxs) return fail(L3_EINVAL, std::string(fn) + ": file_counts and file_pred need file_idxs");
    if (file_idxs && n_files < 1) return fail(L3_EINVAL, std::string(fn) + ": file_idxs needs n_files >= 1");
    const int64_t nQ = h->nQ, F = file_idxs ? n_files : 0;
    for (int64_t f = 0; f < F; ++f)
        if (file_idxs[2 * f] < 0 || file_idxs[2 * f] >= file_idxs[2 * f + 1] || file_idxs[2 * f + 1] > nQ ||
            (file_idxs[2 * f + 1] - file_idxs[2 * f]) * k > INT32_MAX)
            return fail(L3_EINVAL, std::string(fn) + ": file " + std::to_string(f) + " = [" + std::to_string(file_idxs[2 * f]) + ", " + std::to_string(file_idxs[2 * f + 1]) +
                                       ") is empty, outside the " + std::to_string(nQ) + " queries or holds more than 2^31 votes");
    const size_t SC = (size_t)S * n_classes;
    const size_t n_counts = counts ? (size_t)nQ * SC : 0, n_pred = (size_t)nQ * S, n_fc = (size_t)F * SC, n_fp = (size_t)F * S;
    Lists got;
    if (int rc = run_topk(h, k, 0, group_q, group_c, VOTE_MAX_SIZES + n_counts + n_pred + n_fc + n_fp, fn, &got)) return rc;
    int32_t *d_ks = got.extra, *d_counts = d_ks + VOTE_MAX_SIZES, *d_pred = d_counts + n_counts, *d_fc = d_pred + n_pred, *d_fp = d_fc + n_fc;
    if (F && (grow(h, &h->files, &h->cap_files, (size_t)F * 2, fn) != L3_OK)) return L3_ENOMEM;
    bool ok = hipMemcpyAsync(d_ks, ks, (size_t)S * 4, hipMemcpyHostToDevice, h->s) == hipSuccess;
    if (F) ok = ok && hipMemcpyAsync(h->files, file_idxs, (size_t)F * 16, hipMemcpyHostToDevice, h->s) == hipSuccess;
    if (!ok) return fail(L3_EHIP, std::string(fn) + ": copy to the device failed");
    if (counts || pred)
        hipLaunchKernelGGL(knn_vote_kernel, dim3((unsigned)((nQ + BLOCK / 64 - 1) / (BLOCK / 64))), dim3(BLOCK), 0, h->s, got.idx, h->labels, nQ, k, d_ks, S,
                           n_classes, counts ? d_counts : nullptr, d_pred);
    if (file_counts || file_pred)
        hipLaunchKernelGGL(knn_file_vote_kernel, dim3((unsigned)F), dim3(BLOCK), 0, h->s, got.idx, h->labels, k, d_ks, S, n_classes, h->files, d_fc, d_fp);
    if (counts) ok = ok && hipMemcpyAsync(counts, d_counts, n_counts * 4, hipMemcpyDeviceToHost, h->s) == hipSuccess;
    if (pred) ok = ok && hipMemcpyAsync(pred, d_pred, n_pred * 4, hipMemcpyDeviceToHost, h->s) == hipSuccess;
    if (file_counts) ok = ok && hipMemcpyAsync(file_counts, d_fc, n_fc * 4, hipMemcpyDeviceToHost, h->s) == hipSuccess;
    if (file_pred) ok = ok && hipMemcpyAsync(file_pred, d_fp, n_fp * 4, hipMemcpyDeviceToHost, h->s) == hipSuccess;
    if (!ok || !finished(h->s)) return fail(L3_EHIP, std::string(fn) + ": the kernels or the copy from the device failed");
    return L3_OK;
}

int l3_op_knn_topk(int device, const float* Q, const float* Cd, int64_t nq, int64_t nc, int D, int metric, int k, int segments,
                   const int32_t* group_q, const int32_t* group_c, int32_t* idx, float* dist) {
    const char* fn = "l3_op_knn_topk";
    if (!Q || !Cd || !idx || !dist) return fail(L3_EINVAL, std::string(fn) + ": Q, C, idx and dist must not be NULL");
    if (D < 1 || D > (1 << 20)) return fail(L3_EINVAL, std::string(fn) + ": need 1 <= D <= 2^20 features, not " + std::to_string(D));
    if (int rc = check_k(k, fn)) return rc;
    if (segments < 0 || segments > MAX_SEGMENTS) return fail(L3_EINVAL, std::string(fn) + ": need 0 <= segments <= " + std::to_string(MAX_SEGMENTS));
    if (int rc = check_groups(group_q, group_c, fn)) return rc;
    if (int rc = check_rows(Q, nq, fn)) return rc;
    if (int rc = check_rows(Cd, nc, fn)) return rc;
    l3_knn* h = nullptr;
    int rc = l3_knn_create(device, D, metric, &h);
    if (rc == L3_OK) rc = set_side(h, true, Cd, nullptr, nc, fn);
    if (rc == L3_OK) rc = set_side(h, false, Q, nullptr, nq, fn);
    if (rc == L3_OK) rc = topk_to_host(h, k, segments, group_q, group_c, idx, dist, fn);
    l3_knn_destroy(h);
    return rc;
}

// Device time of `reps` launches on the resident sets, in ms per launch (hipEvents; one untimed launch first).  what 0: the top-k
// pass at k (the lists of every segment and their merge, no groups, the library's segment count); 1: the tile kernel storing the
// block [0, min(nQ, 8192)) x [0, min(nX, 8192)) of the matrix.  For profiles/ records; no test asserts a time.
int l3_knn_time(l3_knn* h, int what, int k, int reps, double* ms) {
    const char* fn = "l3_knn_time";
    if (int rc = enter(h, fn)) return rc;
    if (!ms || reps < 1 || what < 0 || what > 1) return fail(L3_EINVAL, std::string(fn) + ": need ms, reps >= 1 and what in [0, 1]");
    if (what == 0)
        if (int rc = check_k(k, fn)) return rc;
    if (int rc = need_sets(h, fn)) return rc;
    const int64_t bq = std::min(h->nQ, TIME_BLOCK), bc = std::min(h->nX, TIME_BLOCK);
    if (what == 1)
        if (int rc = grow(h, &h->out, &h->cap_out, (size_t)bq * bc, fn)) return rc;
    hipEvent_t a, b;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return fail(L3_EHIP, std::string(fn) + ": hipEventCreate failed");
    int rc = L3_OK;
    auto run = [&](int n) {
        for (int r = 0; r < n && rc == L3_OK; ++r) {
            Lists got;
            if (what == 0)
                rc = run_topk(h, k, 0, nullptr, nullptr, 0, fn, &got);
            else
                launch_tile(h, 0, bq, 0, bc, h->out, h->s);
        }
    };
    run(1);
    float t = 0.0f;
    if (rc == L3_OK && hipEventRecord(a, h->s) != hipSuccess) rc = fail(L3_EHIP, std::string(fn) + ": hipEventRecord failed");
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
