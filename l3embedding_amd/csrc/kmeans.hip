// kmeans.hip -- Lloyd's k-means over resident embedding rows, its seeding and the label statistics.
//
// The arithmetic, which is the contract (include/l3hip.h, "K-means"):
//     d(i, c)     the bits of l3_knn_matrix under L3_KNN_SQEUCLIDEAN: the tile and the epilogue of knn_tile.h, nn(x) once per row
//                 and once per centroid after every update
//     label(i)    the smallest (distance, index) in the strict order of a neighbour list; a NaN distance never wins; no winner: -1
//     float64 sums  the members in ascending row index, cut into runs of L3_KMEANS_RUN; a run summed sequentially from 0.0, the run
//                 sums added sequentially in ascending order.  No float atomics anywhere: the only atomics are integer counts.
// The file is compiled with -ffp-contract=off (_build.py), like knn.hip.
//
//   kmeans_norm_kernel      a lane per row: nn(x), the chain of knn.hip's knn_side_kernel
//   kmeans_assign_kernel    128 rows a workgroup of 4 waves, which walks every tile of 128 centroids itself: knn_tile.h's accumulation
//                           and distances, then two lanes per row scan the row's 128 distances in LDS (a rotated column order: 64
//                           lanes, 64 banks) and keep the running (distance, index) minimum in registers across the tiles.  No lists,
//                           no segments, no merge.  The last tile writes labels, distances and the count of changed labels.
//   kmeans_hist / colscan / keyscan / scatter_kernel   the stable counting sort of the rows by key (the label; or "has a label"):
//                           per-block histograms (integer atomics), a scan down the blocks, a scan over the keys, and a scatter that
//                           ranks a chunk of 256 rows by counting the equal keys before each.
//   kmeans_runsum_kernel    a workgroup per run of 256 members and 256 features: the member loop is sequential, the lanes run across
//                           features; a float64 partial per run.  kmeans_finish_kernel adds a cluster's partials in order, divides and
//                           narrows; an empty cluster keeps its centroid.
//   kmeans_inertia_*        the same two levels over the float32 distances of the rows that have a label.
//   kmeans_pp_*             k-means++: one centre against every row (a lane per row, the fmaf chain of knn_list_kernel, rows staged
//                           through LDS as [row][33]), the min, the run totals, and one workgroup that walks the runs to the pick.
//   kmeans_contingency_kernel, kmeans_file_hist_kernel   integer adds only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/l3hip.h"
#include "device_common.h"
#include "featprep.h"
#include "host_common.h"
#include "kmeans.h"
#include "knn_tile.h"

namespace l3 {
namespace {

using namespace knn_tile;          // BLOCK, TQ, TC, KC, LDK, distance_of and the tile's dot products

constexpr int RUN = L3_KMEANS_RUN;
static_assert(RUN == BLOCK, "a run is a workgroup's worth of members");
constexpr int EMPTY = INT32_MAX;            // a real index is at most 65535
constexpr int K_MAX = L3_KMEANS_MAX_CLUSTERS;
constexpr int C_MAX = L3_KMEANS_MAX_CLASSES;
constexpr int64_t MAX_ROWS = INT32_MAX;
constexpr int SCAN_LDS = 2048;              // run totals a single workgroup stages at a time
// (the label of a row before its first assignment is the byte pattern 0xFE: no label and not -1)

__device__ __forceinline__ bool ahead(float d, int j, float d2, int j2) { return (d < d2) | ((d == d2) & (j < j2)); }

__global__ __launch_bounds__(BLOCK) void kmeans_norm_kernel(const float* __restrict__ x, int64_t n, int D, float* __restrict__ out) {
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
    out[r] = acc;
}

// ---- assignment -------------------------------------------------------------------------------------------------------------------
// Workgroup x: the rows [128 x, 128 x + 128) against every centroid.  After a tile's distances are in the stage as [row][centroid],
// lane (r, h) of wave w scans row 32 w + r (one of the rows its own wave wrote): at step s the columns (2 r + h + 2 s) & 63 and that
// + 64, so the 64 lanes of a step read 64 different banks and the two lanes of a row take the even and the odd columns.  The order
// is strict, so the order of the scan does not enter.  labels: read (when `changed` is given) and written.
__global__ __launch_bounds__(BLOCK) void kmeans_assign_kernel(const float* __restrict__ X, const float* __restrict__ Cd, const float* __restrict__ nx,
                                                              const float* __restrict__ ncn, int D, int n, int K, int32_t* __restrict__ labels,
                                                              float* __restrict__ mind, unsigned long long* __restrict__ changed) {
    __shared__ __attribute__((aligned(16))) float stage[TQ * TC];          // the staged chunks, then the tile's distances
    __shared__ float qs[TQ], cs[TC];
    __shared__ int moved;
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5, w = tid >> 6;
    const int64_t i0 = (int64_t)blockIdx.x * TQ;
    if (tid < TQ) qs[tid] = i0 + tid < n ? nx[i0 + tid] : 0.0f;
    if (tid == 0) moved = 0;
    float bd = INFINITY;
    int bj = EMPTY;
    const float* m = stage + (32 * w + r) * TC;
    __syncthreads();
    for (int j0 = 0; j0 < K; j0 += TC) {
        if (tid < TC) cs[tid] = j0 + tid < K ? ncn[j0 + tid] : 0.0f;          // (read after the barriers of the accumulation)
        f32x16 acc[4] = {};
        accumulate_tile(acc, stage, X, Cd, D, i0, n, j0, K, tid);
        __syncthreads();          // every wave has read the last chunk: the stage becomes the distances
        tile_distances(acc, stage, qs, cs, L3_KNN_SQEUCLIDEAN, tid);
#pragma unroll 8
        for (int s = 0; s < 32; ++s) {          // (the wave's own LDS writes are in order before these reads)
            const int c0 = (2 * r + h + 2 * s) & 63, c1 = c0 + 64;
            const float d0 = m[c0], d1 = m[c1];
            if (j0 + c0 < K && ahead(d0, j0 + c0, bd, bj)) bd = d0, bj = j0 + c0;
            if (j0 + c1 < K && ahead(d1, j0 + c1, bd, bj)) bd = d1, bj = j0 + c1;
        }
        __syncthreads();          // the distances have been read: the next tile's chunks, and its cs, may come
    }
    const float od = __shfl_xor(bd, 32);
    const int oj = __shfl_xor(bj, 32);
    if (ahead(od, oj, bd, bj)) bd = od, bj = oj;
    const int64_t i = i0 + 32 * w + r;
    bool differs = false;
    if (h == 0 && i < n) {
        const int lab = bj == EMPTY ? -1 : bj;
        if (changed) differs = labels[i] != lab;
        labels[i] = lab;
        mind[i] = bj == EMPTY ? __int_as_float(0x7fc00000) : bd;
    }
    if (changed) {
        const int cnt = __popcll(__ballot(differs));
        if (lane == 0 && cnt) atomicAdd(&moved, cnt);
        __syncthreads();
        if (tid == 0 && moved) atomicAdd(changed, (unsigned long long)moved);
    }
}

// ---- the stable counting sort of the rows by key -----------------------------------------------------------------------------------
// mode 0: the key is the label, and K for a row without one (NK = K + 1 keys); mode 1: 0 for a row with a label, 1 without (NK = 2).
__device__ __forceinline__ int key_of(int lab, int mode, int K) { return mode == 0 ? (lab < 0 ? K : lab) : (lab < 0 ? 1 : 0); }

// block b: the rows [b rb, (b + 1) rb); hist[b NK + key] counts them (zeroed before)
__global__ __launch_bounds__(BLOCK) void kmeans_hist_kernel(const int32_t* __restrict__ labels, int64_t n, int rb, int mode, int K, int NK,
                                                            int32_t* __restrict__ hist) {
    const int64_t b = blockIdx.x, lo = b * rb, hi = min(n, lo + rb);
    for (int64_t i = lo + threadIdx.x; i < hi; i += BLOCK) atomicAdd(&hist[b * NK + key_of(labels[i], mode, K)], 1);
}

// a lane per key: hist[b][key] becomes the number of the key's rows in the blocks before b, count[key] their number in all
__global__ __launch_bounds__(BLOCK) void kmeans_colscan_kernel(int32_t* __restrict__ hist, int64_t nb, int NK, int32_t* __restrict__ count) {
    const int key = blockIdx.x * BLOCK + threadIdx.x;
    if (key >= NK) return;
    int run = 0;
    for (int64_t b = 0; b < nb; ++b) {
        const int t = hist[b * NK + key];
        hist[b * NK + key] = run;
        run += t;
    }
    count[key] = run;
}

// One workgroup: start[key] = the rows of smaller keys, runoff[key] = the runs of smaller keys among the first KR (the others have
// none); start[NK] and runoff[NK] the totals.  Also the iteration's integer scalars.
__global__ __launch_bounds__(BLOCK) void kmeans_keyscan_kernel(const int32_t* __restrict__ count, int NK, int KR, int mode, int32_t* __restrict__ start,
                                                               int32_t* __restrict__ runoff, l3_kmeans_stats* __restrict__ stats) {
    __shared__ int sc[BLOCK], sr[BLOCK], empties;
    const int tid = threadIdx.x, chunk = (NK + BLOCK - 1) / BLOCK, lo = min(NK, tid * chunk), hi = min(NK, lo + chunk);
    if (tid == 0) empties = 0;
    __syncthreads();
    int a = 0, b = 0, e = 0;
    for (int k = lo; k < hi; ++k) {
        const int c = count[k];
        a += c;
        if (k < KR) b += (c + RUN - 1) / RUN, e += c == 0;
    }
    sc[tid] = a, sr[tid] = b;
    if (e) atomicAdd(&empties, e);
    __syncthreads();
    if (tid == 0) {
        int ta = 0, tb = 0;
        for (int t = 0; t < BLOCK; ++t) {
            const int va = sc[t], vb = sr[t];
            sc[t] = ta, sr[t] = tb;
            ta += va, tb += vb;
        }
        if (mode == 0) stats->empty = empties;
        else stats->valid = count[0];
    }
    __syncthreads();
    a = sc[tid], b = sr[tid];
    for (int k = lo; k < hi; ++k) {
        start[k] = a, runoff[k] = b;
        const int c = count[k];
        a += c;
        if (k < KR) b += (c + RUN - 1) / RUN;
    }
    if (hi == NK && lo < NK) start[NK] = a, runoff[NK] = b;
}

// block b again, 256 rows at a time in ascending order: a row's place is its key's start, the key's rows in earlier blocks and
// chunks (hist, moved on by each chunk) and the equal keys before it in the chunk.
__global__ __launch_bounds__(BLOCK) void kmeans_scatter_kernel(const int32_t* __restrict__ labels, int64_t n, int rb, int mode, int K, int NK,
                                                               int32_t* __restrict__ hist, const int32_t* __restrict__ start,
                                                               int32_t* __restrict__ ids) {
    __shared__ int lk[BLOCK];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x, lo = b * rb, hi = min(n, lo + rb);
    for (int64_t c0 = lo; c0 < hi; c0 += BLOCK) {
        const int64_t i = c0 + tid;
        const bool valid = i < hi;
        const int key = valid ? key_of(labels[i], mode, K) : -1;
        lk[tid] = key;
        __syncthreads();
        int rank = 0, total = 0;
        for (int t = 0; t < BLOCK; ++t) {
            const int same = lk[t] == key;
            rank += same & (t < tid);
            total += same;
        }
        if (valid) ids[start[key] + hist[b * NK + key] + rank] = (int)i;
        __syncthreads();          // every lane has read the chunk's keys and its key's place
        if (valid && rank == 0) hist[b * NK + key] += total;
        __syncthreads();
    }
}

// ---- the update --------------------------------------------------------------------------------------------------------------------
// Workgroup (x, y): run x of all clusters' runs (past their number: nothing) and the features 256 y .. 256 y + 255.
__global__ __launch_bounds__(BLOCK) void kmeans_runsum_kernel(const float* __restrict__ X, int D, int K, const int32_t* __restrict__ ids,
                                                              const int32_t* __restrict__ start, const int32_t* __restrict__ runoff,
                                                              double* __restrict__ part) {
    __shared__ int member[RUN];
    const int tid = threadIdx.x, r = blockIdx.x;
    if (r >= runoff[K]) return;          // (the whole workgroup)
    int lo = 0, hi = K;                  // the cluster c with runoff[c] <= r < runoff[c + 1]
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (runoff[mid + 1] <= r) lo = mid + 1;
        else hi = mid;
    }
    const int c = lo, m0 = start[c] + RUN * (r - runoff[c]), cnt = min(RUN, start[c + 1] - m0);
    member[tid] = tid < cnt ? ids[m0 + tid] : 0;
    __syncthreads();
    const int f = blockIdx.y * BLOCK + tid;
    if (f >= D) return;
    const float* p = X + f;
    double acc = 0.0;
    int q = 0;
    for (; q + 8 <= cnt; q += 8) {
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = p[(int64_t)member[q + e] * D];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc += (double)v[e];
    }
    for (; q < cnt; ++q) acc += (double)p[(int64_t)member[q] * D];
    part[(int64_t)r * D + f] = acc;
}

// Workgroup (x, y): cluster x, the features 256 y .. 256 y + 255
__global__ __launch_bounds__(BLOCK) void kmeans_finish_kernel(float* __restrict__ Cd, int D, const int32_t* __restrict__ count,
                                                              const int32_t* __restrict__ runoff, const double* __restrict__ part) {
    const int c = blockIdx.x, f = blockIdx.y * BLOCK + threadIdx.x, nc = count[c];
    if (f >= D || nc == 0) return;          // an empty cluster keeps its centroid
    double s = 0.0;
    for (int r = runoff[c]; r < runoff[c + 1]; ++r) s += part[(int64_t)r * D + f];
    Cd[(int64_t)c * D + f] = (float)(s / (double)nc);
}

// ---- the inertia -------------------------------------------------------------------------------------------------------------------
// a lane per run of the rows that have a label (ids: the mode 1 sort, whose key 0 comes first)
__global__ __launch_bounds__(BLOCK) void kmeans_inertia_run_kernel(const float* __restrict__ mind, const int32_t* __restrict__ ids,
                                                                   const int32_t* __restrict__ start, double* __restrict__ runs) {
    const int64_t r = (int64_t)blockIdx.x * BLOCK + threadIdx.x, valid = start[1], m0 = r * RUN;
    if (m0 >= valid) return;
    const int64_t m1 = min(valid, m0 + RUN);
    double acc = 0.0;
    for (int64_t q = m0; q < m1; ++q) acc += (double)mind[ids[q]];
    runs[r] = acc;
}

// One workgroup: the run totals added in order by one lane, staged through LDS by all
__global__ __launch_bounds__(BLOCK) void kmeans_inertia_final_kernel(const double* __restrict__ runs, const int32_t* __restrict__ start,
                                                                     l3_kmeans_stats* __restrict__ stats) {
    __shared__ double buf[SCAN_LDS];
    const int64_t R = ((int64_t)start[1] + RUN - 1) / RUN;
    double acc = 0.0;
    for (int64_t base = 0; base < R; base += SCAN_LDS) {
        const int cnt = (int)min((int64_t)SCAN_LDS, R - base);
        __syncthreads();
        for (int q = threadIdx.x; q < cnt; q += BLOCK) buf[q] = runs[base + q];
        __syncthreads();
        if (threadIdx.x == 0)
            for (int q = 0; q < cnt; ++q) acc += buf[q];
    }
    if (threadIdx.x == 0) stats->inertia = acc;
}

// ---- seeding -----------------------------------------------------------------------------------------------------------------------
// Workgroup x: the rows [256 x, 256 x + 256) against the row chosen[t]; mind = d at t == 0, else the smaller of the two (a NaN on
// either side leaves mind as it is, so the mind of a row with a NaN stays NaN).
__global__ __launch_bounds__(BLOCK) void kmeans_pp_dist_kernel(const float* __restrict__ X, const float* __restrict__ nx, int D, int64_t n,
                                                               const int64_t* __restrict__ chosen, int t, float* __restrict__ mind) {
    __shared__ float stage[RUN * LDK];
    __shared__ float cv[KC];
    const int tid = threadIdx.x;
    const int64_t pick = chosen[t], i0 = (int64_t)blockIdx.x * RUN;
    const float* c = X + pick * D;
    const bool vec = (D & 3) == 0;
    float acc = 0.0f;
    for (int k0 = 0; k0 < D; k0 += KC) {
        __syncthreads();          // the chunk before has been read
#pragma unroll
        for (int e8 = 0; e8 < 8; ++e8) {
            const int e = tid + BLOCK * e8, row = e >> 3, k = k0 + (e & 7) * 4;
            const int64_t g = i0 + row;
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (g < n && k < D) {
                const float* p = X + g * D + k;
                if (vec) {
                    v = *reinterpret_cast<const float4*>(p);
                } else {
                    v.x = p[0];
                    if (k + 1 < D) v.y = p[1];
                    if (k + 2 < D) v.z = p[2];
                    if (k + 3 < D) v.w = p[3];
                }
            }
            float* s = stage + row * LDK + (e & 7) * 4;
            s[0] = v.x, s[1] = v.y, s[2] = v.z, s[3] = v.w;
        }
        if (tid < KC) cv[tid] = k0 + tid < D ? c[k0 + tid] : 0.0f;
        __syncthreads();
        const int kn = min(KC, D - k0);
        const float* mine = stage + tid * LDK;
        for (int k = 0; k < kn; ++k) acc = __fmaf_rn(mine[k], cv[k], acc);
    }
    const int64_t i = i0 + tid;
    if (i >= n) return;
    const float d = distance_of(L3_KNN_SQEUCLIDEAN, acc, nx[i], nx[pick]);
    if (t == 0) {
        mind[i] = d;
    } else {
        const float old = mind[i];
        mind[i] = d < old ? d : old;
    }
}

__device__ __forceinline__ double potential_of(float v) { return v == v ? (double)v : 0.0; }

// a lane per run of 256 rows: the run's total
__global__ __launch_bounds__(BLOCK) void kmeans_pp_run_kernel(const float* __restrict__ mind, int64_t n, double* __restrict__ runs) {
    const int64_t r = (int64_t)blockIdx.x * BLOCK + threadIdx.x, m0 = r * RUN;
    if (m0 >= n) return;
    const int64_t m1 = min(n, m0 + RUN);
    double acc = 0.0;
    for (int64_t q = m0; q < m1; ++q) acc += potential_of(mind[q]);
    runs[r] = acc;
}

// One workgroup: chosen[t] by the rule of l3hip.h.  Lane 0 walks the run totals (staged through LDS by all) twice, for the total and
// for the run that holds the pick, then walks that run.
__global__ __launch_bounds__(BLOCK) void kmeans_pp_pick_kernel(const float* __restrict__ mind, int64_t n, const double* __restrict__ runs,
                                                               const double* __restrict__ u, int t, int64_t* __restrict__ chosen) {
    __shared__ double buf[SCAN_LDS];
    __shared__ float vals[RUN];
    __shared__ long long s_run, s_last, s_walk;
    __shared__ double s_off;
    const int tid = threadIdx.x;
    const int64_t R = (n + RUN - 1) / RUN;
    double total = 0.0, thr = 0.0, off = 0.0;
    for (int pass = 0; pass < 2; ++pass) {
        if (tid == 0) s_run = -1, s_last = -1, s_off = 0.0;
        for (int64_t base = 0; base < R; base += SCAN_LDS) {
            const int cnt = (int)min((int64_t)SCAN_LDS, R - base);
            __syncthreads();
            for (int q = tid; q < cnt; q += BLOCK) buf[q] = runs[base + q];
            __syncthreads();
            if (tid == 0) {
                for (int q = 0; q < cnt; ++q) {
                    if (pass == 0) {
                        total += buf[q];
                    } else {
                        const double next = off + buf[q];
                        if (s_run < 0 && next > thr) s_run = base + q, s_off = off;
                        if (buf[q] > 0.0) s_last = base + q;
                        off = next;
                    }
                }
            }
        }
        if (pass == 0) thr = u[t] * total;
    }
    if (tid == 0) {
        // the total is 0 (or, with a NaN or an infinite total, no run has a positive total): the uniform pick
        const int64_t run = s_run >= 0 ? s_run : s_last;
        s_walk = run;
        if (total == 0.0 || run < 0) {
            const int64_t p = (int64_t)floor(u[t] * (double)n);
            chosen[t] = p < 0 ? 0 : p >= n ? n - 1 : p;
            s_walk = -1;
        }
    }
    __syncthreads();
    const int64_t run = s_walk;
    if (run < 0) return;          // (the whole workgroup)
    const int64_t m0 = run * RUN;
    const int cnt = (int)min((int64_t)RUN, n - m0);
    vals[tid] = tid < cnt ? mind[m0 + tid] : 0.0f;
    __syncthreads();
    if (tid != 0) return;
    int64_t pick = -1;
    if (s_run >= 0) {
        double pre = 0.0;
        for (int q = 0; q < cnt; ++q) {
            pre += potential_of(vals[q]);
            if (s_off + pre > thr) {
                pick = m0 + q;
                break;
            }
        }
    }
    if (pick < 0)          // nobody qualifies: the last row with a positive potential
        for (int q = cnt - 1; q >= 0; --q)
            if (potential_of(vals[q]) > 0.0) {
                pick = m0 + q;
                break;
            }
    chosen[t] = pick < 0 ? m0 : pick;
}

// Workgroup (x, y): centroid x becomes the row chosen[x]
__global__ __launch_bounds__(BLOCK) void kmeans_gather_kernel(const float* __restrict__ X, const float* __restrict__ nx, int D,
                                                              const int64_t* __restrict__ chosen, float* __restrict__ Cd, float* __restrict__ ncn) {
    const int c = blockIdx.x, f = blockIdx.y * BLOCK + threadIdx.x;
    const int64_t row = chosen[c];
    if (f < D) Cd[(int64_t)c * D + f] = X[row * D + f];
    if (f == 0) ncn[c] = nx[row];
}

// ---- label statistics ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void kmeans_contingency_kernel(const int32_t* __restrict__ labels, const int32_t* __restrict__ classes, int64_t n,
                                                                   int C, unsigned long long* __restrict__ table) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const int lab = labels[i];
    if (lab >= 0) atomicAdd(&table[(int64_t)lab * C + classes[i]], 1ull);
}

// A workgroup per file: the labels of the rows [files[2 f], files[2 f + 1]) counted into hist[f][label] (zeroed before)
__global__ __launch_bounds__(BLOCK) void kmeans_file_hist_kernel(const int32_t* __restrict__ labels, const int64_t* __restrict__ files, int K,
                                                                 int32_t* __restrict__ hist) {
    const int64_t f = blockIdx.x, r0 = files[2 * f], r1 = files[2 * f + 1];
    for (int64_t i = r0 + threadIdx.x; i < r1; i += BLOCK) {
        const int lab = labels[i];
        if (lab >= 0) atomicAdd(&hist[f * K + lab], 1);
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
bool finished(hipStream_t s) { return hipStreamSynchronize(s) == hipSuccess && hipGetLastError() == hipSuccess; }

unsigned blocks_of(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

template <class T>
int grow(l3_kmeans* h, T** buf, size_t* cap, size_t count, const char* fn) {
    if (*buf && count <= *cap) return L3_OK;
    // whatever read the old buffer has finished: every call on the handle waits for its stream before it returns
    h->bufs.grow(buf, cap, count);
    if (*buf) return L3_OK;
    return fail(L3_ENOMEM, std::string(fn) + ": device allocation of " + std::to_string(DeviceBufs::bytes_of<T>(count)) + " bytes failed");
}

int enter(l3_kmeans* h, const char* fn) {
    if (!h) return fail(L3_EINVAL, std::string(fn) + ": NULL handle");
    if (hipSetDevice(h->device) != hipSuccess) return fail(L3_EHIP, no_gpu_message(fn, h->device));
    return L3_OK;
}

int need_rows(const l3_kmeans* h, const char* fn) {
    if (h->n < 1) return fail(L3_EINVAL, std::string(fn) + ": the rows come first (l3_kmeans_set_rows)");
    return L3_OK;
}

int need_centroids(const l3_kmeans* h, const char* fn) {
    if (!h->has_centroids)
        return fail(L3_EINVAL, std::string(fn) + ": the centroids come first (l3_kmeans_set_centroids, l3_kmeans_seed_rows or l3_kmeans_seed_pp)");
    return L3_OK;
}

int check_rows(const l3_kmeans* h, const float* rows, int64_t n, bool fitted, const char* fn) {
    if (!rows) return fail(L3_EINVAL, std::string(fn) + ": rows is NULL");
    if (n < 1 || n > MAX_ROWS) return fail(L3_EINVAL, std::string(fn) + ": need 1 <= n <= 2^31 - 1 rows, not " + std::to_string(n));
    if (fitted && n < h->K)
        return fail(L3_EINVAL, std::string(fn) + ": " + std::to_string(h->K) + " clusters need at least as many rows, not " + std::to_string(n));
    return L3_OK;
}

int check_feat(const l3_kmeans* h, const l3_feat* f, int64_t lo, int64_t hi, bool fitted, const char* fn) {
    if (!f) return fail(L3_EINVAL, std::string(fn) + ": the feature matrix is NULL");
    if (f->device != h->device)
        return fail(L3_EINVAL, std::string(fn) + ": the features are on device " + std::to_string(f->device) + ", the handle on device " + std::to_string(h->device));
    if (f->D != h->D)
        return fail(L3_EINVAL, std::string(fn) + ": the features have " + std::to_string(f->D) + " columns, the handle's rows " + std::to_string(h->D));
    if (lo < 0 || hi > f->n || lo >= hi)
        return fail(L3_EINVAL, std::string(fn) + ": rows [" + std::to_string(lo) + ", " + std::to_string(hi) + ") are empty or outside the " +
                                   std::to_string(f->n) + " rows of the features");
    if (hi - lo > MAX_ROWS) return fail(L3_EINVAL, std::string(fn) + ": at most 2^31 - 1 rows");
    if (fitted && hi - lo < h->K)
        return fail(L3_EINVAL, std::string(fn) + ": " + std::to_string(h->K) + " clusters need at least as many rows, not " + std::to_string(hi - lo));
    return L3_OK;
}

void launch_norm(const float* x, int64_t n, int D, float* out, hipStream_t s) {
    hipLaunchKernelGGL(kmeans_norm_kernel, dim3(blocks_of(n, BLOCK)), dim3(BLOCK), 0, s, x, n, D, out);
}

// the fitted rows: x_host or x_dev (n, D) -> the handle's copy, nn(x), no labels yet
int set_rows(l3_kmeans* h, const float* x_host, const float* x_dev, int64_t n, const char* fn) {
    h->n = 0, h->sorted = false;
    if (int rc = grow(h, &h->X, &h->cap_X, (size_t)n * h->D, fn)) return rc;
    if (int rc = grow(h, &h->nnX, &h->cap_nnX, (size_t)n, fn)) return rc;
    if (int rc = grow(h, &h->mind, &h->cap_mind, (size_t)n, fn)) return rc;
    if (int rc = grow(h, &h->labels, &h->cap_labels, (size_t)n, fn)) return rc;
    if (int rc = grow(h, &h->ids, &h->cap_ids, (size_t)n, fn)) return rc;
    if (int rc = grow(h, &h->runs, &h->cap_runs, (size_t)((n + RUN - 1) / RUN), fn)) return rc;
    const hipMemcpyKind kind = x_host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
    if (hipMemcpyAsync(h->X, x_host ? x_host : x_dev, (size_t)n * h->D * sizeof(float), kind, h->s) != hipSuccess ||
        hipMemsetAsync(h->labels, 0xFE, (size_t)n * 4, h->s) != hipSuccess)
        return fail(L3_EHIP, std::string(fn) + ": copy to the handle's rows failed");
    launch_norm(h->X, n, h->D, h->nnX, h->s);
    if (!finished(h->s)) return fail(L3_EHIP, std::string(fn) + ": the norms failed on the device");
    h->n = n;
    return L3_OK;
}

// rows per block of the sort: the per-block histograms stay about as large as the rows
int sort_block_rows(int NK) { return RUN * ((std::max(1024, NK) + RUN - 1) / RUN); }

// the stable sort of the fitted rows by key (mode 0: label, mode 1: has a label) -> ids, count, start, runoff, and the scalars
int launch_sort(l3_kmeans* h, int mode, const char* fn) {
    const int K = h->K, NK = mode == 0 ? K + 1 : 2, KR = mode == 0 ? K : 1, rb = sort_block_rows(NK);
    const int64_t nb = (h->n + rb - 1) / rb;
    if (int rc = grow(h, &h->hist, &h->cap_hist, (size_t)nb * NK, fn)) return rc;
    if (hipMemsetAsync(h->hist, 0, (size_t)nb * NK * 4, h->s) != hipSuccess) return fail(L3_EHIP, std::string(fn) + ": hipMemsetAsync failed");
    hipLaunchKernelGGL(kmeans_hist_kernel, dim3((unsigned)nb), dim3(BLOCK), 0, h->s, h->labels, h->n, rb, mode, K, NK, h->hist);
    hipLaunchKernelGGL(kmeans_colscan_kernel, dim3(blocks_of(NK, BLOCK)), dim3(BLOCK), 0, h->s, h->hist, nb, NK, h->count);
    hipLaunchKernelGGL(kmeans_keyscan_kernel, dim3(1), dim3(BLOCK), 0, h->s, h->count, NK, KR, mode, h->start, h->runoff, h->stats);
    hipLaunchKernelGGL(kmeans_scatter_kernel, dim3((unsigned)nb), dim3(BLOCK), 0, h->s, h->labels, h->n, rb, mode, K, NK, h->hist, h->start, h->ids);
    h->sorted = mode == 0;
    return L3_OK;
}

void launch_assign(l3_kmeans* h, const float* rows, const float* nn, int64_t n, int32_t* labels, float* mind, bool count_changed) {
    hipLaunchKernelGGL(kmeans_assign_kernel, dim3(blocks_of(n, TQ)), dim3(BLOCK), 0, h->s, rows, h->C, nn, h->nnC, h->D, (int)n, h->K, labels, mind,
                       count_changed ? &h->stats->changed : nullptr);
}

int launch_inertia(l3_kmeans* h, const char* fn) {
    if (int rc = launch_sort(h, 1, fn)) return rc;
    const int64_t R = (h->n + RUN - 1) / RUN;
    hipLaunchKernelGGL(kmeans_inertia_run_kernel, dim3(blocks_of(R, BLOCK)), dim3(BLOCK), 0, h->s, h->mind, h->ids, h->start, h->runs);
    hipLaunchKernelGGL(kmeans_inertia_final_kernel, dim3(1), dim3(BLOCK), 0, h->s, h->runs, h->start, h->stats);
    return L3_OK;
}

// One assignment of the fitted rows with everything an iteration reads from it: labels, distances, changed, the inertia, and the
// sort by label with its counts (which the update and `empty` need).  Nothing waits and nothing is downloaded.
int launch_assign_all(l3_kmeans* h, const char* fn) {
    if (hipMemsetAsync(&h->stats->changed, 0, sizeof(unsigned long long), h->s) != hipSuccess) return fail(L3_EHIP, std::string(fn) + ": hipMemsetAsync failed");
    launch_assign(h, h->X, h->nnX, h->n, h->labels, h->mind, true);
    if (int rc = launch_inertia(h, fn)) return rc;
    return launch_sort(h, 0, fn);
}

int64_t max_runs(const l3_kmeans* h) { return (h->n + (int64_t)(RUN - 1) * h->K) / RUN + 1; }

// the centroids of the current labels (launch_assign_all came before): the run sums, the finish, nn(c)
int launch_update(l3_kmeans* h, const char* fn) {
    const int64_t R = max_runs(h);
    if (int rc = grow(h, &h->part, &h->cap_part, (size_t)R * h->D, fn)) return rc;
    const unsigned fy = blocks_of(h->D, BLOCK);
    hipLaunchKernelGGL(kmeans_runsum_kernel, dim3((unsigned)R, fy), dim3(BLOCK), 0, h->s, h->X, h->D, h->K, h->ids, h->start, h->runoff, h->part);
    hipLaunchKernelGGL(kmeans_finish_kernel, dim3((unsigned)h->K, fy), dim3(BLOCK), 0, h->s, h->C, h->D, h->count, h->runoff, h->part);
    launch_norm(h->C, h->K, h->D, h->nnC, h->s);
    return L3_OK;
}

int read_stats(l3_kmeans* h, l3_kmeans_stats* got, const char* fn) {
    if (hipMemcpyAsync(got, h->stats, sizeof(*got), hipMemcpyDeviceToHost, h->s) != hipSuccess || !finished(h->s))
        return fail(L3_EHIP, std::string(fn) + ": the kernels or the copy from the device failed");
    return L3_OK;
}

// the centroids become the rows chosen[0 .. K) (on the device)
void launch_gather(l3_kmeans* h) {
    hipLaunchKernelGGL(kmeans_gather_kernel, dim3((unsigned)h->K, blocks_of(h->D, BLOCK)), dim3(BLOCK), 0, h->s, h->X, h->nnX, h->D, h->chosen, h->C, h->nnC);
}

// k-means++ with the draws h->u and the first centre chosen[0] already on the device
void launch_pp(l3_kmeans* h) {
    const int64_t R = (h->n + RUN - 1) / RUN;
    for (int t = 1; t < h->K; ++t) {
        hipLaunchKernelGGL(kmeans_pp_dist_kernel, dim3((unsigned)R), dim3(BLOCK), 0, h->s, h->X, h->nnX, h->D, h->n, h->chosen, t - 1, h->mind);
        hipLaunchKernelGGL(kmeans_pp_run_kernel, dim3(blocks_of(R, BLOCK)), dim3(BLOCK), 0, h->s, h->mind, h->n, h->runs);
        hipLaunchKernelGGL(kmeans_pp_pick_kernel, dim3(1), dim3(BLOCK), 0, h->s, h->mind, h->n, h->runs, h->u, t, h->chosen);
    }
    launch_gather(h);
}

int first_centre(const double* u, int64_t n) {
    const int64_t p = (int64_t)std::floor(u[0] * (double)n);
    return (int)std::max<int64_t>(0, std::min<int64_t>(n - 1, p));
}

int upload_draws(l3_kmeans* h, const double* u, const char* fn) {
    const int64_t first = first_centre(u, h->n);
    if (hipMemcpyAsync(h->u, u, (size_t)h->K * 8, hipMemcpyHostToDevice, h->s) != hipSuccess ||
        hipMemcpyAsync(h->chosen, &first, 8, hipMemcpyHostToDevice, h->s) != hipSuccess || hipStreamSynchronize(h->s) != hipSuccess)
        return fail(L3_EHIP, std::string(fn) + ": copy to the device failed");
    return L3_OK;
}

int other_rows(l3_kmeans* h, const float* x_host, const float* x_dev, int64_t n, int32_t* labels, float* dist, const char* fn) {
    h->nP = 0;
    if (int rc = grow(h, &h->P, &h->cap_P, (size_t)n * h->D, fn)) return rc;
    if (int rc = grow(h, &h->nnP, &h->cap_nnP, (size_t)n, fn)) return rc;
    if (int rc = grow(h, &h->pd, &h->cap_pd, (size_t)n, fn)) return rc;
    if (int rc = grow(h, &h->pl, &h->cap_pl, (size_t)n, fn)) return rc;
    const hipMemcpyKind kind = x_host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
    if (hipMemcpyAsync(h->P, x_host ? x_host : x_dev, (size_t)n * h->D * sizeof(float), kind, h->s) != hipSuccess)
        return fail(L3_EHIP, std::string(fn) + ": copy to the handle's rows failed");
    launch_norm(h->P, n, h->D, h->nnP, h->s);
    launch_assign(h, h->P, h->nnP, n, h->pl, h->pd, false);
    bool ok = true;
    if (labels) ok = ok && hipMemcpyAsync(labels, h->pl, (size_t)n * 4, hipMemcpyDeviceToHost, h->s) == hipSuccess;
    if (dist) ok = ok && hipMemcpyAsync(dist, h->pd, (size_t)n * 4, hipMemcpyDeviceToHost, h->s) == hipSuccess;
    if (!ok || !finished(h->s)) return fail(L3_EHIP, std::string(fn) + ": the kernels or the copy from the device failed");
    h->nP = n;
    return L3_OK;
}

int download_labels(l3_kmeans* h, int32_t* labels, float* dist, const char* fn) {
    bool ok = true;
    if (labels) ok = ok && hipMemcpyAsync(labels, h->labels, (size_t)h->n * 4, hipMemcpyDeviceToHost, h->s) == hipSuccess;
    if (dist) ok = ok && hipMemcpyAsync(dist, h->mind, (size_t)h->n * 4, hipMemcpyDeviceToHost, h->s) == hipSuccess;
    if (!ok) return fail(L3_EHIP, std::string(fn) + ": copy from the device failed");
    return L3_OK;
}

}  // namespace
}  // namespace l3

using namespace l3;

extern "C" {

int l3_kmeans_create(int device, int D, int K, int metric, l3_kmeans** out) {
    const char* fn = "l3_kmeans_create";
    if (!out) return fail(L3_EINVAL, std::string(fn) + ": out is NULL");
    *out = nullptr;
    if (D < 1 || D > (1 << 20)) return fail(L3_EINVAL, std::string(fn) + ": need 1 <= D <= 2^20 features, not " + std::to_string(D));
    if (K < 1 || K > K_MAX) return fail(L3_EINVAL, std::string(fn) + ": need 1 <= K <= " + std::to_string(K_MAX) + " clusters, not " + std::to_string(K));
    if (metric == L3_KNN_COSINE)
        return fail(L3_EINVAL, std::string(fn) + ": k-means is defined for the squared Euclidean distance only: the mean of a cluster minimises it and "
                                   "not the cosine distance (normalise the rows and use L3_KNN_SQEUCLIDEAN)");
    if (metric != L3_KNN_SQEUCLIDEAN) return fail(L3_EINVAL, std::string(fn) + ": metric must be L3_KNN_SQEUCLIDEAN, not " + std::to_string(metric));
    if (!device_ok(device)) return fail(L3_EHIP, no_gpu_message(fn, device));
    l3_kmeans* h = new l3_kmeans();
    h->device = device, h->D = D, h->K = K;
    if (hipStreamCreateWithFlags(&h->s, hipStreamNonBlocking) != hipSuccess) {
        h->s = nullptr;
        l3_kmeans_destroy(h);
        return fail(L3_EHIP, std::string(fn) + ": hipStreamCreate failed");
    }
    h->C = h->bufs.alloc<float>((size_t)K * D);
    h->nnC = h->bufs.alloc<float>((size_t)K);
    h->count = h->bufs.alloc<int32_t>((size_t)K + 1);
    h->start = h->bufs.alloc<int32_t>((size_t)K + 2);
    h->runoff = h->bufs.alloc<int32_t>((size_t)K + 2);
    h->chosen = h->bufs.alloc<int64_t>((size_t)K);
    h->u = h->bufs.alloc<double>((size_t)K);
    h->stats = h->bufs.alloc<l3_kmeans_stats>(1);
    if (!h->bufs.ok() || hipMemset(h->stats, 0, sizeof(l3_kmeans_stats)) != hipSuccess) {
        l3_kmeans_destroy(h);
        return fail(L3_ENOMEM, std::string(fn) + ": device allocation of the centroids failed");
    }
    *out = h;
    return L3_OK;
}

void l3_kmeans_destroy(l3_kmeans* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->s) (void)hipStreamSynchronize(h->s);
    if (h->s) (void)hipStreamDestroy(h->s);
    delete h;
}

int l3_kmeans_set_rows(l3_kmeans* h, const float* rows, int64_t n) {
    const char* fn = "l3_kmeans_set_rows";
    if (int rc = enter(h, fn)) return rc;
    if (int rc = check_rows(h, rows, n, true, fn)) return rc;
    return set_rows(h, rows, nullptr, n, fn);
}

int l3_kmeans_set_rows_dev(l3_kmeans* h, const l3_feat* f, int64_t lo, int64_t hi) {
    const char* fn = "l3_kmeans_set_rows_dev";
    if (int rc = enter(h, fn)) return rc;
    if (int rc = check_feat(h, f, lo, hi, true, fn)) return rc;
    // (every l3_feat call has finished on its handle's stream when it returns: the rows hold their final values)
    return set_rows(h, nullptr, f->x + lo * f->D, hi - lo, fn);
}

int l3_kmeans_set_centroids(l3_kmeans* h, const float* centroids) {
    const char* fn = "l3_kmeans_set_centroids";
    if (int rc = enter(h, fn)) return rc;
    if (!centroids) return fail(L3_EINVAL, std::string(fn) + ": centroids is NULL");
    h->has_centroids = false, h->sorted = false;
    if (hipMemcpyAsync(h->C, centroids, (size_t)h->K * h->D * sizeof(float), hipMemcpyHostToDevice, h->s) != hipSuccess)
        return fail(L3_EHIP, std::string(fn) + ": copy to the device failed");
    launch_norm(h->C, h->K, h->D, h->nnC, h->s);
    if (!finished(h->s)) return fail(L3_EHIP, std::string(fn) + ": the norms failed on the device");
    h->has_centroids = true;
    return L3_OK;
}

int l3_kmeans_seed_rows(l3_kmeans* h, const int64_t* rows) {
    const char* fn = "l3_kmeans_seed_rows";
    if (int rc = enter(h, fn)) return rc;
    if (!rows) return fail(L3_EINVAL, std::string(fn) + ": rows is NULL");
    if (int rc = need_rows(h, fn)) return rc;
    for (int c = 0; c < h->K; ++c)
        if (rows[c] < 0 || rows[c] >= h->n)
            return fail(L3_EINVAL, std::string(fn) + ": rows[" + std::to_string(c) + "] = " + std::to_string(rows[c]) + " outside the " + std::to_string(h->n) + " rows");
    h->has_centroids = false, h->sorted = false;
    if (hipMemcpyAsync(h->chosen, rows, (size_t)h->K * 8, hipMemcpyHostToDevice, h->s) != hipSuccess)
        return fail(L3_EHIP, std::string(fn) + ": copy to the device failed");
    launch_gather(h);
    if (!finished(h->s)) return fail(L3_EHIP, std::string(fn) + ": the kernel failed on the device");
    h->has_centroids = true;
    return L3_OK;
}

int l3_kmeans_seed_pp(l3_kmeans* h, const double* u, int64_t* chosen_out) {
    const char* fn = "l3_kmeans_seed_pp";
    if (int rc = enter(h, fn)) return rc;
    if (!u) return fail(L3_EINVAL, std::string(fn) + ": u is NULL");
    if (int rc = need_rows(h, fn)) return rc;
    for (int c = 0; c < h->K; ++c)
        if (!(u[c] >= 0.0 && u[c] < 1.0)) return fail(L3_EINVAL, std::string(fn) + ": u[" + std::to_string(c) + "] is outside [0, 1)");
    h->has_centroids = false, h->sorted = false;
    if (int rc = upload_draws(h, u, fn)) return rc;
    launch_pp(h);
    // the seeding used the rows' distance buffer: the labels no longer go with it
    if (hipMemsetAsync(h->labels, 0xFE, (size_t)h->n * 4, h->s) != hipSuccess) return fail(L3_EHIP, std::string(fn) + ": hipMemsetAsync failed");
    if (chosen_out && hipMemcpyAsync(chosen_out, h->chosen, (size_t)h->K * 8, hipMemcpyDeviceToHost, h->s) != hipSuccess)
        return fail(L3_EHIP, std::string(fn) + ": copy from the device failed");
    if (!finished(h->s)) return fail(L3_EHIP, std::string(fn) + ": the kernels failed on the device");
    h->has_centroids = true;
    return L3_OK;
}

int l3_kmeans_assign(l3_kmeans* h, int32_t* labels, float* dist, double* inertia, int64_t* changed) {
    const char* fn = "l3_kmeans_assign";
    if (int rc = enter(h, fn)) return rc;
    if (int rc = need_rows(h, fn)) return rc;
    if (int rc = need_centroids(h, fn)) return rc;
    if (int rc = launch_assign_all(h, fn)) return rc;
    if (int rc = download_labels(h, labels, dist, fn)) return rc;
    l3_kmeans_stats got;
    if (int rc = read_stats(h, &got, fn)) return rc;
    if (inertia) *inertia = got.inertia;
    if (changed) *changed = (int64_t)got.changed;
    return L3_OK;
}

int l3_kmeans_get_labels(l3_kmeans* h, int32_t* labels, float* dist, double* inertia) {
    const char* fn = "l3_kmeans_get_labels";
    if (int rc = enter(h, fn)) return rc;
    if (int rc = need_rows(h, fn)) return rc;
    if (!h->sorted) return fail(L3_EINVAL, std::string(fn) + ": an assignment comes first (l3_kmeans_assign or l3_kmeans_fit)");
    if (int rc = download_labels(h, labels, dist, fn)) return rc;
    l3_kmeans_stats got;
    if (int rc = read_stats(h, &got, fn)) return rc;
    if (inertia) *inertia = got.inertia;
    return L3_OK;
}

int l3_kmeans_update(l3_kmeans* h, int64_t* counts_out) {
    const char* fn = "l3_kmeans_update";
    if (int rc = enter(h, fn)) return rc;
    if (int rc = need_rows(h, fn)) return rc;
    if (!h->sorted) return fail(L3_EINVAL, std::string(fn) + ": an assignment comes first (l3_kmeans_assign)");
    if (int rc = launch_update(h, fn)) return rc;
    std::vector<int32_t> counts(counts_out ? h->K : 0);
    if (counts_out && hipMemcpyAsync(counts.data(), h->count, (size_t)h->K * 4, hipMemcpyDeviceToHost, h->s) != hipSuccess)
        return fail(L3_EHIP, std::string(fn) + ": copy from the device failed");
    if (!finished(h->s)) return fail(L3_EHIP, std::string(fn) + ": the kernels failed on the device");
    for (size_t c = 0; c < counts.size(); ++c) counts_out[c] = counts[c];
    return L3_OK;
}

int l3_kmeans_fit(l3_kmeans* h, int max_iter, double* history_out, int* n_iter_out) {
    const char* fn = "l3_kmeans_fit";
    if (int rc = enter(h, fn)) return rc;
    if (max_iter < 1) return fail(L3_EINVAL, std::string(fn) + ": need max_iter >= 1, not " + std::to_string(max_iter));
    if (int rc = need_rows(h, fn)) return rc;
    if (int rc = need_centroids(h, fn)) return rc;
    if (hipMemsetAsync(h->labels, 0xFE, (size_t)h->n * 4, h->s) != hipSuccess) return fail(L3_EHIP, std::string(fn) + ": hipMemsetAsync failed");
    int it = 0;
    bool settled = false;
    for (; it < max_iter && !settled; ++it) {
        if (int rc = launch_assign_all(h, fn)) return rc;
        l3_kmeans_stats got;
        if (int rc = read_stats(h, &got, fn)) return rc;          // the iteration's only read-back
        if (history_out) history_out[3 * it] = got.inertia, history_out[3 * it + 1] = (double)got.changed, history_out[3 * it + 2] = (double)got.empty;
        settled = got.changed == 0;
        if (!settled)
            if (int rc = launch_update(h, fn)) return rc;
    }
    if (!settled)          // max_iter is used up: the labels and the inertia of the centroids that are returned
        if (int rc = launch_assign_all(h, fn)) return rc;
    if (!finished(h->s)) return fail(L3_EHIP, std::string(fn) + ": the kernels failed on the device");
    if (n_iter_out) *n_iter_out = it;
    return L3_OK;
}

int l3_kmeans_get_centroids(l3_kmeans* h, float* out) {
    const char* fn = "l3_kmeans_get_centroids";
    if (int rc = enter(h, fn)) return rc;
    if (!out) return fail(L3_EINVAL, std::string(fn) + ": out is NULL");
    if (int rc = need_centroids(h, fn)) return rc;
    if (hipMemcpyAsync(out, h->C, (size_t)h->K * h->D * sizeof(float), hipMemcpyDeviceToHost, h->s) != hipSuccess || !finished(h->s))
        return fail(L3_EHIP, std::string(fn) + ": copy from the device failed");
    return L3_OK;
}

int l3_kmeans_predict(l3_kmeans* h, const float* rows, int64_t n, int32_t* labels, float* dist) {
    const char* fn = "l3_kmeans_predict";
    if (int rc = enter(h, fn)) return rc;
    if (int rc = check_rows(h, rows, n, false, fn)) return rc;
    if (int rc = need_centroids(h, fn)) return rc;
    return other_rows(h, rows, nullptr, n, labels, dist, fn);
}

int l3_kmeans_predict_dev(l3_kmeans* h, const l3_feat* f, int64_t lo, int64_t hi, int32_t* labels, float* dist) {
    const char* fn = "l3_kmeans_predict_dev";
    if (int rc = enter(h, fn)) return rc;
    if (int rc = check_feat(h, f, lo, hi, false, fn)) return rc;
    if (int rc = need_centroids(h, fn)) return rc;
    return other_rows(h, nullptr, f->x + lo * f->D, hi - lo, labels, dist, fn);
}

// which 0: the fitted rows' labels (an assignment came before); 1: the labels of the last l3_kmeans_predict
static int labels_of(l3_kmeans* h, int which, const int32_t** labels, int64_t* n, const char* fn) {
    if (which != 0 && which != 1) return fail(L3_EINVAL, std::string(fn) + ": which must be 0 (the fitted rows) or 1 (the last l3_kmeans_predict)");
    if (which == 0 && !(h->n > 0 && h->sorted)) return fail(L3_EINVAL, std::string(fn) + ": an assignment of the fitted rows comes first");
    if (which == 1 && h->nP < 1) return fail(L3_EINVAL, std::string(fn) + ": l3_kmeans_predict comes first");
    *labels = which == 0 ? h->labels : h->pl, *n = which == 0 ? h->n : h->nP;
    return L3_OK;
}

int l3_kmeans_contingency(l3_kmeans* h, int which, const int32_t* classes, int n_classes, int64_t* table) {
    const char* fn = "l3_kmeans_contingency";
    if (int rc = enter(h, fn)) return rc;
    if (!classes || !table) return fail(L3_EINVAL, std::string(fn) + ": classes and table must not be NULL");
    if (n_classes < 1 || n_classes > C_MAX)
        return fail(L3_EINVAL, std::string(fn) + ": need 1 <= n_classes <= " + std::to_string(C_MAX) + ", not " + std::to_string(n_classes));
    const int32_t* labels = nullptr;
    int64_t n = 0;
    if (int rc = labels_of(h, which, &labels, &n, fn)) return rc;
    for (int64_t i = 0; i < n; ++i)
        if (classes[i] < 0 || classes[i] >= n_classes)
            return fail(L3_EINVAL, std::string(fn) + ": classes[" + std::to_string(i) + "] = " + std::to_string(classes[i]) + " outside [0, " + std::to_string(n_classes) + ")");
    const size_t cells = (size_t)h->K * n_classes;
    if (int rc = grow(h, &h->classes, &h->cap_classes, (size_t)n, fn)) return rc;
    if (int rc = grow(h, &h->table, &h->cap_table, cells, fn)) return rc;
    if (hipMemcpyAsync(h->classes, classes, (size_t)n * 4, hipMemcpyHostToDevice, h->s) != hipSuccess ||
        hipMemsetAsync(h->table, 0, cells * 8, h->s) != hipSuccess)
        return fail(L3_EHIP, std::string(fn) + ": copy to the device failed");
    hipLaunchKernelGGL(kmeans_contingency_kernel, dim3(blocks_of(n, BLOCK)), dim3(BLOCK), 0, h->s, labels, h->classes, n, n_classes, h->table);
    if (hipMemcpyAsync(table, h->table, cells * 8, hipMemcpyDeviceToHost, h->s) != hipSuccess || !finished(h->s))
        return fail(L3_EHIP, std::string(fn) + ": the kernel or the copy from the device failed");
    return L3_OK;
}

int l3_kmeans_file_hist(l3_kmeans* h, int which, const int64_t* file_idxs, int64_t n_files, int32_t* hist) {
    const char* fn = "l3_kmeans_file_hist";
    if (int rc = enter(h, fn)) return rc;
    if (!file_idxs || !hist) return fail(L3_EINVAL, std::string(fn) + ": file_idxs and hist must not be NULL");
    if (n_files < 1 || n_files > INT32_MAX) return fail(L3_EINVAL, std::string(fn) + ": need 1 <= n_files <= 2^31 - 1");
    const int32_t* labels = nullptr;
    int64_t n = 0;
    if (int rc = labels_of(h, which, &labels, &n, fn)) return rc;
    for (int64_t f = 0; f < n_files; ++f)
        if (file_idxs[2 * f] < 0 || file_idxs[2 * f] >= file_idxs[2 * f + 1] || file_idxs[2 * f + 1] > n)
            return fail(L3_EINVAL, std::string(fn) + ": file " + std::to_string(f) + " = [" + std::to_string(file_idxs[2 * f]) + ", " + std::to_string(file_idxs[2 * f + 1]) +
                                       ") is empty or outside the " + std::to_string(n) + " rows");
    const size_t cells = (size_t)n_files * h->K;
    if (int rc = grow(h, &h->files, &h->cap_files, (size_t)n_files * 2, fn)) return rc;
    if (int rc = grow(h, &h->fh, &h->cap_fh, cells, fn)) return rc;
    if (hipMemcpyAsync(h->files, file_idxs, (size_t)n_files * 16, hipMemcpyHostToDevice, h->s) != hipSuccess ||
        hipMemsetAsync(h->fh, 0, cells * 4, h->s) != hipSuccess)
        return fail(L3_EHIP, std::string(fn) + ": copy to the device failed");
    hipLaunchKernelGGL(kmeans_file_hist_kernel, dim3((unsigned)n_files), dim3(BLOCK), 0, h->s, labels, h->files, h->K, h->fh);
    if (hipMemcpyAsync(hist, h->fh, cells * 4, hipMemcpyDeviceToHost, h->s) != hipSuccess || !finished(h->s))
        return fail(L3_EHIP, std::string(fn) + ": the kernel or the copy from the device failed");
    return L3_OK;
}

int l3_op_kmeans_step(int device, const float* rows, const float* centroids, int64_t n, int K, int D, int32_t* labels, float* dist, double* inertia,
                      int64_t* counts, float* new_centroids) {
    const char* fn = "l3_op_kmeans_step";
    if (!rows || !centroids) return fail(L3_EINVAL, std::string(fn) + ": rows and centroids must not be NULL");
    if (n < 1 || n > MAX_ROWS || K > n)
        return fail(L3_EINVAL, std::string(fn) + ": need 1 <= K <= n <= 2^31 - 1, not K = " + std::to_string(K) + ", n = " + std::to_string(n));
    l3_kmeans* h = nullptr;
    int rc = l3_kmeans_create(device, D, K, L3_KNN_SQEUCLIDEAN, &h);
    if (rc == L3_OK) rc = l3_kmeans_set_rows(h, rows, n);
    if (rc == L3_OK) rc = l3_kmeans_set_centroids(h, centroids);
    if (rc == L3_OK) rc = l3_kmeans_assign(h, labels, dist, inertia, nullptr);
    if (rc == L3_OK) rc = l3_kmeans_update(h, counts);
    if (rc == L3_OK && new_centroids) rc = l3_kmeans_get_centroids(h, new_centroids);
    l3_kmeans_destroy(h);
    return rc;
}

// Device time of `reps` rounds on the resident rows and centroids, in ms per round (hipEvents; one untimed round first).  what 0: the
// assignment kernel alone; 1: the update (run sums, finish, norms) of the current labels; 2: one whole iteration (assignment, inertia,
// sort, update: the centroids move on); 3: a k-means++ seeding of all K centres with every draw 0.5 (the centroids are replaced);
// 4: the sort by label alone; 5: the inertia alone.  For profiles/ records; no test asserts a time.
int l3_kmeans_time(l3_kmeans* h, int what, int reps, double* ms) {
    const char* fn = "l3_kmeans_time";
    if (int rc = enter(h, fn)) return rc;
    if (!ms || reps < 1 || what < 0 || what > 5) return fail(L3_EINVAL, std::string(fn) + ": need ms, reps >= 1 and what in [0, 5]");
    if (int rc = need_rows(h, fn)) return rc;
    if (what != 3)
        if (int rc = need_centroids(h, fn)) return rc;
    int rc = L3_OK;
    if (what == 3) {
        std::vector<double> u((size_t)h->K, 0.5);
        rc = upload_draws(h, u.data(), fn);
        h->sorted = false;
    } else if (what != 0 && what != 2) {
        rc = launch_assign_all(h, fn);
    }
    if (rc != L3_OK) return rc;
    hipEvent_t a, b;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return fail(L3_EHIP, std::string(fn) + ": hipEventCreate failed");
    auto run = [&](int count) {
        for (int r = 0; r < count && rc == L3_OK; ++r) {
            if (what == 0) launch_assign(h, h->X, h->nnX, h->n, h->labels, h->mind, false);
            else if (what == 1) rc = launch_update(h, fn);
            else if (what == 2) {
                rc = launch_assign_all(h, fn);
                if (rc == L3_OK) rc = launch_update(h, fn);
            } else if (what == 3) launch_pp(h);
            else if (what == 4) rc = launch_sort(h, 0, fn);
            else rc = launch_inertia(h, fn);
        }
    };
    run(1);
    float t = 0.0f;
    if (rc == L3_OK && hipEventRecord(a, h->s) != hipSuccess) rc = fail(L3_EHIP, std::string(fn) + ": hipEventRecord failed");
    if (rc == L3_OK) run(reps);
    if (rc == L3_OK && (hipEventRecord(b, h->s) != hipSuccess || !finished(h->s) || hipEventElapsedTime(&t, a, b) != hipSuccess))
        rc = fail(L3_EHIP, std::string(fn) + ": the timed launches failed");
    if (rc != L3_OK) (void)hipStreamSynchronize(h->s);
    // the labels, their sort and the distances may no longer go together: the next assignment restores them
    h->sorted = false;
    if (what == 3 && rc == L3_OK) h->has_centroids = true;
    if (hipMemsetAsync(h->labels, 0xFE, (size_t)h->n * 4, h->s) != hipSuccess || hipStreamSynchronize(h->s) != hipSuccess)
        rc = rc != L3_OK ? rc : fail(L3_EHIP, std::string(fn) + ": hipMemsetAsync failed");
    *ms = (double)t / reps;
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    return rc;
}

}  // extern "C"
