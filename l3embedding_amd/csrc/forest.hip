// forest.hip -- the reference's random-forest sound classifier (classifier/train.py:169-227: sklearn.ensemble.RandomForestClassifier
// with sklearn 0.19's defaults) grown on the GPU as a level-wise histogram forest, and the l3_forest handle of the C ABI
// (DESIGN.md 8i).
//
// One fit:
//   forest_cuts      one workgroup per feature sorts the column of the row sample in LDS and takes at most 255 float32 cuts
//   forest_codes     code[f][i] = number of cuts of f below X[i][f], uint8, feature-major: X read row-major, transposed in LDS
// then, for all trees at once, one launch group per level of the trees:
//   search_wide      a workgroup per (node, drawn feature): the (bin x class) histogram of bootstrap-weighted counts in LDS by
//                    integer atomics, prefix sums over the bins, a thread per bin for the split's worth, one candidate per draw
//   pick_wide        a thread per node: the best of its K candidates, the earlier draw on ties
//   search_narrow    a wave per node of at most 64 distinct rows, a lane per row, looping over the node's K draws: the rows
//                    sorted by code across the wave, the sums of squared class counts carried by wave scans
//   partition_*      a split node's segment of its tree's row list, stably partitioned into the other list buffer
//   number           a workgroup per tree numbers the children level by level in parent order, left before right, and files
//                    them for the next level's two searches
// and one read-back of the new node counts.  A split's worth is double(sum L_k^2) / double(nL) + double(sum R_k^2) / double(nR)
// over integer counts, the sums of squares in int64: it does not depend on the order of any accumulation, both searches give the
// same trees, and tests/forest_ref.py restates the whole in NumPy with equal results.  Compiled with -ffp-contract=off.
// A node's K features come from Floyd's subset sampling driven by a counter-based mixer of (tree seed, node, draw).
//
// Scoring at nested forest sizes (l3_forest_score; the parameter search over n_estimators, classifier/train.py:623-630):
//   forest_score     a workgroup per 4 rows, a wave per row, a lane per tree of a 64-tree pass: the rows staged in LDS when they fit,
//                    the walk over packed 16-byte node records, the pass's count / total fractions computed across the wave into
//                    LDS, then a lane per class adds them in tree order and emits arg-max, hit and probabilities at every prefix
//   forest_file_*    a thread per (size, file, class) adds a file's rows in row order; a thread per (size, file) takes the arg-max
// The sums are those of forest_predict_kernel, operation for operation: the outputs are its bits.
//
// Out-of-bag scoring at nested forest sizes (l3_forest_oob; what oob_score=True adds to the fit, at every size of the
// grid):
//   forest_oob_mask  a lane per row over a slab of 64 trees' bootstrap multiplicities: one 64-bit word per (row, pass), bit j set iff
//                    tree j of the pass left the row out of its bag
//   forest_oob       forest_score's walk under the row's word: a lane whose bit is clear neither walks nor adds; the set lanes'
//                    fractions are added in tree order, and at every prefix the sums as they stand, the number of trees that left
//                    the row out, the arg-max and the hit are written.  Nothing is divided on the device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/l3hip.h"
#include "featprep.h"
#include "host_common.h"

namespace l3 {
namespace {

constexpr int NB = 256;                          // bins per feature (codes 0 .. 255)
constexpr int MAXCUTS = L3_FOREST_MAX_CUTS;
constexpr int NARROW = L3_FOREST_NARROW_ROWS;
constexpr uint64_t GOLD = 0x9E3779B97F4A7C15ull;

struct Cand {          // the best split of one (node, draw): bin -1 if there is none
    double proxy;
    int32_t bin, nleft, feat, pad;
};

struct Grow {          // what the level kernels share
    const uint8_t* codes;      // (D, n)
    const int32_t* ncuts;      // (D)
    const uint8_t* y;          // (n)
    const uint16_t* boot;      // (T, n)
    const int64_t* seeds;      // (T)
    int32_t *nstart, *nend, *nfeat, *nbin, *nleft, *nchild, *ncounts;      // per node, tree t's node i at t * cap + i
    int32_t *tree_fs, *tree_fe, *newcnt;                                    // per tree: the frontier [fs, fe), the nodes added
    int32_t* listcnt;          // [0] wide, [1] narrow: entries of the next level's lists
    int64_t n;
    int32_t cap, D, C, K, mss, msl, wide_min;
};

// ---- the mixer and the draws ------------------------------------------------------------------------------------------------
__host__ __device__ inline uint64_t fmix64(uint64_t z) {          // splitmix64's finaliser
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}
// rand(n) of draw i under the node's key a: ((h >> 32) n) >> 32
__device__ __forceinline__ uint32_t draw_rand(uint64_t a, int i, uint32_t n) {
    const uint64_t h = fmix64(a + (uint64_t)(i + 1) * GOLD);
    return (uint32_t)(((h >> 32) * (uint64_t)n) >> 32);
}

// Floyd's subset sampling by one whole wave: draw q ends up in register q >> 6 of lane q & 63 (K <= 256)
struct Picks {
    int32_t r[4];
};
__device__ __forceinline__ Picks floyd_draws(uint64_t seed, uint32_t node, int D, int K, int lane) {
    Picks p;
    p.r[0] = p.r[1] = p.r[2] = p.r[3] = -1;
    const uint64_t a = fmix64(seed * GOLD + (uint64_t)node);
    for (int i = 0; i < K; ++i) {
        const int j = D - K + i;
        const int32_t t = (int32_t)draw_rand(a, i, (uint32_t)(j + 1));
        const bool hit = p.r[0] == t || p.r[1] == t || p.r[2] == t || p.r[3] == t;      // unset slots hold -1
        const int32_t v = __any(hit) ? j : t;
        if (lane == (i & 63)) {
            const int s = i >> 6;
            if (s == 0) p.r[0] = v;
            else if (s == 1) p.r[1] = v;
            else if (s == 2) p.r[2] = v;
            else p.r[3] = v;
        }
    }
    return p;
}
__device__ __forceinline__ int32_t pick_of(const Picks& p, int d) {
    const int s = d >> 6;
    const int32_t v = s == 0 ? p.r[0] : s == 1 ? p.r[1] : s == 2 ? p.r[2] : p.r[3];
    return __shfl(v, d & 63);
}

// ---- wave and workgroup helpers ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int64_t shfl_up64(int64_t v, int off) {
    const int lo = __shfl_up((int)(uint32_t)(uint64_t)v, off), hi = __shfl_up((int)((uint64_t)v >> 32), off);
    return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}
__device__ __forceinline__ int64_t shfl_xor64(int64_t v, int m) {
    const int lo = __shfl_xor((int)(uint32_t)(uint64_t)v, m), hi = __shfl_xor((int)((uint64_t)v >> 32), m);
    return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}
__device__ __forceinline__ int64_t wave_scan64(int64_t v, int lane) {          // inclusive
    for (int off = 1; off < 64; off <<= 1) {
        const int64_t o = shfl_up64(v, off);
        if (lane >= off) v += o;
    }
    return v;
}
__device__ __forceinline__ int wave_scan32(int v, int lane) {
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(v, off);
        if (lane >= off) v += o;
    }
    return v;
}
__device__ __forceinline__ int64_t wave_sum64(int64_t v) {
    for (int m = 32; m > 0; m >>= 1) v += shfl_xor64(v, m);
    return v;
}
__device__ __forceinline__ double shfl_xor_f64(double v, int m) { return __longlong_as_double(shfl_xor64(__double_as_longlong(v), m)); }
// the largest worth over the wave, the lowest position among equals: every lane gets both
__device__ __forceinline__ void wave_argmax(double& proxy, int& pos) {
    for (int m = 32; m > 0; m >>= 1) {
        const double op = shfl_xor_f64(proxy, m);
        const int oq = __shfl_xor(pos, m);
        if (op > proxy || (op == proxy && oq < pos)) proxy = op, pos = oq;
    }
}
// rank of a set flag among the workgroup's (256 threads) set flags in thread order, and their number; ws: 4 ints of LDS
__device__ __forceinline__ int block_rank(bool flag, int* ws, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(flag);
    if (lane == 0) ws[wave] = __popcll(m);
    __syncthreads();
    int before = 0, all = 0;
    for (int w = 0; w < 4; ++w) {
        const int c = ws[w];
        if (w < wave) before += c;
        all += c;
    }
    __syncthreads();
    total = all;
    return before + __popcll(m & ((1ull << lane) - 1ull));
}

// ---- cuts and codes ---------------------------------------------------------------------------------------------------------------
// one workgroup per feature: s = the sorted column of the sample; a cut between s[p - 1] < s[p] at the candidate positions p
__global__ __launch_bounds__(256) void forest_cuts_kernel(const float* __restrict__ X, int64_t D, const int32_t* __restrict__ rows,
                                                           int S, int P2, float* __restrict__ cuts, int32_t* __restrict__ ncuts) {
    extern __shared__ float s[];
    __shared__ int ws[4];
    const int f = blockIdx.x, tid = threadIdx.x;
    for (int i = tid; i < P2; i += 256) s[i] = i < S ? X[(int64_t)(rows ? rows[i] : i) * D + f] : INFINITY;
    __syncthreads();
    for (int k = 2; k <= P2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P2; i += 256) {
                const int o = i ^ j;
                if (o > i) {
                    const float a = s[i], b = s[o];
                    const bool up = (i & k) == 0;
                    if ((a > b) == up) s[i] = b, s[o] = a;
                }
            }
            __syncthreads();
        }
    const int npos = S <= 256 ? S - 1 : 255;
    bool ok = false;
    float t = 0.f;
    if (tid < npos) {
        const int p = S <= 256 ? tid + 1 : (int)(((int64_t)(tid + 1) * S) / 256);
        const float a = s[p - 1], b = s[p];
        ok = a < b;
        t = (float)(((double)a + (double)b) / 2.0);
        if (t >= b) t = a;
    }
    int total;
    const int at = block_rank(ok, ws, total);
    if (ok) cuts[(int64_t)f * MAXCUTS + at] = t;
    if (tid == 0) ncuts[f] = total;
}

// a 64-row by 64-feature tile per workgroup: X read along its rows, the codes written along the feature-major rows of `codes`
__global__ __launch_bounds__(256) void forest_codes_kernel(const float* __restrict__ X, int64_t n, int D, const float* __restrict__ cuts,
                                                            const int32_t* __restrict__ ncuts, uint8_t* __restrict__ codes) {
    __shared__ uint8_t tile[64][68];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int64_t row0 = (int64_t)blockIdx.x * 64;
    const int f0 = blockIdx.y * 64;
    const int f = f0 + tx;
    if (f < D) {
        const float* c = cuts + (int64_t)f * MAXCUTS;
        const int nc = ncuts[f];
        for (int r = ty; r < 64; r += 4) {
            const int64_t row = row0 + r;
            if (row >= n) break;
            const float x = X[row * D + f];
            int lo = 0, hi = nc;          // the first cut that is not below x
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (c[mid] < x) lo = mid + 1;
                else hi = mid;
            }
            tile[tx][r] = (uint8_t)lo;
        }
    }
    __syncthreads();
    const int64_t row = row0 + tx;
    if (row < n)
        for (int ff = ty; ff < 64 && f0 + ff < D; ff += 4) codes[(int64_t)(f0 + ff) * n + row] = tile[ff][tx];
}

// ---- the level kernels ----------------------------------------------------------------------------------------------------------
__global__ void forest_init_roots_kernel(Grow p, const int32_t* __restrict__ n_tree, int T) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    const int64_t g = (int64_t)t * p.cap;
    p.nstart[g] = 0, p.nend[g] = n_tree[t], p.nfeat[g] = -1, p.nbin[g] = -1, p.nleft[g] = 0, p.nchild[g] = -1;
    p.tree_fs[t] = 0, p.tree_fe[t] = 1;
}

// a node may split at this level and by its size
__device__ __forceinline__ bool may_split(const Grow& p, int n, int search) { return search && n >= p.mss && n >= 2 * p.msl; }

__global__ __launch_bounds__(256) void forest_search_wide_kernel(Grow p, const int32_t* __restrict__ list, const int32_t* __restrict__ idx,
                                                                  Cand* __restrict__ cand, int search) {
    extern __shared__ int lds[];
    int* hist = lds;                    // (NB, C), then prefix sums over the bins
    int* cnt = lds + NB * p.C;          // (NB) distinct rows
    __shared__ int s_f;
    __shared__ double s_proxy[4];
    __shared__ int s_bin[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int item = blockIdx.x, d = blockIdx.y;
    const int g = list[item];
    const int t = g / p.cap, node = g - t * p.cap;
    const int start = p.nstart[g], end = p.nend[g], n = end - start, C = p.C;
    if (wave == 0) {
        const Picks pk = floyd_draws((uint64_t)p.seeds[t], (uint32_t)node, p.D, p.K, lane);
        const int f = pick_of(pk, d);
        if (lane == 0) s_f = f;
    }
    for (int i = tid; i < NB * C + NB; i += 256) lds[i] = 0;
    __syncthreads();
    const int f = s_f;
    const uint8_t* col = p.codes + (int64_t)f * p.n;
    const int32_t* rows = idx + (int64_t)t * p.n;
    const uint16_t* w = p.boot + (int64_t)t * p.n;
    for (int i = start + tid; i < end; i += 256) {
        const int r = rows[i];
        const int c = col[r];
        atomicAdd(&hist[c * C + p.y[r]], (int)w[r]);
        atomicAdd(&cnt[c], 1);
    }
    __syncthreads();
    if (tid <= C) {          // a thread per class, and one for the distinct rows: running sums over the bins
        int* a = tid < C ? hist + tid : cnt;
        const int stride = tid < C ? C : 1;
        int acc = 0;
        for (int b = 0; b < NB; ++b) {
            acc += a[b * stride];
            a[b * stride] = acc;
        }
    }
    __syncthreads();
    const int* tot = hist + (NB - 1) * C;
    if (d == 0 && tid < C) p.ncounts[(int64_t)g * C + tid] = tot[tid];
    if (!search) return;
    // a thread per bin: the worth of `code <= bin` against the rest
    const int nc = p.ncuts[f];
    double proxy = -1.0;
    int bin = tid;
    {
        int present = 0;
        int64_t sl2 = 0, sr2 = 0, nl = 0, nr = 0;
        const int* h = hist + tid * C;
        for (int k = 0; k < C; ++k) {
            const int64_t tk = tot[k], lk = h[k], rk = tk - lk;
            present += tk > 0;
            sl2 += lk * lk, sr2 += rk * rk, nl += lk, nr += rk;
        }
        const int nld = cnt[tid], nrd = n - nld;
        if (may_split(p, n, search) && present > 1 && tid < nc && nld >= p.msl && nrd >= p.msl)
            proxy = (double)sl2 / (double)nl + (double)sr2 / (double)nr;
    }
    wave_argmax(proxy, bin);
    if (lane == 0) s_proxy[wave] = proxy, s_bin[wave] = bin;
    __syncthreads();
    if (tid == 0) {
        for (int v = 1; v < 4; ++v)
            if (s_proxy[v] > proxy || (s_proxy[v] == proxy && s_bin[v] < bin)) proxy = s_proxy[v], bin = s_bin[v];
        Cand c;
        c.proxy = proxy, c.bin = proxy >= 0.0 ? bin : -1, c.nleft = proxy >= 0.0 ? cnt[bin] : 0, c.feat = f, c.pad = 0;
        cand[(int64_t)item * p.K + d] = c;
    }
}

__global__ void forest_pick_wide_kernel(Grow p, const int32_t* __restrict__ list, int n_items, const Cand* __restrict__ cand) {
    const int item = blockIdx.x * blockDim.x + threadIdx.x;
    if (item >= n_items) return;
    const int g = list[item];
    double best = -1.0;
    int bf = -1, bb = -1, bl = 0;
    for (int d = 0; d < p.K; ++d) {
        const Cand c = cand[(int64_t)item * p.K + d];
        if (c.bin >= 0 && c.proxy > best) best = c.proxy, bf = c.feat, bb = c.bin, bl = c.nleft;
    }
    p.nfeat[g] = bf, p.nbin[g] = bb, p.nleft[g] = bl;
}

// a wave per node of at most 64 distinct rows
__global__ __launch_bounds__(256) void forest_search_narrow_kernel(Grow p, const int32_t* __restrict__ list, int n_items,
                                                                    const int32_t* __restrict__ idx, int search) {
    const int lane = threadIdx.x & 63;
    const int item = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= n_items) return;          // no workgroup barrier below
    const int g = list[item];
    const int t = g / p.cap, node = g - t * p.cap;
    const int start = p.nstart[g], C = p.C;
    const int n = __builtin_amdgcn_readfirstlane(p.nend[g] - start);          // the same in every lane: a scalar loop bound
    const bool act = lane < n;
    int r = 0, y = 0, w = 0;
    if (act) {
        r = idx[(int64_t)t * p.n + start + lane];
        y = p.y[r];
        w = p.boot[(int64_t)t * p.n + r];
    }
    // lane k < C: the weighted count of class k
    int ktot = 0;
    for (int j = 0; j < n; ++j) {
        const int yj = __builtin_amdgcn_readlane(y, j), wj = __builtin_amdgcn_readlane(w, j);
        if (yj == lane) ktot += wj;
    }
    if (lane < C) p.ncounts[(int64_t)g * C + lane] = ktot;
    const int present = __popcll(__ballot(ktot > 0));
    if (!may_split(p, n, search) || present <= 1) return;          // a leaf: the node keeps feature -1
    const int64_t T2 = wave_sum64((int64_t)ktot * ktot), W = wave_sum64(ktot);
    const Picks pk = floyd_draws((uint64_t)p.seeds[t], (uint32_t)node, p.D, p.K, lane);
    double best = -1.0;
    int bf = -1, bb = -1, bl = 0;
    for (int d = 0; d < p.K; ++d) {
        const int f = pick_of(pk, d);
        if (p.ncuts[f] == 0) continue;
        const unsigned c = act ? p.codes[(int64_t)f * p.n + r] : 0u;
        unsigned key = act ? (c << 24) | ((unsigned)y << 16) | (unsigned)w : 0xFFFFFFFFu;
        // bitonic sort of the keys across the wave, ascending: the rows by code
        for (int k = 2; k <= 64; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                const unsigned o = (unsigned)__shfl_xor((int)key, j);
                const bool keep_min = ((lane & k) == 0) == ((lane & j) == 0);
                key = keep_min ? min(key, o) : max(key, o);
            }
        const int cs = (int)(key >> 24), ys = (int)((key >> 16) & 0xFFu), wsr = act ? (int)(key & 0xFFFFu) : 0;
        const int stot = __shfl(ktot, ys & 63);
        int prev = 0;          // the weight of the earlier rows of this row's class
        for (int q = 0; q < n; ++q) {
            const unsigned kq = (unsigned)__builtin_amdgcn_readlane((int)key, q);
            if (q < lane && (int)((kq >> 16) & 0xFFu) == ys) prev += (int)(kq & 0xFFFFu);
        }
        // with the rows up to this one on the left: sum L_k^2, sum tot_k L_k, nL
        const int64_t A = wave_scan64(act ? 2 * (int64_t)wsr * prev + (int64_t)wsr * wsr : 0, lane);
        const int64_t B = wave_scan64(act ? (int64_t)wsr * stot : 0, lane);
        const int64_t nl = wave_scan32(wsr, lane);
        const int next_c = __shfl_down(cs, 1);
        const int nld = lane + 1, nrd = n - nld;
        double proxy = -1.0;
        if (act && lane < n - 1 && cs != next_c && nld >= p.msl && nrd >= p.msl)
            proxy = (double)A / (double)nl + (double)(T2 - 2 * B + A) / (double)(W - nl);
        int pos = lane;
        wave_argmax(proxy, pos);
        if (proxy > best) best = proxy, bf = f, bb = __shfl(cs, pos), bl = pos + 1;
    }
    if (lane == 0) p.nfeat[g] = bf, p.nbin[g] = bb, p.nleft[g] = bl;
}

// stable partition of a split node's rows: `code <= bin` first.  src and dst are the two buffers of the trees' row lists.
__global__ __launch_bounds__(256) void forest_partition_wide_kernel(Grow p, const int32_t* __restrict__ list, const int32_t* __restrict__ src,
                                                                     int32_t* __restrict__ dst) {
    __shared__ int ws[4];
    const int g = list[blockIdx.x];
    const int f = p.nfeat[g];
    if (f < 0) return;
    const int t = g / p.cap, bin = p.nbin[g], start = p.nstart[g], end = p.nend[g];
    const uint8_t* col = p.codes + (int64_t)f * p.n;
    const int32_t* in = src + (int64_t)t * p.n;
    int32_t* out = dst + (int64_t)t * p.n;
    int at_l = start, at_r = start + p.nleft[g];
    for (int base = start; base < end; base += 256) {
        const int i = base + (int)threadIdx.x;
        const bool in_range = i < end;
        const int r = in_range ? in[i] : 0;
        const bool left = in_range && (int)col[r] <= bin;
        int nl;
        const int rank = block_rank(left, ws, nl);
        if (left) out[at_l + rank] = r;
        else if (in_range) out[at_r + ((int)threadIdx.x - rank)] = r;
        at_l += nl, at_r += min(256, end - base) - nl;
    }
}

__global__ __launch_bounds__(256) void forest_partition_narrow_kernel(Grow p, const int32_t* __restrict__ list, int n_items,
                                                                       const int32_t* __restrict__ src, int32_t* __restrict__ dst) {
    const int lane = threadIdx.x & 63;
    const int item = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= n_items) return;
    const int g = list[item];
    const int f = p.nfeat[g];
    if (f < 0) return;
    const int t = g / p.cap, bin = p.nbin[g], start = p.nstart[g], n = p.nend[g] - start;
    const bool act = lane < n;
    const int r = act ? src[(int64_t)t * p.n + start + lane] : 0;
    const bool left = act && (int)p.codes[(int64_t)f * p.n + r] <= bin;
    const unsigned long long m = __ballot(left);
    const int rank = __popcll(m & ((1ull << lane) - 1ull)), nl = __popcll(m);
    if (act) dst[(int64_t)t * p.n + start + (left ? rank : nl + lane - rank)] = r;
}

// a workgroup per tree: the split nodes of the frontier get their children, numbered in parent order
__global__ __launch_bounds__(256) void forest_number_kernel(Grow p, int32_t* __restrict__ wide, int32_t* __restrict__ narrow) {
    __shared__ int ws[4];
    const int t = blockIdx.x;
    const int fs = p.tree_fs[t], fe = p.tree_fe[t];
    const int64_t g0 = (int64_t)t * p.cap;
    int made = 0;
    for (int base = fs; base < fe; base += 256) {
        const int i = base + (int)threadIdx.x;
        const bool split = i < fe && p.nfeat[g0 + i] >= 0;
        int total;
        const int rank = block_rank(split, ws, total);
        if (split) {
            const int64_t g = g0 + i;
            const int child = fe + 2 * (made + rank);
            p.nchild[g] = child;
            const int s = p.nstart[g], e = p.nend[g], mid = s + p.nleft[g];
            for (int side = 0; side < 2; ++side) {
                const int64_t gc = g0 + child + side;
                const int cs = side ? mid : s, ce = side ? e : mid;
                p.nstart[gc] = cs, p.nend[gc] = ce, p.nfeat[gc] = -1, p.nbin[gc] = -1, p.nleft[gc] = 0, p.nchild[gc] = -1;
                const int rows = ce - cs;
                if (rows >= p.wide_min || rows > NARROW) wide[atomicAdd(&p.listcnt[0], 1)] = (int32_t)gc;
                else narrow[atomicAdd(&p.listcnt[1], 1)] = (int32_t)gc;
            }
        }
        made += total;
    }
    if (threadIdx.x == 0) p.tree_fs[t] = fe, p.tree_fe[t] = fe + 2 * made, p.newcnt[t] = 2 * made;
}

// ---- prediction --------------------------------------------------------------------------------------------------------------------
struct alignas(16) Node {          // a node as the scoring walk reads it, in one 16-byte load: left < 0 at a leaf
    int32_t left, right, feat;
    float thr;
};
struct Model {
    const int64_t* off;
    const int32_t *left, *right, *feat, *counts;
    const float* thr;
    const Node* nodes;             // the same trees, packed
    const int32_t* total;          // per node: the sum of its counts
    int T, C;
};
__global__ __launch_bounds__(256) void forest_predict_kernel(Model m, const float* __restrict__ X, int64_t n, int D, double* __restrict__ out) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= n) return;
    const float* x = X + row * D;
    double* o = out + row * m.C;
    for (int k = 0; k < m.C; ++k) o[k] = 0.0;
    for (int t = 0; t < m.T; ++t) {
        const int64_t base = m.off[t];
        int64_t node = base;
        for (int l; (l = m.left[node]) >= 0;) node = base + (x[m.feat[node]] <= m.thr[node] ? l : m.right[node]);
        const int32_t* c = m.counts + node * m.C;
        int total = 0;
        for (int k = 0; k < m.C; ++k) total += c[k];
        for (int k = 0; k < m.C; ++k) o[k] += (double)c[k] / (double)total;
    }
    for (int k = 0; k < m.C; ++k) o[k] /= (double)m.T;
}

// ---- scoring at nested forest sizes ------------------------------------------------------------------------------------------------
constexpr int SCORE_ROWS = 4;                               // rows per workgroup, a wave each
constexpr int SCORE_CHUNK = 64;                             // trees per pass, a lane each
constexpr int SCORE_MAX_PREFIXES = 4096;                    // the hit counters of a workgroup live in LDS
constexpr int64_t SCORE_LDS_MAX = 160 * 1024;               // a CU's LDS
constexpr int64_t SCORE_STAGE_BYTES = 96 * 1024;            // the default budget of the staged rows: 4 rows of 6144 floats
constexpr int64_t SCORE_CHUNK_BYTES = (int64_t)1 << 28;     // the default bound of a host chunk's rows, as float32

struct Score {
    const float* X;                  // the chunk's rows
    const int32_t* prefix;           // (G) forest sizes, ascending
    const int32_t* labels;           // the chunk's, or null
    int32_t* pred;                   // (G, n) of the chunk, or null
    unsigned long long* correct;     // (G), or null
    double* proba;                   // (G, n, C) of the chunk, or null
    double* fproba;                  // (G, span, C): the chunk's rows [f_lo, f_hi) are its rows f_at ..., or null
    int64_t n, f_lo, f_hi, f_at, span;
    int D, G, T;                     // T: the largest size
};

// the leaf (a node number over all trees) that row x reaches in tree t
__device__ __forceinline__ int score_walk(const Model& m, const float* x, int t) {
    const int64_t base = m.off[t];
    const Node* nd = m.nodes + base;
    int node = 0;
    for (Node r; (r = nd[node]).left >= 0;) node = x[r.feat] <= r.thr ? r.left : r.right;
    return (int)base + node;
}
// the count / total fractions of a pass's (tree, class) pairs, spread over the wave's lanes, into frac (cnt, C); lane j holds
// the leaf of the pass's tree j.  MASKED: only the trees whose bit of `use` is set; the others' entries are left as they are.
template <bool MASKED>
__device__ __forceinline__ void score_fractions(const Model& m, int leaf, int cnt, int lane, unsigned long long use, double* frac) {
    const int C = m.C, pairs = cnt * C;
    for (int p0 = 0; p0 < pairs; p0 += 64) {
        const int p = p0 + lane;
        const int tr = (p < pairs ? p : pairs - 1) / C;
        const int lf = __shfl(leaf, tr);
        if (p < pairs && (!MASKED || ((use >> tr) & 1ull))) frac[p] = (double)m.counts[(int64_t)lf * C + (p - tr * C)] / (double)m.total[lf];
    }
}

// LDS: the waves' fractions (SCORE_ROWS, SCORE_CHUNK, C) float64, the workgroup's hits (G, padded to 16 bytes), the staged rows
template <bool STAGED>
__global__ __launch_bounds__(256) void forest_score_kernel(Model m, Score a) {
    extern __shared__ double score_lds[];
    const int C = m.C, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double* frac = score_lds + (size_t)wave * SCORE_CHUNK * C;
    int* hits = (int*)(score_lds + (size_t)SCORE_ROWS * SCORE_CHUNK * C);
    float* xs = (float*)(hits + ((a.G + 3) & ~3));
    for (int g = threadIdx.x; g < a.G; g += 256) hits[g] = 0;
    const int64_t tiles = (a.n + SCORE_ROWS - 1) / SCORE_ROWS;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t r0 = tile * SCORE_ROWS, row = r0 + wave;
        const bool live = row < a.n;
        if (STAGED) {
            __syncthreads();          // the last tile's walks are over
            const int64_t cnt = (a.n - r0 < SCORE_ROWS ? a.n - r0 : SCORE_ROWS) * a.D;
            const float* src = a.X + r0 * a.D;
            for (int64_t i = threadIdx.x; i < cnt; i += 256) xs[i] = src[i];
        }
        __syncthreads();
        const float* x = STAGED ? xs + (size_t)wave * a.D : a.X + (live ? row : 0) * a.D;
        const int kk = lane < C ? lane : C - 1;
        double acc = 0.0;
        int gi = 0, nextp = a.prefix[0];
        for (int t0 = 0; t0 < a.T; t0 += SCORE_CHUNK) {
            const int cnt = a.T - t0 < SCORE_CHUNK ? a.T - t0 : SCORE_CHUNK;
            if (live) {
                const int leaf = lane < cnt ? score_walk(m, x, t0 + lane) : 0;
                score_fractions<false>(m, leaf, cnt, lane, 0ull, frac);
            }
            __syncthreads();
            if (live)
                for (int j = 0; j < cnt; ++j) {          // a lane per class, in tree order
                    acc += frac[j * C + kk];
                    if (t0 + j + 1 != nextp) continue;
                    const double p = acc / (double)nextp;
                    if (lane < C) {
                        if (a.proba) a.proba[((int64_t)gi * a.n + row) * C + lane] = p;
                        if (a.fproba && row >= a.f_lo && row < a.f_hi) a.fproba[((int64_t)gi * a.span + a.f_at + (row - a.f_lo)) * C + lane] = p;
                    }
                    if (a.pred || a.correct) {
                        double v = lane < C ? p : -1.0;
                        int pos = lane;
                        wave_argmax(v, pos);
                        if (lane == 0) {
                            if (a.pred) a.pred[(int64_t)gi * a.n + row] = pos;
                            if (a.correct && pos == a.labels[row]) atomicAdd(&hits[gi], 1);
                        }
                    }
                    ++gi;
                    nextp = gi < a.G ? a.prefix[gi] : -1;
                }
            __syncthreads();
        }
    }
    if (!a.correct) return;
    __syncthreads();
    for (int g = threadIdx.x; g < a.G; g += 256)
        if (hits[g]) atomicAdd(&a.correct[g], (unsigned long long)hits[g]);
}

// a thread per (size, file, class): the file's rows added in row order, / their number
__global__ void forest_file_mean_kernel(const double* __restrict__ fproba, const int64_t* __restrict__ files, int64_t fmin, int64_t span,
                                        int64_t F, int C, int G, double* __restrict__ mean) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)G * F * C) return;
    const int k = (int)(i % C);
    const int64_t f = (i / C) % F, g = i / ((int64_t)C * F);
    const int64_t s = files[2 * f], e = files[2 * f + 1];
    const double* p = fproba + (g * span + (s - fmin)) * C + k;
    double sum = 0.0;
    for (int64_t r = s; r < e; ++r, p += C) sum += *p;
    mean[i] = sum / (double)(e - s);
}
// a thread per (size, file): the first of the largest means
__global__ void forest_file_pred_kernel(const double* __restrict__ mean, int64_t GF, int C, int32_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= GF) return;
    const double* v = mean + i * C;
    int best = 0;
    for (int k = 1; k < C; ++k)
        if (v[k] > v[best]) best = k;
    out[i] = best;
}

// ---- out-of-bag scoring at nested forest sizes (l3_forest_oob) ------------------------------------------------------
// a lane per row over a slab of at most 64 trees' bootstrap multiplicities (cnt, n): bit j of the row's word is set iff tree j of
// the slab left the row out of its bag.  Every read runs along a tree's row; the bits of trees past cnt stay 0.
__global__ __launch_bounds__(256) void forest_oob_mask_kernel(const uint16_t* __restrict__ slab, int cnt, int64_t n,
                                                               unsigned long long* __restrict__ out) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= n) return;
    unsigned long long w = 0;
    for (int j = 0; j < cnt; ++j)
        if (slab[(int64_t)j * n + row] == 0) w |= 1ull << j;
    out[row] = w;
}

struct Oob {
    const float* X;                        // the chunk's rows
    const unsigned long long* mask;        // (passes, n_all): the words of all rows of the matrix, pass-major
    const int32_t* prefix;                 // (G) forest sizes, ascending
    const int32_t* labels;                 // the chunk's, or null
    int32_t* pred;                         // (G, n) of the chunk, or null
    unsigned long long* correct;           // (G), or null
    int32_t* n_oob;                        // (G, n) of the chunk, or null
    double* sums;                          // (G, n, C) of the chunk, or null
    int64_t n, row0, n_all;                // the chunk's rows are the matrix's rows row0 ...
    int D, G, T;                           // T: the largest size
};

// forest_score_kernel's walk under the row's mask: a lane whose bit is clear neither walks nor adds, the set ones' fractions are
// added in tree order, and after tree prefix[g] - 1 the wave writes the sums as they stand.  LDS as in forest_score_kernel.
template <bool STAGED>
__global__ __launch_bounds__(256) void forest_oob_kernel(Model m, Oob a) {
    extern __shared__ double score_lds[];
    const int C = m.C, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double* frac = score_lds + (size_t)wave * SCORE_CHUNK * C;
    int* hits = (int*)(score_lds + (size_t)SCORE_ROWS * SCORE_CHUNK * C);
    float* xs = (float*)(hits + ((a.G + 3) & ~3));
    for (int g = threadIdx.x; g < a.G; g += 256) hits[g] = 0;
    const int64_t tiles = (a.n + SCORE_ROWS - 1) / SCORE_ROWS;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t r0 = tile * SCORE_ROWS, row = r0 + wave;
        const bool live = row < a.n;
        if (STAGED) {
            __syncthreads();          // the last tile's walks are over
            const int64_t cnt = (a.n - r0 < SCORE_ROWS ? a.n - r0 : SCORE_ROWS) * a.D;
            const float* src = a.X + r0 * a.D;
            for (int64_t i = threadIdx.x; i < cnt; i += 256) xs[i] = src[i];
        }
        __syncthreads();
        const float* x = STAGED ? xs + (size_t)wave * a.D : a.X + (live ? row : 0) * a.D;
        const int kk = lane < C ? lane : C - 1;
        double acc = 0.0;
        int seen = 0, gi = 0, nextp = a.prefix[0];
        for (int t0 = 0; t0 < a.T; t0 += SCORE_CHUNK) {
            const int cnt = a.T - t0 < SCORE_CHUNK ? a.T - t0 : SCORE_CHUNK;
            const unsigned long long out = live ? a.mask[(int64_t)(t0 / SCORE_CHUNK) * a.n_all + a.row0 + row] : 0ull;      // one word per wave
            if (live) {
                const int leaf = lane < cnt && ((out >> lane) & 1ull) ? score_walk(m, x, t0 + lane) : 0;
                score_fractions<true>(m, leaf, cnt, lane, out, frac);
            }
            __syncthreads();
            if (live)
                for (int j = 0; j < cnt; ++j) {          // a lane per class, in tree order
                    if ((out >> j) & 1ull) acc += frac[j * C + kk], ++seen;
                    if (t0 + j + 1 != nextp) continue;
                    if (a.sums && lane < C) a.sums[((int64_t)gi * a.n + row) * C + lane] = acc;
                    if (a.n_oob && lane == 0) a.n_oob[(int64_t)gi * a.n + row] = seen;
                    if (a.pred || a.correct) {
                        double v = lane < C ? acc : -1.0;          // no tree yet: every sum is 0 and class 0 is the first of them
                        int pos = lane;
                        wave_argmax(v, pos);
                        if (lane == 0) {
                            if (a.pred) a.pred[(int64_t)gi * a.n + row] = pos;
                            if (a.correct && pos == a.labels[row]) atomicAdd(&hits[gi], 1);
                        }
                    }
                    ++gi;
                    nextp = gi < a.G ? a.prefix[gi] : -1;
                }
            __syncthreads();
        }
    }
    if (!a.correct) return;
    __syncthreads();
    for (int g = threadIdx.x; g < a.G; g += 256)
        if (hits[g]) atomicAdd(&a.correct[g], (unsigned long long)hits[g]);
}

}  // namespace
}  // namespace l3

using namespace l3;

struct l3_forest {
    int device = 0;
    hipStream_t s = nullptr;
    DeviceBufs bufs;          // owns x
    float* x = nullptr;
    int64_t n = 0;
    int D = 0;
    // the forest, on the host as l3_forest_get_trees gives it and on the device (mbufs) as the prediction reads it
    bool has_model = false;
    int T = 0, C = 0, mD = 0;
    std::vector<int64_t> off;
    std::vector<int32_t> left, right, feat, bin, counts, ndist;
    std::vector<float> thr;
    DeviceBufs mbufs;
    Model dm{};
    // the last fit's cuts and course
    std::vector<float> cuts;
    std::vector<int32_t> ncuts;
    std::vector<int64_t> lvl_nodes, lvl_wide;
    std::vector<double> lvl_ms;
};

namespace {

int install_matrix(l3_forest* m, const float* src, hipMemcpyKind kind, int64_t n, int D, const char* fn) {
    (void)hipSetDevice(m->device);
    (void)hipStreamSynchronize(m->s);
    m->bufs.release(m->x);
    m->x = nullptr, m->n = 0;
    if (!(m->x = m->bufs.alloc<float>((size_t)n * D)))
        return fail(L3_ENOMEM, std::string(fn) + ": device allocation of " + std::to_string(n * D * 4) + " bytes failed");
    if (hipMemcpyAsync(m->x, src, (size_t)n * D * sizeof(float), kind, m->s) != hipSuccess || hipStreamSynchronize(m->s) != hipSuccess)
        return fail(L3_EHIP, std::string(fn) + ": copy failed");
    m->n = n, m->D = D;
    return L3_OK;
}

// the handle's host arrays -> the device model of the prediction
int upload_model(l3_forest* m, const char* fn) {
    (void)hipSetDevice(m->device);
    (void)hipStreamSynchronize(m->s);
    m->mbufs.clear();
    m->has_model = false;
    DeviceBufs& b = m->mbufs;
    Model dm;
    dm.off = b.put(m->off.data(), m->off.size(), m->s);
    dm.left = b.put(m->left.data(), m->left.size(), m->s);
    dm.right = b.put(m->right.data(), m->right.size(), m->s);
    dm.feat = b.put(m->feat.data(), m->feat.size(), m->s);
    dm.counts = b.put(m->counts.data(), m->counts.size(), m->s);
    dm.thr = b.put(m->thr.data(), m->thr.size(), m->s);
    const size_t total = m->left.size();
    std::vector<Node> nodes(total);          // what the scoring walk reads
    std::vector<int32_t> sums(total);
    for (size_t i = 0; i < total; ++i) {
        nodes[i] = Node{m->left[i], m->right[i], m->feat[i], m->thr[i]};
        int32_t sum = 0;
        for (int k = 0; k < m->C; ++k) sum += m->counts[i * m->C + k];
        sums[i] = sum;
    }
    dm.nodes = b.put(nodes.data(), total, m->s);
    dm.total = b.put(sums.data(), total, m->s);
    dm.T = m->T, dm.C = m->C;
    if (!dm.off || !dm.left || !dm.right || !dm.feat || !dm.counts || !dm.thr || !dm.nodes || !dm.total) {
        b.clear();
        return fail(L3_ENOMEM, std::string(fn) + ": device allocation of the forest failed");
    }
    if (hipStreamSynchronize(m->s) != hipSuccess) return fail(L3_EHIP, std::string(fn) + ": HIP error");
    m->dm = dm;
    m->has_model = true;
    return L3_OK;
}

int predict_device(l3_forest* m, const float* dx, int64_t n, int D, double* out, const char* fn) {
    DeviceBufs b;
    double* d = b.alloc<double>((size_t)n * m->C);
    if (!d) return fail(L3_ENOMEM, std::string(fn) + ": device allocation failed");
    hipLaunchKernelGGL(forest_predict_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, m->s, m->dm, dx, n, D, d);
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(out, d, (size_t)n * m->C * sizeof(double), hipMemcpyDeviceToHost, m->s) != hipSuccess ||
        hipStreamSynchronize(m->s) != hipSuccess)
        return fail(L3_EHIP, std::string(fn) + ": HIP error");
    return L3_OK;
}

// what l3_forest_score and l3_forest_oob check alike before a launch: the forest sizes, the labels, the two test knobs
int check_scoring(const std::string& fn, const l3_forest* m, const int32_t* prefix, int G, const int32_t* labels, int64_t n, bool correct,
                  int64_t chunk_rows, int64_t stage_bytes) {
    if (!prefix || G < 1 || G > SCORE_MAX_PREFIXES) return fail(L3_EINVAL, fn + "need 1 to " + std::to_string(SCORE_MAX_PREFIXES) + " forest sizes");
    for (int g = 0; g < G; ++g)
        if (prefix[g] < 1 || prefix[g] > m->T || (g > 0 && prefix[g] <= prefix[g - 1]))
            return fail(L3_EINVAL, fn + "prefix[" + std::to_string(g) + "] is outside [1, " + std::to_string(m->T) + "] or not above its predecessor");
    if (correct && !labels) return fail(L3_EINVAL, fn + "correct needs labels");
    if (labels)
        for (int64_t i = 0; i < n; ++i)
            if (labels[i] < 0 || labels[i] >= m->C) return fail(L3_EINVAL, fn + "labels[" + std::to_string(i) + "] outside [0, n_classes)");
    if (chunk_rows < 0 || stage_bytes < 0) return fail(L3_EINVAL, fn + "chunk_rows and stage_bytes are 0 (the defaults) or positive");
    return L3_OK;
}

// a scoring launch's LDS, fractions + hits (+ the staged rows when they fit the budget and the CU), and the rows per launch
struct ScorePlan {
    bool staged;
    int64_t lds, chunk;
};
ScorePlan plan_scoring(int C, int G, int D, int64_t n, int64_t chunk_rows, int64_t stage_bytes) {
    const int64_t lds_plain = (int64_t)SCORE_ROWS * SCORE_CHUNK * C * 8 + (int64_t)((G + 3) & ~3) * 4;
    const int64_t row_bytes = (int64_t)SCORE_ROWS * D * 4;
    ScorePlan p;
    p.staged = row_bytes <= (stage_bytes > 0 ? stage_bytes : SCORE_STAGE_BYTES) && lds_plain + row_bytes <= SCORE_LDS_MAX;
    p.lds = lds_plain + (p.staged ? row_bytes : 0);
    p.chunk = std::min(chunk_rows > 0 ? chunk_rows : std::max<int64_t>(SCORE_ROWS, SCORE_CHUNK_BYTES / (4 * (int64_t)D)), n);
    return p;
}

}  // namespace

extern "C" {

int l3_forest_create(int device, l3_forest** out) {
    if (!out) return fail(L3_EINVAL, "l3_forest_create: out is NULL");
    *out = nullptr;
    if (!device_ok(device)) return fail(L3_EHIP, no_gpu_message("l3_forest_create", device));
    l3_forest* m = new l3_forest();
    m->device = device;
    if (hipStreamCreateWithFlags(&m->s, hipStreamNonBlocking) != hipSuccess) {
        delete m;
        return fail(L3_EHIP, "l3_forest_create: stream creation failed");
    }
    *out = m;
    return L3_OK;
}

void l3_forest_destroy(l3_forest* m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    if (m->s) (void)hipStreamSynchronize(m->s);
    if (m->s) (void)hipStreamDestroy(m->s);
    delete m;
}

int l3_forest_set_data(l3_forest* m, const float* X, int64_t n, int D) {
    if (!m || !X) return fail(L3_EINVAL, "l3_forest_set_data: NULL argument");
    if (n <= 0 || n > INT32_MAX || D <= 0 || D > (1 << 21)) return fail(L3_EINVAL, "l3_forest_set_data: need 1 <= n < 2^31, 1 <= D <= 2^21");
    return install_matrix(m, X, hipMemcpyHostToDevice, n, D, "l3_forest_set_data");
}

int l3_forest_set_data_dev(l3_forest* m, const l3_feat* f, int64_t lo, int64_t hi) {
    if (!m || !f) return fail(L3_EINVAL, "l3_forest_set_data_dev: NULL handle");
    if (f->device != m->device) return fail(L3_EINVAL, "l3_forest_set_data_dev: the feature matrix is on another device");
    if (lo < 0 || hi <= lo || hi > f->n) return fail(L3_EINVAL, "l3_forest_set_data_dev: rows [lo, hi) lie outside the matrix or are none");
    if (hi - lo > INT32_MAX || f->D <= 0 || f->D > (1 << 21))
        return fail(L3_EINVAL, "l3_forest_set_data_dev: need 1 <= n < 2^31, 1 <= D <= 2^21");
    return install_matrix(m, f->x + lo * f->D, hipMemcpyDeviceToDevice, hi - lo, (int)f->D, "l3_forest_set_data_dev");
}

int l3_forest_fit(l3_forest* m, const l3_forest_config* cfg, const int32_t* labels, int n_trees, const uint16_t* boot,
                  const int64_t* seeds) {
    const std::string fn = "l3_forest_fit: ";
    if (!m || !cfg || !labels || !boot || !seeds) return fail(L3_EINVAL, fn + "NULL argument");
    if (m->n <= 0) return fail(L3_ESTATE, fn + "no resident matrix (l3_forest_set_data)");
    const int64_t n = m->n;
    const int D = m->D, C = cfg->n_classes, K = cfg->max_features, T = n_trees;
    if (C < 1 || C > L3_FOREST_MAX_CLASSES) return fail(L3_EINVAL, fn + "n_classes must be in [1, " + std::to_string(L3_FOREST_MAX_CLASSES) + "]");
    if (K < 1 || K > D || K > L3_FOREST_MAX_DRAWS)
        return fail(L3_EINVAL, fn + "max_features must be in [1, min(D, " + std::to_string(L3_FOREST_MAX_DRAWS) + ")]");
    if (cfg->min_samples_split < 2 || cfg->min_samples_leaf < 1) return fail(L3_EINVAL, fn + "need min_samples_split >= 2 and min_samples_leaf >= 1");
    if (cfg->wide_min_rows < 0) return fail(L3_EINVAL, fn + "wide_min_rows is negative");
    if (T < 1) return fail(L3_EINVAL, fn + "no trees");
    const int64_t S = cfg->n_bin_rows > 0 ? cfg->n_bin_rows : n;
    if (cfg->n_bin_rows < 0 || (cfg->n_bin_rows > 0) != (cfg->bin_rows != nullptr)) return fail(L3_EINVAL, fn + "bin_rows and n_bin_rows come together");
    if (S > L3_FOREST_MAX_BIN_SAMPLE || S > n)
        return fail(L3_EINVAL, fn + "the cut sample holds " + std::to_string(S) + " rows; at most min(n, " + std::to_string(L3_FOREST_MAX_BIN_SAMPLE) + ")");
    for (int64_t i = 0; i < cfg->n_bin_rows; ++i)
        if (cfg->bin_rows[i] < 0 || cfg->bin_rows[i] >= n || (i > 0 && cfg->bin_rows[i] <= cfg->bin_rows[i - 1]))
            return fail(L3_EINVAL, fn + "bin_rows[" + std::to_string(i) + "] is outside [0, n) or not above its predecessor");
    std::vector<uint8_t> y8((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        if (labels[i] < 0 || labels[i] >= C) return fail(L3_EINVAL, fn + "labels[" + std::to_string(i) + "] outside [0, n_classes)");
        y8[(size_t)i] = (uint8_t)labels[i];
    }
    // the trees' row lists: the rows with a non-zero multiplicity, ascending
    std::vector<int32_t> idx0((size_t)T * n), n_tree((size_t)T);
    int64_t maxn = 0, all_rows = 0;
    for (int t = 0; t < T; ++t) {
        if (seeds[t] < 0 || seeds[t] > INT32_MAX) return fail(L3_EINVAL, fn + "seeds[" + std::to_string(t) + "] outside [0, 2^31)");
        int32_t c = 0;
        for (int64_t i = 0; i < n; ++i)
            if (boot[(size_t)t * n + i]) idx0[(size_t)t * n + c++] = (int32_t)i;
        if (c == 0) return fail(L3_EINVAL, fn + "tree " + std::to_string(t) + " has no row");
        n_tree[(size_t)t] = c;
        maxn = std::max<int64_t>(maxn, c), all_rows += c;
    }
    const int64_t cap = 2 * maxn;          // a tree of r distinct rows has at most 2 r - 1 nodes
    if (cap * T > INT32_MAX || all_rows > INT32_MAX)
        return fail(L3_EINVAL, fn + "n_trees x distinct rows is " + std::to_string(all_rows) + ": the node numbers need 2 x that below 2^31");
    const int wide_min = cfg->wide_min_rows > 0 ? cfg->wide_min_rows : NARROW + 1;

    (void)hipSetDevice(m->device);
    (void)hipStreamSynchronize(m->s);
    hipStream_t s = m->s;
    DeviceBufs b;
    // cuts and codes
    float* d_cuts = b.alloc<float>((size_t)D * MAXCUTS);
    int32_t* d_ncuts = b.alloc<int32_t>((size_t)D);
    uint8_t* d_codes = b.alloc<uint8_t>((size_t)D * n);
    const int32_t* d_binrows = cfg->n_bin_rows > 0 ? b.put(cfg->bin_rows, (size_t)cfg->n_bin_rows, s) : nullptr;
    if (!b.ok()) return fail(L3_ENOMEM, fn + "device allocation of the bin codes failed");
    int P2 = 2;
    while (P2 < S) P2 <<= 1;
    hipLaunchKernelGGL(forest_cuts_kernel, dim3((unsigned)D), dim3(256), (size_t)P2 * sizeof(float), s, m->x, (int64_t)D, d_binrows, (int)S, P2,
                       d_cuts, d_ncuts);
    hipLaunchKernelGGL(forest_codes_kernel, dim3((unsigned)((n + 63) / 64), (unsigned)((D + 63) / 64)), dim3(256), 0, s, m->x, n, D, d_cuts,
                       d_ncuts, d_codes);
    m->cuts.assign((size_t)D * MAXCUTS, 0.f);
    m->ncuts.assign((size_t)D, 0);
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(m->ncuts.data(), d_ncuts, (size_t)D * sizeof(int32_t), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(m->cuts.data(), d_cuts, (size_t)D * MAXCUTS * sizeof(float), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return fail(L3_EHIP, fn + "HIP error in the binning");
    for (int f = 0; f < D; ++f)          // only the first ncuts of a feature's row were written
        std::fill(m->cuts.begin() + (size_t)f * MAXCUTS + m->ncuts[(size_t)f], m->cuts.begin() + (size_t)(f + 1) * MAXCUTS, 0.f);

    // the trees
    Grow p{};
    p.codes = d_codes, p.ncuts = d_ncuts;
    p.y = b.put(y8.data(), (size_t)n, s);
    p.boot = b.put(boot, (size_t)T * n, s);
    p.seeds = b.put(seeds, (size_t)T, s);
    const size_t nodes = (size_t)cap * T;
    p.nstart = b.alloc<int32_t>(nodes), p.nend = b.alloc<int32_t>(nodes), p.nfeat = b.alloc<int32_t>(nodes);
    p.nbin = b.alloc<int32_t>(nodes), p.nleft = b.alloc<int32_t>(nodes), p.nchild = b.alloc<int32_t>(nodes);
    p.ncounts = b.alloc<int32_t>(nodes * C);
    p.tree_fs = b.alloc<int32_t>((size_t)T), p.tree_fe = b.alloc<int32_t>((size_t)T), p.newcnt = b.alloc<int32_t>((size_t)T + 2);
    p.listcnt = p.newcnt + T;          // read back with the new node counts in one copy
    p.n = n, p.cap = (int32_t)cap, p.D = D, p.C = C, p.K = K, p.mss = cfg->min_samples_split, p.msl = cfg->min_samples_leaf, p.wide_min = wide_min;
    int32_t* d_idx[2] = {b.put(idx0.data(), (size_t)T * n, s), b.alloc<int32_t>((size_t)T * n)};
    const int32_t* d_ntree = b.put(n_tree.data(), (size_t)T, s);
    int32_t* d_wide = b.alloc<int32_t>((size_t)all_rows);          // every node of a level holds a row of its own
    int32_t* d_narrow = b.alloc<int32_t>((size_t)all_rows);
    if (!b.ok()) return fail(L3_ENOMEM, fn + "device allocation of the trees failed");
    std::vector<int32_t> wide0, narrow0;
    for (int t = 0; t < T; ++t) (n_tree[(size_t)t] >= wide_min || n_tree[(size_t)t] > NARROW ? wide0 : narrow0).push_back((int32_t)(t * cap));
    int64_t n_wide = (int64_t)wide0.size(), n_narrow = (int64_t)narrow0.size();
    if ((n_wide && hipMemcpyAsync(d_wide, wide0.data(), wide0.size() * 4, hipMemcpyHostToDevice, s) != hipSuccess) ||
        (n_narrow && hipMemcpyAsync(d_narrow, narrow0.data(), narrow0.size() * 4, hipMemcpyHostToDevice, s) != hipSuccess))
        return fail(L3_EHIP, fn + "copy of the root lists failed");
    hipLaunchKernelGGL(forest_init_roots_kernel, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, s, p, d_ntree, T);

    std::vector<int32_t> tree_nodes((size_t)T, 1), back((size_t)T + 2);
    Cand* d_cand = nullptr;
    size_t cand_cap = 0;
    const size_t wide_lds = (size_t)(NB * C + NB) * sizeof(int);
    m->lvl_nodes.clear(), m->lvl_wide.clear(), m->lvl_ms.clear();
    for (int64_t level = 0; level <= n; ++level) {          // a tree of n rows is at most n - 1 deep
        const auto t0 = std::chrono::steady_clock::now();
        const int search = cfg->max_depth <= 0 || level < cfg->max_depth;
        const int32_t *src = d_idx[level & 1];
        int32_t* dst = d_idx[(level + 1) & 1];
        const unsigned narrow_blocks = (unsigned)((n_narrow + 3) / 4);
        if (n_wide) {
            if (search) {
                b.grow(&d_cand, &cand_cap, (size_t)n_wide * K);
                if (!d_cand) return fail(L3_ENOMEM, fn + "device allocation of the candidates failed");
            }
            hipLaunchKernelGGL(forest_search_wide_kernel, dim3((unsigned)n_wide, (unsigned)(search ? K : 1)), dim3(256), wide_lds, s, p, d_wide, src,
                               d_cand, search);
            if (search)
                hipLaunchKernelGGL(forest_pick_wide_kernel, dim3((unsigned)((n_wide + 255) / 256)), dim3(256), 0, s, p, d_wide, (int)n_wide, d_cand);
        }
        if (n_narrow)
            hipLaunchKernelGGL(forest_search_narrow_kernel, dim3(narrow_blocks), dim3(256), 0, s, p, d_narrow, (int)n_narrow, src, search);
        if (search) {
            if (n_wide) hipLaunchKernelGGL(forest_partition_wide_kernel, dim3((unsigned)n_wide), dim3(256), 0, s, p, d_wide, src, dst);
            if (n_narrow)
                hipLaunchKernelGGL(forest_partition_narrow_kernel, dim3(narrow_blocks), dim3(256), 0, s, p, d_narrow, (int)n_narrow, src, dst);
            if (hipMemsetAsync(p.listcnt, 0, 2 * sizeof(int32_t), s) != hipSuccess) return fail(L3_EHIP, fn + "HIP error");
            hipLaunchKernelGGL(forest_number_kernel, dim3((unsigned)T), dim3(256), 0, s, p, d_wide, d_narrow);
            if (hipGetLastError() != hipSuccess ||
                hipMemcpyAsync(back.data(), p.newcnt, ((size_t)T + 2) * sizeof(int32_t), hipMemcpyDeviceToHost, s) != hipSuccess)
                return fail(L3_EHIP, fn + "HIP error at level " + std::to_string(level));
        }
        if (hipStreamSynchronize(s) != hipSuccess || hipGetLastError() != hipSuccess)
            return fail(L3_EHIP, fn + "HIP error at level " + std::to_string(level));
        m->lvl_nodes.push_back(n_wide + n_narrow), m->lvl_wide.push_back(n_wide);
        m->lvl_ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        if (!search) break;
        int64_t made = 0;
        for (int t = 0; t < T; ++t) tree_nodes[(size_t)t] += back[(size_t)t], made += back[(size_t)t];
        n_wide = back[(size_t)T], n_narrow = back[(size_t)T + 1];
        if (made == 0) break;
        if (n_wide + n_narrow != made || made > all_rows) return fail(L3_EHIP, fn + "the level's lists do not add up");
    }

    // the trees, flat
    std::vector<int64_t> off((size_t)T + 1, 0);
    for (int t = 0; t < T; ++t) off[(size_t)t + 1] = off[(size_t)t] + tree_nodes[(size_t)t];
    const size_t total = (size_t)off[(size_t)T];
    std::vector<int32_t> left(total), feat(total), bin(total), st(total), en(total), counts(total * C);
    for (int t = 0; t < T; ++t) {
        const size_t g0 = (size_t)t * cap, o = (size_t)off[(size_t)t], c = (size_t)tree_nodes[(size_t)t];
        const struct { const int32_t* src; int32_t* dst; size_t w; } jobs[] = {
            {p.nchild, left.data(), 1}, {p.nfeat, feat.data(), 1}, {p.nbin, bin.data(), 1}, {p.nstart, st.data(), 1}, {p.nend, en.data(), 1},
            {p.ncounts, counts.data(), (size_t)C}};
        for (const auto& j : jobs)
            if (hipMemcpyAsync(j.dst + o * j.w, j.src + g0 * j.w, c * j.w * sizeof(int32_t), hipMemcpyDeviceToHost, s) != hipSuccess)
                return fail(L3_EHIP, fn + "copy of the trees failed");
    }
    if (hipStreamSynchronize(s) != hipSuccess) return fail(L3_EHIP, fn + "HIP error");
    m->T = T, m->C = C, m->mD = D;
    m->off = off, m->left = left, m->feat = feat, m->bin = bin, m->counts = counts;
    m->right.assign(total, -1), m->thr.assign(total, 0.f), m->ndist.assign(total, 0);
    for (size_t i = 0; i < total; ++i) {
        m->ndist[i] = en[i] - st[i];
        if (left[i] >= 0) {
            m->right[i] = left[i] + 1;
            m->thr[i] = m->cuts[(size_t)feat[i] * MAXCUTS + bin[i]];
        } else {
            m->feat[i] = m->bin[i] = -1;
        }
    }
    return upload_model(m, "l3_forest_fit");
}

int l3_forest_sizes(const l3_forest* m, int* n_trees, int64_t* n_nodes, int* n_classes, int* D) {
    if (!m) return fail(L3_EINVAL, "l3_forest_sizes: NULL handle");
    if (!m->has_model) return fail(L3_ESTATE, "l3_forest_sizes: no forest (l3_forest_fit or l3_forest_set_trees)");
    if (n_trees) *n_trees = m->T;
    if (n_nodes) *n_nodes = m->off[(size_t)m->T];
    if (n_classes) *n_classes = m->C;
    if (D) *D = m->mD;
    return L3_OK;
}

int l3_forest_get_trees(l3_forest* m, int64_t* tree_off, int32_t* left, int32_t* right, int32_t* feature, float* threshold, int32_t* bin,
                        int32_t* counts, int32_t* n_distinct) {
    if (!m || !tree_off || !left || !right || !feature || !threshold || !bin || !counts || !n_distinct)
        return fail(L3_EINVAL, "l3_forest_get_trees: NULL argument");
    if (!m->has_model) return fail(L3_ESTATE, "l3_forest_get_trees: no forest (l3_forest_fit or l3_forest_set_trees)");
    const size_t total = (size_t)m->off[(size_t)m->T];
    memcpy(tree_off, m->off.data(), m->off.size() * sizeof(int64_t));
    memcpy(left, m->left.data(), total * 4), memcpy(right, m->right.data(), total * 4), memcpy(feature, m->feat.data(), total * 4);
    memcpy(threshold, m->thr.data(), total * 4), memcpy(bin, m->bin.data(), total * 4), memcpy(n_distinct, m->ndist.data(), total * 4);
    memcpy(counts, m->counts.data(), total * m->C * 4);
    return L3_OK;
}

int l3_forest_set_trees(l3_forest* m, int n_trees, int n_classes, int D, const int64_t* tree_off, const int32_t* left, const int32_t* right,
                        const int32_t* feature, const float* threshold, const int32_t* counts) {
    const std::string fn = "l3_forest_set_trees: ";
    if (!m || !tree_off || !left || !right || !feature || !threshold || !counts) return fail(L3_EINVAL, fn + "NULL argument");
    if (n_trees < 1 || n_classes < 1 || n_classes > L3_FOREST_MAX_CLASSES || D < 1 || D > (1 << 21))
        return fail(L3_EINVAL, fn + "need n_trees >= 1, 1 <= n_classes <= " + std::to_string(L3_FOREST_MAX_CLASSES) + ", 1 <= D <= 2^21");
    if (tree_off[0] != 0) return fail(L3_EINVAL, fn + "tree_off[0] must be 0");
    for (int t = 0; t < n_trees; ++t)
        if (tree_off[t + 1] <= tree_off[t] || tree_off[t + 1] > INT32_MAX) return fail(L3_EINVAL, fn + "tree " + std::to_string(t) + " is empty or the forest has 2^31 nodes");
    const int64_t total = tree_off[n_trees];
    for (int t = 0; t < n_trees; ++t) {
        const int64_t size = tree_off[t + 1] - tree_off[t];
        for (int64_t i = 0; i < size; ++i) {
            const int64_t g = tree_off[t] + i;
            const std::string at = "node " + std::to_string(i) + " of tree " + std::to_string(t);
            int64_t sum = 0;
            for (int k = 0; k < n_classes; ++k) {
                if (counts[g * n_classes + k] < 0) return fail(L3_EINVAL, fn + at + " has a negative count");
                sum += counts[g * n_classes + k];
            }
            if (sum > INT32_MAX) return fail(L3_EINVAL, fn + at + " holds 2^31 rows");
            if (left[g] < 0 || right[g] < 0) {
                if (left[g] != -1 || right[g] != -1) return fail(L3_EINVAL, fn + at + " has one child");
                if (sum <= 0) return fail(L3_EINVAL, fn + at + " is a leaf without rows");
                continue;
            }
            if (left[g] <= i || left[g] >= size || right[g] <= i || right[g] >= size)
                return fail(L3_EINVAL, fn + at + " has a child outside (node, tree size)");
            if (feature[g] < 0 || feature[g] >= D) return fail(L3_EINVAL, fn + at + " tests a feature outside [0, D)");
        }
    }
    m->T = n_trees, m->C = n_classes, m->mD = D;
    m->off.assign(tree_off, tree_off + n_trees + 1);
    m->left.assign(left, left + total), m->right.assign(right, right + total), m->feat.assign(feature, feature + total);
    m->thr.assign(threshold, threshold + total), m->counts.assign(counts, counts + total * n_classes);
    m->bin.assign((size_t)total, -1), m->ndist.assign((size_t)total, 0);
    return upload_model(m, "l3_forest_set_trees");
}

int l3_forest_predict_proba(l3_forest* m, const float* X, int64_t n, int D, double* out) {
    if (!m || !X || !out) return fail(L3_EINVAL, "l3_forest_predict_proba: NULL argument");
    if (!m->has_model) return fail(L3_ESTATE, "l3_forest_predict_proba: no forest (l3_forest_fit or l3_forest_set_trees)");
    if (n <= 0 || D != m->mD) return fail(L3_EINVAL, "l3_forest_predict_proba: need n >= 1 rows of the forest's " + std::to_string(m->mD) + " features");
    (void)hipSetDevice(m->device);
    DeviceBufs b;
    const float* dx = b.put(X, (size_t)n * D, m->s);
    if (!dx) return fail(L3_ENOMEM, "l3_forest_predict_proba: device allocation failed");
    return predict_device(m, dx, n, D, out, "l3_forest_predict_proba");
}

int l3_forest_predict_proba_dev(l3_forest* m, const l3_feat* f, int64_t lo, int64_t hi, double* out) {
    if (!m || !f || !out) return fail(L3_EINVAL, "l3_forest_predict_proba_dev: NULL argument");
    if (!m->has_model) return fail(L3_ESTATE, "l3_forest_predict_proba_dev: no forest (l3_forest_fit or l3_forest_set_trees)");
    if (f->device != m->device) return fail(L3_EINVAL, "l3_forest_predict_proba_dev: the feature matrix is on another device");
    if (lo < 0 || hi <= lo || hi > f->n || f->D != m->mD)
        return fail(L3_EINVAL, "l3_forest_predict_proba_dev: rows [lo, hi) lie outside the matrix, are none, or have another width than the forest");
    (void)hipSetDevice(m->device);
    return predict_device(m, f->x + lo * f->D, hi - lo, (int)f->D, out, "l3_forest_predict_proba_dev");
}

int l3_forest_score(l3_forest* m, const float* X, const l3_feat* f, int64_t lo, int64_t hi, int D, int resident, const int32_t* prefix,
                    int n_prefix, const int32_t* labels, const int64_t* files, int64_t n_files, int64_t chunk_rows, int64_t stage_bytes,
                    int32_t* pred, int64_t* correct, double* file_mean, int32_t* file_pred, double* proba) {
    const std::string fn = "l3_forest_score: ";
    if (!m) return fail(L3_EINVAL, fn + "NULL handle");
    if (!m->has_model) return fail(L3_ESTATE, fn + "no forest (l3_forest_fit or l3_forest_set_trees)");
    if ((X != nullptr) + (f != nullptr) + (resident != 0) != 1) return fail(L3_EINVAL, fn + "the rows come from exactly one of X, a device matrix and the resident matrix");
    const float* dx = nullptr;          // the rows where they already are on the device
    if (resident) {
        if (m->n <= 0) return fail(L3_ESTATE, fn + "no resident matrix (l3_forest_set_data)");
        if (lo < 0 || hi <= lo || hi > m->n) return fail(L3_EINVAL, fn + "rows [lo, hi) lie outside the resident matrix or are none");
        D = m->D, dx = m->x + lo * m->D;
    } else if (f) {
        if (f->device != m->device) return fail(L3_EINVAL, fn + "the feature matrix is on another device");
        if (lo < 0 || hi <= lo || hi > f->n) return fail(L3_EINVAL, fn + "rows [lo, hi) lie outside the matrix or are none");
        D = (int)f->D, dx = f->x + lo * f->D;
    } else if (lo != 0 || hi <= 0) {
        return fail(L3_EINVAL, fn + "host rows are [0, hi) with hi >= 1");
    }
    const int64_t n = hi - lo;
    const int C = m->C, G = n_prefix;
    if (D != m->mD) return fail(L3_EINVAL, fn + "the rows have " + std::to_string(D) + " features, the forest " + std::to_string(m->mD));
    if (const int rc = check_scoring(fn, m, prefix, G, labels, n, correct != nullptr, chunk_rows, stage_bytes)) return rc;
    const bool file_out = file_mean || file_pred;
    if (n_files < 0 || (n_files > 0) != (files != nullptr)) return fail(L3_EINVAL, fn + "files and n_files come together");
    if ((n_files > 0) != file_out) return fail(L3_EINVAL, fn + "files and the file outputs (file_mean, file_pred) come together");
    int64_t fmin = n, fmax = 0;
    for (int64_t i = 0; i < n_files; ++i) {
        const int64_t s = files[2 * i], e = files[2 * i + 1];
        if (s < 0 || e <= s || e > n) return fail(L3_EINVAL, fn + "file " + std::to_string(i) + " is empty or lies outside the rows");
        fmin = std::min(fmin, s), fmax = std::max(fmax, e);
    }
    if (!pred && !correct && !file_out && !proba) return fail(L3_EINVAL, fn + "no output is asked for");

    const ScorePlan plan = plan_scoring(C, G, D, n, chunk_rows, stage_bytes);
    const bool staged = plan.staged;
    const int64_t lds = plan.lds, chunk = plan.chunk;
    const int64_t span = n_files > 0 ? fmax - fmin : 0;

    (void)hipSetDevice(m->device);
    hipStream_t s = m->s;
    (void)hipStreamSynchronize(s);
    const void* kernel = staged ? (const void*)forest_score_kernel<true> : (const void*)forest_score_kernel<false>;
    if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SCORE_LDS_MAX) != hipSuccess)
        return fail(L3_EHIP, fn + "the kernel's LDS size could not be set");
    DeviceBufs b;
    Score a{};
    a.prefix = b.put(prefix, (size_t)G, s);
    const int32_t* d_labels = labels ? b.put(labels, (size_t)n, s) : nullptr;
    float* d_x = dx ? nullptr : b.alloc<float>((size_t)chunk * D);
    int32_t* d_pred = pred ? b.alloc<int32_t>((size_t)G * chunk) : nullptr;
    double* d_proba = proba ? b.alloc<double>((size_t)G * chunk * C) : nullptr;
    unsigned long long* d_correct = correct ? b.alloc<unsigned long long>((size_t)G) : nullptr;
    double* d_fproba = n_files ? b.alloc<double>((size_t)G * span * C) : nullptr;
    double* d_fmean = n_files ? b.alloc<double>((size_t)G * n_files * C) : nullptr;
    int32_t* d_fpred = file_pred ? b.alloc<int32_t>((size_t)G * n_files) : nullptr;
    const int64_t* d_files = n_files ? b.put(files, (size_t)2 * n_files, s) : nullptr;
    if (!b.ok()) return fail(L3_ENOMEM, fn + "device allocation failed");
    if (d_correct && hipMemsetAsync(d_correct, 0, (size_t)G * sizeof(unsigned long long), s) != hipSuccess) return fail(L3_EHIP, fn + "HIP error");
    a.pred = d_pred, a.correct = d_correct, a.proba = d_proba, a.span = span, a.D = D, a.G = G, a.T = prefix[G - 1];
    for (int64_t c0 = 0; c0 < n; c0 += chunk) {
        const int64_t cn = std::min(chunk, n - c0);
        if (d_x && hipMemcpyAsync(d_x, X + c0 * D, (size_t)cn * D * sizeof(float), hipMemcpyHostToDevice, s) != hipSuccess)
            return fail(L3_EHIP, fn + "copy of the rows failed");
        a.X = d_x ? d_x : dx + c0 * D;
        a.labels = d_labels ? d_labels + c0 : nullptr;
        a.n = cn;
        const int64_t flo = std::max(fmin, c0), fhi = std::min(fmax, c0 + cn);          // the chunk's rows inside the files' span
        a.fproba = n_files && flo < fhi ? d_fproba : nullptr;
        a.f_lo = flo - c0, a.f_hi = fhi - c0, a.f_at = flo - fmin;
        const unsigned grid = (unsigned)std::min<int64_t>((cn + SCORE_ROWS - 1) / SCORE_ROWS, 2048);
        if (staged) hipLaunchKernelGGL(forest_score_kernel<true>, dim3(grid), dim3(256), (size_t)lds, s, m->dm, a);
        else hipLaunchKernelGGL(forest_score_kernel<false>, dim3(grid), dim3(256), (size_t)lds, s, m->dm, a);
        if (hipGetLastError() != hipSuccess) return fail(L3_EHIP, fn + "launch failed");
        for (int g = 0; g < G; ++g) {
            if (pred && hipMemcpyAsync(pred + (int64_t)g * n + c0, d_pred + (int64_t)g * cn, (size_t)cn * 4, hipMemcpyDeviceToHost, s) != hipSuccess)
                return fail(L3_EHIP, fn + "copy of the predictions failed");
            if (proba && hipMemcpyAsync(proba + ((int64_t)g * n + c0) * C, d_proba + (int64_t)g * cn * C, (size_t)cn * C * 8, hipMemcpyDeviceToHost,
                                        s) != hipSuccess)
                return fail(L3_EHIP, fn + "copy of the probabilities failed");
        }
        if (hipStreamSynchronize(s) != hipSuccess) return fail(L3_EHIP, fn + "HIP error in the scoring kernel");
    }
    if (n_files) {
        const int64_t items = (int64_t)G * n_files * C, gf = (int64_t)G * n_files;
        hipLaunchKernelGGL(forest_file_mean_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, d_fproba, d_files, fmin, span, n_files, C,
                           G, d_fmean);
        if (file_pred) hipLaunchKernelGGL(forest_file_pred_kernel, dim3((unsigned)((gf + 255) / 256)), dim3(256), 0, s, d_fmean, gf, C, d_fpred);
        if (hipGetLastError() != hipSuccess ||
            (file_mean && hipMemcpyAsync(file_mean, d_fmean, (size_t)items * 8, hipMemcpyDeviceToHost, s) != hipSuccess) ||
            (file_pred && hipMemcpyAsync(file_pred, d_fpred, (size_t)gf * 4, hipMemcpyDeviceToHost, s) != hipSuccess))
            return fail(L3_EHIP, fn + "HIP error in the file means");
    }
    static_assert(sizeof(unsigned long long) == sizeof(int64_t), "the hit counters are read back as int64");
    if (correct && hipMemcpyAsync(correct, d_correct, (size_t)G * 8, hipMemcpyDeviceToHost, s) != hipSuccess) return fail(L3_EHIP, fn + "HIP error");
    if (hipStreamSynchronize(s) != hipSuccess) return fail(L3_EHIP, fn + "HIP error");
    return L3_OK;
}

int l3_forest_oob(l3_forest* m, const uint16_t* boot, int n_trees, const int32_t* prefix, int n_prefix, const int32_t* labels,
                  int64_t chunk_rows, int64_t stage_bytes, int32_t* pred, int64_t* correct, int32_t* n_oob, double* sums) {
    const std::string fn = "l3_forest_oob: ";
    if (!m || !boot) return fail(L3_EINVAL, fn + "NULL argument");
    if (!m->has_model) return fail(L3_ESTATE, fn + "no forest (l3_forest_fit or l3_forest_set_trees)");
    if (m->n <= 0) return fail(L3_ESTATE, fn + "no resident matrix (l3_forest_set_data)");
    const int64_t n = m->n;
    const int C = m->C, D = m->D, G = n_prefix;
    if (n_trees != m->T) return fail(L3_EINVAL, fn + "boot holds " + std::to_string(n_trees) + " trees, the forest " + std::to_string(m->T));
    if (D != m->mD) return fail(L3_EINVAL, fn + "the rows have " + std::to_string(D) + " features, the forest " + std::to_string(m->mD));
    if (const int rc = check_scoring(fn, m, prefix, G, labels, n, correct != nullptr, chunk_rows, stage_bytes)) return rc;
    if (!pred && !correct && !n_oob && !sums) return fail(L3_EINVAL, fn + "no output is asked for");

    const ScorePlan plan = plan_scoring(C, G, D, n, chunk_rows, stage_bytes);
    const int64_t chunk = plan.chunk;
    const int T = prefix[G - 1], passes = (T + SCORE_CHUNK - 1) / SCORE_CHUNK;          // the trees past the largest size are not read

    (void)hipSetDevice(m->device);
    hipStream_t s = m->s;
    (void)hipStreamSynchronize(s);
    const void* kernel = plan.staged ? (const void*)forest_oob_kernel<true> : (const void*)forest_oob_kernel<false>;
    if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SCORE_LDS_MAX) != hipSuccess)
        return fail(L3_EHIP, fn + "the kernel's LDS size could not be set");
    DeviceBufs b;
    Oob a{};
    a.prefix = b.put(prefix, (size_t)G, s);
    const int32_t* d_labels = labels ? b.put(labels, (size_t)n, s) : nullptr;
    uint16_t* d_slab = b.alloc<uint16_t>((size_t)std::min(T, SCORE_CHUNK) * n);
    unsigned long long* d_mask = b.alloc<unsigned long long>((size_t)passes * n);
    int32_t* d_pred = pred ? b.alloc<int32_t>((size_t)G * chunk) : nullptr;
    int32_t* d_noob = n_oob ? b.alloc<int32_t>((size_t)G * chunk) : nullptr;
    double* d_sums = sums ? b.alloc<double>((size_t)G * chunk * C) : nullptr;
    unsigned long long* d_correct = correct ? b.alloc<unsigned long long>((size_t)G) : nullptr;
    if (!b.ok()) return fail(L3_ENOMEM, fn + "device allocation failed");
    if (d_correct && hipMemsetAsync(d_correct, 0, (size_t)G * sizeof(unsigned long long), s) != hipSuccess) return fail(L3_EHIP, fn + "HIP error");
    // the masks: a slab of 64 trees' multiplicities at a time, in stream order through one buffer
    for (int p = 0; p < passes; ++p) {
        const int t0 = p * SCORE_CHUNK, cnt = std::min(T - t0, SCORE_CHUNK);
        if (hipMemcpyAsync(d_slab, boot + (size_t)t0 * n, (size_t)cnt * n * sizeof(uint16_t), hipMemcpyHostToDevice, s) != hipSuccess)
            return fail(L3_EHIP, fn + "copy of the multiplicities failed");
        hipLaunchKernelGGL(forest_oob_mask_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, d_slab, cnt, n, d_mask + (size_t)p * n);
        if (hipGetLastError() != hipSuccess) return fail(L3_EHIP, fn + "launch failed");
    }
    a.mask = d_mask, a.pred = d_pred, a.correct = d_correct, a.n_oob = d_noob, a.sums = d_sums;
    a.n_all = n, a.D = D, a.G = G, a.T = T;
    for (int64_t c0 = 0; c0 < n; c0 += chunk) {
        const int64_t cn = std::min(chunk, n - c0);
        a.X = m->x + c0 * D;
        a.labels = d_labels ? d_labels + c0 : nullptr;
        a.n = cn, a.row0 = c0;
        const unsigned grid = (unsigned)std::min<int64_t>((cn + SCORE_ROWS - 1) / SCORE_ROWS, 2048);
        if (plan.staged) hipLaunchKernelGGL(forest_oob_kernel<true>, dim3(grid), dim3(256), (size_t)plan.lds, s, m->dm, a);
        else hipLaunchKernelGGL(forest_oob_kernel<false>, dim3(grid), dim3(256), (size_t)plan.lds, s, m->dm, a);
        if (hipGetLastError() != hipSuccess) return fail(L3_EHIP, fn + "launch failed");
        for (int g = 0; g < G; ++g) {
            if (pred && hipMemcpyAsync(pred + (int64_t)g * n + c0, d_pred + (int64_t)g * cn, (size_t)cn * 4, hipMemcpyDeviceToHost, s) != hipSuccess)
                return fail(L3_EHIP, fn + "copy of the predictions failed");
            if (n_oob && hipMemcpyAsync(n_oob + (int64_t)g * n + c0, d_noob + (int64_t)g * cn, (size_t)cn * 4, hipMemcpyDeviceToHost, s) != hipSuccess)
                return fail(L3_EHIP, fn + "copy of the tree counts failed");
            if (sums && hipMemcpyAsync(sums + ((int64_t)g * n + c0) * C, d_sums + (int64_t)g * cn * C, (size_t)cn * C * 8, hipMemcpyDeviceToHost,
                                       s) != hipSuccess)
                return fail(L3_EHIP, fn + "copy of the sums failed");
        }
        if (hipStreamSynchronize(s) != hipSuccess) return fail(L3_EHIP, fn + "HIP error in the scoring kernel");
    }
    if (correct && hipMemcpyAsync(correct, d_correct, (size_t)G * 8, hipMemcpyDeviceToHost, s) != hipSuccess) return fail(L3_EHIP, fn + "HIP error");
    if (hipStreamSynchronize(s) != hipSuccess) return fail(L3_EHIP, fn + "HIP error");
    return L3_OK;
}

int l3_forest_get_cuts(l3_forest* m, float* cuts, int32_t* ncuts) {
    if (!m || !cuts || !ncuts) return fail(L3_EINVAL, "l3_forest_get_cuts: NULL argument");
    if (m->ncuts.empty()) return fail(L3_ESTATE, "l3_forest_get_cuts: no fit yet");
    memcpy(cuts, m->cuts.data(), m->cuts.size() * sizeof(float));
    memcpy(ncuts, m->ncuts.data(), m->ncuts.size() * sizeof(int32_t));
    return L3_OK;
}

int l3_forest_level_stats(const l3_forest* m, int max_levels, int64_t* nodes, int64_t* wide, double* ms) {
    if (!m) return 0;
    const int L = (int)m->lvl_nodes.size();
    for (int i = 0; i < L && i < max_levels; ++i) {
        if (nodes) nodes[i] = m->lvl_nodes[(size_t)i];
        if (wide) wide[i] = m->lvl_wide[(size_t)i];
        if (ms) ms[i] = m->lvl_ms[(size_t)i];
    }
    return L;
}

}  // extern "C"
