// locmap.hip -- sound localisation maps: the AVC head scored at every location of a tower's last feature map.
//
// Both towers end in a global max pool (model.py:25-31 concatenates the two pooled rows), so a pooled feature is the maximum of a
// per-location activation, and the head has a value at every location: the location's C channels take the place of the pooled row.
// dense_1 splits over the concatenation (pairs.hip), so a location is scored like an item: its row is projected with its side's half
// of W1 by project_kernel (vision: W1v; audio: W1a, + b1) into the resident map M (n_items * L, head), location-major, and a
// (location, query) margin is pair_step() over k = 0 .. head-1 from 0 with bd added last -- the bits l3_pairs_list gives when that
// location row is set as an item (fl32(u + t) is commutative, so it does not matter which side the map is).
//
//   map_kernel   a workgroup owns one item and up to 64 queries; it walks the item's ceil(L / 64) tiles of locations with
//                accumulate_rows (pair_tile.h: the 4 x 4 register block of pair_tile_kernel, the query rows gathered by index) and
//                keeps, per lane and query column, the running (peak, location) in registers; the 16 lanes of a column are joined
//                through LDS at the end.  LIST stores the map rows as it goes (float4 over 4 locations) and / or the peaks of listed
//                (item, query) pairs; PEAKS stores the block of S_ij = max_l margin_ijl and its location, never a map; RANKS stores
//                nothing and counts S against the truth pairs' S with integer adds (one per item and workgroup, one per query that is
//                beaten): exact and the same from run to run.
// The order of a peak (l3hip.h) is strict and total, so the result does not depend on the tiling or on the order the lanes are
// joined in.  No float atomics.
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

constexpr int64_t MAP_MAX_ROWS = ((int64_t)1 << 31) - 1 - TILE;          // location rows of a map; outputs of one call
constexpr int ROWG = BLOCK / 16;                                         // lanes that share a query column

enum { MAP_LIST = 0, MAP_PEAKS = 1, MAP_RANKS = 2 };

// (m, l) stands before (bm, bl): the larger margin, then the smaller location; NaN never; the empty peak is (-inf, -1)
__device__ __forceinline__ bool peak_before(float m, int l, float bm, int bl) { return (m > bm) | ((m == bm) & ((unsigned)l < (unsigned)bl)); }

// LIST: workgroup b takes work[3 b .. 3 b + 2] = {item, first, count}: the queries qidx[first .. first + count), outputs at first + c.
// PEAKS / RANKS: workgroup b takes item i0 + b / chunks and the queries j0 + 64 (b % chunks) ..., below j1; PEAKS writes at
// (item - i0) (j1 - j0) + (j - j0).  RANKS: r_item[i] += #{j: S_ij > s_item[i]}, r_query[j] += #{i: S_ij > s_query[j]}, pairs of one
// group left out; s_item / r_item or s_query / r_query may be null, g_item and g_query are null together.
template <int MODE>
__global__ __launch_bounds__(BLOCK) void map_kernel(const float* __restrict__ M, const float* __restrict__ Q, const float* __restrict__ wd,
                                                    float bd, int H, int L, const int32_t* __restrict__ work,
                                                    const int32_t* __restrict__ qidx, float* __restrict__ maps, int i0, int j0, int j1,
                                                    int chunks, float* __restrict__ peak, int32_t* __restrict__ arg,
                                                    const float* __restrict__ s_item, const float* __restrict__ s_query,
                                                    const int32_t* __restrict__ g_item, const int32_t* __restrict__ g_query,
                                                    int32_t* __restrict__ r_item, int32_t* __restrict__ r_query) {
    __shared__ __attribute__((aligned(16))) float Us[KC][TILE];
    __shared__ __attribute__((aligned(16))) float Ts[KC][TILE];
    __shared__ float jm[ROWG][TILE];
    __shared__ int jl[ROWG][TILE];
    __shared__ int qrow[TILE];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    int item, first, count;
    int64_t opos;
    if (MODE == MAP_LIST) {
        item = work[3 * (int64_t)blockIdx.x], first = work[3 * (int64_t)blockIdx.x + 1], count = work[3 * (int64_t)blockIdx.x + 2];
        opos = first;
    } else {
        item = i0 + (int)(blockIdx.x / chunks);
        first = j0 + (int)(blockIdx.x % chunks) * TILE;
        count = min(TILE, j1 - first);
        opos = (int64_t)(item - i0) * (j1 - j0) + (first - j0);
    }
    if (tid < TILE) qrow[tid] = tid < count ? (MODE == MAP_LIST ? qidx[first + tid] : first + tid) : -1;
    __syncthreads();
    const float* Mi = M + (int64_t)item * L * H;
    float bm[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    int bl[4] = {-1, -1, -1, -1};
    for (int l0 = 0; l0 < L; l0 += TILE) {
        float acc[4][4] = {};
        accumulate_rows(
            acc, Us, Ts, Mi, Q, wd, H, [=](int r) { return l0 + r < L ? (int64_t)(l0 + r) : (int64_t)-1; },
            [&](int r) { return (int64_t)qrow[r]; }, tid, tx, ty);
        const int l = l0 + ty * 4;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float m[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                m[a] = __fadd_rn(acc[a][c], bd);
                if (l + a < L && peak_before(m[a], l + a, bm[c], bl[c])) bm[c] = m[a], bl[c] = l + a;
            }
            if (MODE == MAP_LIST && maps && tx * 4 + c < count) {
                float* o = maps + (opos + tx * 4 + c) * L + l;
                if (l + 3 < L && (L & 3) == 0) {
                    *reinterpret_cast<float4*>(o) = make_float4(m[0], m[1], m[2], m[3]);
                } else {
#pragma unroll
                    for (int a = 0; a < 4; ++a)
                        if (l + a < L) o[a] = m[a];
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) jm[ty][tx * 4 + c] = bm[c], jl[ty][tx * 4 + c] = bl[c];
    __syncthreads();
    if (tid >= TILE) return;          // the first wave, whole, goes on
    float best = -INFINITY;
    int at = -1;
    for (int g = 0; g < ROWG; ++g)
        if (peak_before(jm[g][tid], jl[g][tid], best, at)) best = jm[g][tid], at = jl[g][tid];
    const bool valid = tid < count;
    if (MODE != MAP_RANKS) {
        if (valid && peak) peak[opos + tid] = best;
        if (valid && arg) arg[opos + tid] = at;
        return;
    }
    const int j = valid ? qrow[tid] : 0;
    const bool neg = valid && (!g_item || g_item[item] != g_query[j]);
    if (s_item) {
        const int n = __popcll(__ballot(neg && best > s_item[item]));
        if (tid == 0 && n) atomicAdd(&r_item[item], n);
    }
    if (s_query && neg && best > s_query[j]) atomicAdd(&r_query[j], 1);
}

// out[dest[q]] = x[q]: the truth pairs' peaks from the order of the list to the order of the items and of the queries
__global__ __launch_bounds__(BLOCK) void scatter_kernel(const float* __restrict__ x, const int32_t* __restrict__ dest, float* __restrict__ out,
                                                        int n) {
    const int q = blockIdx.x * BLOCK + threadIdx.x;
    if (q < n) out[dest[q]] = x[q];
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
void launch_list(const float* M, const float* Q, const float* wd, float bd, int H, int L, const int32_t* work, int64_t n_work,
                 const int32_t* qidx, float* maps, float* peak, int32_t* arg, hipStream_t s) {
    hipLaunchKernelGGL(map_kernel<MAP_LIST>, dim3((unsigned)n_work), dim3(BLOCK), 0, s, M, Q, wd, bd, H, L, work, qidx, maps, 0, 0, 0, 1, peak,
                       arg, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
}

void launch_peaks(const float* M, const float* Q, const float* wd, float bd, int H, int L, int64_t i0, int64_t i1, int64_t j0, int64_t j1,
                  float* S, int32_t* arg, hipStream_t s) {
    const int64_t chunks = (j1 - j0 + TILE - 1) / TILE;
    hipLaunchKernelGGL(map_kernel<MAP_PEAKS>, dim3((unsigned)((i1 - i0) * chunks)), dim3(BLOCK), 0, s, M, Q, wd, bd, H, L, nullptr, nullptr,
                       nullptr, (int)i0, (int)j0, (int)j1, (int)chunks, S, arg, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
}

void launch_ranks(const float* M, const float* Q, const float* wd, float bd, int H, int L, int64_t n_items, int64_t n_q, const float* s_item,
                  const float* s_query, const int32_t* g_item, const int32_t* g_query, int32_t* r_item, int32_t* r_query, hipStream_t s) {
    const int64_t chunks = (n_q + TILE - 1) / TILE;
    hipLaunchKernelGGL(map_kernel<MAP_RANKS>, dim3((unsigned)(n_items * chunks)), dim3(BLOCK), 0, s, M, Q, wd, bd, H, L, nullptr, nullptr,
                       nullptr, 0, 0, (int)n_q, (int)chunks, nullptr, nullptr, s_item, s_query, g_item, g_query, r_item, r_query);
}

// The listed pairs in CSR form by item -> the work list {item, first, count} of at most 64 queries each.  Returns an error message,
// or nullptr: item_ptr[0] == 0, not decreasing, at least one and at most MAP_MAX_ROWS pairs, every query in [0, n_q).
std::string list_work(const int64_t* item_ptr, const int32_t* query_idx, int64_t n_items, int64_t n_q, int64_t L, bool with_maps,
                      std::vector<int32_t>* work) {
    if (item_ptr[0] != 0) return "item_ptr[0] must be 0";
    for (int64_t i = 0; i < n_items; ++i)
        if (item_ptr[i + 1] < item_ptr[i]) return "item_ptr decreases at item " + std::to_string(i);
    const int64_t n = item_ptr[n_items];
    if (n < 1 || n > MAP_MAX_ROWS) return "need between 1 and 2^31 - 65 listed pairs, not " + std::to_string(n);
    if (with_maps && n > MAP_MAX_ROWS / L) return std::to_string(n) + " maps of " + std::to_string(L) + " locations are more than 2^31 - 65 values: list fewer pairs a call";
    for (int64_t q = 0; q < n; ++q)
        if (query_idx[q] < 0 || query_idx[q] >= n_q)
            return "query_idx[" + std::to_string(q) + "] = " + std::to_string(query_idx[q]) + " outside [0, " + std::to_string(n_q) + ")";
    work->clear();
    for (int64_t i = 0; i < n_items; ++i)
        for (int64_t f = item_ptr[i]; f < item_ptr[i + 1]; f += TILE) {
            work->push_back((int32_t)i);
            work->push_back((int32_t)f);
            work->push_back((int32_t)std::min<int64_t>(TILE, item_ptr[i + 1] - f));
        }
    return std::string();
}

// the query set of the map's side: the opposite set
const float* query_rows(const l3_pairs* p) { return p->map_side == 0 ? p->T : p->U; }
int64_t query_count(const l3_pairs* p) { return p->map_side == 0 ? p->Na : p->Nv; }

int need_map(const l3_pairs* p, const char* fn) {
    if (!p->head_set) return fail(L3_ESTATE, std::string(fn) + ": l3_pairs_set_head has not been called");
    if (p->map_side < 0) return fail(L3_ESTATE, std::string(fn) + ": l3_pairs_map_reserve has not been called");
    if (p->map_done != p->map_items)
        return fail(L3_ESTATE, std::string(fn) + ": " + std::to_string(p->map_items - p->map_done) + " of the map's " + std::to_string(p->map_items) +
                                   " items have not been put (l3_pairs_map_put) since the head was set");
    if (query_count(p) < 1)
        return fail(L3_ESTATE, std::string(fn) + ": the query set comes first: " + (p->map_side == 0 ? "l3_pairs_set_audio" : "l3_pairs_set_vision"));
    return L3_OK;
}

}  // namespace
}  // namespace l3

using namespace l3;

extern "C" {

int l3_pairs_map_reserve(l3_pairs* p, int side, int64_t n_items, int H, int W) {
    const char* fn = "l3_pairs_map_reserve";
    if (int rc = pairs_enter(p, fn)) return rc;
    if (side != 0 && side != 1) return fail(L3_EINVAL, std::string(fn) + ": side must be 0 (vision locations) or 1 (audio locations), not " + std::to_string(side));
    if (H < 1 || W < 1 || n_items < 1 || (int64_t)H * W > MAP_MAX_ROWS || n_items > MAP_MAX_ROWS / ((int64_t)H * W))
        return fail(L3_EINVAL, std::string(fn) + ": need n_items >= 1 and H, W >= 1 (L = H W >= 1) with n_items L <= 2^31 - 65; got " + std::to_string(n_items) +
                                   " items of " + std::to_string(H) + " x " + std::to_string(W));
    p->map_side = -1, p->map_done = 0;
    const int64_t L = (int64_t)H * W;
    if (int rc = pairs_grow(p, &p->M, &p->cap_M, (size_t)n_items * L * p->head, fn)) return rc;
    p->map_side = side, p->map_H = H, p->map_W = W, p->map_L = L, p->map_items = n_items;
    p->map_put.assign((size_t)n_items, 0);
    return L3_OK;
}

int l3_pairs_map_put(l3_pairs* p, const l3_feat* loc, int64_t lo_row, int64_t item0, int64_t n_items) {
    const char* fn = "l3_pairs_map_put";
    if (int rc = pairs_enter(p, fn)) return rc;
    if (!loc) return fail(L3_EINVAL, std::string(fn) + ": the location rows are NULL");
    if (p->map_side < 0) return fail(L3_ESTATE, std::string(fn) + ": l3_pairs_map_reserve has not been called");
    if (!p->head_set) return fail(L3_ESTATE, std::string(fn) + ": l3_pairs_set_head has not been called");
    const bool vision = p->map_side == 0;
    const int K = vision ? p->nv : p->na;
    const int64_t L = p->map_L;
    if (loc->device != p->device)
        return fail(L3_EINVAL, std::string(fn) + ": the location rows are on device " + std::to_string(loc->device) + ", the scorer on device " + std::to_string(p->device));
    if (loc->D != K)
        return fail(L3_EINVAL, std::string(fn) + ": the location rows have " + std::to_string(loc->D) + " columns, the tower's last feature map " + std::to_string(K) + " channels");
    if (n_items < 1 || item0 < 0 || item0 > p->map_items - n_items)
        return fail(L3_EINVAL, std::string(fn) + ": items [" + std::to_string(item0) + ", " + std::to_string(item0) + " + " + std::to_string(n_items) +
                                   ") are empty or outside the " + std::to_string(p->map_items) + " items of the map");
    if (lo_row < 0 || n_items * L > loc->n || lo_row > loc->n - n_items * L)
        return fail(L3_EINVAL, std::string(fn) + ": rows [" + std::to_string(lo_row) + ", " + std::to_string(lo_row) + " + " + std::to_string(n_items * L) +
                                   ") outside the " + std::to_string(loc->n) + " rows of the location matrix");
    // (every l3_feat call has finished on its handle's stream when it returns: the rows hold their final values)
    pairs_project(loc->x + lo_row * K, K, p->w1 + (vision ? 0 : (size_t)p->nv * p->head), vision ? nullptr : p->b1,
                  p->M + (size_t)item0 * L * p->head, n_items * L, K, p->head, p->s);
    if (!pairs_finished(p->s)) return fail(L3_EHIP, std::string(fn) + ": the projection failed on the device");
    for (int64_t i = item0; i < item0 + n_items; ++i)
        if (!p->map_put[(size_t)i]) p->map_put[(size_t)i] = 1, ++p->map_done;
    return L3_OK;
}

int l3_pairs_map_list(l3_pairs* p, const int64_t* item_ptr, const int32_t* query_idx, float* maps, float* peak, int32_t* arg) {
    const char* fn = "l3_pairs_map_list";
    if (int rc = pairs_enter(p, fn)) return rc;
    if (!item_ptr || !query_idx) return fail(L3_EINVAL, std::string(fn) + ": item_ptr and query_idx must not be NULL");
    if (!maps && !peak && !arg) return fail(L3_EINVAL, std::string(fn) + ": maps, or peak / arg, or all of them are needed");
    if (int rc = need_map(p, fn)) return rc;
    const int64_t L = p->map_L;
    std::vector<int32_t> work;
    const std::string why = list_work(item_ptr, query_idx, p->map_items, query_count(p), L, maps != nullptr, &work);
    if (!why.empty()) return fail(L3_EINVAL, std::string(fn) + ": " + why);
    const int64_t n = item_ptr[p->map_items], nw = (int64_t)work.size() / 3;
    // midx: work (3 nw), queries (n), arg (n); mout: peak (n), maps (n L)
    if (int rc = pairs_grow(p, &p->midx, &p->cap_midx, (size_t)(3 * nw + 2 * n), fn)) return rc;
    if (int rc = pairs_grow(p, &p->mout, &p->cap_mout, (size_t)n + (maps ? (size_t)n * L : 0), fn)) return rc;
    int32_t *d_work = p->midx, *d_q = d_work + 3 * nw, *d_arg = d_q + n;
    float *d_peak = p->mout, *d_maps = maps ? p->mout + n : nullptr;
    if (hipMemcpyAsync(d_work, work.data(), (size_t)nw * 12, hipMemcpyHostToDevice, p->s) != hipSuccess ||
        hipMemcpyAsync(d_q, query_idx, (size_t)n * 4, hipMemcpyHostToDevice, p->s) != hipSuccess)
        return fail(L3_EHIP, std::string(fn) + ": copy to the device failed");
    launch_list(p->M, query_rows(p), p->wd, p->bd, p->head, (int)L, d_work, nw, d_q, d_maps, d_peak, d_arg, p->s);
    bool ok = true;
    if (maps) ok = ok && hipMemcpyAsync(maps, d_maps, (size_t)n * L * 4, hipMemcpyDeviceToHost, p->s) == hipSuccess;
    if (peak) ok = ok && hipMemcpyAsync(peak, d_peak, (size_t)n * 4, hipMemcpyDeviceToHost, p->s) == hipSuccess;
    if (arg) ok = ok && hipMemcpyAsync(arg, d_arg, (size_t)n * 4, hipMemcpyDeviceToHost, p->s) == hipSuccess;
    if (!ok || !pairs_finished(p->s)) return fail(L3_EHIP, std::string(fn) + ": the kernel or the copy from the device failed");
    return L3_OK;
}

int l3_pairs_map_peaks(l3_pairs* p, int64_t i0, int64_t i1, int64_t j0, int64_t j1, float* S, int32_t* arg) {
    const char* fn = "l3_pairs_map_peaks";
    if (int rc = pairs_enter(p, fn)) return rc;
    if (!S) return fail(L3_EINVAL, std::string(fn) + ": S is NULL");
    if (int rc = need_map(p, fn)) return rc;
    const int64_t nq = query_count(p);
    if (i0 < 0 || i1 > p->map_items || i0 >= i1 || j0 < 0 || j1 > nq || j0 >= j1)
        return fail(L3_EINVAL, std::string(fn) + ": the block [" + std::to_string(i0) + ", " + std::to_string(i1) + ") x [" + std::to_string(j0) + ", " +
                                   std::to_string(j1) + ") is empty or outside the " + std::to_string(p->map_items) + " items x " + std::to_string(nq) + " queries");
    if (i1 - i0 > MAP_MAX_ROWS / (j1 - j0)) return fail(L3_EINVAL, std::string(fn) + ": a block holds at most 2^31 - 65 peaks");
    const size_t count = (size_t)(i1 - i0) * (size_t)(j1 - j0);
    if (int rc = pairs_grow(p, &p->mout, &p->cap_mout, count, fn)) return rc;
    if (int rc = pairs_grow(p, &p->midx, &p->cap_midx, count, fn)) return rc;
    launch_peaks(p->M, query_rows(p), p->wd, p->bd, p->head, (int)p->map_L, i0, i1, j0, j1, p->mout, p->midx, p->s);
    bool ok = hipMemcpyAsync(S, p->mout, count * 4, hipMemcpyDeviceToHost, p->s) == hipSuccess;
    if (arg) ok = ok && hipMemcpyAsync(arg, p->midx, count * 4, hipMemcpyDeviceToHost, p->s) == hipSuccess;
    if (!ok || !pairs_finished(p->s)) return fail(L3_EHIP, std::string(fn) + ": the kernel or the copy from the device failed");
    return L3_OK;
}

int l3_pairs_map_ranks(l3_pairs* p, const int32_t* truth_a, const int32_t* truth_v, const int32_t* group_v, const int32_t* group_a,
                       int32_t* rank_v2a, int32_t* rank_a2v) {
    const char* fn = "l3_pairs_map_ranks";
    if (int rc = pairs_enter(p, fn)) return rc;
    if ((truth_a == nullptr) != (rank_v2a == nullptr) || (truth_v == nullptr) != (rank_a2v == nullptr) || (!truth_a && !truth_v))
        return fail(L3_EINVAL, std::string(fn) + ": a direction needs both its truth and its rank vector, and one direction at least is needed");
    if ((group_v == nullptr) != (group_a == nullptr))
        return fail(L3_EINVAL, std::string(fn) + ": group_v and group_a are given together or both NULL");
    if (int rc = need_map(p, fn)) return rc;
    const bool vmap = p->map_side == 0;          // the items are the frames
    const int64_t Ni = p->map_items, Nq = query_count(p), Nv = vmap ? Ni : Nq, Na = vmap ? Nq : Ni, N = Ni + Nq, L = p->map_L;
    for (int64_t i = 0; truth_a && i < Nv; ++i)
        if (truth_a[i] < 0 || truth_a[i] >= Na)
            return fail(L3_EINVAL, std::string(fn) + ": truth_a[" + std::to_string(i) + "] = " + std::to_string(truth_a[i]) + " outside [0, " + std::to_string(Na) + ")");
    for (int64_t j = 0; truth_v && j < Na; ++j)
        if (truth_v[j] < 0 || truth_v[j] >= Nv)
            return fail(L3_EINVAL, std::string(fn) + ": truth_v[" + std::to_string(j) + "] = " + std::to_string(truth_v[j]) + " outside [0, " + std::to_string(Nv) + ")");
    // in terms of the map: every item's true query and its rank among the queries, every query's true item and its rank among the items
    const int32_t *tq = vmap ? truth_a : truth_v, *ti = vmap ? truth_v : truth_a;
    const int32_t *gi = vmap ? group_v : group_a, *gq = vmap ? group_a : group_v;
    int32_t *ri = vmap ? rank_v2a : rank_a2v, *rq = vmap ? rank_a2v : rank_v2a;
    // the truth pairs by item: (i, tq[i]) -> s_item[i] = slot i, (ti[j], j) -> s_query[j] = slot Ni + j
    std::vector<int64_t> ptr((size_t)Ni + 1, 0);
    for (int64_t i = 0; tq && i < Ni; ++i) ++ptr[(size_t)i + 1];
    for (int64_t j = 0; ti && j < Nq; ++j) ++ptr[(size_t)ti[j] + 1];
    for (int64_t i = 0; i < Ni; ++i) ptr[(size_t)i + 1] += ptr[(size_t)i];
    const int64_t n = ptr[(size_t)Ni];
    std::vector<int32_t> qs((size_t)n), dest((size_t)n);
    {
        std::vector<int64_t> at(ptr.begin(), ptr.end() - 1);
        for (int64_t i = 0; tq && i < Ni; ++i) qs[(size_t)at[(size_t)i]] = tq[i], dest[(size_t)at[(size_t)i]++] = (int32_t)i;
        for (int64_t j = 0; ti && j < Nq; ++j) qs[(size_t)at[(size_t)ti[j]]] = (int32_t)j, dest[(size_t)at[(size_t)ti[j]]++] = (int32_t)(Ni + j);
    }
    std::vector<int32_t> work;
    const std::string why = list_work(ptr.data(), qs.data(), Ni, Nq, L, false, &work);
    if (!why.empty()) return fail(L3_EINVAL, std::string(fn) + ": " + why);
    const int64_t nw = (int64_t)work.size() / 3;
    // midx: work (3 nw), queries (n), destinations (n), groups (N), counts (N); mout: listed peaks (n), truth peaks (N)
    if (int rc = pairs_grow(p, &p->midx, &p->cap_midx, (size_t)(3 * nw + 2 * n + 2 * N), fn)) return rc;
    if (int rc = pairs_grow(p, &p->mout, &p->cap_mout, (size_t)(n + N), fn)) return rc;
    int32_t *d_work = p->midx, *d_q = d_work + 3 * nw, *d_dest = d_q + n, *d_g = d_dest + n, *d_cnt = d_g + N;
    float *d_peak = p->mout, *d_s = p->mout + n;
    std::vector<int32_t> groups((size_t)N, 0);
    for (int64_t i = 0; gi && i < Ni; ++i) groups[(size_t)i] = gi[i];
    for (int64_t j = 0; gq && j < Nq; ++j) groups[(size_t)(Ni + j)] = gq[j];
    if (hipMemcpyAsync(d_work, work.data(), (size_t)nw * 12, hipMemcpyHostToDevice, p->s) != hipSuccess ||
        hipMemcpyAsync(d_q, qs.data(), (size_t)n * 4, hipMemcpyHostToDevice, p->s) != hipSuccess ||
        hipMemcpyAsync(d_dest, dest.data(), (size_t)n * 4, hipMemcpyHostToDevice, p->s) != hipSuccess ||
        hipMemcpyAsync(d_g, groups.data(), (size_t)N * 4, hipMemcpyHostToDevice, p->s) != hipSuccess ||
        hipMemsetAsync(d_cnt, 0, (size_t)N * 4, p->s) != hipSuccess)
        return fail(L3_EHIP, std::string(fn) + ": copy to the device failed");
    launch_list(p->M, query_rows(p), p->wd, p->bd, p->head, (int)L, d_work, nw, d_q, nullptr, d_peak, nullptr, p->s);
    hipLaunchKernelGGL(scatter_kernel, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, p->s, d_peak, d_dest, d_s, (int)n);
    launch_ranks(p->M, query_rows(p), p->wd, p->bd, p->head, (int)L, Ni, Nq, tq ? d_s : nullptr, ti ? d_s + Ni : nullptr, gi ? d_g : nullptr,
                 gi ? d_g + Ni : nullptr, tq ? d_cnt : nullptr, ti ? d_cnt + Ni : nullptr, p->s);
    bool ok = true;
    if (ri) ok = ok && hipMemcpyAsync(ri, d_cnt, (size_t)Ni * 4, hipMemcpyDeviceToHost, p->s) == hipSuccess;
    if (rq) ok = ok && hipMemcpyAsync(rq, d_cnt + Ni, (size_t)Nq * 4, hipMemcpyDeviceToHost, p->s) == hipSuccess;
    if (!ok || !pairs_finished(p->s)) return fail(L3_EHIP, std::string(fn) + ": the kernels or the copy from the device failed");
    return L3_OK;
}

// Device time of `reps` launches on the resident map and query set, in ms per launch (hipEvents; one untimed launch first).  what 0:
// the list mode over the diagonal (item i with query i; as many items as queries), maps and peaks stored; 1: the peaks mode over the
// whole block; 2: the counting pass of the rank mode with the diagonal as truth and no groups (its truth peaks come from one untimed
// list launch).  For profiles/ records; no test asserts a time.
int l3_pairs_map_time(l3_pairs* p, int what, int reps, double* ms) {
    const char* fn = "l3_pairs_map_time";
    if (int rc = pairs_enter(p, fn)) return rc;
    if (!ms || reps < 1 || what < 0 || what > 2) return fail(L3_EINVAL, std::string(fn) + ": need ms, reps >= 1 and what in [0, 2]");
    if (int rc = need_map(p, fn)) return rc;
    const int64_t Ni = p->map_items, Nq = query_count(p), L = p->map_L;
    if (what != 1 && Ni != Nq) return fail(L3_EINVAL, std::string(fn) + ": the list and rank modes are timed with as many items as queries");
    if (Ni > MAP_MAX_ROWS / std::max(Nq, L)) return fail(L3_EINVAL, std::string(fn) + ": too many items to time in one launch");
    int rc = L3_OK;
    // midx: the diagonal (Ni), work (3 Ni), arg (Ni Nq | Ni) or counts (2 Ni); mout: peaks (Ni Nq | Ni), maps (Ni L) or truth peaks
    const size_t n_idx = (size_t)4 * Ni + (what == 1 ? (size_t)Ni * Nq : (size_t)2 * Ni);
    const size_t n_out = what == 1 ? (size_t)Ni * Nq : (size_t)Ni + (what == 0 ? (size_t)Ni * L : (size_t)Ni);
    if ((rc = pairs_grow(p, &p->midx, &p->cap_midx, n_idx, fn))) return rc;
    if ((rc = pairs_grow(p, &p->mout, &p->cap_mout, n_out, fn))) return rc;
    int32_t *d_diag = p->midx, *d_work = d_diag + Ni, *d_int = d_work + 3 * Ni;
    float *d_peak = p->mout, *d_more = p->mout + Ni;
    if (what != 1) {
        std::vector<int32_t> host((size_t)4 * Ni);
        for (int64_t i = 0; i < Ni; ++i) host[(size_t)i] = (int32_t)i, host[(size_t)(Ni + 3 * i)] = (int32_t)i, host[(size_t)(Ni + 3 * i + 1)] = (int32_t)i, host[(size_t)(Ni + 3 * i + 2)] = 1;
        if (hipMemcpyAsync(d_diag, host.data(), host.size() * 4, hipMemcpyHostToDevice, p->s) != hipSuccess || !pairs_finished(p->s))
            return fail(L3_EHIP, std::string(fn) + ": copy to the device failed");
    }
    if (what == 2) {          // s_item = s_query = the diagonal's peaks
        launch_list(p->M, query_rows(p), p->wd, p->bd, p->head, (int)L, d_work, Ni, d_diag, nullptr, d_peak, nullptr, p->s);
        if (hipMemsetAsync(d_int, 0, (size_t)2 * Ni * 4, p->s) != hipSuccess) return fail(L3_EHIP, std::string(fn) + ": memset failed");
    }
    auto run = [&](int n) {
        for (int r = 0; r < n; ++r) {
            if (what == 0) launch_list(p->M, query_rows(p), p->wd, p->bd, p->head, (int)L, d_work, Ni, d_diag, d_more, d_peak, d_int, p->s);
            else if (what == 1) launch_peaks(p->M, query_rows(p), p->wd, p->bd, p->head, (int)L, 0, Ni, 0, Nq, d_peak, d_int, p->s);
            else launch_ranks(p->M, query_rows(p), p->wd, p->bd, p->head, (int)L, Ni, Nq, d_peak, d_peak, nullptr, nullptr, d_int, d_int + Ni, p->s);
        }
    };
    hipEvent_t a, b;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return fail(L3_EHIP, std::string(fn) + ": hipEventCreate failed");
    run(1);
    float t = 0.0f;
    if (hipEventRecord(a, p->s) != hipSuccess) rc = fail(L3_EHIP, std::string(fn) + ": hipEventRecord failed");
    run(reps);
    if (rc == L3_OK && (hipEventRecord(b, p->s) != hipSuccess || !pairs_finished(p->s) || hipEventElapsedTime(&t, a, b) != hipSuccess))
        rc = fail(L3_EHIP, std::string(fn) + ": the timed launches failed");
    *ms = (double)t / reps;
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    return rc;
}

// The kernels alone on projected rows from the host: m (n_items L, H) location-major, t (n_q, H) the queries.
static int op_map_check(const char* fn, const float* m, const float* t, const float* wd, int64_t n_items, int64_t L, int64_t n_q, int H) {
    if (!m || !t || !wd) return fail(L3_EINVAL, std::string(fn) + ": m, t and wd must not be NULL");
    if (n_items < 1 || L < 1 || n_q < 1 || L > MAP_MAX_ROWS || n_items > MAP_MAX_ROWS / L || n_q > MAP_MAX_ROWS || !pairs_head_ok(H))
        return fail(L3_EINVAL, std::string(fn) + ": need n_items, L, n_q >= 1, n_items L <= 2^31 - 65 and H a multiple of 32 in [32, 4096]");
    return L3_OK;
}

int l3_op_map_list(int device, const float* m, const float* t, const float* wd, float bd, int64_t n_items, int64_t L, int64_t n_q, int H,
                   const int64_t* item_ptr, const int32_t* query_idx, float* maps, float* peak, int32_t* arg) {
    const char* fn = "l3_op_map_list";
    if (int rc = op_map_check(fn, m, t, wd, n_items, L, n_q, H)) return rc;
    if (!item_ptr || !query_idx) return fail(L3_EINVAL, std::string(fn) + ": item_ptr and query_idx must not be NULL");
    if (!maps && !peak && !arg) return fail(L3_EINVAL, std::string(fn) + ": maps, or peak / arg, or all of them are needed");
    std::vector<int32_t> work;
    const std::string why = list_work(item_ptr, query_idx, n_items, n_q, L, maps != nullptr, &work);
    if (!why.empty()) return fail(L3_EINVAL, std::string(fn) + ": " + why);
    if (!device_ok(device)) return fail(L3_EHIP, no_gpu_message(fn, device));
    const int64_t n = item_ptr[n_items], nw = (int64_t)work.size() / 3;
    DeviceBufs bufs;
    float* dm = bufs.put(m, (size_t)n_items * L * H, nullptr);
    float* dt = bufs.put(t, (size_t)n_q * H, nullptr);
    float* dw = bufs.put(wd, (size_t)H, nullptr);
    int32_t* dwork = bufs.put(work.data(), work.size(), nullptr);
    int32_t* dq = bufs.put(query_idx, (size_t)n, nullptr);
    float* dmaps = maps ? bufs.alloc<float>((size_t)n * L) : nullptr;
    float* dpeak = bufs.alloc<float>((size_t)n);
    int32_t* darg = bufs.alloc<int32_t>((size_t)n);
    if (!bufs.ok()) return fail(L3_ENOMEM, std::string(fn) + ": device allocation or upload failed");
    launch_list(dm, dt, dw, bd, H, (int)L, dwork, nw, dq, dmaps, dpeak, darg, nullptr);
    bool ok = true;
    if (maps) ok = ok && hipMemcpy(maps, dmaps, (size_t)n * L * 4, hipMemcpyDeviceToHost) == hipSuccess;
    if (peak) ok = ok && hipMemcpy(peak, dpeak, (size_t)n * 4, hipMemcpyDeviceToHost) == hipSuccess;
    if (arg) ok = ok && hipMemcpy(arg, darg, (size_t)n * 4, hipMemcpyDeviceToHost) == hipSuccess;
    if (!ok || hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess)
        return fail(L3_EHIP, std::string(fn) + ": the kernel or the copy from the device failed");
    return L3_OK;
}

int l3_op_map_peaks(int device, const float* m, const float* t, const float* wd, float bd, int64_t n_items, int64_t L, int64_t n_q, int H,
                    int64_t i0, int64_t i1, int64_t j0, int64_t j1, float* S, int32_t* arg) {
    const char* fn = "l3_op_map_peaks";
    if (int rc = op_map_check(fn, m, t, wd, n_items, L, n_q, H)) return rc;
    if (!S) return fail(L3_EINVAL, std::string(fn) + ": S is NULL");
    if (i0 < 0 || i1 > n_items || i0 >= i1 || j0 < 0 || j1 > n_q || j0 >= j1 || i1 - i0 > MAP_MAX_ROWS / (j1 - j0))
        return fail(L3_EINVAL, std::string(fn) + ": the block [" + std::to_string(i0) + ", " + std::to_string(i1) + ") x [" + std::to_string(j0) + ", " +
                                   std::to_string(j1) + ") is empty, too large or outside the " + std::to_string(n_items) + " items x " + std::to_string(n_q) + " queries");
    if (!device_ok(device)) return fail(L3_EHIP, no_gpu_message(fn, device));
    const size_t count = (size_t)(i1 - i0) * (size_t)(j1 - j0);
    DeviceBufs bufs;
    float* dm = bufs.put(m, (size_t)n_items * L * H, nullptr);
    float* dt = bufs.put(t, (size_t)n_q * H, nullptr);
    float* dw = bufs.put(wd, (size_t)H, nullptr);
    float* dS = bufs.alloc<float>(count);
    int32_t* darg = bufs.alloc<int32_t>(count);
    if (!bufs.ok()) return fail(L3_ENOMEM, std::string(fn) + ": device allocation or upload failed");
    launch_peaks(dm, dt, dw, bd, H, (int)L, i0, i1, j0, j1, dS, darg, nullptr);
    bool ok = hipMemcpy(S, dS, count * 4, hipMemcpyDeviceToHost) == hipSuccess;
    if (arg) ok = ok && hipMemcpy(arg, darg, count * 4, hipMemcpyDeviceToHost) == hipSuccess;
    if (!ok || hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess)
        return fail(L3_EHIP, std::string(fn) + ": the kernel or the copy from the device failed");
    return L3_OK;
}

}  // extern "C"
