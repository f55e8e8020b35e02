// pairs.h -- the l3_pairs handle of csrc/pairs.hip: the AVC head factored over (frame, second) pairs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "host_common.h"

struct l3_pairs {
    int device = 0;
    int nv = 0, na = 0, head = 0;
    hipStream_t s = nullptr;
    l3::DeviceBufs bufs;
    // the head: dense_1 as it is, dense_2 as the difference of its two columns
    float *w1 = nullptr, *b1 = nullptr, *wd = nullptr;
    float bd = 0.0f;
    bool head_set = false;
    // the projected sets: U (Nv, head) = V W1v, T (Na, head) = A W1a + b1; 0 rows: not set
    float *U = nullptr, *T = nullptr;
    size_t cap_U = 0, cap_T = 0;
    int64_t Nv = 0, Na = 0;
    // scratch, grown on demand
    float* rows = nullptr;          // host rows on their way to a projection
    size_t cap_rows = 0;
    float* out = nullptr;           // a block of the matrix, listed margins, truth scores
    size_t cap_out = 0;
    int32_t* idx = nullptr;         // pair lists, groups, rank counts
    size_t cap_idx = 0;
    // the location map of one side (csrc/locmap.hip): M (map_items * map_L, head), the projected location rows
    // of map_items items, location-major; map_side -1: none reserved.  A set_head voids what was put, not the reservation.
    int map_side = -1, map_H = 0, map_W = 0;
    int64_t map_items = 0, map_L = 0, map_done = 0;          // map_done: items that have been put
    std::vector<uint8_t> map_put;                            // per item: put since the last reserve / set_head
    float* M = nullptr;
    size_t cap_M = 0;
    float* mout = nullptr;          // maps, peaks and truth peaks on their way to the host
    size_t cap_mout = 0;
    int32_t* midx = nullptr;        // work lists, query indices, arg-max, groups, rank counts
    size_t cap_midx = 0;
};

namespace l3 {
void pairs_project(const float* x, int64_t ldx, const float* w, const float* b, float* y, int64_t n, int K, int H, hipStream_t s);
bool pairs_head_ok(int H);
bool pairs_finished(hipStream_t s);
int pairs_enter(l3_pairs* p, const char* fn);
int pairs_grow(l3_pairs* p, float** buf, size_t* cap, size_t count, const char* fn);
int pairs_grow(l3_pairs* p, int32_t** buf, size_t* cap, size_t count, const char* fn);
}  // namespace l3
