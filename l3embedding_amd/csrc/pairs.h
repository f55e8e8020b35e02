// pairs.h -- the l3_pairs handle of csrc/pairs.hip: the AVC head factored over (frame, second) pairs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

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
};
