// knn.h -- the l3_knn handle of csrc/knn.hip: nearest neighbours among embedding rows.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "host_common.h"

struct l3_knn {
    int device = 0;
    int D = 0, metric = 0;
    hipStream_t s = nullptr;
    l3::DeviceBufs bufs;
    // the database: rows X (nX, D), their side value sX (nn(x) under sqeuclidean, r(x) under cosine), labels or none
    float *X = nullptr, *sX = nullptr;
    size_t cap_X = 0, cap_sX = 0;
    int64_t nX = 0;
    int32_t* labels = nullptr;
    size_t cap_labels = 0;
    bool has_labels = false;
    int32_t label_max = -1;
    // the queries: rows of their own, or the database's (self: Q == X, no second copy)
    float *Q = nullptr, *sQ = nullptr;
    size_t cap_Q = 0, cap_sQ = 0;
    int64_t nQ = 0;
    bool self = false;
    // scratch, grown on demand
    float* out = nullptr;           // a block of the matrix, listed distances, partial and final list distances
    size_t cap_out = 0;
    int32_t* idx = nullptr;         // pair lists, groups, partial and final list indices, sizes, votes
    size_t cap_idx = 0;
    int64_t* files = nullptr;       // file row ranges
    size_t cap_files = 0;
};
