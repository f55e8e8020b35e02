// kmeans.h -- the l3_kmeans handle of csrc/kmeans.hip: Lloyd's k-means over resident embedding rows.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "host_common.h"

// what an assignment leaves for the host: the handful of scalars of an iteration
struct l3_kmeans_stats {
    double inertia;
    unsigned long long changed;
    long long empty, valid;
};

struct l3_kmeans {
    int device = 0;
    int D = 0, K = 0;
    hipStream_t s = nullptr;
    l3::DeviceBufs bufs;
    // the rows X (n, D), nn(x), their labels (-2 before the first assignment) and distances to their centroid
    float *X = nullptr, *nnX = nullptr, *mind = nullptr;
    int32_t* labels = nullptr;
    size_t cap_X = 0, cap_nnX = 0, cap_mind = 0, cap_labels = 0;
    int64_t n = 0;
    // the centroids C (K, D) and nn(c)
    float *C = nullptr, *nnC = nullptr;
    bool has_centroids = false;
    bool sorted = false;          // ids / start / runoff / count hold the stable sort of the current labels
    // other rows (l3_kmeans_predict): their copy, nn(x), labels and distances
    float *P = nullptr, *nnP = nullptr, *pd = nullptr;
    int32_t* pl = nullptr;
    size_t cap_P = 0, cap_nnP = 0, cap_pd = 0, cap_pl = 0;
    int64_t nP = 0;
    // scratch of the sort and the sums, grown on demand
    int32_t *hist = nullptr, *count = nullptr, *start = nullptr, *runoff = nullptr, *ids = nullptr;
    size_t cap_hist = 0, cap_count = 0, cap_start = 0, cap_runoff = 0, cap_ids = 0;
    double *part = nullptr, *runs = nullptr;
    size_t cap_part = 0, cap_runs = 0;
    int64_t* chosen = nullptr;          // K seed rows
    double* u = nullptr;                // K uniform draws
    l3_kmeans_stats* stats = nullptr;
    int32_t* classes = nullptr;         // class indices of the rows, then file ranges as int64 pairs behind `files`
    size_t cap_classes = 0;
    int64_t* files = nullptr;
    size_t cap_files = 0;
    unsigned long long* table = nullptr;          // contingency table
    size_t cap_table = 0;
    int32_t* fh = nullptr;              // file histograms
    size_t cap_fh = 0;
};
