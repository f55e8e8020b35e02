// tsne.h -- the l3_tsne handle of csrc/tsne.hip: exact t-SNE of n points in the plane over a sparse symmetric P.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "host_common.h"

// the two scalars of an iteration, which stay on the device: Z for the update kernel, the KL part for a record
struct l3_tsne_scalars {
    double Z;           // sum of z_i in the run order
    double kl_rows;     // sum over rows of sum_j P_ij log1p(d_ij^2) in the run order
};

struct l3_tsne {
    int device = 0;
    int64_t n = 0;
    int row_block = 0, segments = 0, runs_per_segment = 0;          // l3_tsne_geometry(n)
    hipStream_t s = nullptr;
    l3::DeviceBufs bufs;
    // the map y (n, 2), its last update u and the gains, float32
    float *Y = nullptr, *U = nullptr, *G = nullptr;
    bool has_embedding = false;
    // P as CSR: indptr (n + 1), cols, vals; sum P log P from the host
    int64_t* indptr = nullptr;
    int32_t* cols = nullptr;
    float* vals = nullptr;
    size_t cap_cols = 0, cap_vals = 0;
    bool has_affinities = false;
    double plogp = 0.0;
    // one iteration's float64 terms: the segments' partials (segments, n, 3), R (n, 2), z (n), A (n, 2), the rows' KL parts (n),
    // the run totals of z and of the KL parts
    double *part = nullptr, *R = nullptr, *z = nullptr, *A = nullptr, *klrow = nullptr, *runs = nullptr;
    l3_tsne_scalars* scal = nullptr;
    int64_t iteration = 0;          // iterations run since l3_tsne_set_embedding
};
