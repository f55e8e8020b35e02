// pca.h -- the l3_pca handle of csrc/pca.hip: mean, scatter matrix and projections of resident embedding rows.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "host_common.h"

struct l3_pca {
    int device = 0;
    int D = 0;
    hipStream_t s = nullptr;
    l3::DeviceBufs bufs;
    // the fitted rows X (n, D), their mean in float64 and its float32 rounding, the first row that is not finite
    float* X = nullptr;
    size_t cap_X = 0;
    int64_t n = 0;
    double* m64 = nullptr;
    float* m32 = nullptr;
    bool has_mean = false;
    unsigned long long* bad = nullptr;
    // scratch of the mean (segment sums) and of the scatter (one float64 D x D partial per split), and the scatter matrix
    double *seg = nullptr, *part = nullptr, *S = nullptr;
    size_t cap_seg = 0, cap_part = 0, cap_S = 0;
    bool has_S = false;          // S is the result of a finished l3_pca_scatter of the rows and the mean the handle holds now
    // the model: k components W (k, D), their transpose WT (D, k), the model's mean and, when whitening, scale (k)
    int k = 0;
    float *W = nullptr, *WT = nullptr, *mean = nullptr, *scale = nullptr;
    size_t cap_W = 0, cap_WT = 0, cap_scale = 0;
    bool has_scale = false;
    // other rows (l3_pca_transform / l3_pca_inverse from the host): their copy and the result
    float *P = nullptr, *Y = nullptr;
    size_t cap_P = 0, cap_Y = 0;
};

// the scatter matrix (D, D) that the last l3_pca_scatter left on the device, or nullptr when there is none: what l3_eig_set_matrix_pca
// (eig.hip) copies, so that the eigensolver starts from S without a trip through the host
inline const double* pca_resident_scatter(const l3_pca* h) { return h->has_S ? h->S : nullptr; }
