// mlp.h -- launch functions of the downstream MLP classifier (mlp.hip): the fp32 training step of
// classifier/train.py:230-257 construct_mlp_model, Dense(512, relu) -> Dense(128, relu) -> Dense(C, softmax), L2 on the kernels,
// keras-2.0.9 Adam.  Every launch goes to the given stream and never syncs; every result is deterministic (no float atomics).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

namespace l3 {

constexpr int MLP_H1 = 512, MLP_H2 = 128;      // hidden widths of construct_mlp_model
constexpr int MLP_MAX_CLASSES = 64;            // one wave per row in the loss kernel: a class per lane
constexpr int MLP_MAX_BATCH = 4096;
constexpr int64_t MLP_PART_FLOATS = 4 << 20;   // split-K partial buffer (16 MiB)
constexpr int MLP_FWD_COUNTERS = 4096;         // one per output tile of a split-K forward launch

// ---- the member dimension ---------------------------------------------------------------------------------------------------------
// Every kernel of the step runs a group of models of one shape per launch: block row y (blockIdx.y) works on member
// (ids >> 4y) & 15, so `ids` is a table of up to MLP_MAX_MEMBERS member numbers, four bits each, in any order and with holes (the
// live members of a parameter search).  A member's pointer is the launch's pointer + member * its stride, in elements; a stride of
// 0 shares the buffer (the features, the labels, the permutation).  A member's tiles, split count, sums and counters are those of
// the launch's shape alone: what the other block rows do does not enter its result.  The launchers without a member argument run
// one member with every stride 0 (MLP_ONE_MEMBER): the same kernels.
constexpr int MLP_MAX_MEMBERS = 16;
struct MlpMembers { uint64_t ids; int n; };
constexpr MlpMembers MLP_ONE_MEMBER{0, 1};
__host__ __device__ inline int mlp_member(const MlpMembers& m, int y) { return (int)((m.ids >> (4 * y)) & 15); }
struct MlpFwdStride { int64_t x, w, b, y, part, ctr; };
struct MlpBwdStride { int64_t dy, w, h, dx; };
struct MlpCeStride { int64_t z, probs, dz, ce; };          // ce: of ce and of correct
// x, dy: per layer; p: of w, b and the four moments (one arena per member); ce: of ce and correct (acc: 2 doubles per member).
// par: MLP_MEMBER_PARS floats per member, {lr, wd, 2 wd} (null: the launch's lr_t, wd, l2x2); lr_t = lr * lr_scale.
constexpr int MLP_MEMBER_PARS = 4;
struct MlpWgStride {
    int64_t x[3], dy[3], p, w2part, ctr, ce;
    const float* par;
    float lr_scale;
};

// Y = act(X[idx] . W + b): X (rows of ldx floats; row r of the product is X row idx[r], or r when idx is null), W (K, N) row major.
// Split-K over `part` (MLP_PART_FLOATS) when the output has too few 32x32 tiles to fill the GPU; the last wave to finish a tile sums
// its partials in split order and applies the epilogue.  ctr: MLP_FWD_COUNTERS ints, zero between launches (the last wave resets).
void mlp_dense_fwd(const float* x, const int* idx, int64_t ldx, const float* w, const float* b, float* y, int rows, int K, int N,
                   int relu, float* part, int* ctr, hipStream_t s);
int mlp_fwd_splits(int rows, int K, int N);     // the split count mlp_dense_fwd picks

// dX (rows, K) = (dY (rows, N) . W^T) * [h > 0]  (h null: no mask)
void mlp_dense_bwd_x(const float* dy, const float* w, const float* h, float* dx, int rows, int K, int N, hipStream_t s);

// softmax + keras categorical_crossentropy, C <= 64, one wave per row.  labels[idx[r]] (idx null: labels[r]) is row r's class.
// probs / dz / ce / correct may each be null.  dz = d(sum of the rows' losses * gscale) / dz.
void mlp_softmax_ce(const float* z, const int* labels, const int* idx, int rows, int C, float gscale, float* probs, float* dz,
                    float* ce, float* correct, hipStream_t s);

// Per file i = rows [files[2i], files[2i + 1]) of probs (n, C), C <= 64: file_mean (n_files, C) = the float32 mean of its rows
// (sum in row order, one division) and file_pred (n_files) its first maximum.  One wave per file; either output may be null.
void mlp_file_mean(const float* probs, int C, const int64_t* files, int64_t n_files, float* file_mean, int* file_pred, hipStream_t s);
// "" when the n_files host ranges are non-empty and inside [0, n), else what is wrong with them
std::string mlp_file_ranges_error(const int64_t* files, int64_t n_files, int64_t n);

// Weight gradient of up to three Dense layers in one launch: dW = X[idx]^T . dY (K = rows), db = column sums of dY.  With
// adam != 0 the gradient never leaves registers: dW + l2x2 * W feeds the keras Adam update of adam_kernel (elementwise.hip), and
// every weight tile writes the sum of its PRE-update W^2 to w2part; the last wave sums w2part in tile order into w2out and, when
// ce is given, adds the batch's loss (mean ce + wd * sum W^2) * rows and its correct count to acc[0], acc[1] (double).
struct MlpWgLayer {
    const float* x;
    const int* idx;
    int64_t ldx;
    const float* dy;
    float *w, *b, *mw, *vw, *mb, *vb;   // adam
    float *dw, *db;                     // gradient only
    int K, N;
};
struct MlpWgrad {
    MlpWgLayer L[3];
    int nl, rows, adam;
    float l2x2, lr_t, b1, b2, eps, wd;
    const float *ce, *correct;
    double* acc;
    float* w2out;
};
int mlp_wgrad_tiles(const MlpWgrad& a);        // waves of the launch = floats of w2part
void mlp_wgrad(const MlpWgrad& a, float* w2part, int* ctr, hipStream_t s);

// The four launches over the members `mem` of a group (above): the arguments are member 0's, the strides lead to the others'.
void mlp_dense_fwd_members(const float* x, const int* idx, int64_t ldx, const float* w, const float* b, float* y, int rows, int K,
                           int N, int relu, float* part, int* ctr, const MlpMembers& mem, const MlpFwdStride& stride, hipStream_t s);
void mlp_dense_bwd_x_members(const float* dy, const float* w, const float* h, float* dx, int rows, int K, int N,
                             const MlpMembers& mem, const MlpBwdStride& stride, hipStream_t s);
void mlp_softmax_ce_members(const float* z, const int* labels, const int* idx, int rows, int C, float gscale, float* probs, float* dz,
                            float* ce, float* correct, const MlpMembers& mem, const MlpCeStride& stride, hipStream_t s);
void mlp_wgrad_members(const MlpWgrad& a, float* w2part, int* ctr, const MlpMembers& mem, const MlpWgStride& stride, hipStream_t s);

}  // namespace l3
