// svm_eval.h -- launchers of svm_eval.hip (what follows the pair decisions of the SVM: vote, ovr values, hinge terms, Platt
// probabilities, pairwise coupling, per-file means).  svm.hip's l3_svm_score calls them per row block.  Every pointer is device memory;
// a launcher only enqueues on `s`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace l3 {

constexpr int SVM_HINGE_CHUNK = 256;      // rows per partial sum of the hinge terms (as L3_FEAT_CHUNK_ROWS)

// dec (rows, P): pred (rows) / ovr (rows, C), or (rows) at C = 2 / hinge (rows; needs labels) / pairprob (rows, P; needs A and B);
// any output may be NULL
void svm_tail(hipStream_t s, const double* dec, int64_t rows, int C, const double* A, const double* B, const int* labels, int* pred,
              double* ovr, double* hinge, double* pairprob);
// pairprob (rows, P) -> proba (rows, C), iters (rows; may be NULL)
void svm_coupling(hipStream_t s, const double* pairprob, int64_t rows, int C, double* proba, int* iters);
// files (n_files, 2) row ranges of proba (., C) -> file_proba (n_files, C) and file_pred (n_files); either may be NULL
void svm_file_mean(hipStream_t s, const double* proba, int C, const int64_t* files, int64_t n_files, double* file_proba,
                   int* file_pred);
// out[0] = the n terms added in chunks of SVM_HINGE_CHUNK rows in row order, then the chunk sums in chunk order; partial holds
// ceil(n / SVM_HINGE_CHUNK) doubles
void svm_hinge_sum(hipStream_t s, const double* terms, int64_t n, double* partial, double* out);

}  // namespace l3
