/* gsum_loo.h -- leave-one-out and leave-group-out diagnostics from one Cholesky factor on an AMD Instinct GPU (gfx950): libgsum_loo.so.
 *
 * With K = L L^T, r = y - mean, a = K^-1 r and p = diag(K^-1), every leave-one-out quantity is closed-form (Rasmussen & Williams
 * 5.4.2): loo_mean_i = y_i - a_i / p_i, loo_var_i = 1 / p_i.  This library forms W = L^-1 on the device once, reduces
 * p_j = sum_{i >= j} W_ij^2 from it and applies a = W^T (W r) to any number of curves.  A separate library from libgsum_hip.so,
 * libgsum_vario.so, libgsum_refdist.so and libgsum_pointwise.so: it shares no state with them.  Every call is synchronous at return
 * and returns 0 on success; on failure it returns nonzero and gsum_loo_last_error() (per thread) says why.  Nothing falls back to
 * the host.  Every sum has one fixed order and there are no floating-point atomics, so results are bitwise reproducible from call
 * to call, and a column of alpha does not depend on which other columns are in the call.
 *
 * gsum_loo_open takes the n x n row-major lower factor L from the host (the upper triangle is never read), pads it to a multiple
 *   of 128 with an identity tail and inverts it by blocked recursive doubling: every 128 x 128 diagonal block by substitution, then
 *   level by level W21 = -W22 (L21 W11) for neighbouring pairs, followed by one step of refinement W21 -= W22 (L21 W11 + L22 W21),
 *   as fp64 MFMA products that skip the tiles that are structurally zero.  L and the product scratch are freed before it returns; W stays resident (8 N^2 bytes, N = n rounded up to 128).
 *   Refused with a message, before anything is read or allocated: null pointers, n < 1, and an n whose three padded matrices do not
 *   fit the device's free memory.  Refused after the first kernel, which checks the diagonal on the device: an L_ii that is not a
 *   finite positive number (the message names the first such row).
 *
 * gsum_loo_precision_diag: p[n] = diag((L L^T)^-1) and *sum_log_diag = sum_i log L_ii (both were reduced on the device by open).
 *
 * gsum_loo_solve: alpha = (L L^T)^-1 R for R n x k row-major, any k >= 1 (the columns go through the device in chunks).  alpha may
 *   not alias R.  Refused: null pointers, k < 1.
 *
 * gsum_loo_times: ms[0..5] = device time in milliseconds (HIP events) the object has spent so far in: 0 the upload of L,
 *   1 the inverse, 2 the reduction of p, 3 the uploads of R, 4 the two products of solve, 5 the downloads of alpha.  reset != 0
 *   zeroes them.
 *
 * Leave-group-out (k-fold, leave-a-block-out): with P = K^-1 = W^T W, every point of a group G is predicted from the points outside
 * it by  y_G - E[y_G | y_-G] = P_GG^-1 a_G  and  Cov[y_G | y_-G] = P_GG^-1.  The library gathers the group's columns of W, forms
 * P_GG on the fp64 MFMA, factors it P_GG = C C^T by a blocked right-looking Cholesky factorisation and inverts C the way open inverts
 * L; the log-determinant gets the first-order correction tr(V P_GG V^T) - g, V = C^-1, from the gathered columns themselves; many groups go through every kernel together, in chunks sized to the device's free memory.
 *
 * gsum_loo_precision_block: P (g x g row-major) = the rows and columns idx[0 .. g) of (L L^T)^-1, in the order idx lists them.
 *   Refused before anything is launched or allocated: g < 1, null pointers, g > n, an index outside 0 .. n - 1, an index that
 *   appears twice, and a block whose N x g panel does not fit the device's free memory (the message names g).
 *
 * gsum_loo_folds: the n points are split into n_folds groups, group q being fold_idx[fold_ptr[q] .. fold_ptr[q + 1]).  For the
 *   residual curves R (n x k row-major, r = y - mean) it writes, in the caller's row order, resid (n x k) = y - E[y | the other
 *   groups] and var (n) = the marginal predictive variances, and per group md2 (n_folds x k) = the squared Mahalanobis distance of
 *   the group's residual under its predictive distribution and logdet (n_folds) = log det Cov[y_G | y_-G].
 *   Refused before anything is launched or allocated: n_folds < 1, k < 1, null pointers, n_folds > n, a fold_ptr that does not
 *   start at 0, end at n and increase strictly, a fold_idx that is not a permutation of 0 .. n - 1, and a single group whose
 *   buffers do not fit (the message names the group and its size).  No index reaches a kernel unchecked; a group's indices are
 *   sorted inside the library.  A group whose block does not factor (a pivot that is not a finite positive number: the message
 *   names the group and the row inside it, counted along its ascending indices) ends the call with a nonzero status, and nothing
 *   is written to the four outputs; the object stays usable.
 *   Reproducibility: as everywhere in this library, results are bitwise the same from call to call.  A group's outputs depend on
 *   its set of indices alone: not on the order the caller lists them in, not on the other groups of the call or their order, and
 *   not on how the groups were cut into chunks.  A curve's outputs do not depend on the other curves of the call.
 *
 * gsum_loo_fold_budget: the bytes one chunk of groups may take in gsum_loo_folds from now on; 0 (the start) is what hipMemGetInfo
 *   leaves free at the call.  For tests and measurements of the chunking.  Refused: a null handle, bytes < 0.
 *
 * gsum_loo_fold_times: ms[0..6] = device time in milliseconds of the two calls above, by phase: 0 the gathers (columns of W, rows
 *   of alpha), 1 the block Gram products, 2 the Cholesky factorisation, 3 the inverse of the factors, 4 the correction of the
 *   log-determinants, 5 the two products with a and the reductions, 6 the scatter and the downloads.  The solve a = K^-1 R of
 *   gsum_loo_folds is charged to phases 3 and 4 of gsum_loo_times.  reset != 0 zeroes them.
 */
#ifndef GSUM_LOO_H
#define GSUM_LOO_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gsum_loo gsum_loo;

const char* gsum_loo_last_error(void);
int gsum_loo_open(const double* L, int64_t n, int device, gsum_loo** out);
int gsum_loo_precision_diag(gsum_loo* h, double* p, double* sum_log_diag);
int gsum_loo_solve(gsum_loo* h, const double* R, int64_t k, double* alpha);
int gsum_loo_times(gsum_loo* h, double* ms, int32_t reset);
int gsum_loo_precision_block(gsum_loo* h, const int64_t* idx, int64_t g, double* P);
int gsum_loo_folds(gsum_loo* h, const int64_t* fold_ptr, const int64_t* fold_idx, int64_t n_folds, const double* R, int64_t k,
                   double* resid, double* var, double* md2, double* logdet);
int gsum_loo_fold_budget(gsum_loo* h, int64_t bytes);
int gsum_loo_fold_times(gsum_loo* h, double* ms, int32_t reset);
void gsum_loo_free(gsum_loo* h);

#ifdef __cplusplus
}
#endif
#endif
