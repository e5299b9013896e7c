/* gsum_loo.h -- leave-one-out diagnostics from one Cholesky factor on an AMD Instinct GPU (gfx950): libgsum_loo.so.
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
void gsum_loo_free(gsum_loo* h);

#ifdef __cplusplus
}
#endif
#endif
