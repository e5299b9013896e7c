/* gsum_pointwise.h -- the two heavy methods of gsum's TruncationPointwise on an AMD Instinct GPU (gfx950): libgsum_pointwise.so.
 *
 * The pointwise (uncorrelated) truncation model: the log likelihood of the expansion parameter on a whole grid of candidates in one
 * call, and the success rates of the credible-interval diagnostic.  A separate library from libgsum_hip.so, libgsum_vario.so and
 * libgsum_refdist.so: it shares no state with them.  Every call is synchronous at return and returns 0 on success; on failure it
 * returns nonzero and gsum_pointwise_last_error() (per thread) says why.  Nothing falls back to the host, every result is bitwise
 * reproducible from call to call, and every call allocates the device memory it needs before its first launch.  The work is fp64
 * vector arithmetic (divisions, integer powers, logarithms, compares); there is no matrix product in it.
 *
 * gsum_pointwise_create uploads the partial sums y (n x k, row-major float64) once, with the k integer orders and the k flags of
 *   the orders that are kept (mask[j] != 0; kp of them).  The device forms the first differences of the kept columns,
 *   y[i, j] - y[i, j - 1] and y[i, 0] itself, one rounding each as numpy.diff, and keeps only those.
 *   Refused: null pointers, n < 1, k < 1, no kept order, more than GSUM_POINTWISE_MAX_ORDERS kept orders, n * k >= 2^31.
 *
 * gsum_pointwise_loglike_grid: for every row g < G
 *     out[g] = sum_i 0.5 * df * log((df0 * scale0^2 + sum_j c_gij^2) / 2)  +  sum_B (log|ref| + S * log(ratio)),
 *   c_gij = dy[i, j] / (ref * ratio^order_j) over the kept orders, df = df0 + kp, S = the sum of the kept orders.  This is minus
 *   the part of TruncationPointwise.log_likelihood that depends on ratio and ref; the caller adds the constants.
 *   ratios is G scalars (ratio_is_row == 0; no G x n array is read) or G x n row-major (ratio_is_row != 0).
 *   refs is, by ref_mode, GSUM_POINTWISE_REF_SCALAR one number for all rows and points, _POINTS n numbers shared by all rows,
 *   _ROW_SCALAR G numbers, _ROW_POINTS G x n row-major.
 *   The second sum runs over what ratio and ref broadcast to, as the reference's does: over the n points when either is given per
 *   point, and over ONE term when both are scalars of the row.
 *   ratio^order is taken by repeated multiplication (binary exponentiation; a negative order gives the reciprocal).
 *   A row is reduced over a partition of its points and a tree that depend on n alone, with no floating-point atomics: its bits do
 *   not depend on G, on which other rows are in the call, or on the run.  Refused: null pointers, G < 1, a ref_mode not listed.
 *
 * gsum_pointwise_coverage: counts[d * kp + j] = #{ i : t_lo[d] * scale[i, j] + loc[i, j] < data[i, j] < t_hi[d] * scale[i, j] +
 *   loc[i, j] } (int64, D x kp).  loc and scale are n x kp row-major; data is n x kp (data_cols == kp) or n (data_cols == 1, the
 *   same data for every order).  Each bound is a multiply rounded, then an add rounded (never fused), as scipy forms
 *   ppf * scale + loc; both comparisons are strict and false for NaN.  The D x n x kp bounds are never stored.
 *   Refused: null pointers, D < 1 or D > 8388480, data_cols neither 1 nor kp.
 *
 * gsum_pointwise_times: ms[0..4] = device time in milliseconds (HIP events) the object has spent so far in: 0 host-to-device
 * copies, 1 first differences, 2 the grid likelihood, 3 coverage, 4 device-to-host copies.  reset != 0 zeroes them.
 */
#ifndef GSUM_POINTWISE_H
#define GSUM_POINTWISE_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSUM_POINTWISE_MAX_ORDERS 64
#define GSUM_POINTWISE_REF_SCALAR 0
#define GSUM_POINTWISE_REF_POINTS 1
#define GSUM_POINTWISE_REF_ROW_SCALAR 2
#define GSUM_POINTWISE_REF_ROW_POINTS 3

typedef struct gsum_pointwise gsum_pointwise;

const char* gsum_pointwise_last_error(void);
int gsum_pointwise_create(int32_t device, const double* y, const int32_t* orders, const int32_t* mask, int64_t n, int32_t k,
                          gsum_pointwise** out);
int gsum_pointwise_loglike_grid(gsum_pointwise* h, const double* ratios, int32_t ratio_is_row, const double* refs, int32_t ref_mode,
                                int64_t G, double df0, double scale0, double* out);
int gsum_pointwise_coverage(gsum_pointwise* h, const double* loc, const double* scale, const double* data, int32_t data_cols,
                            const double* t_lo, const double* t_hi, int32_t D, int64_t* counts);
int gsum_pointwise_times(gsum_pointwise* h, double* ms, int32_t reset);
void gsum_pointwise_free(gsum_pointwise* h);

#ifdef __cplusplus
}
#endif
#endif
