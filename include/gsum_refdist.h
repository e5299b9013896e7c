/* gsum_refdist.h -- reference distributions of gsum's GraphicalDiagnostic on an AMD Instinct GPU (gfx950): libgsum_refdist.so.
 *
 * The stage after the errors: a diagnostic of nref simulated curves is turned into percentile bands (numpy.sort along the points,
 * numpy.percentile across the curves) and into credible-interval coverages.  A separate library from libgsum_hip.so and
 * libgsum_vario.so: it shares no state with either.  Every call is synchronous at return and returns 0 on success; on failure it
 * returns nonzero and gsum_refdist_last_error() (per thread) says why.  Nothing falls back to the host, every result is bitwise
 * reproducible from call to call, and every call allocates the device memory it needs before its first launch.
 *
 * gsum_refdist_create uploads A (n x m, row-major float64) once; the object keeps it on the device ("the matrix") with a scratch
 * matrix of the same size.  Refused: null pointers, n < 1, m < 1, n * m >= 2^31.
 *
 * gsum_refdist_sort_columns: the matrix becomes numpy.sort(matrix, axis=0) and stays on the device; sorted (n x m), when not null,
 *   receives it.  Finite and infinite values are bit-equal to numpy's; -0.0 and +0.0 compare equal (the device puts -0.0 first);
 *   a NaN of either sign sorts last and comes back as a positive NaN with its payload (NaNs are ordered by payload among
 *   themselves: the NaN tail holds numpy's positions, not necessarily its bit patterns).  The matrix is transposed on the device
 *   (64 x 64 tiles through LDS), every column sorted as one contiguous segment, and transposed back.
 *
 * gsum_refdist_row_percentiles: out (nq x n) = numpy.percentile(matrix, q, axis=1), the default 'linear' method.  With
 *   v = (m - 1) * (q / 100), i = floor(v), g = v - i and a, b the i-th and (i+1)-th smallest of the row: a + (b - a) g, and
 *   b - (b - a)(1 - g) where g >= 0.5, every operation rounded on its own (no fused multiply-add).  A row with a NaN gives NaN.
 *   The matrix is left as it was (the rows are sorted into the scratch matrix).  Refused: nq < 1, a q outside [0, 100] or NaN.
 *
 * gsum_refdist_qq_bands = gsum_refdist_sort_columns(h, sorted) then gsum_refdist_row_percentiles(h, q, nq, bands): the bands
 *   (nq x n) of a QQ plot; with sorted == NULL the n x m sorted matrix never crosses the host link.
 *
 * gsum_refdist_coverage: counts[j * K + k] = #{ i : lower[k * n + i] < matrix[i, j] < upper[k * n + i] } (int64, m x K), both
 *   comparisons strict and false for NaN; lower, upper are K x n row-major.  The intervals need not be nested or sorted.
 *   Refused: K < 1 or K > 524280.
 *
 * Segments (columns for the sort, rows for the percentiles) of up to GSUM_REFDIST_LDS_SORT_MAX = 16384 doubles are sorted inside
 * one workgroup's LDS (128 KiB of the CU's 160 KiB; a bitonic network on order-preserving 64-bit keys).  Longer segments are
 * correct, not tuned: LDS-sorted chunks of 16384 merged by ceil(log2(chunks)) rank-and-scatter passes in global memory.
 *
 * gsum_refdist_times: ms[0..5] = device time in milliseconds (HIP events) the object has spent so far in: 0 host-to-device copies,
 * 1 transposes, 2 column sorts, 3 row sorts + percentile picks, 4 coverage, 5 device-to-host copies.  reset != 0 zeroes them.
 */
#ifndef GSUM_REFDIST_H
#define GSUM_REFDIST_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSUM_REFDIST_LDS_SORT_MAX 16384

typedef struct gsum_refdist gsum_refdist;

const char* gsum_refdist_last_error(void);
int gsum_refdist_create(int32_t device, const double* A, int64_t n, int64_t m, gsum_refdist** out);
int gsum_refdist_sort_columns(gsum_refdist* h, double* sorted);
int gsum_refdist_row_percentiles(gsum_refdist* h, const double* q, int32_t nq, double* out);
int gsum_refdist_qq_bands(gsum_refdist* h, const double* q, int32_t nq, double* bands, double* sorted);
int gsum_refdist_coverage(gsum_refdist* h, const double* lower, const double* upper, int32_t K, int64_t* counts);
int gsum_refdist_times(gsum_refdist* h, double* ms, int32_t reset);
void gsum_refdist_free(gsum_refdist* h);

#ifdef __cplusplus
}
#endif
#endif
