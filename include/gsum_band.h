/* gsum_band.h -- Gram matrices and log determinants of symmetric positive definite band matrices on an AMD Instinct GPU (gfx950):
 * libgsum_band.so.
 *
 * A stationary kernel with a short length scale on sorted one-dimensional points gives a kernel matrix that is banded in fp64: the
 * exponential is exactly 0.0 beyond 745 in its argument (RBF: from 38.6 length scales on).  A band Cholesky of half-bandwidth b costs
 * n b^2 operations on n (b + 1) doubles, where the dense factorisation costs n^3 / 3 on n^2; the points need not be uniform.  A
 * separate library from libgsum_hip.so and the other side libraries: it shares no state with them.  Every call is synchronous at
 * return and returns 0 on success; on failure it returns nonzero and gsum_band_last_error() (per thread) says why, naming the
 * argument.  Nothing falls back to the host.
 *
 * BAND LAYOUT (LAPACK's lower band storage, dpbtrf with uplo = 'L', seen row-major): per matrix AB[k, j] = A[j + k, j], k = 0 .. b,
 * j = 0 .. n - 1, as (b + 1) x n row-major doubles: row k is the k-th sub-diagonal.  Entries with j + k >= n are ignored on input and
 * zero on output.  m matrices are m such blocks one after the other, all at the same b.
 *
 * LIMITS, constants of the library (the handle may be NULL):
 *   gsum_band_max_halfwidth  the widest b (GSUM_BAND_MAX_HALFWIDTH): the rows under a diagonal block are one thread each of one workgroup.
 *   gsum_band_block          the columns the factorisation advances per step (GSUM_BAND_BLOCK).
 *
 * gsum_band_open makes a handle on a device (a stream and buffers that grow with the calls); gsum_band_close frees it (NULL allowed).
 *
 * gsum_band_width: descs are m kernel descriptors (gsum_hip.h), X the n points (one feature).  width_out[i] = the smallest b such that
 *   every entry K_i(x_j, x_{j+k}), 1 <= k <= max_halfwidth + 1, whose bits are not +-0 (NaN and Inf count as nonzero) has k <= b; it is
 *   max_halfwidth + 1 when there is no such b within the limit.  n * (max_halfwidth + 1) entries per descriptor are evaluated and
 *   nothing else.  PREMISE of a caller that takes width_out for the half-bandwidth of the whole matrix: the kernel does not increase
 *   with |x_i - x_j| and X is sorted, so that zeros at k = b + 1 .. max_halfwidth + 1 are followed by zeros only.  The library checks
 *   neither.  nugget is accepted for symmetry with gsum_band_build; it sits on the diagonal and moves no width.
 *
 * gsum_band_build: the bands of the m kernel matrices at half-bandwidth b, kept on the device for the next gsum_band_gram and, when
 *   AB_out is not NULL, copied to the host (m x (b + 1) x n).  AB[k, j], k >= 1, is the two-argument kernel value between x_{j+k} and
 *   x_j with the arithmetic of the dense device build (gsum_kernel_build of libgsum_hip.so with Y = X): bit for bit its entry
 *   [j + k, j], for flattened descriptors and trees.  AB[0, j] is the one-argument diagonal (every stationary leaf exactly 1,
 *   WhiteKernel noise included) plus nugget.  Whatever the kernel has beyond diagonal b is dropped: the caller chooses b.
 *
 * gsum_band_gram: AB as above, or NULL for the bands the last gsum_band_build left on the device (its m, n and b must be the ones
 *   given).  Z is n x (n_sets * cols) column-major: n_sets sets of cols right-hand sides, 1 <= cols <= GSUM_BAND_MAX_COLS, shared by
 *   the matrices.  Per matrix i < m, with A_i = L L^T its band Cholesky factorisation and Y = L^-1 Z:
 *     G_out[i, s]  = Y_s^T Y_s = Z_s^T A_i^-1 Z_s      (m x n_sets x cols x cols row-major; bitwise symmetric)
 *     sld_out[i]   = sum_j log L_jj                      (half the log determinant)
 *     info_out[i]  = LAPACK dpbtrf's info: 0, or the 1-based order of the first leading minor whose pivot is not finite and positive
 *                    (a NaN fails the comparison).  Then G_out[i] and sld_out[i] are NaN; the other matrices are not disturbed.
 *     L_out        = the factors in the band layout (m x (b + 1) x n), or NULL.  What it holds where info_out[i] != 0 is unspecified.
 *   The bands on the device are not changed: the factorisation works on a copy.
 *   ORDER.  The factorisation is right-looking in blocks of gsum_band_block columns: the diagonal block, the at most b rows under it,
 *   then the window those rows span, updated on v_mfma_f64_16x16x4_f64 from the band in device memory.  Every sum has an order fixed by
 *   n and the block alone, and a term that is exactly zero leaves its sum as it is: G, sld, info and L of a matrix are bitwise
 *   reproducible, do not depend on m, on the other matrices of the call, on their order or on the chunking, and are the same when the
 *   band is stored with further all-zero diagonals (a larger b).  sld sums the binary exponents of L_jj as integers and the
 *   logarithms of the fractions in [sqrt(1/2), sqrt(2)) separately.
 *   CHUNKS.  m matrices go through in chunks whose bands hold fewer than 2^31 doubles and whose solved columns stay within 2^27
 *   doubles (one matrix and one set at least); the sets of one matrix are chunked likewise.  n is limited by memory only.
 *   gsum_band_set_chunk lowers the number of doubles a chunk's bands, and its solved columns, may hold (tests; < 1 or >= 2^31 restores
 *   the default).
 *
 * gsum_band_forward: Y_out[i] = L_i^-1 Z for m factors in the band layout; Z is n x ncols column-major, ncols >= 1 without an upper
 *   limit but n * ncols < 2^31; Y_out is m blocks of n x ncols column-major.  The substitution of gsum_band_gram, bit for bit.
 *
 * gsum_band_times: ms[0..5] = device time in milliseconds (HIP events) the handle has spent so far in: 0 host-to-device copies, 1 the
 *   width search and the build, 2 the factorisation (with sld and the copy of resident bands), 3 the forward substitution, 4 the Gram
 *   matrices, 5 device-to-host copies.  reset != 0 zeroes them.
 *
 * REFUSED, before a device is touched: null pointers (AB of gsum_band_gram, AB_out and L_out excepted); m, n, n_sets, ncols < 1; b < 0 or
 *   b > gsum_band_max_halfwidth; cols outside 1 .. GSUM_BAND_MAX_COLS; n * (b + 1) >= 2^31 or n * cols >= 2^31 (one matrix, one
 *   set: the smallest chunk); a descriptor with a length scale per feature (anisotropic: more than one feature).  The handle is
 *   bound to one device and is not thread-safe.
 */
#ifndef GSUM_BAND_H
#define GSUM_BAND_H
#include <stdint.h>

#include "gsum_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define GSUM_BAND_MAX_HALFWIDTH 255
#define GSUM_BAND_BLOCK 16
#define GSUM_BAND_MAX_COLS 16

typedef struct gsum_band gsum_band;

const char* gsum_band_last_error(void);
int gsum_band_open(int32_t device, gsum_band** out);
void gsum_band_close(gsum_band* h);
int32_t gsum_band_max_halfwidth(const gsum_band* h);
int32_t gsum_band_block(const gsum_band* h);
int gsum_band_set_chunk(gsum_band* h, int64_t max_elements);
int gsum_band_width(gsum_band* h, const gsum_kernel_desc* descs, int64_t m, const double* X, int64_t n, double nugget, int32_t* width_out);
int gsum_band_build(gsum_band* h, const gsum_kernel_desc* descs, int64_t m, const double* X, int64_t n, double nugget, int32_t b,
                    double* AB_out);
int gsum_band_gram(gsum_band* h, const double* AB, int64_t m, int64_t n, int32_t b, const double* Z, int64_t n_sets, int32_t cols,
                   double* G_out, double* sld_out, int32_t* info_out, double* L_out);
int gsum_band_forward(gsum_band* h, const double* L, int64_t m, int64_t n, int32_t b, const double* Z, int64_t ncols, double* Y_out);
int gsum_band_times(gsum_band* h, double* ms, int32_t reset);

#ifdef __cplusplus
}
#endif
#endif
