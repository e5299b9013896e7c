/* gsum_toep.h -- Gram matrices and log determinants of symmetric positive definite Toeplitz matrices on an AMD Instinct GPU
 * (gfx950): libgsum_toep.so.
 *
 * A stationary kernel on a uniform one-dimensional grid gives a symmetric Toeplitz matrix T, fixed by its first column t.  The Schur
 * (Bareiss) recursion yields the columns of its Cholesky factor L one after the other in O(n) each; a forward substitution runs
 * beside it, so that G = Z^T T^-1 Z and sum_j log L_jj cost O(n^2 c) and nothing of size n x n is stored.  A separate library from
 * libgsum_hip.so and the other side libraries: it shares no state with them.  Every call is synchronous at return and returns 0 on
 * success; on failure it returns nonzero and gsum_toep_last_error() (per thread) says why.  Nothing falls back to the host.
 *
 * gsum_toep_open makes a handle on a device (a stream and buffers that grow with the calls); gsum_toep_close frees it (NULL is
 *   allowed).
 *
 * gsum_toep_max_n: the largest n gsum_toep_gram takes: one workgroup holds a whole generator (GSUM_TOEP_MAX_N).  h may be NULL.
 *
 * gsum_toep_gram: t is m x n row-major, one first column per row: t[0] is the diagonal of T, t[k] its k-th sub-diagonal.  Z is n x
 *   (n_sets * cols) column-major: n_sets sets of cols right-hand sides, 1 <= cols <= GSUM_TOEP_MAX_COLS.  Per first column i < m:
 *     G_out[i, s]  = Z_s^T T_i^-1 Z_s                    (m x n_sets x cols x cols, row-major; exactly symmetric)
 *     sld_out[i]   = sum_j log L_jj,  T_i = L L^T        (half the log determinant)
 *     info_out[i]  = 0, or the 1-based step at which the pivot of the recursion stops being finite and positive (t[0] <= 0 or not
 *                    finite: 1; a reflection coefficient with |rho| >= 1 or a NaN at step k: k + 1).  In exact arithmetic this is
 *                    LAPACK's potrf info of T_i.  Then sld_out[i] and G_out[i] are NaN; the other first columns are not disturbed.
 *   The generator of the recursion is carried in double-double arithmetic (about 106 bits); the forward substitution runs in fp64 with
 *   the high word of each entry of L, and what the low words contribute is summed beside each residual in an fp32 word and taken
 *   off at its pivot; every sum has a fixed order that depends on n alone: the result of a (first column, set) is bitwise
 *   reproducible and does not depend on m, on the other sets, on their order or on how the columns are chunked.
 *   Range: each right-hand-side column is scaled on the device by the power of two that brings its largest finite magnitude into
 *   [1, 2), and G is scaled back, both exactly, so the scale of Z is free as far as G itself is representable.  The scale of T is not
 *   normalised: the fp32 word holds products of lo(L) ~ 2^-53 sqrt(t[0]) and y ~ 1 / sqrt(t[0]), and a positive finite t[0] outside
 *   2^-64 .. 2^64 is refused (scale t by a power of 4: G scales by its inverse, sum_log_diag moves by n / 2 times its logarithm).
 *   Refused: null pointers, m, n, n_sets < 1, cols outside 1 .. GSUM_TOEP_MAX_COLS, n > gsum_toep_max_n, n * n_sets * cols >= 2^31,
 *   a positive finite t[0] outside 2^-64 .. 2^64.
 *
 * gsum_toep_times: ms[0..3] = device time in milliseconds (HIP events) the handle has spent so far in: 0 host-to-device copies,
 *   1 the recursion with its forward substitution, 2 the Gram matrices, 3 device-to-host copies.  reset != 0 zeroes them.
 */
#ifndef GSUM_TOEP_H
#define GSUM_TOEP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSUM_TOEP_MAX_N 8192
#define GSUM_TOEP_MAX_COLS 16

typedef struct gsum_toep gsum_toep;

const char* gsum_toep_last_error(void);
int gsum_toep_open(int32_t device, gsum_toep** out);
void gsum_toep_close(gsum_toep* h);
int64_t gsum_toep_max_n(const gsum_toep* h);
int gsum_toep_gram(gsum_toep* h, const double* t, int64_t m, int64_t n, const double* Z, int64_t n_sets, int32_t cols, double* G_out,
                   double* sld_out, int32_t* info_out);
int gsum_toep_times(gsum_toep* h, double* ms, int32_t reset);

#ifdef __cplusplus
}
#endif
#endif
