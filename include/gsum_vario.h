/* gsum_vario.h -- the empirical variogram of gsum.helpers.VariogramFourthRoot on an AMD Instinct GPU (gfx950): libgsum_vario.so.
 *
 * A separate library from libgsum_hip.so: it shares no state with the factorisation context.  Every call is synchronous at return
 * and returns 0 on success; on failure it returns nonzero and gsum_vario_last_error() (per thread) says why.  Nothing falls back to
 * the host.
 *
 * gsum_vario_create uploads X (n x d, row-major), Z (n_curves x n, row-major: curve c is Z[c*n .. c*n+n-1]) and the bounds, and runs
 * the pair stage: for every pair i > j (numpy.tril_indices(n, -1) order) h_ij = |X_i - X_j| bit-identical to
 * numpy.linalg.norm(X[:, None, :] - X, axis=-1) and its bin numpy.digitize(h_ij, bounds) = #{bounds <= h_ij}.  Per bin b (Nb =
 * n_bounds + 1 bins) it returns counts[b], h_sum[b] = sum of h and dij_sum[b * n_curves + c] = sum of sqrt|z_ci - z_cj|.  The sums
 * are taken in a fixed order (bitwise reproducible), not numpy's.  It keeps the pairs of every bin (tril order) and the n x n table
 * of bins (2 n^2 bytes) on the device for gsum_vario_cov.  All device memory is allocated here (gsum_vario_cov grows its tile
 * buffers before its launches when a request list needs more).
 *   Refused: n < 1 or n > 65535, d < 1 or d > 64, n_curves < 1, n_bounds < 1 or Nb > 32767, a non-finite X or bound, decreasing
 *   bounds (numpy.digitize would accept those; this library does not).  Z may hold anything: NaN propagates.
 *
 * gsum_vario_cov: for each request r, bins b1 = bin1[r], b2 = bin2[r] in [0, Nb), and each curve c,
 *   sums[r * n_curves + c] = sum over pairs p = (i, j) of b1 and q = (k, l) of b2 of corr(p, q, c) sqrt(var1 var2)
 * with gt = gamma_tilde (Nb x n_curves, NaN allowed), g(a, b) = gt[bin(a, b), c], var_b = var_factor sqrt(gt[b, c]),
 *   rho  = (g(j,k) + g(i,l) - g(i,k) - g(j,l)) / (2 sqrt(gt[b1, c] gt[b2, c]))  (left to right, bit-identical to the reference),
 *   corr = corr_factor ((1 - rho^2) 2F1(3/4, 3/4; 1/2; rho^2) - 1), 1 for rho >= 1, -1 for rho <= -1, NaN for NaN, and exactly 1
 *          when p == q.
 * The sum is NOT divided by the pair counts; a request with an empty bin gives 0.  All requests are one launch set.  Results are
 * bitwise reproducible from call to call.
 *
 * gsum_vario_corr: out[k] = corr(rho[k]) as above (the device's correlation map, elementwise, for testing).
 */
#ifndef GSUM_VARIO_H
#define GSUM_VARIO_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gsum_vario gsum_vario;

const char* gsum_vario_last_error(void);
int gsum_vario_create(int32_t device, const double* X, int64_t n, int32_t d, const double* Z, int32_t n_curves, const double* bounds,
                      int32_t n_bounds, gsum_vario** out, int64_t* counts, double* h_sum, double* dij_sum);
int gsum_vario_cov(gsum_vario* v, const double* gamma_tilde, double var_factor, double corr_factor, const int32_t* bin1,
                   const int32_t* bin2, int32_t n_pairs, double* sums);
int gsum_vario_corr(int32_t device, const double* rho, int64_t m, double corr_factor, double* out);
void gsum_vario_free(gsum_vario* v);

#ifdef __cplusplus
}
#endif
#endif
