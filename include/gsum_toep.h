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
 *   Calls of gsum_toep_gram alone are charged here.
 *
 * The gradient of a likelihood also needs tr(T^-1 dT_p) and alpha^T dT_p alpha, alpha = T^-1 Z, for the derivative dT_p of T by each
 * hyperparameter p -- itself symmetric Toeplitz, with the first column dt_p.  Both follow from x = T^-1 e_0, the first column of the
 * inverse (Gohberg-Semencul: T^-1 = (1 / x_0) [L(x) L(x)^T - L(xt) L(xt)^T], L(.) lower-triangular Toeplitz, xt = (0, x_{n-1}, ..,
 * x_1)), which Levinson's recursion in its normalised form yields from the reflection coefficients the Schur recursion has formed
 * already: a second pass of n barrier-separated steps per first column, in double-double, replaying the coefficients.  Then the sums
 * s_d = (1 / x_0) sum_m (n - d - 2 m) x_m x_{m+d} of the diagonals of T^-1 give the traces, four triangular Toeplitz products per
 * column give alpha, and a Toeplitz product and a dot product give each entry of H; every sum is accumulated in double-double in an
 * order fixed by n alone (alpha itself is rounded to fp64), so the determinism stated above for G holds for every output here.
 *
 * gsum_toep_grad: t, Z, n_sets, cols, G_out, sld_out, info_out as gsum_toep_gram, and bit for bit its results.  dt is m x P x n
 *   row-major, P >= 1 derivative columns per first column.  Per first column i:
 *     trace_out[i, p] = tr(T_i^-1 dT_ip)                                   (m x P)
 *     H_out[i, s, p]  = alpha_s^T dT_ip alpha_s,  alpha_s = T_i^-1 Z_s     (m x n_sets x P x cols x cols, exactly symmetric)
 *   info_out[i] = n + 1: the recursion went through but x is not finite.  Where info_out[i] != 0 every output of i is NaN.
 *   Refused: what gsum_toep_gram refuses, a null pointer, P < 1 or P > 65535.
 *
 * gsum_toep_solve: x_out[i] = T_i^-1 e_0 (m x n) and alpha_out[i] = T_i^-1 Z (m x n x ncols row-major; Z is n x ncols column-major,
 *   ncols >= 1 with no limit but n * ncols < 2^31).  Either output may be NULL (then so may Z, with alpha_out), not both.  info_out
 *   as above; NaN where it is not 0.  The column scaling of gsum_toep_gram applies to alpha: the scale of Z is free.
 *
 * gsum_toep_grad_times: ms[0..7] = device milliseconds spent by gsum_toep_grad and gsum_toep_solve in: 0 host-to-device copies, 1 the
 *   Schur recursion, 2 the coefficients and Levinson's recursion, 3 the Gram matrices, 4 the diagonal sums and traces, 5 the
 *   Gohberg-Semencul products (alpha), 6 the Toeplitz products and contractions of H, 7 device-to-host copies.
 *
 * The posterior of a process on such a grid needs, for q new points with the cross-covariance columns K (n x q) and the residual
 * columns Z (n x c), the column sums of squares of L^-1 K, its products with L^-1 Z and, for a predictive covariance, (L^-1 K)^T
 * (L^-1 K): the substitution of the value path, run on [K | Z], and sums over its solved columns.  Leave-one-out diagnostics need
 * p = diag(T^-1), which x = T^-1 e_0 gives by Gohberg-Semencul: p_i = (1 / x_0) sum_{r <= i} (x_r^2 - x_{n-r}^2), x_n = 0.
 *
 * gsum_toep_predict: one first column t (n).  K is n x q column-major, q >= 1; Z is n x c column-major, 0 <= c <=
 *   GSUM_TOEP_MAX_COLS (Z, cross_out and G_out may be NULL iff c == 0).  With V = L^-1 K and W = L^-1 Z:
 *     quad_out[j]     = sum_k V[k, j]^2              = K_j^T T^-1 K_j     (q)
 *     cross_out[j, b] = sum_k V[k, j] W[k, b]        = K_j^T T^-1 Z_b     (q x c row-major)
 *     cov_out[a, b]   = sum_k V[k, a] V[k, b]        = K_a^T T^-1 K_b     (q x q, or NULL: not computed; bitwise symmetric)
 *     G_out           = Z^T T^-1 Z                                        (c x c; bit for bit gsum_toep_gram's for one set)
 *     sld_out[0], info_out[0] as gsum_toep_gram gives them.  Where info_out[0] != 0 every output is NaN and the call returns 0.
 *   quad and cross are summed in double-double and rounded once, cov in fp64 on the matrix unit (v_mfma_f64_16x16x4_f64), each in
 *   an order fixed by n alone: a column's quad and cross are bitwise independent of the other columns, of their order and of q, and
 *   cov[a, b] depends on the columns a and b and on n alone.  The columns of K are scaled like those of Z, exactly.
 *   Refused: a null pointer other than those named, q < 1, c outside 0 .. GSUM_TOEP_MAX_COLS, n > gsum_toep_max_n,
 *   n * (q + c) >= 2^31, cov_out with q > 1048560, a positive finite t[0] outside 2^-64 .. 2^64.  The caller bounds the device
 *   memory: n * (q + c) doubles of solved columns twice over, and q * q with cov_out.
 *
 * gsum_toep_loo: gsum_toep_solve's schedule, and p_out[i] = diag(T_i^-1) (m x n; may not be NULL) from the same x, in double-double
 *   up to one rounding.  alpha_out (m x n x ncols) is bit for bit gsum_toep_solve's; alpha_out and Z may be NULL together.  info_out
 *   as gsum_toep_solve; NaN where it is not 0.
 *
 * gsum_toep_post_times: ms[0..6] = device milliseconds spent by gsum_toep_predict and gsum_toep_loo in: 0 host-to-device copies, 1 the
 *   Schur recursion with its substitution, 2 the coefficients and Levinson's recursion, 3 the sums quad, cross and G, 4 cov, 5 the
 *   inverse's diagonal and the Gohberg-Semencul products, 6 device-to-host copies.  The other two clocks are not charged by them.
 *
 * The panel route (opt-in; the entry points above are unchanged).  gsum_toep_gram and gsum_toep_predict keep the residuals of a few
 * right-hand sides (16, 12, 5 or 3, by n) in the registers of the workgroup that runs the recursion, and every further few columns
 * cost a second, identical recursion in another workgroup.  The recursion needs none of the columns: the entry points below run it
 * once per first column, in panels of B = gsum_toep_panel_width() columns of L, and solve all right-hand sides against each panel:
 * the B x B triangular block by the substitution of the entry points above, literally (y_k = (z_k - zc_k) (1 / hi(L_kk)), an fp64
 * FMA chain with the high words of L, the low words summed in an fp32 word beside each residual), the rows below the panel by a
 * trailing update on the matrix unit (v_mfma_f64_16x16x4_f64, the panel's columns in ascending order, never split).  Nothing n x n
 * is stored: one panel (n x B, 12 bytes an entry) per first column in flight.  The per-entry arithmetic is that of the column
 * entry points cut into panels; the results agree with theirs to the accuracy of either, not bit for bit in general;
 * sum_log_diag and info are bit for bit theirs.  A (first column, right-hand side) result is bitwise reproducible and does not
 * depend on the other columns, on their order or number, on m or on how the first columns are chunked.
 *
 * gsum_toep_panel_width: B, a compile-time constant of the library.  h may be NULL.
 *
 * gsum_toep_gram_panel: the arguments, outputs and refusals of gsum_toep_gram.  All n_sets * cols columns ride one recursion per
 *   first column; the first columns go through in chunks that keep their solved columns, panels and generator states within 1 GiB.
 *
 * gsum_toep_predict_panel: the arguments, outputs and refusals of gsum_toep_predict; [K | Z] rides one recursion.  G_out agrees with
 *   gsum_toep_gram_panel's for one set bit for bit.
 *
 * gsum_toep_panel_times: ms[0..6] = device milliseconds spent by the two in: 0 host-to-device copies, 1 the recursion, 2 the
 *   triangular blocks, 3 the trailing updates (with the scaling of the right-hand sides), 4 the sums G, quad and cross, 5 cov,
 *   6 device-to-host copies.  The other three clocks are not charged by them.
 *
 * The blocked route (opt-in; the entry points above are unchanged, and they keep refusing n > gsum_toep_max_n).  On the panel route one
 * workgroup still holds a whole generator and runs its recursion alone.  But a step is local -- u'[i] and v'[i] need u[i-1], v[i] and
 * the step's (rho, 1 / c), which need u[k] and v[k+1] alone -- so the B steps of a panel split into a lead, one wave per first column
 * that runs them on the B + 1 rows under the pivot and yields the B coefficient pairs and info, and tiles: one wave per R =
 * gsum_toep_blocked_tile_rows() rows, which loads its rows and a halo of B rows above them, replays the coefficients, stores its
 * rows of the panel's columns of L and its rows of the next state.  The state lives in device memory, two buffers of 4 n doubles
 * per first column, read from one and written to the other.  Every element sees the expressions of the panel route in its order,
 * and the panel is consumed by the panel route's own triangular block and trailing update: for n <= gsum_toep_max_n every output is
 * bit for bit that of the panel entry points.  Nothing holds a whole generator, so n is bounded by the grids alone.  Nothing n x n
 * is stored: one panel (12 n B bytes), the right-hand sides (12 bytes an entry) and 9 n + 4 B doubles per first column in flight.
 *
 * gsum_toep_blocked_max_n: the largest n the two entry points below take, GSUM_TOEP_BLOCKED_MAX_N (the trailing update's grid).  h may
 *   be NULL.
 *
 * gsum_toep_blocked_tile_rows: R, a compile-time constant of the library.  h may be NULL.
 *
 * gsum_toep_gram_blocked: the arguments, outputs and refusals of gsum_toep_gram_panel, with n <= gsum_toep_blocked_max_n in place
 *   of gsum_toep_max_n.  The first columns go through in chunks that keep their solved columns, panels, states, coefficients and
 *   diagonals within 1 GiB.  sum_log_diag is summed in the order of the entry points above, which for n > gsum_toep_max_n continues
 *   as ceil(n / 512) consecutive entries per thread of 512, then the binary tree: fixed by n alone.
 *
 * gsum_toep_predict_blocked: the arguments, outputs and refusals of gsum_toep_predict_panel, with the same limit on n.  The caller
 *   bounds the device memory: 12 n (q + c + B) bytes and q * q doubles with cov_out.
 *
 * gsum_toep_blocked_times: ms[0..7] = device milliseconds spent by the two in: 0 host-to-device copies, 1 the leads, 2 the tiles (with
 *   the formation of the state and the sum of the logarithms), 3 the triangular blocks, 4 the trailing updates (with the scaling of
 *   the right-hand sides), 5 the sums G, quad and cross, 6 cov, 7 device-to-host copies.  The other four clocks are not charged by
 *   them.
 *
 * The tiled replay (opt-in; the entry points above are unchanged, and gsum_toep_grad, gsum_toep_solve and gsum_toep_loo keep refusing
 * n > gsum_toep_max_n).  Their replay of Levinson's recursion keeps A and B of a whole first column in one workgroup.  Its step is as
 * local as the Schur step -- A'[i] and B'[i] need A[i], B[i-1] and the step's (rho, 1 / c) -- and every (rho, 1 / c) is known before it
 * starts, so a panel of B steps is independent tiles of R rows with a halo of B rows above them: one wave each, A and B in device
 * memory, two zero-filled buffers of 4 n doubles per first column, read from one and written to the other.  After step k only the
 * rows 0 .. k are nonzero, so a panel launches the tiles up to its last step's.  The coefficients are those of the blocked route,
 * whose lead overwrites them panel after panel: the entry points below keep them (4 n doubles per first column, row n - 1 both words
 * of L[n-1, n-1]).  Every element sees the expressions of the entry points above in their order: for n <= gsum_toep_max_n x, alpha,
 * p, trace, H, sum_log_diag and info are bit for bit those of gsum_toep_grad, gsum_toep_solve and gsum_toep_loo, and G that of
 * gsum_toep_gram_blocked.  The limit is gsum_toep_blocked_max_n: the kernels from x on index in 64 bits wherever a product with n or
 * the number of columns occurs, and their grids are covered by n * n_sets * cols < 2^31.  Their cost stays O(n^2) per column.
 *
 * gsum_toep_grad_blocked: the arguments, outputs and refusals of gsum_toep_grad, with n <= gsum_toep_blocked_max_n.  The first columns
 *   go through in chunks that keep what gsum_toep_gram_blocked keeps and the coefficients, the two states, x, the diagonal sums and
 *   (5 + 2 P) doubles per entry of Z within 1 GiB.
 *
 * gsum_toep_solve_blocked, gsum_toep_loo_blocked: the arguments, outputs and refusals of gsum_toep_solve and gsum_toep_loo, with the
 *   same limit.  The recursion runs without right-hand sides.  diag(T^-1) is summed in gsum_toep_loo's order, which for n >
 *   gsum_toep_max_n continues as ceil(n / 512) consecutive terms per thread of 512, then the scan: fixed by n alone.
 *
 * gsum_toep_levinson_times: ms[0..10] = device milliseconds spent by the three in: 0 host-to-device copies, 1 the leads (with the
 *   copies that keep their coefficients), 2 the Schur tiles, 3 the triangular blocks, 4 the trailing updates (with the scaling of
 *   the right-hand sides), 5 the tiled replay, 6 the Gram matrices, 7 the diagonal sums and traces, 8 the inverse's diagonal and the
 *   Gohberg-Semencul products, 9 the Toeplitz products and contractions of H, 10 device-to-host copies.  The other five clocks are
 *   not charged by them, nor this one by the other entry points.
 */
#ifndef GSUM_TOEP_H
#define GSUM_TOEP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSUM_TOEP_MAX_N 8192
#define GSUM_TOEP_MAX_COLS 16
#define GSUM_TOEP_BLOCKED_MAX_N 1048576

typedef struct gsum_toep gsum_toep;

const char* gsum_toep_last_error(void);
int gsum_toep_open(int32_t device, gsum_toep** out);
void gsum_toep_close(gsum_toep* h);
int64_t gsum_toep_max_n(const gsum_toep* h);
int gsum_toep_gram(gsum_toep* h, const double* t, int64_t m, int64_t n, const double* Z, int64_t n_sets, int32_t cols, double* G_out,
                   double* sld_out, int32_t* info_out);
int gsum_toep_times(gsum_toep* h, double* ms, int32_t reset);
int gsum_toep_grad(gsum_toep* h, const double* t, int64_t m, int64_t n, const double* dt, int64_t P, const double* Z, int64_t n_sets,
                   int32_t cols, double* G_out, double* sld_out, int32_t* info_out, double* trace_out, double* H_out);
int gsum_toep_solve(gsum_toep* h, const double* t, int64_t m, int64_t n, const double* Z, int64_t ncols, double* x_out, double* alpha_out,
                    int32_t* info_out);
int gsum_toep_grad_times(gsum_toep* h, double* ms, int32_t reset);
int gsum_toep_predict(gsum_toep* h, const double* t, int64_t n, const double* K, int64_t q, const double* Z, int32_t c, double* quad_out,
                      double* cross_out, double* cov_out, double* G_out, double* sld_out, int32_t* info_out);
int gsum_toep_loo(gsum_toep* h, const double* t, int64_t m, int64_t n, const double* Z, int64_t ncols, double* p_out, double* alpha_out,
                  int32_t* info_out);
int gsum_toep_post_times(gsum_toep* h, double* ms, int32_t reset);
int32_t gsum_toep_panel_width(const gsum_toep* h);
int gsum_toep_gram_panel(gsum_toep* h, const double* t, int64_t m, int64_t n, const double* Z, int64_t n_sets, int32_t cols, double* G_out,
                         double* sld_out, int32_t* info_out);
int gsum_toep_predict_panel(gsum_toep* h, const double* t, int64_t n, const double* K, int64_t q, const double* Z, int32_t c, double* quad_out,
                            double* cross_out, double* cov_out, double* G_out, double* sld_out, int32_t* info_out);
int gsum_toep_panel_times(gsum_toep* h, double* ms, int32_t reset);
int64_t gsum_toep_blocked_max_n(const gsum_toep* h);
int32_t gsum_toep_blocked_tile_rows(const gsum_toep* h);
int gsum_toep_gram_blocked(gsum_toep* h, const double* t, int64_t m, int64_t n, const double* Z, int64_t n_sets, int32_t cols, double* G_out,
                           double* sld_out, int32_t* info_out);
int gsum_toep_predict_blocked(gsum_toep* h, const double* t, int64_t n, const double* K, int64_t q, const double* Z, int32_t c, double* quad_out,
                              double* cross_out, double* cov_out, double* G_out, double* sld_out, int32_t* info_out);
int gsum_toep_blocked_times(gsum_toep* h, double* ms, int32_t reset);
int gsum_toep_grad_blocked(gsum_toep* h, const double* t, int64_t m, int64_t n, const double* dt, int64_t P, const double* Z, int64_t n_sets,
                           int32_t cols, double* G_out, double* sld_out, int32_t* info_out, double* trace_out, double* H_out);
int gsum_toep_solve_blocked(gsum_toep* h, const double* t, int64_t m, int64_t n, const double* Z, int64_t ncols, double* x_out,
                            double* alpha_out, int32_t* info_out);
int gsum_toep_loo_blocked(gsum_toep* h, const double* t, int64_t m, int64_t n, const double* Z, int64_t ncols, double* p_out, double* alpha_out,
                          int32_t* info_out);
int gsum_toep_levinson_times(gsum_toep* h, double* ms, int32_t reset);

#ifdef __cplusplus
}
#endif
#endif
