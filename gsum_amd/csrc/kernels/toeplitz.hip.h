// Kernels of libgsum_toep.so (gfx950 only): the Schur (Bareiss) recursion of a symmetric positive definite Toeplitz matrix T with a
// forward substitution beside it, and the Gram matrices of the solved columns.  DESIGN.md section 18.
//
// k_schur<E, C, VL, R>: one workgroup per (first column t, chunk of C right-hand-side columns).  The generator pair (u, v) of T = L L^T is
//   held in double-double (two fp64 words, error-free transformations in plain C++) in registers, E consecutive elements per thread in
//   the fixed frame: at step k, u[i] = L[i, k] for i >= k.  A step publishes the pivot pair through LDS (one barrier per step, two
//   buffers), forms rho = v[k+1] / u[k] and 1 / sqrt((1 - rho)(1 + rho)) in every thread, shifts u down by one element (register
//   moves; the element that crosses a thread boundary goes through LDS) and applies the hyperbolic rotation.  With VL (the largest
//   size class) v, which never moves, lives in LDS instead, one 16-byte slot per element, read and written by its own thread alone.
//   The residuals of the C right-hand sides live in registers beside their generator elements and take z[i] -= fl(L[i, k]) * y_k in
//   fp64.  What rounding L[i, k] to fp64 leaves out, lo(L[i, k]) * y_k, is far below an ulp of z at every step but adds up over the
//   columns to the largest error of the path on ill-conditioned matrices, so it is summed beside z in an fp32 word (24 bits of a
//   correction of a few hundred ulps) and taken off when the row becomes the pivot: y_k = (z[k] - zc[k]) * (1 / L[k, k]).  y_k is
//   written to Y (row k), so a column's values do not depend on which other columns share its chunk.
//   An element at or above the pivot is never written again, so at the end u[i] holds L[i, i]: their logarithms are summed in a
//   fixed order (E per thread, then a binary tree over the threads).
// k_colexp: the binary exponent of the largest finite magnitude of each right-hand-side column, one wave per column.  k_schur loads a
//   column scaled by that power of two (exact), so that its largest entry lies in [1, 2) and y_k and the correction word stay inside
//   fp32's range whatever the scale of Z; k_gram scales G[a, b] back by the two exponents (exact short of over- and underflow of G
//   itself).  A column of zeros, or with an infinite entry, is taken as it is.
// k_gram: G[a, b] = sum_k Y[k, a] Y[k, b] of one set of columns, one wave per (first column, set, a): lane l sums the rows l, l + 64,
//   ... in order, then a butterfly over the lanes.  The order depends on n alone.
// The gradient pieces (the comments stand at the kernels): k_schur<.., R = true> hands out the pivot pair of every
//   step, k_coeffs turns them into (rho, 1 / c), k_levinson<E> replays those into x = T^-1 e_0 in double-double, k_diagsums / k_traces
//   give tr(T^-1 dT_p), k_gs_first / k_gs_second alpha = T^-1 Z by Gohberg-Semencul, k_tprod / k_hdot alpha^T dT_p alpha.
// The posterior pieces (the comments stand at the kernels): k_pred_sums gives the column sums of squares of
//   L^-1 K and its products with L^-1 Z in double-double, k_pred_cov (L^-1 K)^T (L^-1 K) on the fp64 MFMA, k_invdiag diag(T^-1) from x.
// The panel route (the comments stand at the kernels): k_schur_panel runs k_schur's sweep without residual
//   columns and writes L in panels, k_panel_diag solves a panel's triangular block for every right-hand side, k_panel_update applies the
//   panel to the rows below on the fp64 MFMA, k_panel_load lays the scaled right-hand sides out row-major.
// The blocked route (the comments stand at the kernels): k_schur_lead runs a panel's steps on the rows under the
//   pivot and hands out their (rho, 1 / c), k_schur_tiles replays them on every row, tile by tile, from one state buffer in HBM
//   into another, and writes the panel; k_blocked_init forms the state, k_blocked_sld sums the logarithms of the diagonal.
// The tiled replay (the comments stand at the kernels): k_levinson_tiles replays a panel of (rho, 1 / c) on the
//   rows of A and B tile by tile, from one state buffer in HBM into another, k_levinson_finish divides by the last pivot and tests x,
//   k_invdiag_n is k_invdiag with E a runtime number.
// The step itself is written once, after the double-double functions: step_coeffs (rho, the failure test, 1 / c), rotate, the
//   generator from t and its state in HBM, a column of L in the panel layout, the tree of sum log L_jj.  Every recursion kernel calls
//   those, so the routes cannot differ in an expression; the order of their sweeps is their own, and the tests compare them.
// Every value is written with ordinary vector stores; there are no atomics.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

// the error-free transformations below must be evaluated as written (no a * b + c contracted into an fma behind their back)
#pragma clang fp contract(off)

namespace gt {

constexpr int kThreads = 512;                      // of a k_schur workgroup
constexpr int kMaxE = 16;                          // elements of the generator per thread, at most
constexpr int kMaxN = kThreads * kMaxE;            // 8192
constexpr int kMaxCols = 16;                       // columns of one set (GSUM_MAX_RHS)
constexpr int kWave = 64;

struct dd {
    double h, l;
};

__device__ __forceinline__ dd two_sum(double a, double b) {
    const double s = a + b, bb = s - a;
    return {s, (a - (s - bb)) + (b - bb)};
}
__device__ __forceinline__ dd quick_two_sum(double a, double b) {          // |a| >= |b|
    const double s = a + b;
    return {s, b - (s - a)};
}
__device__ __forceinline__ dd two_prod(double a, double b) {
    const double p = a * b;
    return {p, fma(a, b, -p)};
}
__device__ __forceinline__ dd dd_add(dd a, dd b) {
    dd s = two_sum(a.h, b.h);
    const dd t = two_sum(a.l, b.l);
    s.l += t.h;
    s = quick_two_sum(s.h, s.l);
    s.l += t.l;
    return quick_two_sum(s.h, s.l);
}
__device__ __forceinline__ dd dd_neg(dd a) { return {-a.h, -a.l}; }
__device__ __forceinline__ dd dd_sub(dd a, dd b) { return dd_add(a, dd_neg(b)); }
__device__ __forceinline__ dd dd_mul(dd a, dd b) {
    dd p = two_prod(a.h, b.h);
    p.l = fma(a.h, b.l, fma(a.l, b.h, p.l));
    return quick_two_sum(p.h, p.l);
}
__device__ __forceinline__ dd dd_mul_d(dd a, double b) {
    dd p = two_prod(a.h, b);
    p.l = fma(a.l, b, p.l);
    return quick_two_sum(p.h, p.l);
}
// a / b, b.h finite and not zero: three quotient digits
__device__ __forceinline__ dd dd_div(dd a, dd b) {
    const double q1 = a.h / b.h;
    dd r = dd_sub(a, dd_mul_d(b, q1));
    const double q2 = r.h / b.h;
    r = dd_sub(r, dd_mul_d(b, q2));
    const double q3 = r.h / b.h;
    const dd q = quick_two_sum(q1, q2);
    return dd_add(q, dd{q3, 0.0});
}
// 1 / sqrt(a), a.h > 0 and finite: the fp64 value and one Newton step whose residual 1 - a x^2 is taken in double-double
__device__ __forceinline__ dd dd_rsqrt(dd a) {
    const double x = 1.0 / sqrt(a.h);
    const dd r = dd_sub(dd{1.0, 0.0}, dd_mul_d(dd_mul_d(a, x), x));
    return quick_two_sum(x, x * r.h * 0.5);
}

// ---- the Schur step ---------------------------------------------------------------------------------------------------------------------
// What every route of the recursion computes with, written here and nowhere else: the kernels below differ in where the generator
// lives, how the shifted u reaches an element and which elements they keep, never in an expression.  Results come back by value:
// with reference outputs the same rotate took k_schur<8, ..> from 0 to 8 / 16 bytes of scratch per lane and <16, ..> from 104 / 112 to
// 200 / 208 (which also says why k_schur and k_schur_panel each keep their sweep loop).

// (rho, 1 / c) of a step from its pivot pair pu = u[k], pv = v[k+1].  False where !(|rho| < 1), a NaN included: T is not positive
// definite at order k + 2, the caller reports k + 2 and does not use ic.  The test reads rho.h alone.
struct coeffs {
    dd rho, ic;
    bool ok;
};
__device__ __forceinline__ coeffs step_coeffs(dd pu, dd pv) {
    const dd rho = dd_div(pv, pu);
    const bool ok = fabs(rho.h) < 1.0;
    return {rho, dd_rsqrt(dd_mul(dd_sub(dd{1.0, 0.0}, rho), dd_add(dd{1.0, 0.0}, rho))), ok};
}
struct uv {                                        // one element of the generator pair
    dd u, v;
};
// The hyperbolic rotation of one element: us = u[i-1] (u shifted down by one), v = v[i], nrho = -rho.
__device__ __forceinline__ uv rotate(dd us, dd v, dd nrho, dd ic) {
    return {dd_mul(dd_add(us, dd_mul(nrho, v)), ic), dd_mul(dd_add(v, dd_mul(nrho, us)), ic)};
}
// The generator of T from its first column tt: 1 where t0 admits none, else rs = 1 / sqrt(t0), u[i] = rs t[i] (zero beyond n) and
// v = u under the first row.
__device__ __forceinline__ int t0_bad(double t0) { return (t0 > 0.0 && t0 < INFINITY) ? 0 : 1; }
__device__ __forceinline__ dd t0_rsqrt(double t0) { return dd_rsqrt(dd{t0, 0.0}); }
__device__ __forceinline__ uv generator_from_t(const double* __restrict__ tt, dd rs, int i, int n) {
    const dd u = i < n ? dd_mul_d(rs, tt[i]) : dd{0.0, 0.0};
    return {u, i > 0 ? u : dd{0.0, 0.0}};
}
// The generator state in HBM between launches: four planes of `stride` doubles, u.h, u.l, v.h, v.l.
__device__ __forceinline__ uv state_load(const double* __restrict__ s, int64_t stride, int i) {
    return {{s[i], s[stride + i]}, {s[2 * stride + i], s[3 * stride + i]}};
}
__device__ __forceinline__ void state_store(double* __restrict__ s, int64_t stride, int i, uv g) {
    s[i] = g.u.h;
    s[stride + i] = g.u.l;
    s[2 * stride + i] = g.v.h;
    s[3 * stride + i] = g.v.l;
}
// Row i of a column of L in the panel layout: the high word in pk, the low word as fp32 in qk.
__device__ __forceinline__ void store_column(double* __restrict__ pk, float* __restrict__ qk, int i, dd u) {
    pk[i] = u.h;
    qk[i] = (float)u.l;
}
// sum log L_jj from the partial sum s of each of the kThreads threads (its consecutive entries in ascending order): the binary tree
// over the threads through red[kThreads] in LDS; thread 0 writes the sum, NaN for a first column that failed.  Every thread calls it.
__device__ __forceinline__ void sum_log_diag_tree(double* red, int tid, double s, int bad, double* __restrict__ sld) {
    red[tid] = s;
    __syncthreads();
    for (int stride = kThreads / 2; stride > 0; stride >>= 1) {
        if (tid < stride) red[tid] += red[tid + stride];
        __syncthreads();
    }
    if (tid == 0) *sld = bad ? NAN : red[0];
}

// v of a thread's E generator elements in k_schur and k_schur_panel: in registers, or with VL (the largest size class) in LDS, where
// slot points at the thread's own 16-byte slot of element 0 and element e lies kThreads slots further ([e][tid]).
template <int E, bool VL>
struct VStore {
    double (*slot)[2];
    double h[VL ? 1 : E], l[VL ? 1 : E];
    __device__ __forceinline__ dd get(int e) const {
        if constexpr (VL) return {slot[e * kThreads][0], slot[e * kThreads][1]};
        else return {h[e], l[e]};
    }
    __device__ __forceinline__ void set(int e, dd x) {
        if constexpr (VL) {
            slot[e * kThreads][0] = x.h;
            slot[e * kThreads][1] = x.l;
        } else {
            h[e] = x.h;
            l[e] = x.l;
        }
    }
};

// ze[col] = ilogb(max_k |Z[k, col]|) over the finite entries, 0 where that maximum is zero or infinite.  grid = ncols, block = kWave.
__global__ __launch_bounds__(kWave) void k_colexp(const double* __restrict__ Z, int n, int32_t* __restrict__ ze) {
    const int lane = threadIdx.x;
    const double* z = Z + (int64_t)blockIdx.x * n;
    double mx = 0.0;
    for (int k = lane; k < n; k += kWave) mx = fmax(mx, fabs(z[k]));       // fmax drops a NaN
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) mx = fmax(mx, __shfl_xor(mx, off, kWave));
    if (lane == 0) ze[blockIdx.x] = (mx > 0.0 && mx < INFINITY) ? ilogb(mx) : 0;
}

// Y is (m, n, ncols) row-major; Z is column-major n x ncols, ze its column exponents (k_colexp); t is (m, n).  grid = (chunks, m),
// block = kThreads.  Y holds the solved columns of the scaled Z.
// LDS: pub[buffer] = {u[k].h, u[k].l, v[k+1].h, v[k+1].l, z[k][0..C)}, edge[buffer][thread] = the thread's last u element.
// R (the gradient path): chunk 0 of a first column also hands out the pivot pair it publishes, steps (m, n, 4): row k = {u[k].h,
// u[k].l, v[k+1].h, v[k+1].l}, straight from LDS (four threads, a word each), so the step itself holds no more registers than the
// value path's; k_coeffs turns the rows into (rho, 1 / c).  Without R the kernel is the value path's.
template <int E, int C, bool VL, bool R>
__global__ __launch_bounds__(kThreads) void k_schur(const double* __restrict__ t, int n, const double* __restrict__ Z,
                                                     const int32_t* __restrict__ ze, int ncols, double* __restrict__ Y,
                                                     double* __restrict__ sld, int32_t* __restrict__ info, double* __restrict__ steps) {
    __shared__ double s_pub[2][4 + C];
    __shared__ double s_edge[2][kThreads][2];
    __shared__ alignas(16) double s_v[VL ? E : 1][VL ? kThreads : 1][2];      // VL: v lives here, element e of thread tid at [e][tid]
    const int tid = threadIdx.x, base = tid * E;
    const int col0 = blockIdx.x * C, nc = min(C, ncols - col0);
    const int64_t theta = blockIdx.y;
    const double* tt = t + theta * n;
    double* Yt = Y + theta * (int64_t)n * ncols;

    const double t0 = tt[0];
    int bad = t0_bad(t0);                                                    // the same in every thread
    double uh[E], ul[E], z[E][C];
    float zc[E][C];                                                          // sum of lo(L[i, k]) * y_k: the residual is z - zc
    VStore<E, VL> vs{&s_v[0][VL ? tid : 0]};
    if (!bad) {
        const dd rs = t0_rsqrt(t0);
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int i = base + e;
            const uv g = generator_from_t(tt, rs, i, n);
            const dd u = g.u;
            uh[e] = u.h;
            ul[e] = u.l;
            vs.set(e, g.v);
#pragma unroll
            for (int c = 0; c < C; ++c) {
                z[e][c] = (i < n && c < nc) ? ldexp(Z[(int64_t)(col0 + c) * n + i], -ze[col0 + c]) : 0.0;
                zc[e][c] = 0.f;
            }
            if (i == 0) {
                s_pub[0][0] = u.h;
                s_pub[0][1] = u.l;
#pragma unroll
                for (int c = 0; c < C; ++c) s_pub[0][4 + c] = z[e][c];
            }
            if (i == 1) {
                s_pub[0][2] = u.h;
                s_pub[0][3] = u.l;
            }
        }
        s_edge[0][tid][0] = uh[E - 1];
        s_edge[0][tid][1] = ul[E - 1];
    }
    __syncthreads();

    for (int k = 0; k < n && !bad; ++k) {
        const int b = k & 1, nb = b ^ 1;
        const dd pu = {s_pub[b][0], s_pub[b][1]};
        const double inv = 1.0 / pu.h;
        double y[C];
        float yf[C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            y[c] = s_pub[b][4 + c] * inv;
            yf[c] = (float)y[c];
        }
        if (tid < nc) Yt[(int64_t)k * ncols + col0 + tid] = s_pub[b][4 + tid] * inv;
        if constexpr (R) {
            if (tid < 4 && blockIdx.x == 0) steps[(theta * n + k) * 4 + tid] = s_pub[b][tid];
        }
        if (k == n - 1) break;
        const coeffs co = step_coeffs(pu, dd{s_pub[b][2], s_pub[b][3]});
        if (!co.ok) {                                                         // the same in every thread
            bad = k + 2;
            break;
        }
        const dd nrho = dd_neg(co.rho), ic = co.ic;
        if (base + E - 1 > k && base < n) {                                  // the thread still holds elements below the pivot
            dd edge = {0.0, 0.0};
            if (tid > 0) edge = {s_edge[b][tid - 1][0], s_edge[b][tid - 1][1]};
#pragma unroll
            for (int e = E - 1; e >= 0; --e) {
                const int i = base + e;
#pragma unroll
                for (int c = 0; c < C; ++c) z[e][c] = fma(-uh[e], y[c], z[e][c]);
                const float ulf = (float)ul[e];
#pragma unroll
                for (int c = 0; c < C; ++c) zc[e][c] = fmaf(ulf, yf[c], zc[e][c]);
                const dd us = e > 0 ? dd{uh[e > 0 ? e - 1 : 0], ul[e > 0 ? e - 1 : 0]} : edge;      // u shifted down by one
                const uv r = rotate(us, vs.get(e), nrho, ic);
                const bool live = i > k;                                      // at or above the pivot: u[i] keeps L[i, i]
                uh[e] = live ? r.u.h : uh[e];
                ul[e] = live ? r.u.l : ul[e];
                vs.set(e, r.v);
                if (i == k + 1) {
                    s_pub[nb][0] = r.u.h;
                    s_pub[nb][1] = r.u.l;
#pragma unroll
                    for (int c = 0; c < C; ++c) s_pub[nb][4 + c] = z[e][c] - (double)zc[e][c];
                }
                if (i == k + 2) {
                    s_pub[nb][2] = r.v.h;
                    s_pub[nb][3] = r.v.l;
                }
            }
            s_edge[nb][tid][0] = uh[E - 1];
            s_edge[nb][tid][1] = ul[E - 1];
        }
        __syncthreads();
    }

    if (blockIdx.x != 0) return;                                             // every chunk of a first column finds the same two numbers
    __syncthreads();
    double s = 0.0;
    if (!bad) {
#pragma unroll
        for (int e = 0; e < E; ++e)
            if (base + e < n) s += log(uh[e]);
    }
    sum_log_diag_tree(&s_edge[0][0][0], tid, s, bad, sld + theta);
    if (tid == 0) info[theta] = bad;
}

// G is (m, n_sets, cols, cols), scaled back by the column exponents ze.  grid = (cols, n_sets, m), block = kWave.
__global__ __launch_bounds__(kWave) void k_gram(const double* __restrict__ Y, int n, int cols, int n_sets, const int32_t* __restrict__ ze,
                                                 const int32_t* __restrict__ info, double* __restrict__ G) {
    const int a = blockIdx.x, set = blockIdx.y, lane = threadIdx.x;
    const int64_t theta = blockIdx.z;
    const int ncols = n_sets * cols;
    double* g = G + ((theta * n_sets + set) * cols + a) * (int64_t)cols;
    if (info[theta] != 0) {
        if (lane < cols) g[lane] = NAN;
        return;
    }
    const double* Ys = Y + theta * (int64_t)n * ncols + (int64_t)set * cols;
    double acc[kMaxCols];
#pragma unroll
    for (int bcol = 0; bcol < kMaxCols; ++bcol) acc[bcol] = 0.0;
    for (int k = lane; k < n; k += kWave) {
        const double* row = Ys + (int64_t)k * ncols;
        const double ya = row[a];
#pragma unroll
        for (int bcol = 0; bcol < kMaxCols; ++bcol)
            if (bcol < cols) acc[bcol] = fma(ya, row[bcol], acc[bcol]);
    }
#pragma unroll
    for (int bcol = 0; bcol < kMaxCols; ++bcol) {
        double x = acc[bcol];
#pragma unroll
        for (int off = 1; off < kWave; off <<= 1) x += __shfl_xor(x, off, kWave);
        if (lane == 0 && bcol < cols) g[bcol] = ldexp(x, ze[set * cols + a] + ze[set * cols + bcol]);
    }
}

// ---- the gradient pieces ---------------------------------------------------------------------------------------
// Everything below works from x = T^-1 e_0 (Gohberg-Semencul).  Sums run in double-double in an order fixed by n alone: lane l of a wave
// takes the terms l, l + 64, ... in order, then the lanes are folded 32, 16, ... 1 onto lane 0.

__device__ __forceinline__ dd wave_fold(dd a) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) a = dd_add(a, dd{__shfl_down(a.h, off, kWave), __shfl_down(a.l, off, kWave)});
    return a;                                                                 // the sum is lane 0's
}
__device__ __forceinline__ bool dd_finite(dd a) { return fabs(a.h) < INFINITY && fabs(a.l) < INFINITY; }

// steps row k < n - 1: {u[k], v[k+1]} -> {rho, 1 / c} by step_coeffs, as in k_schur's step, so the words are the ones the generator
// was rotated with; row n - 1 keeps u[n-1] = L[n-1, n-1].  Independent rows: no serial chain.  grid = (ceil(n / 256), m), block = 256.
__global__ __launch_bounds__(256) void k_coeffs(double* __restrict__ steps, int n, const int32_t* __restrict__ info) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    const int64_t theta = blockIdx.y;
    if (k >= n - 1 || info[theta] != 0) return;
    double* st = steps + (theta * n + k) * 4;
    const coeffs c = step_coeffs(dd{st[0], st[1]}, dd{st[2], st[3]});         // info is 0: k_schur's test of this pair passed
    st[0] = c.rho.h;
    st[1] = c.rho.l;
    st[2] = c.ic.h;
    st[3] = c.ic.l;
}

// Levinson's recursion in its normalised form, replaying the (rho, 1 / c) of k_schur<.., R = true> and k_coeffs: A = B = e_0 / sqrt(t_0), then for
// k = 1 .. n - 1  A <- (A - rho_k shift(B)) / c_k, B <- (shift(B) - rho_k A) / c_k (shift: down by one), and x = A / L[n-1, n-1].  A
// and B in double-double in registers, E consecutive elements per thread as in k_schur; B's element that crosses a thread boundary
// goes through edge[buffer][thread], one barrier per step.  The coefficients of the next step are loaded a step ahead.  grid = m,
// block = kThreads.  xd is (m, n, 2) (both words), xf (m, n) its fp64 rounding; a first column with info != 0 gives NaN; one whose x
// is not finite gets info = n + 1 and a NaN sld.
template <int E>
__global__ __launch_bounds__(kThreads) void k_levinson(const double* __restrict__ t, int n, const double* __restrict__ steps,
                                                        double* __restrict__ xd, double* __restrict__ xf, double* __restrict__ sld,
                                                        int32_t* __restrict__ info) {
    __shared__ double s_edge[2][kThreads][2];
    const int tid = threadIdx.x, base = tid * E;
    const int64_t theta = blockIdx.x;
    const double* st = steps + theta * n * 4;
    double* xo = xd + theta * n * 2;
    double* xr = xf + theta * n;
    if (info[theta] != 0) {                                                   // the same in every thread
#pragma unroll
        for (int e = 0; e < E; ++e)
            if (base + e < n) xo[2 * (base + e)] = xo[2 * (base + e) + 1] = xr[base + e] = NAN;
        return;
    }
    double ah[E], al[E], bh[E], bl[E];
#pragma unroll
    for (int e = 0; e < E; ++e) ah[e] = al[e] = bh[e] = bl[e] = 0.0;
    if (tid == 0) {
        const dd rs = t0_rsqrt(t[theta * n]);
        ah[0] = bh[0] = rs.h;
        al[0] = bl[0] = rs.l;
    }
    s_edge[0][tid][0] = bh[E - 1];
    s_edge[0][tid][1] = bl[E - 1];
    s_edge[1][tid][0] = s_edge[1][tid][1] = 0.0;
    double c0 = 0.0, c1 = 0.0, c2 = 1.0, c3 = 0.0;                            // the coefficients of the coming step
    if (n > 1) {
        c0 = st[0];
        c1 = st[1];
        c2 = st[2];
        c3 = st[3];
    }
    __syncthreads();
    for (int k = 1; k < n; ++k) {
        const int b = (k - 1) & 1, nb = b ^ 1;
        const dd nrho = {-c0, -c1}, ic = {c2, c3};
        if (k + 1 < n) {                                                      // step k + 1 replays row k
            const double* nx = st + (int64_t)k * 4;
            c0 = nx[0];
            c1 = nx[1];
            c2 = nx[2];
            c3 = nx[3];
        }
        if (base <= k) {                                                      // elements beyond k are still zero
            dd edge = {0.0, 0.0};
            if (tid > 0) edge = {s_edge[b][tid - 1][0], s_edge[b][tid - 1][1]};
#pragma unroll
            for (int e = E - 1; e >= 0; --e) {
                const dd bs = e > 0 ? dd{bh[e > 0 ? e - 1 : 0], bl[e > 0 ? e - 1 : 0]} : edge;       // B shifted down by one
                const uv r = rotate(dd{ah[e], al[e]}, bs, nrho, ic);         // (A, shift(B)) in the roles of (u shifted, v)
                ah[e] = r.u.h;
                al[e] = r.u.l;
                bh[e] = r.v.h;
                bl[e] = r.v.l;
            }
            s_edge[nb][tid][0] = bh[E - 1];
            s_edge[nb][tid][1] = bl[E - 1];
        }
        __syncthreads();
    }
    const dd last = {st[(int64_t)(n - 1) * 4], st[(int64_t)(n - 1) * 4 + 1]};
    int notfinite = 0;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const dd x = dd_div(dd{ah[e], al[e]}, last);
        ah[e] = x.h;
        al[e] = x.l;
        if (base + e < n && !dd_finite(x)) notfinite = 1;
    }
    notfinite = __syncthreads_or(notfinite);
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = base + e;
        if (i < n) {
            xo[2 * i] = notfinite ? NAN : ah[e];
            xo[2 * i + 1] = notfinite ? NAN : al[e];
            xr[i] = notfinite ? NAN : ah[e];
        }
    }
    if (notfinite && tid == 0) {
        info[theta] = n + 1;
        sld[theta] = NAN;
    }
}

// sd[theta, d] = the sum of the d-th diagonal of T^-1 = (1 / x_0) sum_{m <= n-1-d} (n - d - 2 m) x_m x_{m+d}, both words.  The weight is
// an integer below 2^14 in magnitude: exact.  grid = (n, m), block = kWave.
__global__ __launch_bounds__(kWave) void k_diagsums(const double* __restrict__ xd, int n, const int32_t* __restrict__ info,
                                                     double* __restrict__ sd) {
    const int d = blockIdx.x, lane = threadIdx.x;
    const int64_t theta = blockIdx.y;
    double* out = sd + (theta * n + d) * 2;
    if (info[theta] != 0) {
        if (lane == 0) out[0] = out[1] = NAN;
        return;
    }
    const double* x = xd + theta * n * 2;
    dd acc = {0.0, 0.0};
    for (int m = lane; m <= n - 1 - d; m += kWave) {
        const dd p = dd_mul(dd{x[2 * m], x[2 * m + 1]}, dd{x[2 * (m + d)], x[2 * (m + d) + 1]});
        acc = dd_add(acc, dd_mul_d(p, (double)(n - d - 2 * m)));
    }
    acc = wave_fold(acc);
    if (lane == 0) {
        const dd s = dd_div(acc, dd{x[0], x[1]});
        out[0] = s.h;
        out[1] = s.l;
    }
}

// trace[theta, p] = dt_p[0] s_0 + 2 sum_{d >= 1} dt_p[d] s_d.  dt is (m, P, n).  grid = (P, m), block = kWave.
__global__ __launch_bounds__(kWave) void k_traces(const double* __restrict__ sd, const double* __restrict__ dt, int n, int P,
                                                   const int32_t* __restrict__ info, double* __restrict__ trace) {
    const int p = blockIdx.x, lane = threadIdx.x;
    const int64_t theta = blockIdx.y;
    if (info[theta] != 0) {
        if (lane == 0) trace[theta * P + p] = NAN;
        return;
    }
    const double* s = sd + theta * n * 2;
    const double* d = dt + (theta * P + p) * n;
    dd acc = {0.0, 0.0};
    for (int k = lane; k < n; k += kWave) acc = dd_add(acc, dd_mul_d(dd{s[2 * k], s[2 * k + 1]}, k ? 2.0 * d[k] : d[k]));
    acc = wave_fold(acc);
    if (lane == 0) trace[theta * P + p] = acc.h;
}

// The first half of alpha = T^-1 z = (1 / x_0) [L(x) L(x)^T - L(xt) L(xt)^T] z, L(.) the lower-triangular Toeplitz matrix of a first
// column and xt = (0, x_{n-1}, .., x_1):  W[theta, col, j] = {w1.h, w1.l, w2.h, w2.l},  w1[j] = sum_{r <= n-1-j} x_r z_{j+r},
// w2[j] = sum_{1 <= r <= n-1-j} x_{n-r} z_{j+r}.  z is loaded scaled by 2^-ze[col] as in k_schur.  Z is column-major n x ncols.
// grid = (n * ncols, m), block = kWave.
__global__ __launch_bounds__(kWave) void k_gs_first(const double* __restrict__ xd, int n, const double* __restrict__ Z,
                                                     const int32_t* __restrict__ ze, int ncols, const int32_t* __restrict__ info,
                                                     double* __restrict__ W) {
    const int col = blockIdx.x / n, j = blockIdx.x % n, lane = threadIdx.x;
    const int64_t theta = blockIdx.y;
    if (info[theta] != 0) return;                                             // k_gs_second writes the NaN
    const double* x = xd + theta * n * 2;
    const double* z = Z + (int64_t)col * n + j;
    const int sh = -ze[col];
    dd a1 = {0.0, 0.0}, a2 = {0.0, 0.0};
    for (int r = lane; r <= n - 1 - j; r += kWave) {
        const double zz = ldexp(z[r], sh);
        a1 = dd_add(a1, dd_mul_d(dd{x[2 * r], x[2 * r + 1]}, zz));
        if (r > 0) a2 = dd_add(a2, dd_mul_d(dd{x[2 * (n - r)], x[2 * (n - r) + 1]}, zz));
    }
    a1 = wave_fold(a1);
    a2 = wave_fold(a2);
    if (lane == 0) {
        double* w = W + ((theta * ncols + col) * n + j) * 4;
        w[0] = a1.h;
        w[1] = a1.l;
        w[2] = a2.h;
        w[3] = a2.l;
    }
}

// The second half: alpha[i] = (sum_{j <= i} x_{i-j} w1[j] - sum_{j < i} x_{n-i+j} w2[j]) / x_0, rounded to fp64.  As (m, ncols, n) keeps
// alpha of the scaled columns for the contraction; alpha_out (m, n, ncols), if not null, is scaled back by 2^ze[col] (exact).
// grid = (n * ncols, m), block = kWave.
__global__ __launch_bounds__(kWave) void k_gs_second(const double* __restrict__ xd, int n, const double* __restrict__ W,
                                                      const int32_t* __restrict__ ze, int ncols, const int32_t* __restrict__ info,
                                                      double* __restrict__ As, double* __restrict__ alpha_out) {
    const int col = blockIdx.x / n, i = blockIdx.x % n, lane = threadIdx.x;
    const int64_t theta = blockIdx.y;
    double* as = As + (theta * ncols + col) * n + i;
    double* ao = alpha_out ? alpha_out + (theta * n + i) * ncols + col : nullptr;
    if (info[theta] != 0) {
        if (lane == 0) {
            *as = NAN;
            if (ao) *ao = NAN;
        }
        return;
    }
    const double* x = xd + theta * n * 2;
    const double* w = W + (theta * ncols + col) * n * 4;
    dd acc = {0.0, 0.0};
    for (int j = lane; j <= i; j += kWave) {
        acc = dd_add(acc, dd_mul(dd{x[2 * (i - j)], x[2 * (i - j) + 1]}, dd{w[4 * j], w[4 * j + 1]}));
        if (j < i) acc = dd_sub(acc, dd_mul(dd{x[2 * (n - i + j)], x[2 * (n - i + j) + 1]}, dd{w[4 * j + 2], w[4 * j + 3]}));
    }
    acc = wave_fold(acc);
    if (lane == 0) {
        const double a = dd_div(acc, dd{x[0], x[1]}).h;
        *as = a;
        if (ao) *ao = ldexp(a, ze[col]);
    }
}

// Q[theta, p, col, i] = (dT_p alpha_col)[i] = sum_j dt_p[|i - j|] alpha_col[j], both words.  grid = (n * ncols, P, m), block = kWave.
__global__ __launch_bounds__(kWave) void k_tprod(const double* __restrict__ dt, int n, int P, const double* __restrict__ As, int ncols,
                                                  const int32_t* __restrict__ info, double* __restrict__ Q) {
    const int col = blockIdx.x / n, i = blockIdx.x % n, p = blockIdx.y, lane = threadIdx.x;
    const int64_t theta = blockIdx.z;
    if (info[theta] != 0) return;                                             // k_hdot writes the NaN
    const double* d = dt + (theta * P + p) * n;
    const double* a = As + (theta * ncols + col) * n;
    dd acc = {0.0, 0.0};
    for (int j = lane; j < n; j += kWave) acc = dd_add(acc, two_prod(d[j > i ? j - i : i - j], a[j]));
    acc = wave_fold(acc);
    if (lane == 0) {
        double* q = Q + (((theta * P + p) * ncols + col) * n + i) * 2;
        q[0] = acc.h;
        q[1] = acc.l;
    }
}

// H[theta, set, p, a, b] = alpha_a^T (dT_p alpha_b) for a <= b, mirrored, scaled back by the two column exponents.
// grid = (cols * cols * P, n_sets, m), block = kWave.
__global__ __launch_bounds__(kWave) void k_hdot(const double* __restrict__ As, const double* __restrict__ Q, int n, int P, int cols,
                                                 int n_sets, const int32_t* __restrict__ ze, const int32_t* __restrict__ info,
                                                 double* __restrict__ H) {
    const int b = blockIdx.x % cols, a = (blockIdx.x / cols) % cols, p = blockIdx.x / (cols * cols), set = blockIdx.y, lane = threadIdx.x;
    const int64_t theta = blockIdx.z;
    if (a > b) return;
    const int ncols = n_sets * cols;
    double* h = H + ((theta * n_sets + set) * P + p) * (int64_t)cols * cols;
    if (info[theta] != 0) {
        if (lane == 0) h[a * cols + b] = h[b * cols + a] = NAN;
        return;
    }
    const double* al = As + (theta * ncols + set * cols + a) * n;
    const double* q = Q + ((theta * P + p) * ncols + set * cols + b) * n * 2;
    dd acc = {0.0, 0.0};
    for (int i = lane; i < n; i += kWave) acc = dd_add(acc, dd_mul_d(dd{q[2 * i], q[2 * i + 1]}, al[i]));
    acc = wave_fold(acc);
    if (lane == 0) h[a * cols + b] = h[b * cols + a] = ldexp(acc.h, ze[set * cols + a] + ze[set * cols + b]);
}

// ---- the posterior pieces ---------------------------------------------------------------------------------------
// k_pred_sums and k_pred_cov work on the solved columns Y = L^-1 [K | Z] of one first column: q cross-covariance columns, then c
// residual columns, (n, q + c) row-major, each scaled by 2^-ze[col] as k_schur loaded it.  k_invdiag works from xd (k_levinson).

// quad[j] = sum_k Y[k, j]^2 (blockIdx.x == 0) and cross[j, b] = sum_k Y[k, j] Y[k, q + b] (blockIdx.x == 1 + b): k_gram's sum in
// double-double and the house order (lane l takes the rows l, l + 64, ..., then the fold), scaled back by the two exponents.  An
// output depends on its own two columns and on n alone.  grid = (q, 1 + c), block = kWave.
__global__ __launch_bounds__(kWave) void k_pred_sums(const double* __restrict__ Y, int n, int q, int c, const int32_t* __restrict__ ze,
                                                      const int32_t* __restrict__ info, double* __restrict__ quad,
                                                      double* __restrict__ cross) {
    const int j = blockIdx.x, lane = threadIdx.x;
    const bool is_quad = blockIdx.y == 0;
    const int b = is_quad ? j : q + (int)blockIdx.y - 1;                      // the other column
    double* out = is_quad ? quad + j : cross + (int64_t)j * c + (blockIdx.y - 1);
    if (info[0] != 0) {
        if (lane == 0) *out = NAN;
        return;
    }
    const int64_t ld = (int64_t)q + c;
    dd acc = {0.0, 0.0};
    for (int k = lane; k < n; k += kWave) acc = dd_add(acc, two_prod(Y[k * ld + j], Y[k * ld + b]));
    acc = wave_fold(acc);
    if (lane == 0) *out = ldexp(acc.h, ze[j] + ze[b]);
}

typedef double cov_acc __attribute__((ext_vector_type(4)));

// cov[a, b] = sum_k Y[k, a] Y[k, b], a, b < q, on v_mfma_f64_16x16x4_f64: one wave per 16 x 16 tile on or below the diagonal, the
// tile above it stored from the same accumulators.  A K step takes four rows of Y: lane l holds Y[k0 + (l >> 4), tile * 16 + (l & 15)]
// of the row tile as the A operand (A[i][k], i = l & 15) and of the column tile as the B operand (B[k][j], j = l & 15): four
// contiguous 128-byte segments each, straight from global memory.  In a diagonal tile the two are one fragment, so (i, j) and (j, i)
// see the same products in the same chain: cov is bitwise symmetric.  The K loop runs 0 .. n in steps of four in every tile, never
// split; rows beyond n and columns beyond q enter as zeros and are neither read nor written.  The accumulator map is col = lane & 15,
// row = (lane >> 4) + 4 * reg.  grid = (tiles, tiles), block = kWave; the blocks above the diagonal return at once.
__global__ __launch_bounds__(kWave) void k_pred_cov(const double* __restrict__ Y, int n, int q, int c, const int32_t* __restrict__ ze,
                                                     const int32_t* __restrict__ info, double* __restrict__ cov) {
    const int ti = blockIdx.y, tj = blockIdx.x, lane = threadIdx.x;
    if (tj > ti) return;
    const int fr = lane & 15, fq = lane >> 4;
    const int ca = ti * 16 + fr, cb = tj * 16 + fr;                          // the operand columns this lane loads
    const bool bad = info[0] != 0;
    const int64_t ld = (int64_t)q + c;
    cov_acc acc = {0.0, 0.0, 0.0, 0.0};
    if (!bad) {
        const bool diag = ti == tj, ina = ca < q, inb = cb < q;
        for (int k0 = 0; k0 < n; k0 += 4) {
            const int k = k0 + fq;
            const double af = (ina && k < n) ? Y[k * ld + ca] : 0.0;
            const double bf = diag ? af : ((inb && k < n) ? Y[k * ld + cb] : 0.0);
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(af, bf, acc, 0, 0, 0);
        }
    }
    const int col = tj * 16 + fr;
    if (col >= q) return;
    const int ec = ze[col];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = ti * 16 + fq + 4 * r;
        if (row >= q) continue;
        const double v = bad ? NAN : ldexp(acc[r], ze[row] + ec);
        cov[(int64_t)row * q + col] = v;
        if (ti != tj) cov[(int64_t)col * q + row] = v;
    }
}

// p = diag(T^-1) from x = T^-1 e_0 (Gohberg-Semencul): p_i = (1 / x_0) sum_{r <= i} (x_r^2 - x_{n-r}^2), x_n = 0, the term taken as
// (x_r - x_{n-r}) (x_r + x_{n-r}).  The terms cancel heavily on an ill-conditioned T, so everything up to the one rounding at the end
// is double-double: thread tid forms its E consecutive terms and their running sums, the threads' totals are scanned through LDS
// (nine doubling steps, two buffers, an order fixed by the thread count), then the division by x_0.  pd is (m, n); a first column
// with info != 0 gives NaN.  grid = m, block = kThreads.
template <int E>
__global__ __launch_bounds__(kThreads) void k_invdiag(const double* __restrict__ xd, int n, const int32_t* __restrict__ info,
                                                       double* __restrict__ pd) {
    __shared__ double s_tot[2][kThreads][2];
    const int tid = threadIdx.x, base = tid * E;
    const int64_t theta = blockIdx.x;
    double* p = pd + theta * n;
    if (info[theta] != 0) {                                                   // the same in every thread
#pragma unroll
        for (int e = 0; e < E; ++e)
            if (base + e < n) p[base + e] = NAN;
        return;
    }
    const double* x = xd + theta * n * 2;
    dd run[E];
    dd acc = {0.0, 0.0};
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int r = base + e;
        if (r < n) {
            const dd a = {x[2 * r], x[2 * r + 1]};
            const dd b = r > 0 ? dd{x[2 * (n - r)], x[2 * (n - r) + 1]} : dd{0.0, 0.0};
            acc = dd_add(acc, dd_mul(dd_sub(a, b), dd_add(a, b)));
        }
        run[e] = acc;
    }
    s_tot[0][tid][0] = acc.h;
    s_tot[0][tid][1] = acc.l;
    __syncthreads();
    int cur = 0;
    for (int off = 1; off < kThreads; off <<= 1) {                            // inclusive scan of the totals
        dd s = {s_tot[cur][tid][0], s_tot[cur][tid][1]};
        if (tid >= off) s = dd_add(dd{s_tot[cur][tid - off][0], s_tot[cur][tid - off][1]}, s);
        s_tot[cur ^ 1][tid][0] = s.h;
        s_tot[cur ^ 1][tid][1] = s.l;
        cur ^= 1;
        __syncthreads();
    }
    const dd before = tid > 0 ? dd{s_tot[cur][tid - 1][0], s_tot[cur][tid - 1][1]} : dd{0.0, 0.0};
    const dd x0 = {x[0], x[1]};
#pragma unroll
    for (int e = 0; e < E; ++e)
        if (base + e < n) p[base + e] = dd_div(dd_add(before, run[e]), x0).h;
}

// ---- the panel route --------------------------------------------------------------------------------------------
// k_schur's recursion produces the columns of L one after the other and needs none of the right-hand sides; its substitution is an
// ordinary blocked forward solve that consumes them.  Here the two are separate kernels, and any number of columns ride one recursion:
// per panel of kPanelB columns of L, k_schur_panel (one workgroup per first column) writes the panel, k_panel_diag solves its
// triangular block for every column and k_panel_update applies it to the rows below on the fp64 MFMA.  The residuals live in Y itself
// ((n, ncols) row-major per first column, scaled by k_colexp's exponents by k_panel_load): row k holds the residual z_k until the
// panel of k is solved and y_k from then on, the fp32 correction words in Zc beside it.  A panel is (kPanelB, n) per first column,
// column k of L contiguous: Ph the high words, Pl the low words as fp32.  Kernels follow one another in stream order.

#ifndef GSUM_TOEP_PANEL_B
#define GSUM_TOEP_PANEL_B 64
#endif
constexpr int kPanelB = GSUM_TOEP_PANEL_B;         // columns of L per panel: a multiple of 16 (k_panel_diag's blocks, the MFMA's K steps)
constexpr int kDiagR = 16;                         // rows of a register block of k_panel_diag
constexpr int kDiagU = 8;                          // later rows of the block it updates at a time
constexpr int kDiagThreads = 64;                   // columns of a k_panel_diag workgroup
constexpr int kUpdateTiles = 4;                    // 16-column tiles of a k_panel_update wave
static_assert(kPanelB % kDiagR == 0 && kPanelB % 4 == 0 && kPanelB >= 16 && kPanelB <= 256, "k_panel_diag and k_panel_update step through a panel in 16s and 4s");

// Y[theta, i, j] = Z[i, j] * 2^-ze[j] for every first column theta < cnt: the column-major right-hand sides into the row-major
// working residuals, through a 32 x 32 LDS tile.  grid = (ceil(ncols / 32), ceil(n / 32)), block = (32, 8).
__global__ __launch_bounds__(256) void k_panel_load(const double* __restrict__ Z, const int32_t* __restrict__ ze, int n, int ncols, int cnt,
                                                     double* __restrict__ Y) {
    __shared__ double s_t[32][33];
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int i0 = blockIdx.y * 32, j0 = blockIdx.x * 32;
    for (int r = ty; r < 32; r += 8) {                                        // column j0 + r, rows i0 + tx: consecutive in Z
        const int i = i0 + tx, j = j0 + r;
        s_t[r][tx] = (i < n && j < ncols) ? ldexp(Z[(int64_t)j * n + i], -ze[j]) : 0.0;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {                                        // row i0 + r, columns j0 + tx: consecutive in Y
        const int i = i0 + r, j = j0 + tx;
        if (i < n && j < ncols) {
            const double v = s_t[tx][r];
            for (int64_t theta = 0; theta < cnt; ++theta) Y[(theta * n + i) * ncols + j] = v;
        }
    }
}

// k_schur's step without residual columns, for the steps k0 .. min(k0 + kPanelB, n) - 1 of every first column of the launch: the same
// double-double generator, step_coeffs and rotate, the same sweep and publication through LDS.  The generator state lives in st
// between launches (state_load / state_store, stride kThreads * E); k0 == 0 forms it from t as k_schur does (generator_from_t).
// info[theta] is the running failure step: a first column that has failed is skipped by every later launch.  At step k every thread
// stores its elements of column k of L (u before the rotation), rows k .. n - 1: Ph[theta, k - k0, i] and (float) of the low word in
// Pl.  The launch that reaches step n - 1 sums log L_jj from the retained u in k_schur's order (sum_log_diag_tree), so sum_log_diag
// and info are bit for bit k_schur's.  grid = m, block = kThreads.
template <int E, bool VL>
__global__ __launch_bounds__(kThreads) void k_schur_panel(const double* __restrict__ t, int n, int k0, double* __restrict__ st,
                                                           double* __restrict__ Ph, float* __restrict__ Pl, double* __restrict__ sld,
                                                           int32_t* __restrict__ info) {
    __shared__ double s_pub[2][4];
    __shared__ double s_edge[2][kThreads][2];
    __shared__ alignas(16) double s_v[VL ? E : 1][VL ? kThreads : 1][2];
    constexpr int NE = kThreads * E;
    const int tid = threadIdx.x, base = tid * E;
    const int64_t theta = blockIdx.x;
    const double* tt = t + theta * n;
    double* s = st + theta * 4 * NE;
    double* ph = Ph + theta * (int64_t)kPanelB * n;
    float* pl = Pl + theta * (int64_t)kPanelB * n;
    const int k1 = min(k0 + kPanelB, n);

    int bad = k0 == 0 ? t0_bad(tt[0]) : info[theta];                          // the same in every thread
    double uh[E], ul[E];
    VStore<E, VL> vs{&s_v[0][VL ? tid : 0]};
    const int b0 = k0 & 1;
    if (!bad) {
        dd rs = {0.0, 0.0};
        if (k0 == 0) rs = t0_rsqrt(tt[0]);
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int i = base + e;
            const uv g = k0 == 0 ? generator_from_t(tt, rs, i, n) : state_load(s, NE, i);
            const dd u = g.u, v = g.v;
            uh[e] = u.h;
            ul[e] = u.l;
            vs.set(e, v);
            if (i == k0) {
                s_pub[b0][0] = u.h;
                s_pub[b0][1] = u.l;
            }
            if (i == k0 + 1) {
                s_pub[b0][2] = v.h;
                s_pub[b0][3] = v.l;
            }
        }
        s_edge[0][tid][0] = s_edge[1][tid][0] = uh[E - 1];
        s_edge[0][tid][1] = s_edge[1][tid][1] = ul[E - 1];
    }
    __syncthreads();

    for (int k = k0; k < k1 && !bad; ++k) {
        const int b = k & 1, nb = b ^ 1;
        const dd pu = {s_pub[b][0], s_pub[b][1]};
        double* pk = ph + (int64_t)(k - k0) * n;
        float* qk = pl + (int64_t)(k - k0) * n;
#pragma unroll
        for (int e = 0; e < E; ++e) {                                         // column k of L, rows k .. n - 1
            const int i = base + e;
            if (i >= k && i < n) store_column(pk, qk, i, dd{uh[e], ul[e]});
        }
        if (k == n - 1) break;
        const coeffs co = step_coeffs(pu, dd{s_pub[b][2], s_pub[b][3]});
        if (!co.ok) {                                                         // the same in every thread
            bad = k + 2;
            break;
        }
        const dd nrho = dd_neg(co.rho), ic = co.ic;
        if (base + E - 1 > k && base < n) {                                  // the thread still holds elements below the pivot
            dd edge = {0.0, 0.0};
            if (tid > 0) edge = {s_edge[b][tid - 1][0], s_edge[b][tid - 1][1]};
#pragma unroll
            for (int e = E - 1; e >= 0; --e) {
                const int i = base + e;
                const dd us = e > 0 ? dd{uh[e > 0 ? e - 1 : 0], ul[e > 0 ? e - 1 : 0]} : edge;      // u shifted down by one
                const uv r = rotate(us, vs.get(e), nrho, ic);
                const bool live = i > k;                                      // at or above the pivot: u[i] keeps L[i, i]
                uh[e] = live ? r.u.h : uh[e];
                ul[e] = live ? r.u.l : ul[e];
                vs.set(e, r.v);
                if (i == k + 1) {
                    s_pub[nb][0] = r.u.h;
                    s_pub[nb][1] = r.u.l;
                }
                if (i == k + 2) {
                    s_pub[nb][2] = r.v.h;
                    s_pub[nb][3] = r.v.l;
                }
            }
            s_edge[nb][tid][0] = uh[E - 1];
            s_edge[nb][tid][1] = ul[E - 1];
        }
        __syncthreads();
    }

    if (k1 < n) {                                                             // more panels follow: hand the state on
        if (!bad) {
#pragma unroll
            for (int e = 0; e < E; ++e) state_store(s, NE, base + e, uv{{uh[e], ul[e]}, vs.get(e)});
        }
        if (tid == 0) info[theta] = bad;
        return;
    }
    __syncthreads();
    double acc = 0.0;
    if (!bad) {
#pragma unroll
        for (int e = 0; e < E; ++e)
            if (base + e < n) acc += log(uh[e]);
    }
    sum_log_diag_tree(&s_edge[0][0][0], tid, acc, bad, sld + theta);
    if (tid == 0) info[theta] = bad;
}

// The triangular block of a panel, rows and columns k0 .. k1 - 1 (k1 = min(k0 + kPanelB, n)), for every right-hand-side column: one
// thread per column, k_schur's substitution literally.  For each k: y_k = (z_k - zc_k) * (1 / hi(L_kk)), then for the rows i of the
// block below it z_i = fma(-hi(L_ik), y_k, z_i) and zc_i = fmaf(lo(L_ik), (float)y_k, zc_i).  The rows go through the registers 16
// at a time: the 16 x 16 triangle, then those 16 y applied in ascending k to each later row of the block; the 16 columns of L are
// staged in LDS for the workgroup (broadcast reads).  Row k of Y receives y_k in place of z_k.
// grid = (ceil(ncols / kDiagThreads), cnt), block = kDiagThreads.
__global__ __launch_bounds__(kDiagThreads) void k_panel_diag(const double* __restrict__ Ph, const float* __restrict__ Pl, int n, int k0,
                                                              int ncols, double* __restrict__ Y, float* __restrict__ Zc,
                                                              const int32_t* __restrict__ info) {
    __shared__ double s_h[kDiagR][kPanelB + kDiagU];
    __shared__ float s_l[kDiagR][kPanelB + kDiagU];
    const int64_t theta = blockIdx.y;
    if (info[theta] != 0) return;                                             // the same in every thread
    const int tid = threadIdx.x, j = blockIdx.x * kDiagThreads + tid;
    const bool mine = j < ncols;
    const int kb = min(kPanelB, n - k0);                                      // rows and columns of the block
    const double* ph = Ph + theta * (int64_t)kPanelB * n;
    const float* pl = Pl + theta * (int64_t)kPanelB * n;
    double* y = Y + (theta * n + k0) * ncols + j;                             // row r of the block at y[r * ncols]
    float* zc = Zc + (theta * n + k0) * ncols + j;
    for (int s0 = 0; s0 < kb; s0 += kDiagR) {
        const int nr = min(kDiagR, kb - s0);                                  // rows of this register block
        __syncthreads();
        for (int x = tid; x < kDiagR * (kb - s0); x += kDiagThreads) {         // columns s0 .. s0 + nr - 1 of L, rows s0 .. kb - 1 of the block
            const int c = x / (kb - s0), r = s0 + x % (kb - s0);
            const bool in = c < nr && r >= s0 + c;                            // on or below the diagonal: what k_schur_panel stored
            s_h[c][r] = in ? ph[(int64_t)(s0 + c) * n + k0 + r] : 0.0;
            s_l[c][r] = in ? pl[(int64_t)(s0 + c) * n + k0 + r] : 0.f;
        }
        __syncthreads();
        if (!mine) continue;
        double z[kDiagR], yk[kDiagR];
        float c32[kDiagR], yf[kDiagR];
#pragma unroll
        for (int r = 0; r < kDiagR; ++r) {
            z[r] = r < nr ? y[(int64_t)(s0 + r) * ncols] : 0.0;
            c32[r] = r < nr ? zc[(int64_t)(s0 + r) * ncols] : 0.f;
        }
#pragma unroll
        for (int c = 0; c < kDiagR; ++c) {
            yk[c] = 0.0;
            yf[c] = 0.f;
            if (c < nr) {
                yk[c] = (z[c] - (double)c32[c]) * (1.0 / s_h[c][s0 + c]);
                yf[c] = (float)yk[c];
#pragma unroll
                for (int r = c + 1; r < kDiagR; ++r) {
                    if (r < nr) {
                        z[r] = fma(-s_h[c][s0 + r], yk[c], z[r]);
                        c32[r] = fmaf(s_l[c][s0 + r], yf[c], c32[r]);
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < kDiagR; ++r)
            if (r < nr) y[(int64_t)(s0 + r) * ncols] = yk[r];
        for (int r = s0 + kDiagR; r < kb; r += kDiagU) {                       // the later rows of the block, kDiagU loads in flight
            double zr[kDiagU];
            float cr[kDiagU];
#pragma unroll
            for (int u = 0; u < kDiagU; ++u) {
                zr[u] = r + u < kb ? y[(int64_t)(r + u) * ncols] : 0.0;
                cr[u] = r + u < kb ? zc[(int64_t)(r + u) * ncols] : 0.f;
            }
#pragma unroll
            for (int c = 0; c < kDiagR; ++c) {
#pragma unroll
                for (int u = 0; u < kDiagU; ++u) {     // rows beyond kb: whatever the padding holds (never written), and not stored
                    zr[u] = fma(-s_h[c][r + u], yk[c], zr[u]);
                    cr[u] = fmaf(s_l[c][r + u], yf[c], cr[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < kDiagU; ++u) {
                if (r + u < kb) {
                    y[(int64_t)(r + u) * ncols] = zr[u];
                    zc[(int64_t)(r + u) * ncols] = cr[u];
                }
            }
        }
    }
}

// The trailing update of a full panel (k0 + kPanelB < n) on v_mfma_f64_16x16x4_f64: for the rows i >= k0 + kPanelB,
// Z[i, j] -= sum_k hi(L_ik) Y[k, j] over the panel's columns k in ascending order.  One wave per 16 rows and kUpdateTiles 16-column
// tiles: the residual tile is the accumulator (col = lane & 15, row = (lane >> 4) + 4 * reg, as in k_pred_cov), lane l holds
// -L[r0 + (l & 15), k0 + 4 s + (l >> 4)] as the A operand of K step s (16 contiguous doubles of a column of L per quarter wave) and
// Y[k0 + 4 s + (l >> 4), c0 + (l & 15)] as the B operand, straight from global memory.  The K loop is never split, so an entry sees
// one chain in one order, fixed by n and kPanelB alone.  The correction word takes zc[i, j] += lo(L_ik) * (float)y_k for the same k
// in ascending order on the vector unit (k_schur's fmaf chain), its factors shuffled out of the operand fragments.  Rows beyond n
// and columns beyond ncols enter as zeros and are neither read nor written.
// grid = (ceil(ncols / 64), ceil((n - k0 - kPanelB) / 16), cnt), block = kWave.
__global__ __launch_bounds__(kWave) void k_panel_update(const double* __restrict__ Ph, const float* __restrict__ Pl, int n, int k0, int ncols,
                                                         double* __restrict__ Y, float* __restrict__ Zc, const int32_t* __restrict__ info) {
    const int64_t theta = blockIdx.z;
    if (info[theta] != 0) return;
    const int lane = threadIdx.x, fr = lane & 15, fq = lane >> 4;
    const int r0 = k0 + kPanelB + blockIdx.y * 16;
    const int c0 = blockIdx.x * (16 * kUpdateTiles);
    const double* ph = Ph + theta * (int64_t)kPanelB * n;
    const float* pl = Pl + theta * (int64_t)kPanelB * n;
    double* Yt = Y + theta * (int64_t)n * ncols;
    float* Ct = Zc + theta * (int64_t)n * ncols;
    const int arow = r0 + fr;                                                 // the row of L this lane loads as the A operand
    const bool ina = arow < n;
    cov_acc acc[kUpdateTiles];
    float zc[kUpdateTiles][4];
#pragma unroll
    for (int t = 0; t < kUpdateTiles; ++t) {
        const int col = c0 + 16 * t + fr;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = r0 + fq + 4 * r;
            const bool in = row < n && col < ncols;
            acc[t][r] = in ? Yt[(int64_t)row * ncols + col] : 0.0;
            zc[t][r] = in ? Ct[(int64_t)row * ncols + col] : 0.f;
        }
    }
#pragma unroll 2
    for (int s = 0; s < kPanelB / 4; ++s) {
        const int k = 4 * s + fq;
        const double af = ina ? -ph[(int64_t)k * n + arow] : 0.0;
        const float alf = ina ? pl[(int64_t)k * n + arow] : 0.f;             // the low word of the same entry of L
        float bff[kUpdateTiles];
#pragma unroll
        for (int t = 0; t < kUpdateTiles; ++t) {
            bff[t] = 0.f;
            if (c0 + 16 * t >= ncols) continue;                               // the same in every lane
            const int col = c0 + 16 * t + fr;
            const double bf = col < ncols ? Yt[(int64_t)(k0 + k) * ncols + col] : 0.0;
            bff[t] = (float)bf;
            acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(af, bf, acc[t], 0, 0, 0);
        }
        // the correction words of the four columns k0 + 4 s + kk in ascending order: lo(L) of the lane's rows and (float)y of its
        // columns are in the operand fragments of the quarter wave kk, taken from there with lane shuffles
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            float lo[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) lo[r] = __shfl(alf, kk * 16 + fq + 4 * r, kWave);
#pragma unroll
            for (int t = 0; t < kUpdateTiles; ++t) {
                if (c0 + 16 * t >= ncols) continue;
                const float yf = __shfl(bff[t], kk * 16 + fr, kWave);
#pragma unroll
                for (int r = 0; r < 4; ++r) zc[t][r] = fmaf(lo[r], yf, zc[t][r]);
            }
        }
    }
#pragma unroll
    for (int t = 0; t < kUpdateTiles; ++t) {
        const int col = c0 + 16 * t + fr;
        if (col >= ncols) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = r0 + fq + 4 * r;
            if (row >= n) continue;
            Yt[(int64_t)row * ncols + col] = acc[t][r];
            Ct[(int64_t)row * ncols + col] = zc[t][r];
        }
    }
}

// ---- the blocked route ------------------------------------------------------------------------------------------
// A step of the recursion is local: u'[i] and v'[i] need u[i-1], v[i] and the step's (rho, 1 / c), and those need u[k] and v[k+1]
// alone.  So a panel of kPanelB steps splits into a serial lead on the kPanelB + 1 rows under the pivot, which yields the panel's
// coefficients and info (k_schur_lead, one wave per first column), and a replay of those coefficients on every row at or below the
// pivot, tile by tile (k_schur_tiles, one wave per tile): a tile owns kTileR rows and loads kPanelB more above them, which is as far
// up as kPanelB steps reach, so what its halo lacks never arrives in its own rows.  The generator state lives in HBM, (4, n) doubles
// per first column (u.h, u.l, v.h, v.l), twice: the tiles of a panel read one buffer, halo included, and write the other.  Nothing
// holds a whole generator, so n is bounded by the grids and the indices alone.  Every element goes through step_coeffs and rotate in
// k_schur_panel's order; the panel is stored in its layout (store_column), and k_panel_diag and k_panel_update consume it unchanged.
// Kernels follow one another in stream order; no workgroup waits for another.

constexpr int kTileE = 8;                          // generator elements per lane of a tile
constexpr int kTileSpan = kWave * kTileE;          // rows a tile loads
constexpr int kTileR = kTileSpan - kPanelB;        // rows a tile owns
constexpr int kLeadE = (kPanelB + 1 + kWave - 1) / kWave;      // window elements per lane of the lead: row k0 + e * 64 + lane
// What the kernels rely on: the halo (kPanelB rows) and at least a wave of own rows fit the tile's span, the halo is whole lanes
// (a lane is all halo or all own rows), and the lead's window fits its lanes.  Tile and panel boundaries need not line up: the
// tiles of a panel start at the tile that holds row k0, wherever k0 falls in it.
static_assert(kTileR >= kWave && kPanelB % kTileE == 0 && kPanelB + 1 <= kLeadE * kWave, "the halo, the own rows and the lead's window fit their lanes");

// The generator state of every first column from t (generator_from_t, stride n), and info = 1 for a bad t[0] (0 otherwise).
// grid = (ceil(n / 256), m), block = 256.
__global__ __launch_bounds__(256) void k_blocked_init(const double* __restrict__ t, int n, double* __restrict__ st, int32_t* __restrict__ info) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int64_t theta = blockIdx.y;
    const double* tt = t + theta * n;
    const int bad = t0_bad(tt[0]);
    if (i == 0) info[theta] = bad;
    if (bad || i >= n) return;
    state_store(st + theta * 4 * (int64_t)n, n, i, generator_from_t(tt, t0_rsqrt(tt[0]), i, n));
}

// The steps k0 .. min(k0 + kPanelB, n - 1) - 1 of every first column on the rows k0 .. min(k0 + kPanelB, n - 1) of its state st:
// step_coeffs for rho, the failure test and 1 / c, and rotate on the window's rows below the pivot.  Lane l
// holds the rows k0 + l, k0 + 64 + l, ..; the pivot pair and the element shifted in from the row above come by lane shuffles.  Step k
// stores {rho.h, rho.l, ic.h, ic.l} at coef[theta, k - k0]; a failure at step k sets info[theta] = k + 2 and ends the first column,
// which this and every later kernel then skips.  grid = m, block = kWave.
__global__ __launch_bounds__(kWave) void k_schur_lead(int n, int k0, const double* __restrict__ st, double* __restrict__ coef,
                                                       int32_t* __restrict__ info) {
    const int lane = threadIdx.x;
    const int64_t theta = blockIdx.x;
    if (info[theta] != 0) return;                                             // the same in every lane
    const double* s = st + theta * 4 * (int64_t)n;
    double* co = coef + theta * 4 * kPanelB;
    const int last = min(k0 + kPanelB, n - 1);                                // the last row of the window
    double uh[kLeadE], ul[kLeadE], vh[kLeadE], vl[kLeadE];
#pragma unroll
    for (int e = 0; e < kLeadE; ++e) {
        const int i = k0 + e * kWave + lane;
        const uv g = i <= last ? state_load(s, n, i) : uv{};
        uh[e] = g.u.h;
        ul[e] = g.u.l;
        vh[e] = g.v.h;
        vl[e] = g.v.l;
    }
    int bad = 0;
    for (int k = k0; k < last; ++k) {
        const int wu = k - k0, wv = wu + 1;                                   // the window rows of u[k] and v[k + 1]
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll
        for (int e = 0; e < kLeadE; ++e) {
            a0 = (wu >> 6) == e ? uh[e] : a0;
            a1 = (wu >> 6) == e ? ul[e] : a1;
            a2 = (wv >> 6) == e ? vh[e] : a2;
            a3 = (wv >> 6) == e ? vl[e] : a3;
        }
        const dd pu = {__shfl(a0, wu & 63, kWave), __shfl(a1, wu & 63, kWave)};
        const dd pv = {__shfl(a2, wv & 63, kWave), __shfl(a3, wv & 63, kWave)};
        const coeffs c = step_coeffs(pu, pv);
        if (!c.ok) {                                                          // the same in every lane
            bad = k + 2;
            break;
        }
        const dd rho = c.rho, ic = c.ic, nrho = dd_neg(rho);
        if (lane == 0) {
            co[4 * wu] = rho.h;
            co[4 * wu + 1] = rho.l;
            co[4 * wu + 2] = ic.h;
            co[4 * wu + 3] = ic.l;
        }
#pragma unroll
        for (int e = kLeadE - 1; e >= 0; --e) {
            const int i = k0 + e * kWave + lane;
            // u shifted down by one: the row above is the lane before, or lane 63 of the slot before
            double sh = __shfl(uh[e], (lane + kWave - 1) & 63, kWave), sl = __shfl(ul[e], (lane + kWave - 1) & 63, kWave);
            const double ph = e > 0 ? __shfl(uh[e > 0 ? e - 1 : 0], kWave - 1, kWave) : 0.0;
            const double pl = e > 0 ? __shfl(ul[e > 0 ? e - 1 : 0], kWave - 1, kWave) : 0.0;
            const dd us = lane == 0 ? dd{ph, pl} : dd{sh, sl};
            const uv r = rotate(us, dd{vh[e], vl[e]}, nrho, ic);
            const bool live = i > k && i <= last;                             // at or above the pivot: u[i] keeps L[i, i]
            uh[e] = live ? r.u.h : uh[e];
            ul[e] = live ? r.u.l : ul[e];
            vh[e] = live ? r.v.h : vh[e];
            vl[e] = live ? r.v.l : vl[e];
        }
    }
    if (bad && lane == 0) info[theta] = bad;
}

// The panel k0 .. k1 - 1 (k1 = min(k0 + kPanelB, n)) on the rows of one tile, replaying the coefficients of k_schur_lead.  Tile
// k0 / kTileR + blockIdx.x owns the rows r0 .. r0 + kTileR - 1 (r0 a multiple of kTileR) and loads from `cur` the rows from
// r0 - kPanelB on, kTileE consecutive ones per lane in registers; the element a shift brings over a lane boundary comes by a lane
// shuffle, so a step has no barrier and no LDS.  For each k the tile stores its own rows >= k of column k of L (u before the
// rotation) by store_column, Ph[theta, k - k0, i] and (float) of the low word in Pl, the owner of row k also hi(L_kk) in
// dg[theta, k]; then it rotates every element it holds, u only below the pivot.  After s steps the first s rows of the halo are
// stale; the own rows lie kPanelB below its top and stay exact.  At the end it writes its own rows to `nxt`.
// Rows above the pivot are unspecified in both state buffers and never used: v is rotated and stored there too (as k_schur does),
// tiles above the pivot's are not launched, so their rows of `nxt` keep what an earlier panel left, and the pivot tile's halo reads
// such rows of `cur`.  All of that reaches only u[i-1] and v[i] of rows i <= k, which no rotation below the pivot takes.
// grid = (tiles from the pivot's on, cnt), block = kWave.
__global__ __launch_bounds__(kWave) void k_schur_tiles(int n, int k0, const double* __restrict__ cur, double* __restrict__ nxt,
                                                        const double* __restrict__ coef, double* __restrict__ Ph, float* __restrict__ Pl,
                                                        double* __restrict__ dg, const int32_t* __restrict__ info) {
    const int64_t theta = blockIdx.y;
    if (info[theta] != 0) return;                                             // the same in every lane
    const int lane = threadIdx.x;
    const int r0 = (k0 / kTileR + (int)blockIdx.x) * kTileR;                  // the tile's first own row
    const int base = r0 - kPanelB + lane * kTileE;                            // the row of the lane's first element
    const double* s = cur + theta * 4 * (int64_t)n;
    double* so = nxt + theta * 4 * (int64_t)n;
    const double* co = coef + theta * 4 * kPanelB;
    double* ph = Ph + theta * (int64_t)kPanelB * n;
    float* pl = Pl + theta * (int64_t)kPanelB * n;
    double* d = dg + theta * n;
    double uh[kTileE], ul[kTileE], vh[kTileE], vl[kTileE];
#pragma unroll
    for (int e = 0; e < kTileE; ++e) {
        const int i = base + e;
        const uv g = i >= 0 && i < n ? state_load(s, n, i) : uv{};
        uh[e] = g.u.h;
        ul[e] = g.u.l;
        vh[e] = g.v.h;
        vl[e] = g.v.l;
    }
    const int k1 = min(k0 + kPanelB, n);
    for (int k = k0; k < k1; ++k) {
        double* pk = ph + (int64_t)(k - k0) * n;
        float* qk = pl + (int64_t)(k - k0) * n;
#pragma unroll
        for (int e = 0; e < kTileE; ++e) {                                    // column k of L, the tile's own rows k .. n - 1
            const int i = base + e;
            if (i >= r0 && i >= k && i < n) {
                store_column(pk, qk, i, dd{uh[e], ul[e]});
                if (i == k) d[k] = uh[e];
            }
        }
        if (k == n - 1) break;
        const double* ck = co + 4 * (k - k0);
        const dd nrho = {-ck[0], -ck[1]}, ic = {ck[2], ck[3]};
        const double eh = __shfl_up(uh[kTileE - 1], 1, kWave), el = __shfl_up(ul[kTileE - 1], 1, kWave);
        const dd edge = lane > 0 ? dd{eh, el} : dd{0.0, 0.0};
#pragma unroll
        for (int e = kTileE - 1; e >= 0; --e) {
            const int i = base + e;
            const dd us = e > 0 ? dd{uh[e > 0 ? e - 1 : 0], ul[e > 0 ? e - 1 : 0]} : edge;          // u shifted down by one
            const uv r = rotate(us, dd{vh[e], vl[e]}, nrho, ic);
            const bool live = i > k;                                          // at or above the pivot: u[i] keeps L[i, i]
            uh[e] = live ? r.u.h : uh[e];
            ul[e] = live ? r.u.l : ul[e];
            vh[e] = r.v.h;
            vl[e] = r.v.l;
        }
    }
#pragma unroll
    for (int e = 0; e < kTileE; ++e) {
        const int i = base + e;
        if (i >= r0 && i < n) state_store(so, n, i, uv{{uh[e], ul[e]}, {vh[e], vl[e]}});
    }
}

// sld[theta] = sum_j log dg[theta, j] in k_schur's order: thread tid adds the logarithms of its E consecutive entries in ascending
// order, then sum_log_diag_tree; NaN for a first column that failed.  With E the size class of n (n <= kMaxN) this is
// k_schur's sum bit for bit; beyond, E = ceil(n / kThreads).  grid = m, block = kThreads.
__global__ __launch_bounds__(kThreads) void k_blocked_sld(const double* __restrict__ dg, int n, int E, double* __restrict__ sld,
                                                           const int32_t* __restrict__ info) {
    __shared__ double red[kThreads];
    const int tid = threadIdx.x;
    const int64_t theta = blockIdx.x;
    const int bad = info[theta];                                              // the same in every thread
    const double* d = dg + theta * n;
    double s = 0.0;
    if (!bad) {
        const int64_t base = (int64_t)tid * E;
        for (int e = 0; e < E; ++e)
            if (base + e < n) s += log(d[base + e]);
    }
    sum_log_diag_tree(red, tid, s, bad, sld + theta);
}

// ---- the tiled replay -------------------------------------------------------------------------------------------
// Levinson's step is as local as the Schur step: A'[i] and B'[i] need A[i], B[i-1] and the step's (rho, 1 / c), and every (rho, 1 / c)
// is known before the replay starts (steps, k_coeffs' layout: step k replays row k - 1).  So there is no lead: a panel of kPanelB
// steps is independent tiles with k_schur_tiles' geometry.  The state lives in HBM, (4, n) doubles per first column (A.h, A.l, B.h,
// B.l: state_load / state_store with A as u and B as v), twice, both zero-filled before the first panel: the tiles of a panel read
// one buffer, halo included, and write their own rows to the other.  After step k only the rows 0 .. k are nonzero, so the panel that
// ends with step k1 launches the tiles 0 .. k1 / kTileR; the rows of a tile that was never launched are the zeros of the fill in both
// buffers.  Every element goes through rotate in k_levinson's order, so x is k_levinson's bit for bit.

// The steps k0 + 1 .. min(k0 + kPanelB, n - 1) on the rows of tile blockIdx.x, which owns the rows r0 = blockIdx.x * kTileR .. r0 +
// kTileR - 1 and loads from `cur` the rows from r0 - kPanelB on, kTileE consecutive ones per lane in registers; rows above row 0 and
// beyond n are zeros.  The first panel (k0 == 0) takes A[0] = B[0] = 1 / sqrt(t_0) (t0_rsqrt) instead of the fill.  B's element that
// a shift brings over a lane boundary comes by a lane shuffle: no barrier, no LDS.  After s steps the first s rows of the halo are
// stale; the own rows lie kPanelB below its top and stay exact.  At the end the tile writes its own rows to `nxt`.  A first column
// with info != 0 is skipped.  grid = (k1 / kTileR + 1, cnt), block = kWave.
__global__ __launch_bounds__(kWave) void k_levinson_tiles(const double* __restrict__ t, int n, int k0, const double* __restrict__ cur,
                                                           double* __restrict__ nxt, const double* __restrict__ steps,
                                                           const int32_t* __restrict__ info) {
    const int64_t theta = blockIdx.y;
    if (info[theta] != 0) return;                                             // the same in every lane
    const int lane = threadIdx.x;
    const int r0 = (int)blockIdx.x * kTileR;                                  // the tile's first own row
    const int base = r0 - kPanelB + lane * kTileE;                            // the row of the lane's first element
    const double* s = cur + theta * 4 * (int64_t)n;
    double* so = nxt + theta * 4 * (int64_t)n;
    const double* co = steps + theta * 4 * (int64_t)n;
    double ah[kTileE], al[kTileE], bh[kTileE], bl[kTileE];
#pragma unroll
    for (int e = 0; e < kTileE; ++e) {
        const int i = base + e;
        uv g = i >= 0 && i < n ? state_load(s, n, i) : uv{};
        if (k0 == 0 && i == 0) g.u = g.v = t0_rsqrt(t[theta * n]);
        ah[e] = g.u.h;
        al[e] = g.u.l;
        bh[e] = g.v.h;
        bl[e] = g.v.l;
    }
    const int k1 = min(k0 + kPanelB, n - 1);
    for (int k = k0 + 1; k <= k1; ++k) {
        const double* ck = co + 4 * (int64_t)(k - 1);                         // step k replays row k - 1
        const dd nrho = {-ck[0], -ck[1]}, ic = {ck[2], ck[3]};
        const double eh = __shfl_up(bh[kTileE - 1], 1, kWave), el = __shfl_up(bl[kTileE - 1], 1, kWave);
        const dd edge = lane > 0 ? dd{eh, el} : dd{0.0, 0.0};
#pragma unroll
        for (int e = kTileE - 1; e >= 0; --e) {
            const dd bs = e > 0 ? dd{bh[e > 0 ? e - 1 : 0], bl[e > 0 ? e - 1 : 0]} : edge;          // B shifted down by one
            const uv r = rotate(dd{ah[e], al[e]}, bs, nrho, ic);              // (A, shift(B)) in the roles of (u shifted, v)
            ah[e] = r.u.h;
            al[e] = r.u.l;
            bh[e] = r.v.h;
            bl[e] = r.v.l;
        }
    }
#pragma unroll
    for (int e = 0; e < kTileE; ++e) {
        const int i = base + e;
        if (i >= r0 && i < n) state_store(so, n, i, uv{{ah[e], al[e]}, {bh[e], bl[e]}});
    }
}

// x = A / L[n-1, n-1] from the state st the last panel wrote and row n - 1 of steps: xd (m, n, 2) both words, xf (m, n) the fp64
// rounding, k_levinson's division and its finiteness test.  A first column with info != 0 gives NaN; one whose x is not finite gets
// info = n + 1, a NaN sld and NaN in its x.  Thread tid takes the rows tid, tid + kThreads, ...  grid = m, block = kThreads.
__global__ __launch_bounds__(kThreads) void k_levinson_finish(const double* __restrict__ st, int n, const double* __restrict__ steps,
                                                               double* __restrict__ xd, double* __restrict__ xf, double* __restrict__ sld,
                                                               int32_t* __restrict__ info) {
    __shared__ int s_notfinite;                                               // a flag of its own: k_levinson's __syncthreads_or keeps its code
    const int tid = threadIdx.x;
    const int64_t theta = blockIdx.x;
    double* xo = xd + theta * n * 2;
    double* xr = xf + theta * n;
    int notfinite = info[theta] != 0 ? 2 : 0;                                 // the same in every thread
    if (!notfinite) {
        if (tid == 0) s_notfinite = 0;
        __syncthreads();
        const double* s = st + theta * 4 * (int64_t)n;
        const double* row = steps + (theta * n + (n - 1)) * 4;
        const dd last = {row[0], row[1]};
        for (int i = tid; i < n; i += kThreads) {
            const dd x = dd_div(state_load(s, n, i).u, last);
            xo[2 * i] = x.h;
            xo[2 * i + 1] = x.l;
            xr[i] = x.h;
            if (!dd_finite(x)) notfinite = 1;
        }
        if (notfinite) s_notfinite = 1;                                       // every such thread stores the same word
        __syncthreads();
        notfinite = s_notfinite;
    }
    if (!notfinite) return;
    for (int i = tid; i < n; i += kThreads) xo[2 * i] = xo[2 * i + 1] = xr[i] = NAN;
    if (notfinite == 1 && tid == 0) {
        info[theta] = n + 1;
        sld[theta] = NAN;
    }
}

// k_invdiag with E a runtime number (the size class of n up to kMaxN, ceil(n / kThreads) beyond, as k_blocked_sld takes it): thread
// tid sums its E consecutive terms in ascending order, the totals go through the same nine-step scan, and a second pass forms the
// terms and their running sums again, E being no compile-time array's length, and divides.  For n <= kMaxN this is k_invdiag<E>'s
// arithmetic in k_invdiag<E>'s order.  grid = m, block = kThreads.
__global__ __launch_bounds__(kThreads) void k_invdiag_n(const double* __restrict__ xd, int n, int E, const int32_t* __restrict__ info,
                                                         double* __restrict__ pd) {
    __shared__ double s_tot[2][kThreads][2];
    const int tid = threadIdx.x, base = tid * E;
    const int64_t theta = blockIdx.x;
    double* p = pd + theta * n;
    if (info[theta] != 0) {                                                   // the same in every thread
        for (int e = 0; e < E; ++e)
            if (base + e < n) p[base + e] = NAN;
        return;
    }
    const double* x = xd + theta * n * 2;
    const auto term = [&](int r) {
        const dd a = {x[2 * r], x[2 * r + 1]};
        const dd b = r > 0 ? dd{x[2 * (n - r)], x[2 * (n - r) + 1]} : dd{0.0, 0.0};
        return dd_mul(dd_sub(a, b), dd_add(a, b));
    };
    dd acc = {0.0, 0.0};
    for (int e = 0; e < E; ++e)
        if (base + e < n) acc = dd_add(acc, term(base + e));
    s_tot[0][tid][0] = acc.h;
    s_tot[0][tid][1] = acc.l;
    __syncthreads();
    int cur = 0;
    for (int off = 1; off < kThreads; off <<= 1) {                            // inclusive scan of the totals
        dd s = {s_tot[cur][tid][0], s_tot[cur][tid][1]};
        if (tid >= off) s = dd_add(dd{s_tot[cur][tid - off][0], s_tot[cur][tid - off][1]}, s);
        s_tot[cur ^ 1][tid][0] = s.h;
        s_tot[cur ^ 1][tid][1] = s.l;
        cur ^= 1;
        __syncthreads();
    }
    const dd before = tid > 0 ? dd{s_tot[cur][tid - 1][0], s_tot[cur][tid - 1][1]} : dd{0.0, 0.0};
    const dd x0 = {x[0], x[1]};
    acc = {0.0, 0.0};
    for (int e = 0; e < E; ++e) {
        const int r = base + e;
        if (r < n) {
            acc = dd_add(acc, term(r));
            p[r] = dd_div(dd_add(before, acc), x0).h;
        }
    }
}

}  // namespace gt
