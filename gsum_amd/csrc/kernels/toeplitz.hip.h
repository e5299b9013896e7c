// Kernels of libgsum_toep.so (gfx950 only): the Schur (Bareiss) recursion of a symmetric positive definite Toeplitz matrix T with a
// forward substitution beside it, and the Gram matrices of the solved columns.  DESIGN.md section 18.
//
// k_schur<E, C, VL>: one workgroup per (first column t, chunk of C right-hand-side columns).  The generator pair (u, v) of T = L L^T is
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
template <int E, int C, bool VL>
__global__ __launch_bounds__(kThreads) void k_schur(const double* __restrict__ t, int n, const double* __restrict__ Z,
                                                     const int32_t* __restrict__ ze, int ncols, double* __restrict__ Y,
                                                     double* __restrict__ sld, int32_t* __restrict__ info) {
    __shared__ double s_pub[2][4 + C];
    __shared__ double s_edge[2][kThreads][2];
    __shared__ alignas(16) double s_v[VL ? E : 1][VL ? kThreads : 1][2];      // VL: v lives here, element e of thread tid at [e][tid]
    const int tid = threadIdx.x, base = tid * E;
    const int col0 = blockIdx.x * C, nc = min(C, ncols - col0);
    const int64_t theta = blockIdx.y;
    const double* tt = t + theta * n;
    double* Yt = Y + theta * (int64_t)n * ncols;

    const double t0 = tt[0];
    int bad = (t0 > 0.0 && t0 < INFINITY) ? 0 : 1;                          // the same in every thread
    double uh[E], ul[E], vh[VL ? 1 : E], vl[VL ? 1 : E], z[E][C];
    float zc[E][C];                                                          // sum of lo(L[i, k]) * y_k: the residual is z - zc
    auto get_v = [&](int e) -> dd { return VL ? dd{s_v[VL ? e : 0][VL ? tid : 0][0], s_v[VL ? e : 0][VL ? tid : 0][1]} : dd{vh[VL ? 0 : e], vl[VL ? 0 : e]}; };
    auto set_v = [&](int e, dd x) {
        if (VL) {
            s_v[VL ? e : 0][VL ? tid : 0][0] = x.h;
            s_v[VL ? e : 0][VL ? tid : 0][1] = x.l;
        } else {
            vh[VL ? 0 : e] = x.h;
            vl[VL ? 0 : e] = x.l;
        }
    };
    if (!bad) {
        const dd rs = dd_rsqrt(dd{t0, 0.0});
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int i = base + e;
            const dd u = i < n ? dd_mul_d(rs, tt[i]) : dd{0.0, 0.0};
            uh[e] = u.h;
            ul[e] = u.l;
            set_v(e, i > 0 ? u : dd{0.0, 0.0});
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
        if (k == n - 1) break;
        const dd rho = dd_div(dd{s_pub[b][2], s_pub[b][3]}, pu);
        if (!(fabs(rho.h) < 1.0)) {                                          // also a NaN; the same in every thread
            bad = k + 2;
            break;
        }
        const dd ic = dd_rsqrt(dd_mul(dd_sub(dd{1.0, 0.0}, rho), dd_add(dd{1.0, 0.0}, rho)));
        const dd nrho = dd_neg(rho);
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
                const dd v = get_v(e);
                const dd un = dd_mul(dd_add(us, dd_mul(nrho, v)), ic);
                const dd vn = dd_mul(dd_add(v, dd_mul(nrho, us)), ic);
                const bool live = i > k;                                      // at or above the pivot: u[i] keeps L[i, i]
                uh[e] = live ? un.h : uh[e];
                ul[e] = live ? un.l : ul[e];
                set_v(e, vn);
                if (i == k + 1) {
                    s_pub[nb][0] = un.h;
                    s_pub[nb][1] = un.l;
#pragma unroll
                    for (int c = 0; c < C; ++c) s_pub[nb][4 + c] = z[e][c] - (double)zc[e][c];
                }
                if (i == k + 2) {
                    s_pub[nb][2] = vn.h;
                    s_pub[nb][3] = vn.l;
                }
            }
            s_edge[nb][tid][0] = uh[E - 1];
            s_edge[nb][tid][1] = ul[E - 1];
        }
        __syncthreads();
    }

    if (blockIdx.x != 0) return;                                             // every chunk of a first column finds the same two numbers
    __syncthreads();
    double* red = &s_edge[0][0][0];
    double s = 0.0;
    if (!bad) {
#pragma unroll
        for (int e = 0; e < E; ++e)
            if (base + e < n) s += log(uh[e]);
    }
    red[tid] = s;
    __syncthreads();
    for (int stride = kThreads / 2; stride > 0; stride >>= 1) {
        if (tid < stride) red[tid] += red[tid + stride];
        __syncthreads();
    }
    if (tid == 0) {
        sld[theta] = bad ? NAN : red[0];
        info[theta] = bad;
    }
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

}  // namespace gt
