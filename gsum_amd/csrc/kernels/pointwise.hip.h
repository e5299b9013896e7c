// Kernels of libgsum_pointwise.so (TruncationPointwise): first differences, the grid log likelihood, interval coverage.
// All fp64 VALU work: divisions, integer powers, logarithms, compares.  No MFMA, no floating-point atomics.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

namespace gp {

constexpr int kThreads = 256;                      // four waves
constexpr int kWave = 64;
constexpr int kPerThread = 4;                      // points of one thread in k_loglike
constexpr int kSegment = kThreads * kPerThread;    // points of one workgroup in k_loglike: the fixed partition of a row
constexpr int kCovD = 128;                         // intervals of one k_coverage workgroup (blockIdx.y)
constexpr int kMaxOrders = 64;                     // orders a handle takes; bounds k_coverage's LDS at kCovD * 64 * 4 bytes

// how the reference scale reaches the kernel (gsum_pointwise.h: GSUM_POINTWISE_REF_*)
enum RefMode { kRefScalar = 0, kRefPoints = 1, kRefRowScalar = 2, kRefRowPoints = 3 };

// dy[j', i] = y[i, col(j')] - y[i, col(j') - 1] over the kept columns (y[i, 0] itself for column 0), one rounding as numpy.diff;
// stored order-major so that k_loglike reads along the points.
__global__ __launch_bounds__(kThreads) void k_differences(const double* __restrict__ y, int64_t n, int k, const int* __restrict__ cols, int kp,
                                                          double* __restrict__ dy) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= n * kp) return;
    const int64_t i = e / kp;
    const int jp = (int)(e % kp), c = cols[jp];
    const double v = y[i * k + c];
    dy[(int64_t)jp * n + i] = c ? v - y[i * k + c - 1] : v;
}

// r^o for an integer o by binary exponentiation: at most 2 log2|o| roundings
__device__ inline double powi(double r, int o) {
    unsigned u = o < 0 ? 0u - (unsigned)o : (unsigned)o;
    double p = 1.0, b = r;
    while (u) {
        if (u & 1u) p *= b;
        u >>= 1;
        if (u) b *= b;
    }
    return o < 0 ? 1.0 / p : p;
}

// the sum of v over the wave in a fixed tree; every lane must call it, lane 0 holds the result
__device__ inline double wave_sum(double v) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
    return v;
}

// ---- grid log likelihood ----------------------------------------------------------------------------------------------------------
// Row g, segment b (blockIdx.x = (g - g0) * nb + b): partial[g * nb + b] = sum over the segment's points i of
//     0.5 * df * log((prior + sum_j c_ij^2) / 2)  [+ log|ref_i| + S * log(ratio_gi)  when jac_points],
// c_ij = dy[j, i] / (ref_i * ratio_gi^order_j), prior = df0 * scale0^2, S = the sum of the kept orders.
// The partition of a row into segments, the order in which a thread adds its kPerThread points, the shuffle tree of a wave and the
// order in which the four waves are added depend on n alone: a row has the same bits whatever G is and however the grid is batched.
// A scalar ratio (ratio_is_row == 0) reads ratios[g] only; the reference scale is read as ref_mode says.
__global__ __launch_bounds__(kThreads) void k_loglike(const double* __restrict__ dy, const int* __restrict__ orders, int kp, int64_t n,
                                                      const double* __restrict__ ratios, int ratio_is_row, const double* __restrict__ refs,
                                                      int ref_mode, int64_t g0, int64_t nb, double prior, double df, double S, int jac_points,
                                                      double* __restrict__ partial) {
    __shared__ double wsum[kThreads / kWave];
    const int64_t g = g0 + blockIdx.x / nb, b = blockIdx.x % nb;
    const double row_ratio = ratio_is_row ? 0.0 : ratios[g];
    const double row_ref = ref_mode == kRefScalar ? refs[0] : ref_mode == kRefRowScalar ? refs[g] : 0.0;
    double acc = 0.0;
#pragma unroll
    for (int u = 0; u < kPerThread; ++u) {
        const int64_t i = b * kSegment + u * kThreads + threadIdx.x;
        if (i < n) {
            const double ratio = ratio_is_row ? ratios[g * n + i] : row_ratio;
            const double ref = ref_mode == kRefPoints ? refs[i] : ref_mode == kRefRowPoints ? refs[g * n + i] : row_ref;
            double s = 0.0;
            for (int j = 0; j < kp; ++j) {
                const double c = dy[(int64_t)j * n + i] / (ref * powi(ratio, orders[j]));
                s += c * c;
            }
            double term = 0.5 * (df * log((prior + s) / 2.0));
            if (jac_points) term += log(fabs(ref)) + S * log(ratio);
            acc += term;
        }
    }
    acc = wave_sum(acc);
    if (threadIdx.x % kWave == 0) wsum[threadIdx.x / kWave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[g * nb + b] = ((wsum[0] + wsum[1]) + (wsum[2] + wsum[3]));
}

// out[g] = the sum of the nb partials of row g, one wave per row: lane l adds partials l, l + 64, ... in order, then the shuffle
// tree.  When the change of variables counts once (scalar ratio and scalar ref: !jac_points) its one term is added here.
__global__ __launch_bounds__(kWave) void k_loglike_rows(const double* __restrict__ partial, int64_t nb, int64_t g0, const double* __restrict__ ratios,
                                                        const double* __restrict__ refs, int ref_mode, double S, int jac_points,
                                                        double* __restrict__ out) {
    const int64_t g = g0 + blockIdx.x;
    double acc = 0.0;
    for (int64_t b = threadIdx.x; b < nb; b += kWave) acc += partial[g * nb + b];
    acc = wave_sum(acc);
    if (threadIdx.x == 0) {
        if (!jac_points) acc += log(fabs(refs[ref_mode == kRefRowScalar ? g : 0])) + S * log(ratios[g]);
        out[g] = acc;
    }
}

// ---- interval coverage ------------------------------------------------------------------------------------------------------------
// counts[d, j] += #{ i : t_lo[d] * scale[i, j] + loc[i, j] < data[i, j or 0] < t_hi[d] * scale[i, j] + loc[i, j] }, both strict and
// false for NaN.  Each bound is a multiply rounded and then an add rounded (contraction off: scipy's ppf * scale + loc rounds
// twice), and exists only in a register.  A lane per point, the tiles of kThreads points strided over blockIdx.x; blockIdx.y picks
// kCovD intervals.  A wave's lanes are counted with a ballot, the workgroup's counters live in LDS, and one 64-bit atomic per
// non-zero counter leaves the workgroup.  The counters are integers: the order of the adds cannot change the result.
__global__ __launch_bounds__(kThreads) void k_coverage(const double* __restrict__ loc, const double* __restrict__ scale, const double* __restrict__ data,
                                                       int data_cols, int64_t n, int kp, const double* __restrict__ t_lo,
                                                       const double* __restrict__ t_hi, int D, unsigned long long* __restrict__ counts) {
    __shared__ unsigned int c[kCovD * kMaxOrders];
    const int d0 = blockIdx.y * kCovD, nd = D - d0 < kCovD ? D - d0 : kCovD;
    for (int t = threadIdx.x; t < nd * kp; t += kThreads) c[t] = 0;
    __syncthreads();
    const int64_t tiles = (n + kThreads - 1) / kThreads;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t i = tile * kThreads + threadIdx.x;
        const bool live = i < n;
        for (int j = 0; j < kp; ++j) {
            const double nan = __longlong_as_double(0x7ff8000000000000ll);
            const double l = live ? loc[i * kp + j] : nan, s = live ? scale[i * kp + j] : nan;
            const double y = live ? data[data_cols == 1 ? i : i * kp + j] : nan;
            for (int d = 0; d < nd; ++d) {
                bool in;
                {
#pragma clang fp contract(off)
                    const double lo_s = t_lo[d0 + d] * s, hi_s = t_hi[d0 + d] * s;
                    const double lower = lo_s + l, upper = hi_s + l;
                    in = (lower < y) & (y < upper);
                }
                const unsigned long long mask = __ballot(in);
                if (threadIdx.x % kWave == 0 && mask) atomicAdd(&c[d * kp + j], (unsigned int)__popcll(mask));
            }
        }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < nd * kp; t += kThreads)
        if (c[t]) atomicAdd(&counts[(int64_t)(d0 + t / kp) * kp + t % kp], (unsigned long long)c[t]);
}

}  // namespace gp
