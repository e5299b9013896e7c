// Reference-distribution kernels (the band stage of gsum's GraphicalDiagnostic on the device): tile transpose, segment sort on
// order-preserving 64-bit keys (one workgroup's LDS up to kSortLds doubles, chunk sort + merge passes in global memory above),
// percentile picks out of sorted rows, interval coverage counts.  Host side: gsum_refdist.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gr {

constexpr int kSortLds = 16384;          // doubles one workgroup sorts in its LDS (128 KiB of the CU's 160 KiB): THE switch to merge passes
constexpr int kSortThreads = 1024;       // at most; a short segment runs on fewer (one compare-exchange per lane and step at least)
constexpr int kThreads = 256;            // every other kernel here
constexpr int kTile = 64;                // transpose tile (64 x 65 doubles of LDS: the pad keeps the column reads off one bank pair)
constexpr int kCovK = 8;                 // coverage: intervals per workgroup (counters in registers)
constexpr int kCovI = 128;               // coverage: points per LDS stage of the bounds
constexpr uint64_t kPadKey = ~0ull;      // the key of +NaN with a full payload: sorts after everything, pads a segment to a power of 2

// double -> key with key(a) < key(b) <=> a < b for everything but NaN and the zeros: -0.0 sorts just before +0.0 (they compare
// equal, either order is a sorted order) and a NaN of either sign becomes +NaN (payload kept), above +inf, so NaN sorts last.
// NaNs order among themselves by payload, and kPadKey is the key of the +NaN whose payload is all ones: a pad and such a NaN are
// the same key and decode to the same bits, and only the first len keys of a segment are written back, so the sort stays correct;
// the order and sign of NaNs within the NaN tail can differ from numpy's (their positions cannot).
__device__ inline uint64_t to_key(double x) {
    uint64_t u = (uint64_t)__double_as_longlong(x);
    if ((u & 0x7fffffffffffffffull) > 0x7ff0000000000000ull) u &= 0x7fffffffffffffffull;
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

__device__ inline double from_key(uint64_t k) {
    const uint64_t u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)u);
}

// ---- transpose: out (cols x rows) = in (rows x cols)^T, 64 x 64 tiles through LDS, both sides coalesced --------------------------
__global__ __launch_bounds__(kThreads) void k_transpose(const double* __restrict__ in, int64_t rows, int64_t cols,
                                                        double* __restrict__ out) {
    __shared__ double tile[kTile][kTile + 1];
    const int tx = threadIdx.x & (kTile - 1), ty = threadIdx.x / kTile;             // 64 x 4
    const int64_t tiles_x = (cols + kTile - 1) / kTile;                             // 1-D grid: a tall matrix has more tile rows than a grid's y
    const int64_t c0 = (int64_t)(blockIdx.x % tiles_x) * kTile, r0 = (int64_t)(blockIdx.x / tiles_x) * kTile;
    for (int r = ty; r < kTile; r += kThreads / kTile)
        if (r0 + r < rows && c0 + tx < cols) tile[r][tx] = in[(r0 + r) * cols + c0 + tx];
    __syncthreads();
    for (int c = ty; c < kTile; c += kThreads / kTile)
        if (c0 + c < cols && r0 + tx < rows) out[(c0 + c) * rows + r0 + tx] = tile[tx][c];
}

// ---- segment sort in LDS ---------------------------------------------------------------------------------------------------------
// Workgroup b sorts chunk (b % chunks) of segment (b / chunks): P keys (a power of two <= kSortLds; elements past the segment's end
// are kPadKey) through a bitonic network in LDS.  KEYS_OUT = false (chunks == 1): the first len values go back as doubles to
// dst + seg * stride (dst may be src: the whole segment is in LDS before the first store).  KEYS_OUT = true: all P keys go to
// keys + seg * chunks * P + chunk * P, sorted runs for k_merge_pass.
template <bool KEYS_OUT>
__global__ __launch_bounds__(kSortThreads) void k_sort_lds(const double* src, int64_t stride, int64_t len, int chunks,
                                                           int P, double* dst, uint64_t* __restrict__ keys) {
    extern __shared__ uint64_t sk[];
    const int64_t seg = blockIdx.x / chunks;
    const int chunk = (int)(blockIdx.x % chunks);
    const int64_t base = (int64_t)chunk * P;
    const double* s = src + seg * stride;
    for (int t = threadIdx.x; t < P; t += blockDim.x) sk[t] = base + t < len ? to_key(s[base + t]) : kPadKey;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < (P >> 1); t += blockDim.x) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const uint64_t a = sk[i], b = sk[i + j];
                if ((a > b) == ((i & k) == 0)) {
                    sk[i] = b;
                    sk[i + j] = a;
                }
            }
            __syncthreads();
        }
    if (KEYS_OUT) {
        uint64_t* o = keys + (seg * chunks + chunk) * (int64_t)P;
        for (int t = threadIdx.x; t < P; t += blockDim.x) o[t] = sk[t];
    } else {
        double* o = dst + seg * stride;
        for (int t = threadIdx.x; t < P && t < len; t += blockDim.x) o[t] = from_key(sk[t]);
    }
}

// One merge pass over segments of Lp keys made of sorted runs of w: runs (2r, 2r + 1) merge into one run of 2w (the last run of a
// segment may be short or alone).  One lane per key: its place is its index in its own run plus its rank in the other one, lower
// bound for the left run's keys and upper bound for the right run's, so equal keys keep their order and every place is taken once.
__global__ __launch_bounds__(kThreads) void k_merge_pass(const uint64_t* __restrict__ in, uint64_t* __restrict__ out, int64_t Lp,
                                                         int64_t w, int64_t total) {
    const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (g >= total) return;
    const int64_t seg = g / Lp, p = g - seg * Lp;
    const int64_t a0 = p / (2 * w) * (2 * w), off = p - a0;
    const int64_t la = Lp - a0 < w ? Lp - a0 : w;
    const int64_t lb = Lp - a0 - la < w ? Lp - a0 - la : w;
    const uint64_t* A = in + seg * Lp + a0;
    const uint64_t* B = A + la;
    const uint64_t x = A[off];
    int64_t lo = 0, hi, place;
    if (off < la) {                              // #{B < x}
        hi = lb;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (B[mid] < x) lo = mid + 1; else hi = mid;
        }
        place = off + lo;
    } else {                                     // #{A <= x}
        hi = la;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (A[mid] <= x) lo = mid + 1; else hi = mid;
        }
        place = off - la + lo;
    }
    out[seg * Lp + a0 + place] = x;
}

__global__ __launch_bounds__(kThreads) void k_keys_to_double(const uint64_t* __restrict__ keys, int64_t Lp, int64_t len, int64_t stride,
                                                             int64_t total, double* __restrict__ dst) {
    const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (g >= total) return;
    const int64_t seg = g / len, p = g - seg * len;
    dst[seg * stride + p] = from_key(keys[seg * Lp + p]);
}

// ---- percentiles of sorted rows: numpy.percentile's 'linear' method ---------------------------------------------------------------
// S (n x m, every row ascending, NaN last).  A lane per row, every q in turn: a = S[row, idx[q]], b = S[row, min(idx[q] + 1, m - 1)], g = gamma[q]:
// a + (b - a) g, and b - (b - a)(1 - g) where g >= 0.5 (numpy's _lerp), every operation rounded on its own (contraction off: no fused multiply-add); NaN when the row holds
// one (its last entry).  idx and gamma come from the host (numpy's own (m - 1) * (q / 100), floor and difference).
__global__ __launch_bounds__(kThreads) void k_pick(const double* __restrict__ S, int64_t n, int64_t m, const int64_t* __restrict__ idx,
                                                   const double* __restrict__ gamma, int nq, double* __restrict__ out) {
#pragma clang fp contract(off)
    const int64_t row = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (row >= n) return;
    const double* s = S + row * m;
    const double last = s[m - 1];
    for (int q = 0; q < nq; ++q) {
        const int64_t i = idx[q], i1 = i + 1 < m ? i + 1 : m - 1;
        const double a = s[i], b = s[i1], g = gamma[q];
        const double d = b - a;
        double r = a + d * g;
        if (g >= 0.5) r = b - d * (1.0 - g);
        if (last != last) r = last;
        out[(int64_t)q * n + row] = r;
    }
}

// ---- interval coverage ------------------------------------------------------------------------------------------------------------
// counts[j, k] += #{ i in this workgroup's slice : lower[k, i] < Y[i, j] < upper[k, i] } (both strict, false for NaN).  A lane per
// curve j (Y read coalesced along j), kCovK intervals per workgroup with their counters in registers, the bounds of kCovI points at
// a time staged in LDS as (lower, upper) pairs and read as wave-uniform broadcasts.  blockIdx: x = curves, y = interval block,
// z = slice of the points.  The counters are integers: the order of the atomic adds cannot change the result.
__global__ __launch_bounds__(kThreads) void k_coverage(const double* __restrict__ Y, int64_t n, int64_t m, const double* __restrict__ lower,
                                                       const double* __restrict__ upper, int K, int64_t slice,
                                                       unsigned long long* __restrict__ counts) {
    __shared__ double2 lu[kCovI][kCovK];
    const int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int k0 = blockIdx.y * kCovK;
    const int64_t i0 = (int64_t)blockIdx.z * slice, i1 = i0 + slice < n ? i0 + slice : n;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    int c[kCovK];
#pragma unroll
    for (int k = 0; k < kCovK; ++k) c[k] = 0;
    for (int64_t ib = i0; ib < i1; ib += kCovI) {
        __syncthreads();
        for (int t = threadIdx.x; t < kCovI * kCovK; t += kThreads) {      // i fastest: coalesced along a row of the bounds
            const int k = t / kCovI, i = t % kCovI;
            const bool ok = k0 + k < K && ib + i < i1;
            lu[i][k] = ok ? make_double2(lower[(int64_t)(k0 + k) * n + ib + i], upper[(int64_t)(k0 + k) * n + ib + i]) : make_double2(nan, nan);
        }
        __syncthreads();
        if (j < m) {
            const int cnt = (int)(i1 - ib < kCovI ? i1 - ib : kCovI);
            for (int i = 0; i < cnt; ++i) {
                const double y = Y[(ib + i) * m + j];
#pragma unroll
                for (int k = 0; k < kCovK; ++k) c[k] += (lu[i][k].x < y) & (y < lu[i][k].y);
            }
        }
    }
    if (j < m)
#pragma unroll
        for (int k = 0; k < kCovK; ++k)
            if (k0 + k < K && c[k]) atomicAdd(&counts[j * K + k0 + k], (unsigned long long)c[k]);
}

}  // namespace gr
