// Variogram kernels (gsum.helpers.VariogramFourthRoot on the device): the pair stage (distances, bins, per-bin sums, the
// compacted pair list of every bin) and the cov stage (sum over all pairs of two bins of cov_ijkl).  Host side: gsum_vario.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gv {

constexpr int kThreads = 256;            // every kernel here: one workgroup of 256 lanes
constexpr int kTile = 256;               // cov stage: pairs of bin 1 per tile (one per lane) = pairs of bin 2 per tile (the loop)
constexpr int kBoundsLds = 4096;         // bounds searched in LDS up to this many (32 KB), in global memory above
constexpr int kGammaLds = 6144;          // gamma~ entries (bins x curves of a group) kept in LDS up to this many (48 KB)

// ---- distance: bit-identical to numpy.linalg.norm(X[:, None, :] - X, axis=-1) ----------------------------------------------
// s = add.reduce(d * d): numpy's pairwise_sum for n <= 128 (sequential from -0.0 below 8 terms; eight accumulators from 8, folded
// ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then the tail), and the correctly rounded sqrt.  No contraction.
__device__ inline double pair_distance(const double* __restrict__ xi, const double* __restrict__ xj, int d) {
#pragma clang fp contract(off)
    double s;
    if (d < 8) {
        s = -0.0;
        for (int k = 0; k < d; ++k) {
            const double t = xi[k] - xj[k];
            s += t * t;
        }
    } else {
        double r[8];
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            const double t = xi[m] - xj[m];
            r[m] = t * t;
        }
        int k = 8;
        for (; k < d - (d % 8); k += 8) {
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                const double t = xi[k + m] - xj[k + m];
                r[m] += t * t;
            }
        }
        s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; k < d; ++k) {
            const double t = xi[k] - xj[k];
            s += t * t;
        }
    }
    return __builtin_sqrt(s);
}

// numpy.digitize(h, bounds) for non-decreasing bounds = #{bounds <= h}
__device__ inline int digitize(const double* bounds, int nb, double h) {
    int lo = 0, hi = nb;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (bounds[mid] <= h) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// tril index p -> (i, j), i > j, numpy.tril_indices(N, -1) order: p = i (i - 1) / 2 + j
__device__ inline void tril_pair(int64_t p, int& i, int& j) {
    int64_t r = (int64_t)((1.0 + __builtin_sqrt(1.0 + 8.0 * (double)p)) * 0.5);
    while (r * (r - 1) / 2 > p) --r;
    while ((r + 1) * r / 2 <= p) ++r;
    i = (int)r;
    j = (int)(p - r * (r - 1) / 2);
}

__device__ inline const double* stage_bounds(const double* bounds, int nbnd, double* lds) {
    if (nbnd > kBoundsLds) return bounds;
    for (int k = threadIdx.x; k < nbnd; k += blockDim.x) lds[k] = bounds[k];
    __syncthreads();
    return lds;
}

// ---- pair stage ---------------------------------------------------------------------------------------------------------------
// The N x N bin table, both triangles and the diagonal (the bin of distance 0): T[a * N + b] = digitize(|X_a - X_b|).
__global__ void __launch_bounds__(kThreads) k_bin_table(const double* __restrict__ X, int n, int d, const double* __restrict__ bounds,
                                                        int nbnd, int16_t* __restrict__ T) {
    __shared__ double lb[kBoundsLds];
    const double* bb = stage_bounds(bounds, nbnd, lb);
    const int b = blockIdx.x * 64 + (threadIdx.x & 63);
    const int a = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (a >= n || b >= n) return;
    const double h = pair_distance(X + (size_t)a * d, X + (size_t)b * d, d);
    T[(size_t)a * n + b] = (int16_t)digitize(bb, nbnd, h);
}

// Per chunk of the tril order, the number of pairs in each bin (integer atomics: exact).
__global__ void __launch_bounds__(kThreads) k_pair_count(const int16_t* __restrict__ T, int n, int64_t P, int64_t chunk, int nbin,
                                                         int* __restrict__ cnt) {
    const int64_t p0 = (int64_t)blockIdx.x * chunk, p1 = min(P, p0 + chunk);
    int* c = cnt + (size_t)blockIdx.x * nbin;
    for (int64_t p = p0 + threadIdx.x; p < p1; p += blockDim.x) {
        int i, j;
        tril_pair(p, i, j);
        atomicAdd(&c[T[(size_t)i * n + j]], 1);
    }
}

// Stable scatter of each chunk's pairs into the per-bin lists: cur[chunk][bin] starts at the pair's list position (host scan) and
// advances by sub-tiles of 256 in tril order; within a sub-tile a pair's rank among equal bins is counted from LDS.
__global__ void __launch_bounds__(kThreads) k_pair_scatter(const int16_t* __restrict__ T, int n, int64_t P, int64_t chunk, int nbin,
                                                           int* __restrict__ cur, uint32_t* __restrict__ pairs) {
    __shared__ int sb[kThreads];
    const int64_t p0 = (int64_t)blockIdx.x * chunk, p1 = min(P, p0 + chunk);
    int* c = cur + (size_t)blockIdx.x * nbin;
    for (int64_t s = p0; s < p1; s += kThreads) {
        const int64_t p = s + threadIdx.x;
        int i = 0, j = 0, b = -1;
        if (p < p1) {
            tril_pair(p, i, j);
            b = T[(size_t)i * n + j];
        }
        sb[threadIdx.x] = b;
        __syncthreads();
        int rank = 0, last = 1;
        for (int u = 0; u < kThreads; ++u) {
            const int e = sb[u] == b;
            rank += (u < (int)threadIdx.x) & e;
            last &= !((u > (int)threadIdx.x) & e);
        }
        if (b >= 0) {
            const int base = __hip_atomic_load(&c[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            pairs[base + rank] = ((uint32_t)i << 16) | (uint32_t)j;
        }
        __threadfence();
        __syncthreads();
        if (b >= 0 && last) __hip_atomic_fetch_add(&c[b], rank + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __threadfence();
        __syncthreads();
    }
}

__device__ inline double block_sum(double v, double* red) {           // fixed tree order: deterministic
    red[threadIdx.x] = v;
    __syncthreads();
    for (int w = kThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// One workgroup per bin: sum h over the bin's pairs, and per curve sum sqrt|z_i - z_j|.  Lane-strided, then a fixed tree.
__global__ void __launch_bounds__(kThreads) k_bin_sums(const double* __restrict__ X, int n, int d, const double* __restrict__ Z,
                                                       int ncurves, const uint32_t* __restrict__ pairs, const int* __restrict__ start,
                                                       double* __restrict__ h_sum, double* __restrict__ dij_sum) {
    __shared__ double red[kThreads];
    const int bin = blockIdx.x;
    const int q0 = start[bin], q1 = start[bin + 1];
    double acc = 0.0;
    for (int q = q0 + threadIdx.x; q < q1; q += kThreads) {
        const uint32_t pr = pairs[q];
        acc += pair_distance(X + (size_t)(pr >> 16) * d, X + (size_t)(pr & 0xffff) * d, d);
    }
    double s = block_sum(acc, red);
    if (threadIdx.x == 0) h_sum[bin] = s;
    for (int c = 0; c < ncurves; ++c) {
        const double* z = Z + (size_t)c * n;
        acc = 0.0;
        for (int q = q0 + threadIdx.x; q < q1; q += kThreads) {
            const uint32_t pr = pairs[q];
            acc += __builtin_sqrt(__builtin_fabs(z[pr >> 16] - z[pr & 0xffff]));
        }
        s = block_sum(acc, red);
        if (threadIdx.x == 0) dij_sum[(size_t)bin * ncurves + c] = s;
    }
}

// ---- the correlation map ---------------------------------------------------------------------------------------------------------
// corr(rho) = corr_factor ((1 - rho^2) 2F1(3/4, 3/4; 1/2; rho^2) - 1) = corr_factor (f(rho^2) - 1), f = 2F1(-1/4, -1/4; 1/2; .);
// rho >= 1 -> 1, rho <= -1 -> -1, NaN -> NaN (helpers.py:652-660).  Near x = rho^2 = 1, t = 1 - x = (1 - |rho|)(1 + |rho|) is formed
// from rho (1 - |rho| is exact there), so the t log t term does not inherit the rounding of rho^2.
// BEGIN generated by tools/gen_vario_coeffs.py
constexpr int kVarioPn = 20;
__device__ constexpr double kVarioP[kVarioPn] = {
    0.05552026035340104,
    -0.21767285743682724,
    0.4072042820071081,
    -0.47190887601440956,
    0.3786296561404635,
    -0.22067679402686505,
    0.09743133445794507,
    -0.03212537835246195,
    0.00896154292313246,
    -0.0010490749320131683,
    0.0010297980507541784,
    0.0009268876571756488,
    0.001221614766042665,
    0.001605076691919234,
    0.002209114543547023,
    0.003231048363041569,
    0.005169677738361632,
    0.009570312499962047,
    0.023437500000000142,
    0.125,
};
constexpr int kVarioAn = 19;
__device__ constexpr double kVarioA[kVarioAn] = {
    -0.00985883729625971,
    0.03586449746970802,
    -0.06261274598268556,
    0.06733950264511074,
    -0.050071217442722034,
    0.02669832455843497,
    -0.010892032207249821,
    0.0030613382588376777,
    -0.0009970170083601353,
    -0.00019010053793158796,
    -0.00045305152657250326,
    -0.0006126648509330605,
    -0.0009157660371530022,
    -0.001472686278302665,
    -0.002650666134205225,
    -0.005730364361825522,
    -0.01764889034908005,
    -0.14881811214150087,
    0.18034059901609623,
};
constexpr int kVarioBn = 19;
__device__ constexpr double kVarioB[kVarioBn] = {
    0.15148013237076002,
    -0.5586800639530656,
    0.9811815773505715,
    -1.0616287268996654,
    0.7911610365619158,
    -0.42457968496867116,
    0.1718272657450337,
    -0.05063760528375011,
    0.013374458935784086,
    -0.0005034314858085687,
    0.002165105723637534,
    0.0022329269384738296,
    0.0027802291781834115,
    0.003529192424691503,
    0.004692688440583974,
    0.00667404112204726,
    0.010590214115392446,
    0.02074817459207695,
    0.07377128743850601,
};
// END generated by tools/gen_vario_coeffs.py

template <int N>
__device__ inline double horner(const double (&c)[N], double v) {
    double r = c[0];
#pragma unroll
    for (int k = 1; k < N; ++k) r = __builtin_fma(r, v, c[k]);
    return r;
}

__device__ inline double vario_corr(double rho, double corr_factor) {
    const double x = rho * rho;
    double g;
    if (x < 0.5) {
        g = x * horner(kVarioP, x);
    } else {
        const double a = __builtin_fabs(rho);
        const double t = (1.0 - a) * (1.0 + a);
        g = horner(kVarioA, t) + (t * log(t)) * horner(kVarioB, t);
    }
    double c = g * corr_factor;
    c = rho >= 1.0 ? 1.0 : c;
    c = rho <= -1.0 ? -1.0 : c;
    return c;
}

__global__ void __launch_bounds__(kThreads) k_corr(const double* __restrict__ rho, int64_t m, double corr_factor, double* __restrict__ out) {
    const int64_t k = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (k < m) out[k] = vario_corr(rho[k], corr_factor);
}

// ---- cov stage ---------------------------------------------------------------------------------------------------------------------
struct Tile {
    int32_t req;          // bin pair (request) index
    int32_t p0, np;       // pairs [p0, p0 + np) of bin 1 (one per lane), positions in the pair list
    int32_t q0, nq;       // pairs [q0, q0 + nq) of bin 2 (the loop)
    int32_t kind;         // 0: b1 != b2;  1: b1 == b2, q-tile below the p-tile;  2: b1 == b2, the diagonal tile
};

// S[req, c] partial of one tile and one group of CG curves: sum over p, q of corr(p, q, c) sqrt(var1 var2), where
// rho = (g(j,k) + g(i,l) - g(i,k) - g(j,l)) / den[req, c] left to right, g(a,b) = gamma~[T[a,b], c], den = 2 sqrt(gamma~[b1] gamma~[b2])
// and sq = sqrt(var1 var2) from the host.  For b1 == b2 only q < p is evaluated and doubled (t(p,q) = t(q,p): T is symmetric); the
// q == p term is 1 * sq without any lookup.  Lanes own p, so the table rows read in the loop are the wave-uniform k and l: row k at
// columns i and j, row l likewise (T[k, j] = T[j, k]).
template <int CG>
__global__ void __launch_bounds__(kThreads) k_cov(const Tile* __restrict__ tiles, const int32_t* __restrict__ order,
                                                  const uint32_t* __restrict__ pairs, const int16_t* __restrict__ T, int n,
                                                  const double* __restrict__ gam, int nbin, const double* __restrict__ den,
                                                  const double* __restrict__ sq, int ncp, double corr_factor, double* __restrict__ slab) {
    extern __shared__ double lg[];                                    // dynamic: Nb x CG doubles when that is <= kGammaLds, else none
    __shared__ uint32_t lq[kTile];
    __shared__ double red[kThreads];
    const int tid = order[blockIdx.x];
    const Tile tl = tiles[tid];
    const int c0 = blockIdx.y * CG;
    const double* g = gam + (size_t)blockIdx.y * nbin * CG;            // [bin][CG] of this curve group
    if (nbin * CG <= kGammaLds) {
        for (int k = threadIdx.x; k < nbin * CG; k += kThreads) lg[k] = g[k];
        g = lg;
    }
    if ((int)threadIdx.x < tl.nq) lq[threadIdx.x] = pairs[tl.q0 + threadIdx.x];
    __syncthreads();

    double dn[CG], s[CG], acc[CG];
#pragma unroll
    for (int c = 0; c < CG; ++c) {
        dn[c] = den[(size_t)tl.req * ncp + c0 + c];
        s[c] = sq[(size_t)tl.req * ncp + c0 + c];
        acc[c] = 0.0;
    }
    const bool valid = (int)threadIdx.x < tl.np;
    const uint32_t pp = valid ? pairs[tl.p0 + threadIdx.x] : 0u;
    const int i = (int)(pp >> 16), j = (int)(pp & 0xffff);
    const int lim = !valid ? 0 : tl.kind == 2 ? (int)threadIdx.x : tl.nq;
    // the loop runs to the wave's largest bound (wave-uniform trip count); lanes past their own bound are masked
    int wlim = lim;
    for (int o = 32; o > 0; o >>= 1) wlim = max(wlim, __shfl_xor(wlim, o));
    for (int u = 0; u < wlim; ++u) {
        if (u < lim) {
            const uint32_t qq = lq[u];
            const int16_t* rk = T + (size_t)(qq >> 16) * n;
            const int16_t* rl = T + (size_t)(qq & 0xffff) * n;
            const int bjk = rk[j], bil = rl[i], bik = rk[i], bjl = rl[j];
#pragma unroll
            for (int c = 0; c < CG; ++c) {
                const double num = ((g[bjk * CG + c] + g[bil * CG + c]) - g[bik * CG + c]) - g[bjl * CG + c];
                const double rho = num / dn[c];
                acc[c] += vario_corr(rho, corr_factor) * s[c];
            }
        }
    }
#pragma unroll
    for (int c = 0; c < CG; ++c) {
        double v = tl.kind == 0 ? acc[c] : 2.0 * acc[c];
        if (tl.kind == 2 && valid) v += 1.0 * s[c];
        const double r = block_sum(v, red);
        if (threadIdx.x == 0) slab[(size_t)tid * ncp + c0 + c] = r;
    }
}

// sums[req, c] = the request's tile partials in tile order (tiles of one request are consecutive in [tstart[req], tstart[req + 1]))
__global__ void __launch_bounds__(kThreads) k_cov_reduce(const double* __restrict__ slab, const int32_t* __restrict__ tstart, int nreq,
                                                         int nc, int ncp, double* __restrict__ out) {
    const int k = blockIdx.x * kThreads + threadIdx.x;
    if (k >= nreq * nc) return;
    const int r = k / nc, c = k % nc;
    double s = 0.0;
    for (int t = tstart[r]; t < tstart[r + 1]; ++t) s += slab[(size_t)t * ncp + c];
    out[k] = s;
}

}  // namespace gv
