// the K window of a trailing-update tile from the panel solves' zero flags (grouped batch schedule)
// (plain C++: included by gsum_kernels.hip.h for the device code and, on its own, by host programs -- tests/c_host/zwin_host.cpp)
#pragma once
#include <stdint.h>
#if defined(__HIPCC__) || defined(__CUDACC__)
#define GS_ZW_HD __host__ __device__
#else
#define GS_ZW_HD
#endif

// A flag byte per (outer step p, 16-row group g) of a member: flags[p * pstride + g] != 0 when any of the group's 16 x 256 solved
// entries of panel p has bits other than +-0 (gs_panel256_body writes it).  A tile subtracts, per panel p of its operand
// [first, first + nP), (its rows of A) x (its rows of B)^T: the product is exactly zero when ALL its A groups or ALL its B groups are
// unflagged in p, so the panel is NEEDED only when some A group AND some B group are flagged.  The window is the contiguous span of
// panels from the first to the last needed one (panels inside it are multiplied whether needed or not: same ascending order).
//
// The tile reads its flags 64 at a time, one per lane -- a pass covers four panels, sixteen slots each: slots 0..7 the A groups
// gA0 .. gA0 + nA - 1, slots 8..15 the B groups gB0 .. gB0 + nB - 1 -- and a wave-wide ballot turns them into one word.
#define GS_ZW_PASS 4                     // panels per pass
#define GS_ZW_GROUPS 8                   // 16-row groups of A (and of B) per tile at most: 128 rows

// index of the flag that lane `l` reads in the pass that starts at panel p0 (absolute outer step), or -1: nothing to read
GS_ZW_HD inline int64_t gs_zwin_slot(int l, int p0, int pend, int64_t pstride, int gA0, int nA, int gB0, int nB) {
    const int p = p0 + (l >> 4), i = l & 15;
    if (p >= pend) return -1;
    if (i < GS_ZW_GROUPS) return i < nA ? (int64_t)p * pstride + gA0 + i : -1;
    return i - GS_ZW_GROUPS < nB ? (int64_t)p * pstride + gB0 + i - GS_ZW_GROUPS : -1;
}

// one pass's word (bit l: lane l's flag is set) into the running window [*lo, *hi) in panels relative to the operand's first;
// j0: the pass's first panel relative to the operand's first, nP: panels of the operand.  *lo < 0: nothing needed so far.
GS_ZW_HD inline void gs_zwin_scan(unsigned long long word, int j0, int nP, int* lo, int* hi) {
    for (int j = 0; j < GS_ZW_PASS && j0 + j < nP; ++j) {
        const unsigned m = (unsigned)(word >> (16 * j)) & 0xffffu;
        if ((m & 0xffu) != 0u && (m >> 8) != 0u) {
            if (*lo < 0) *lo = j0 + j;
            *hi = j0 + j + 1;
        }
    }
}

// The whole rule on the host (what a tile's waves compute with gs_zwin_slot, a ballot and gs_zwin_scan): [*k_lo, *k_hi) in COLUMNS
// of the operand, multiples of 256; empty (0, 0) when no panel is needed.
inline void gs_zwin_columns(const unsigned char* flags, int64_t pstride, int first, int nP, int gA0, int nA, int gB0, int nB,
                            int* k_lo, int* k_hi) {
    int lo = -1, hi = -1;
    for (int j0 = 0; j0 < nP; j0 += GS_ZW_PASS) {
        unsigned long long word = 0ull;
        for (int l = 0; l < 64; ++l) {
            const int64_t idx = gs_zwin_slot(l, first + j0, first + nP, pstride, gA0, nA, gB0, nB);
            if (idx >= 0 && flags[idx] != 0) word |= 1ull << l;
        }
        gs_zwin_scan(word, j0, nP, &lo, &hi);
    }
    *k_lo = lo < 0 ? 0 : 256 * lo;
    *k_hi = lo < 0 ? 0 : 256 * hi;
}
