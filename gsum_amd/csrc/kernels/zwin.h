// the K window of a trailing-update tile from the panel solves' zero flags (grouped batch schedule)
// (plain C++: included by gsum_kernels.hip.h for the device code and, on its own, by host programs -- tests/c_host/zwin_host.cpp)
#pragma once
#include <math.h>
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

// ---- the 128 x 64 tile grids without counted tiles (gs_gemm_ld3_body, BNT = 1): tile id -> (tile row bm, column tile bn) ------------
// Lower triangle of an M x M matrix.  M a multiple of 128 (or M <= 128): row bm holds column tiles 0 .. 2 bm + 1.  Otherwise the
// PARTIAL row tile comes FIRST ("shifted"): rows [0, off) (off = M mod 128) form tile row 0 (c0 column tiles), row bm >= 1 covers
// [off + 128 (bm - 1), off + 128 bm) and holds 2 bm + c0 column tiles.
GS_ZW_HD inline bool gs_tri_shifted(int M) { return (M & 127) != 0 && M > 128; }
GS_ZW_HD inline int64_t gs_tri_tiles64(int64_t M) {
    const int64_t tm = (M + 127) / 128;
    if (!gs_tri_shifted((int)M)) return tm * (tm + 1);
    const int64_t off = M & 127, c0 = (off - 1) / 64 + 1, R = 1 + M / 128;
    return c0 + (R - 1) * (R + c0);
}
// the plain grid: row bm holds column tiles 0 .. 2 bm + 1
GS_ZW_HD inline void gs_tile_tri_plain(int bid, int* bm_out, int* bn_out) {
    int bm = (int)((sqrt(4.0 * (double)bid + 1.0) - 1.0) * 0.5);
    while ((int64_t)(bm + 1) * (bm + 2) <= bid) ++bm;
    while ((int64_t)bm * (bm + 1) > bid) --bm;
    *bm_out = bm;
    *bn_out = bid - (int)((int64_t)bm * (bm + 1));
}
// the shifted grid (gs_tri_shifted(M))
GS_ZW_HD inline void gs_tile_tri_shift(int M, int bid, int* bm_out, int* bn_out) {
    const int off = M & 127, c0 = (off - 1) / 64 + 1;
    if (bid < c0) {
        *bm_out = 0;
        *bn_out = bid;
        return;
    }
    const int g = bid - c0;
    int bm = (int)((-(double)(c0 - 1) + sqrt((double)(c0 - 1) * (c0 - 1) + 4.0 * (double)(c0 + g))) * 0.5);
    if (bm < 1) bm = 1;
    while ((int64_t)(bm - 1) * (bm + c0) > g) --bm;
    while ((int64_t)bm * (bm + 1 + c0) <= g) ++bm;
    *bm_out = bm;
    *bn_out = g - (bm - 1) * (bm + c0);
}
// the rectangle: column-major tile order over (M + 127) / 128 tile rows
GS_ZW_HD inline void gs_tile_rect(int M, int bid, int* bm_out, int* bn_out) {
    const int tm = (M + 127) / 128;
    *bm_out = bid % tm;
    *bn_out = bid / tm;
}
// first row and row bound of tile row bm (shifted grid: tile row 0 ends at row off, the full tile rows start there)
GS_ZW_HD inline void gs_tile_rows(int M, bool shifted, int bm, int* m0, int* Mr) {
    *m0 = shifted ? (bm == 0 ? 0 : (M & 127) + (bm - 1) * 128) : bm * 128;
    *Mr = (shifted && bm == 0) ? (M & 127) : M;
}

// Is any operand panel NEEDED by tile `tile` of the lower-triangle update of an M x M matrix (the batch schedule's far updates: 128 x 64
// tiles, N = M, A and B start at the same row, 16-row group g0 of the flags)?  The rule of gs_zwin_columns -- some A group AND some B
// group flagged in the same panel -- as a yes / no; false as well for the one tile past the last column that the plain grid of a small
// triangle carries.  What gs_gemm_ld3_body decides with a ballot, and what k_far_plan_g lists (tile.hip.h, from running counts: below).
// the tile's 16-row groups of A, [*gA0, *gA0 + *nA), and of B, counted from the operands' row 0; false: the tile lies past the last column
GS_ZW_HD inline bool gs_zwin_tile_groups(int M, int tile, int* gA0, int* nA, int* gB0, int* nB) {
    const bool shifted = gs_tri_shifted(M);
    int bm, bn, m0, Mr;
    if (shifted) gs_tile_tri_shift(M, tile, &bm, &bn); else gs_tile_tri_plain(tile, &bm, &bn);
    gs_tile_rows(M, shifted, bm, &m0, &Mr);
    const int n0 = bn * 64;
    if (n0 >= M) return false;
    *nA = ((m0 + 128 < Mr ? 128 : Mr - m0) + 15) >> 4;
    *nB = ((n0 + 64 < M ? 64 : M - n0) + 15) >> 4;
    *gA0 = m0 >> 4;
    *gB0 = n0 >> 4;
    return true;
}
GS_ZW_HD inline bool gs_zwin_tile_live(int M, int tile, const unsigned char* flags, int64_t pstride, int first, int nP, int g0) {
    int gA0, nA, gB0, nB;
    if (!gs_zwin_tile_groups(M, tile, &gA0, &nA, &gB0, &nB)) return false;
    for (int p = first; p < first + nP; ++p) {
        const unsigned char* f = flags + (int64_t)p * pstride + g0;
        bool a = false, b = false;
        for (int i = 0; i < nA; ++i) a = a || f[gA0 + i] != 0;
        for (int i = 0; i < nB; ++i) b = b || f[gB0 + i] != 0;
        if (a && b) return true;
    }
    return false;
}
// The same answer from running counts: pre[p * stride + g] = how many of panel p's groups [0, g) (from the operands' row 0) are flagged,
// g = 0 .. M / 16 -- two reads per side and panel instead of one per group, and no branch (what k_far_plan_g keeps in LDS).
GS_ZW_HD inline bool gs_zwin_tile_live_pre(int M, int tile, const unsigned short* pre, int stride, int nP) {
    int gA0, nA, gB0, nB;
    if (!gs_zwin_tile_groups(M, tile, &gA0, &nA, &gB0, &nB)) return false;
    bool live = false;
    for (int p = 0; p < nP; ++p) {
        const unsigned short* c = pre + p * stride;
        live = live | ((c[gA0 + nA] != c[gA0]) & (c[gB0 + nB] != c[gB0]));
    }
    return live;
}
