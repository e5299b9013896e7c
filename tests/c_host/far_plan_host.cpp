// Stand-alone host check of the far updates' live-tile plan (gsum_amd/csrc/kernels/zwin.h): the id -> tile maps of the 128 x 64 grids hit
// every lower-triangle tile exactly once and agree with the host's tile counts, and the plan's yes / no per tile equals the K-window rule's
// "non-empty" on random, banded and all-set flags:  g++ -O2 -I gsum_amd/csrc far_plan_host.cpp && ./a.out  (no GPU; prints "ok <count>").
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "kernels/zwin.h"

static int fail(const char* what, int M, int a, int b) {
    printf("FAIL %s: M=%d (%d, %d)\n", what, M, a, b);
    return 1;
}

int main() {
    // the batch schedule's trailing matrices have 128 k + 16 rows (the shifted grid, but for the last: 16); 64, 128, 1536: the plain grid
    const int Ms[] = {144, 272, 400, 784, 1296, 1552, 7184, 16, 64, 128, 1536};
    long long checked = 0;
    unsigned rng = 12345u;
    auto next = [&]() { rng = rng * 1664525u + 1013904223u; return rng >> 8; };
    for (int M : Ms) {
        // ---- the maps: every 128 x 64 tile with a column on or left of its last row, once; nothing else but (plain grid) tiles past the last column
        const bool shifted = gs_tri_shifted(M);
        const int tiles = (int)gs_tri_tiles64(M);
        const int off = M & 127;
        const int rows = shifted ? 1 + M / 128 : (M + 127) / 128;
        std::vector<std::vector<int>> seen((size_t)rows);
        for (int id = 0; id < tiles; ++id) {
            int bm, bn, m0, Mr;
            if (shifted) gs_tile_tri_shift(M, id, &bm, &bn); else gs_tile_tri_plain(id, &bm, &bn);
            if (bm < 0 || bm >= rows || bn < 0) return fail("tile row out of range", M, id, bm);
            gs_tile_rows(M, shifted, bm, &m0, &Mr);
            const int want_m0 = shifted ? (bm == 0 ? 0 : off + 128 * (bm - 1)) : 128 * bm;
            if (m0 != want_m0 || Mr != ((shifted && bm == 0) ? off : M)) return fail("tile rows", M, id, m0);
            if ((int)seen[(size_t)bm].size() <= bn) seen[(size_t)bm].resize((size_t)bn + 1, 0);
            if (seen[(size_t)bm][(size_t)bn]++) return fail("tile hit twice", M, bm, bn);
        }
        int needed = 0;
        for (int bm = 0; bm < rows; ++bm) {
            int m0, Mr;
            gs_tile_rows(M, shifted, bm, &m0, &Mr);
            const int m1 = m0 + 128 < Mr ? m0 + 128 : Mr;                // rows [m0, m1): column tiles 0 .. (m1 - 1) / 64 are on or below the diagonal
            const int want = (m1 - 1) / 64 + 1;
            needed += want;
            if ((int)seen[(size_t)bm].size() < want) return fail("tile row too short", M, bm, (int)seen[(size_t)bm].size());
            for (int bn = 0; bn < (int)seen[(size_t)bm].size(); ++bn) {
                if (seen[(size_t)bm][(size_t)bn] != 1) return fail("tile missed", M, bm, bn);
                if (bn >= want && (shifted || 64 * bn < M)) return fail("tile above the diagonal", M, bm, bn);   // (plain grid: only past the last column)
            }
        }
        if (shifted && needed != tiles) return fail("tile count", M, needed, tiles);
        if (!shifted && (tiles < needed || tiles > needed + 1)) return fail("tile count", M, needed, tiles);
        // the rectangle of the near updates: (M + 127) / 128 tile rows x 4 column tiles, each once
        {
            const int tm = (M + 127) / 128;
            std::vector<int> hit((size_t)tm * 4, 0);
            for (int id = 0; id < tm * 4; ++id) {
                int bm, bn;
                gs_tile_rect(M, id, &bm, &bn);
                if (bm < 0 || bm >= tm || bn < 0 || bn >= 4 || hit[(size_t)bn * tm + bm]++) return fail("rectangle", M, bm, bn);
            }
        }
        // ---- the rule: flags of nP panels from `first`, groups g0 .. g0 + M / 16 - 1; everything outside is SET (a stray read shows)
        const int ng = M / 16, g0 = 3, first = 2, pstride = g0 + ng + 5;
        for (int nP = 1; nP <= 5; ++nP) {
            for (int pat = 0; pat < 8; ++pat) {
                std::vector<unsigned char> fl((size_t)(first + nP + 1) * pstride, (unsigned char)1);
                for (int p = 0; p < nP; ++p)
                    for (int g = 0; g < ng; ++g) {
                        unsigned char v;
                        if (pat == 0) v = 1;                                               // all set
                        else if (pat == 1) v = 0;                                          // none
                        else if (pat == 2) v = (g < 6 + 16 * p || g == ng - 1) ? 0xff : 0;   // banded: the first rows and the right-hand sides
                        else if (pat == 3) v = (g >= ng - 1) ? 1 : 0;                      // the right-hand-side rows only
                        else if (pat == 4) v = (p == nP - 1 && g % 7 == 0) ? 1 : 0;        // the last panel only, with holes
                        else v = (next() % (pat == 5 ? 2u : (pat == 6 ? 9u : 40u))) == 0;  // random, three densities
                        fl[(size_t)(first + p) * pstride + g0 + g] = v;
                    }
                // the running counts of the device's plan: pre[p][g] = flagged groups of panel first + p among the operands' first g
                std::vector<unsigned short> pre((size_t)nP * (ng + 1), 0);
                for (int p = 0; p < nP; ++p)
                    for (int g = 0; g < ng; ++g)
                        pre[(size_t)p * (ng + 1) + g + 1] = (unsigned short)(pre[(size_t)p * (ng + 1) + g] + (fl[(size_t)(first + p) * pstride + g0 + g] != 0));
                for (int id = 0; id < tiles; ++id) {
                    int bm, bn, m0, Mr;
                    if (shifted) gs_tile_tri_shift(M, id, &bm, &bn); else gs_tile_tri_plain(id, &bm, &bn);
                    gs_tile_rows(M, shifted, bm, &m0, &Mr);
                    const int n0 = 64 * bn;
                    bool want = false;
                    if (n0 < M) {
                        const int nA = ((m0 + 128 < Mr ? 128 : Mr - m0) + 15) / 16, nB = ((n0 + 64 < M ? 64 : M - n0) + 15) / 16;
                        int k_lo = -1, k_hi = -1;
                        gs_zwin_columns(fl.data(), pstride, first, nP, g0 + m0 / 16, nA, g0 + n0 / 16, nB, &k_lo, &k_hi);
                        want = k_hi > k_lo;
                    }
                    if (gs_zwin_tile_live(M, id, fl.data(), pstride, first, nP, g0) != want) return fail("rule", M, id, pat);
                    if (gs_zwin_tile_live_pre(M, id, pre.data(), ng + 1, nP) != want) return fail("rule on running counts", M, id, pat);
                    ++checked;
                }
            }
        }
    }
    printf("ok %lld\n", checked);
    return 0;
}
