// Stand-alone host check of the K-window rule of the batch schedule's trailing-update tiles (gsum_amd/csrc/kernels/zwin.h) against
// brute force over ALL flag patterns of small tiles: g++ -O2 -I gsum_amd/csrc zwin_host.cpp && ./a.out  (no GPU; prints "ok <count>").
#include <cstdio>
#include <cstring>
#include <vector>
#include "kernels/zwin.h"

int main() {
    const int GROUPS = 4, PSTRIDE = 7, FIRST = 2;                 // the cells that vary: groups [1, 1 + GROUPS) of panels [FIRST, FIRST + nP)
    struct cfg { int gA0, nA, gB0, nB; };
    const cfg cfgs[] = {{1, 2, 3, 2},        // A rows above B rows: an off-diagonal tile
                        {1, 2, 1, 2},        // the same groups on both sides: a diagonal tile
                        {2, 3, 1, 1},        // a near update: B in the first groups
                        {1, 4, 1, 4},        // every group on both sides
                        {4, 1, 1, 2}};       // the right-hand-side rows against matrix rows
    long long checked = 0;
    for (int nP = 1; nP <= 5; ++nP) {                             // (5 panels: two passes of four)
        const int cells = GROUPS * nP;
        std::vector<unsigned char> flags((size_t)(FIRST + nP + 1) * PSTRIDE);
        for (unsigned long pat = 0; pat < (1ul << cells); ++pat) {
            // every flag the rule must NOT read is set: a stray read shows as a window that is too wide
            std::fill(flags.begin(), flags.end(), (unsigned char)1);
            for (int p = 0; p < nP; ++p)
                for (int g = 0; g < GROUPS; ++g) flags[(size_t)(FIRST + p) * PSTRIDE + 1 + g] = (pat >> (p * GROUPS + g)) & 1 ? 0xff : 0;
            for (const cfg& c : cfgs) {
                int lo = -1, hi = -1, k_lo = -7, k_hi = -7;
                for (int p = 0; p < nP; ++p) {
                    bool a = false, b = false;
                    for (int g = 0; g < c.nA; ++g) a = a || flags[(size_t)(FIRST + p) * PSTRIDE + c.gA0 + g];
                    for (int g = 0; g < c.nB; ++g) b = b || flags[(size_t)(FIRST + p) * PSTRIDE + c.gB0 + g];
                    if (a && b) { if (lo < 0) lo = p; hi = p + 1; }
                }
                gs_zwin_columns(flags.data(), PSTRIDE, FIRST, nP, c.gA0, c.nA, c.gB0, c.nB, &k_lo, &k_hi);
                const bool empty = k_lo == k_hi;
                bool ok = (k_lo % 256 == 0) && (k_hi % 256 == 0) && k_lo >= 0 && k_hi <= 256 * nP && k_lo <= k_hi;
                ok = ok && (empty == (lo < 0));                                      // empty iff no panel is needed
                if (lo >= 0) ok = ok && k_lo <= 256 * lo && k_hi >= 256 * hi;           // contains every needed panel
                if (lo >= 0) ok = ok && k_lo == 256 * lo && k_hi == 256 * hi;           // ... and nothing before the first or behind the last
                if (!ok) {
                    printf("FAIL nP=%d pat=%lx cfg=(%d,%d,%d,%d): window [%d, %d), needed panels [%d, %d)\n", nP, pat, c.gA0, c.nA, c.gB0, c.nB,
                           k_lo, k_hi, lo, hi);
                    return 1;
                }
                ++checked;
            }
        }
    }
    printf("ok %lld\n", checked);
    return 0;
}
