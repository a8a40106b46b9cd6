// Host check of the two index maps of the tile binning's count scan (csrc/hsr_common.h); no GPU call.
//   hsr_bin_row_of(k, nblk), nblk = 1 .. 2048: a bijection on [0, nblk); rows of equal b mod 8 consecutive and ascending, the classes
//     in the order 0 .. 7; the identity for nblk < 8; hsr_bin_row_next steps from the k-th row to the (k + 1)-th.
//   hsr_bin_scan_block_of(w, n), n = 1 .. 512: a bijection on [0, n); it permutes inside aligned groups of sixteen only; in a whole
//     group the blocks 2 j and 2 j + 1 (one 128-byte line of every table row) go to workgroups w and w + 8; the ragged last group
//     is the identity.
// build: hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -I hier-slam_amd/csrc tools/micro/bin_row_order.hip -o tools/micro/bin_row_order
//        (the same line with -Xarch_host -fsanitize=address,undefined for the sanitizer run, on the machine that builds)
#include "hsr_common.h"
#include <cstdio>
#include <vector>

static int fails = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (fails < 20) { printf("FAIL: " __VA_ARGS__); printf("\n"); } \
            fails++;                                      \
        }                                                 \
    } while (0)

int main()
{
    long rows_checked = 0, blocks_checked = 0;
    for (int nblk = 1; nblk <= 2048; nblk++) {
        std::vector<int> seen(nblk, 0);
        int prev = -1;
        for (int k = 0; k < nblk; k++) {
            const int b = hsr_bin_row_of(k, nblk);
            CHECK(b >= 0 && b < nblk, "row_of(%d, %d) = %d out of range", k, nblk, b);
            if (b < 0 || b >= nblk) continue;
            CHECK(seen[b] == 0, "row_of(%d, %d) = %d twice", k, nblk, b);
            seen[b]++;
            if (nblk < 8) CHECK(b == k, "row_of(%d, %d) = %d, not the identity", k, nblk, b);
            if (prev >= 0) {
                // same class: the next row of it; otherwise the first row of the next class, the previous class being exhausted
                const bool same = (b & 7) == (prev & 7) && b == prev + 8;
                const bool next_class = (b & 7) == (prev & 7) + 1 && b < 8 && prev + 8 >= nblk;
                CHECK(same || next_class, "row_of(%d, %d) = %d after %d", k, nblk, b, prev);
                CHECK(hsr_bin_row_next(prev, nblk) == b, "row_next(%d, %d) = %d, row_of gives %d", prev, nblk, hsr_bin_row_next(prev, nblk), b);
            } else
                CHECK(b == 0, "row_of(0, %d) = %d", nblk, b);
            prev = b;
            rows_checked++;
        }
        // class sizes: q + (c < r)
        const int q = nblk / 8, r = nblk % 8;
        for (int c = 0, k = 0; c < 8 && nblk >= 8; c++) {
            const int n = q + (c < r);
            for (int j = 0; j < n; j++, k++) CHECK(hsr_bin_row_of(k, nblk) == 8 * j + c, "class %d row %d of nblk %d", c, j, nblk);
        }
    }
    for (int n = 1; n <= 512; n++) {
        std::vector<int> owner(n, -1);
        for (int w = 0; w < n; w++) {
            const int blk = hsr_bin_scan_block_of(w, n);
            CHECK(blk >= 0 && blk < n, "block_of(%d, %d) = %d out of range", w, n, blk);
            if (blk < 0 || blk >= n) continue;
            CHECK(owner[blk] < 0, "block_of(%d, %d) = %d twice", w, n, blk);
            owner[blk] = w;
            CHECK((blk >> 4) == (w >> 4), "block_of(%d, %d) = %d leaves its group of sixteen", w, n, blk);
            if ((w | 15) >= n) CHECK(blk == w, "block_of(%d, %d) = %d in the ragged group", w, n, blk);
            blocks_checked++;
        }
        for (int blk = 0; blk + 1 < n; blk += 2)
            if ((blk | 15) < n && owner[blk] >= 0 && owner[blk + 1] >= 0)
                CHECK(owner[blk + 1] == owner[blk] + 8, "blocks %d, %d of n = %d: workgroups %d, %d", blk, blk + 1, n, owner[blk], owner[blk + 1]);
    }
    printf("bin_row_order: hsr_bin_row_of / hsr_bin_row_next nblk = 1..2048 (%ld rows), hsr_bin_scan_block_of n = 1..512 (%ld blocks): %s (%d failures)\n",
           rows_checked, blocks_checked, fails ? "FAILED" : "ok", fails);
    return fails ? 1 : 0;
}
