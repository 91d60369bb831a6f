// Host build of pcgcv2_amd/csrc/tile_sched.h (g++, no HIP): exhaustive checks of the tile schedules the kernels and launchers use.
// Prints "FAIL ..." lines and exits 1 on the first few violations; on success one line "pk_rows_256 <R values>" (the set of tile sizes
// pk_rows returns at 256 CUs for 512 .. 400 000 rows), one line of counts, and "OK".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <map>
#include <set>
#include <utility>
#include <vector>
#include "../../pcgcv2_amd/csrc/tile_sched.h"

static int g_fail = 0;
#define FAIL(...) do { printf("FAIL " __VA_ARGS__); printf("\n"); if (++g_fail >= 10) exit(1); } while (0)

static const int CUS[] = {1, 2, 8, 256, 304};
static const int NWS[] = {4, 7, 8, 12, 16};                     // the waves per workgroup of every launcher

// every (block, wave) loops i = 0, 1, ... to its first negative tile: every tile of 0 .. ntiles - 1 exactly once, none outside
template <class Tile>
static void check_walk(const char* what, unsigned grid, int nw, int64_t ntiles, std::vector<int>& seen, int stamp, Tile tile_of) {
    int64_t visited = 0;
    for (unsigned b = 0; b < grid; ++b)
        for (int w = 0; w < nw; ++w)
            for (int i = 0;; ++i) {
                const int64_t t = tile_of(b, w, i);
                if (t < 0) break;
                if (t >= ntiles) { FAIL("%s: grid %u nw %d ntiles %lld: tile %lld out of range", what, grid, nw, (long long)ntiles, (long long)t); return; }
                if (seen[t] == stamp) { FAIL("%s: grid %u nw %d ntiles %lld: tile %lld visited twice", what, grid, nw, (long long)ntiles, (long long)t); return; }
                seen[t] = stamp;
                ++visited;
            }
    if (visited != ntiles) FAIL("%s: grid %u nw %d ntiles %lld: %lld tiles visited", what, grid, nw, (long long)ntiles, (long long)visited);
}

int main() {
    // ---- xcd_tile: a permutation of 0 .. nb - 1
    for (unsigned nb = 1; nb <= 4096; ++nb) {
        std::vector<char> hit(nb, 0);
        for (unsigned b = 0; b < nb; ++b) {
            const unsigned t = xcd_tile(b, nb);
            if (t >= nb || hit[t]) { FAIL("xcd_tile: nb %u: block %u -> %u (out of range or twice)", nb, b, t); break; }
            hit[t] = 1;
        }
    }
    // ---- the persistent grid rule: every (capacity = cus x workgroups per CU, nw) it can produce
    struct Rep { int cus; size_t lds; int maxw; };
    std::map<std::pair<int64_t, int>, Rep> caps;               // (cus x workgroups per CU, nw) -> one setting that gives it
    long grids_checked = 0, walks = 0;
    for (int cus : CUS)
        for (int nw : NWS)
            for (size_t lds = 16 * 1024; lds <= 160 * 1024; lds += 16 * 1024)
                for (int maxw : {8, 16}) {
                    const unsigned gmax = sched_child_grid((int64_t)1 << 40, nw, lds, cus, maxw);
                    int per_cu = (int)((160 * 1024) / lds);
                    if (per_cu > maxw / nw) per_cu = maxw / nw;
                    if (per_cu < 1) per_cu = 1;
                    if (gmax != (unsigned)(((int64_t)cus * per_cu + 7) / 8 * 8)) FAIL("grid rule: cus %d nw %d lds %zu maxw %d: full grid %u", cus, nw, lds, maxw, gmax);
                    // the rule depends on (cus, lds, maxw) through cus x per_cu only: check that, then walk each distinct capacity once
                    for (int64_t units : {(int64_t)0, (int64_t)1, (int64_t)nw, (int64_t)nw + 1, (int64_t)gmax * nw - 1, (int64_t)gmax * nw, (int64_t)gmax * nw + 1, (int64_t)1 << 33}) {
                        const unsigned g = sched_child_grid(units, nw, lds, cus, maxw);
                        int64_t want = (units + nw - 1) / nw;
                        if (want > (int64_t)cus * per_cu) want = (int64_t)cus * per_cu;
                        if (g != (unsigned)((want + 7) / 8 * 8)) FAIL("grid rule: cus %d nw %d lds %zu maxw %d units %lld: grid %u", cus, nw, lds, maxw, (long long)units, g);
                        ++grids_checked;
                    }
                    caps.insert({{(int64_t)cus * per_cu, nw}, Rep{cus, lds, maxw}});
                }
    std::vector<int> seen;
    int stamp = 0;
    for (const auto& cn : caps) {
        const int64_t cap = cn.first.first;
        const int nw = cn.first.second;
        const Rep rep = cn.second;
        const int64_t gmax = (cap + 7) / 8 * 8, nmax = 3 * gmax * nw + 19;
        seen.assign((size_t)(nmax > 40 * nw + 19 ? nmax : 40 * nw + 19) + 1, 0);
        stamp = 0;
        for (int64_t ntiles = 0; ntiles <= nmax; ++ntiles) {
            const unsigned grid = sched_child_grid(ntiles, nw, rep.lds, rep.cus, rep.maxw);
            if (grid % 8 != 0 || (ntiles > 0 && grid == 0)) FAIL("grid: cap %lld nw %d ntiles %lld: grid %u", (long long)cap, nw, (long long)ntiles, grid);
            check_walk("child_tile", grid, nw, ntiles, seen, ++stamp,
                       [&](unsigned b, int w, int i) { return sched_child_tile(b, grid, nw, w, i, ntiles); });
            // a wave that is done stays done
            if (ntiles > 0 && sched_child_tile(grid - 1, grid, nw, nw - 1, 4, ntiles) >= 0 && 5 * (int64_t)grid * nw > ntiles + (int64_t)grid * nw)
                FAIL("child_tile: cap %lld nw %d ntiles %lld: a tile in round 4", (long long)cap, nw, (long long)ntiles);
            ++walks;
        }
        // one tile per wave on a grid of ceil(ntiles / nw) workgroups (any size: xcd_tile's remainder path)
        for (int64_t ntiles = 0; ntiles <= 40 * nw + 19; ++ntiles) {
            const unsigned grid = (unsigned)((ntiles + nw - 1) / nw);
            check_walk("child_tile_once", grid, nw, ntiles, seen, ++stamp,
                       [&](unsigned b, int w, int i) { return sched_child_tile_once(b, grid, nw, w, i, ntiles); });
        }
    }
    // ---- k_conv_up2_tab: eight waves, 72 KB (64 -> 32) / 28 KB (32 -> 16) of LDS among the sizes; tiles first, first + step, ...
    {
        struct URep { int cus; size_t lds; };
        std::map<int64_t, URep> ucaps;                          // largest grid -> one setting that gives it
        const int nw = 8;
        for (int cus : CUS)
            for (size_t lds = 16 * 1024; lds <= 160 * 1024; lds += 4 * 1024) ucaps.insert({(int64_t)sched_up2_grid((int64_t)1 << 40, nw, lds, cus), URep{cus, lds}});
        for (const auto& cn : ucaps) {
            const int64_t cap = cn.first;
            const int64_t nmax = 3 * cap * nw + 19;
            seen.assign((size_t)nmax + 1, 0);
            stamp = 0;
            for (int64_t ntiles = 0; ntiles <= nmax; ++ntiles) {
                const unsigned grid = sched_up2_grid(ntiles, nw, cn.second.lds, cn.second.cus);
                int64_t want = (ntiles + nw - 1) / nw;
                if (want > cap) want = cap;
                if ((int64_t)grid != want || (ntiles > 0 && grid == 0)) FAIL("up2 grid: cap %lld ntiles %lld: grid %u", (long long)cap, (long long)ntiles, grid);
                const int64_t step = sched_up2_step(grid, nw);
                check_walk("conv_up2_tab", grid, nw, ntiles, seen, ++stamp, [&](unsigned b, int w, int i) {
                    const int64_t t = sched_up2_first(b, nw, w) + (int64_t)i * step;
                    return t < ntiles ? t : (int64_t)-1;
                });
                ++walks;
            }
        }
    }
    // ---- the packed conv's tile size
    for (int R = PK_RMIN; R <= PK_RMAX; R += 2) {
        if (pk_lds(R, 4) > 160 * 1024) FAIL("pk_lds(%d, 4) = %d", R, pk_lds(R, 4));
        if (pk_tiles(R) * 16 < R || pk_slots(R) != 16 * pk_tiles(R) || pk_occ(R, 4) < 1 || pk_occ(R, 4) > 6) FAIL("pk sizes at R = %d", R);
        if (!pk_rows_allowed(R) || pk_rows_allowed(R + 1) || pk_launch_rows(12345, 256, R) != R) FAIL("pk_rows_allowed / pk_launch_rows at R = %d", R);
    }
    if (!pk_rows_allowed(0) || pk_rows_allowed(-2) || pk_rows_allowed(38) || pk_rows_allowed(130) || pk_rows_allowed(1)) FAIL("pk_rows_allowed at the edges");
    std::set<int> r256;
    long pk_checked = 0;
    for (int cus : CUS)
        for (int64_t n = 1; n <= 400000; n += (n < 20000 ? 1 : 7)) {
            const int R = pk_rows(n, cus);
            if (R < PK_RMIN || R > PK_RMAX || (R & 1) || pk_lds(R, 4) > 160 * 1024) FAIL("pk_rows(%lld, %d) = %d", (long long)n, cus, R);
            if (pk_launch_rows(n, cus, 0) != R || (int64_t)pk_launch_grid(n, R) * R < n || ((int64_t)pk_launch_grid(n, R) - 1) * R >= n)
                FAIL("launch of %lld rows on %d CUs: R %d, grid %u", (long long)n, cus, R, pk_launch_grid(n, R));
            if (cus == 256 && n >= 512) r256.insert(R);
            ++pk_checked;
        }
    for (int64_t n : {(int64_t)71216, (int64_t)149856}) r256.insert(pk_rows(n, 256));
    if (g_fail) return 1;
    printf("pk_rows_256");
    for (int R : r256) printf(" %d", R);
    printf("\npk_rows_levels %d %d\n", pk_rows(71216, 256), pk_rows(149856, 256));
    printf("checked %ld grids, %ld walks over %zu capacities, %ld pk_rows\n", grids_checked, walks, caps.size(), pk_checked);
    printf("OK\n");
    return 0;
}
