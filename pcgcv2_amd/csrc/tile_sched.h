// Tile schedules of the MFMA kernels as pure integer arithmetic: which tile a (workgroup, wave, round) walks, how many workgroups a
// persistent launch gets, and the packed conv's rows per workgroup.  No HIP include: the kernels and launchers call these with blockIdx,
// gridDim and the CU count, and tests/native/tile_sched_check.cpp compiles the same header with g++ and checks the schedules exhaustively
// (every tile visited exactly once, grids a multiple of 8, pk_rows inside the kernel's limits).
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __HIP__
#define TS_HD __attribute__((host)) __attribute__((device))
#else
#define TS_HD
#endif

// XCD-aware tile order: workgroup b is observed to run on XCD b % 8 (each XCD has its own 4 MiB L2).  Remap so every XCD
// walks a contiguous slab of tiles: neighbouring tiles gather overlapping rows, which then hit the same L2.  Bijective
// for any grid size; placement only affects speed, never results.
TS_HD static inline unsigned xcd_tile(unsigned b, unsigned nb) {
    const unsigned q = nb >> 3, r = nb & 7, x = b & 7;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (b >> 3);
}

// Persistent tile order: XCD x (workgroups b = x mod 8; each XCD has its own L2) walks one contiguous eighth of the tiles, and
// inside it consecutive tiles go to different workgroups first, then to the next wave slot: the i-th tile of (workgroup b, wave w) on a
// grid of `grid` workgroups (a multiple of 8) of nw waves, or -1 when that wave is done (every later i is -1 too).
TS_HD static inline int64_t sched_child_tile(unsigned block, unsigned grid, int nw, int wave, int i, int64_t ntiles) {
    const int64_t S = (ntiles + 7) >> 3;
    const int64_t l = (block >> 3) + (int64_t)(grid >> 3) * (wave + nw * i);
    const int64_t tile = (block & 7) * S + l;
    return (l < S && tile < ntiles) ? tile : -1;
}
// one tile per wave (levels with many more tiles than resident waves)
TS_HD static inline int64_t sched_child_tile_once(unsigned block, unsigned grid, int nw, int wave, int i, int64_t ntiles) {
    const int64_t tile = (int64_t)xcd_tile(block, grid) * nw + wave;
    return (i == 0 && tile < ntiles) ? tile : -1;
}

// persistent grid: as many workgroups as stay resident (LDS-limited, at most max_waves_per_cu waves per CU), a multiple of 8 (one share per
// XCD).  n_units: work items of the launch (tiles of 16 MT parents, x 2 for half units)
static inline unsigned sched_child_grid(int64_t n_units, int nw, size_t lds, int cus, int max_waves_per_cu) {
    int per_cu = (int)((160 * 1024) / (lds ? lds : 1));
    if (per_cu > max_waves_per_cu / nw) per_cu = max_waves_per_cu / nw;
    if (per_cu < 1) per_cu = 1;
    int64_t want = (n_units + nw - 1) / nw;
    int64_t g = (int64_t)cus * per_cu;
    if (g > want) g = want;
    g = (g + 7) / 8 * 8;
    return (unsigned)g;
}

// k_conv_up2_tab: wave w of workgroup b starts at tile b nw + w and strides over the whole grid's waves
static inline unsigned sched_up2_grid(int64_t ntiles, int nw, size_t lds, int cus) {
    const int per_cu = (int)((160 * 1024) / lds) > 2 ? 2 : ((160 * 1024) / lds < 1 ? 1 : (int)((160 * 1024) / lds));      // (16 waves per CU at most)
    int64_t g = (ntiles + nw - 1) / nw;
    if (g > (int64_t)cus * per_cu) g = (int64_t)cus * per_cu;
    return (unsigned)g;
}
TS_HD static inline int64_t sched_up2_first(unsigned block, int nw, int wave) { return (int64_t)block * nw + wave; }
TS_HD static inline int64_t sched_up2_step(unsigned grid, int nw) { return (int64_t)grid * nw; }

// ---- k_conv_packed64 (conv_packed.hip) ------------------------------------------------------------------------------------------------
constexpr int PK_RMIN = 40, PK_RMAX = 128;      // output rows per workgroup: even, R <= 128 (two ballots), chosen per launch (pk_rows)
constexpr int PK_ACC_LD = 68;                   // floats per accumulator row in LDS (64 + 4: rows start 4 banks apart)
// LDS of a workgroup of R rows: accumulators (+ one dummy row for the padding slots of the last packed tile) | gathered rows of one offset
// (up to ceil(R / 16) packed tiles x 4 KB) | per wave: gather row + output row of every packed slot
TS_HD constexpr int pk_tiles(int R) { return (R + 15) / 16; }
TS_HD constexpr int pk_acc_bytes(int R) { return (R + 1) * PK_ACC_LD * 4; }
TS_HD constexpr int pk_a_bytes(int R) { return pk_tiles(R) * 4096; }
TS_HD constexpr int pk_slots(int R) { return pk_tiles(R) * 16; }
TS_HD constexpr int pk_lds(int R, int NW) { return pk_acc_bytes(R) + pk_a_bytes(R) + NW * 2 * pk_slots(R) * 4; }

// Rows per workgroup, from a cost model fitted to sweeps of R on both layers of a vox10 frame (profiles/r04_conv_packed.md).  A launch is
// `tiles` workgroups on cus x occ(R) slots (occ: LDS-limited workgroups per CU; LDS is granted in 1280-byte granules); a CU runs c workgroups
// side by side, each offset costing about L + c W tau(c) us: L = what nobody covers (barriers, gather latency), W = R p / 16 + 1/2 packed tiles
// per offset (the + 1/2 is the half-empty last tile), tau = time per packed tile, larger when few waves share a SIMD.  Large R packs better
// but leaves two workgroups per CU; and e.g. 71 216 rows in tiles of 96 are 742 workgroups on 512 slots — two rounds — where tiles of 94
// are 758 on 768: one.  p = 0.6 (a surface level has 14-19 of 27 neighbours; the choice is flat in p).
static inline int pk_occ(int R, int nw) {
    const int granules = (pk_lds(R, nw) + 1279) / 1280;
    int occ = (160 * 1024) / (granules * 1280);
    const int by_waves = 24 / nw;                               // 84 VGPRs: six waves per SIMD
    if (occ > by_waves) occ = by_waves;
    return occ < 1 ? 1 : occ;
}
static inline int pk_rows(int64_t n, int cus) {
    auto tau = [](int c) { return c >= 4 ? 0.219 : (c == 3 ? 0.240 : (c == 2 ? 0.276 : 0.370)); };      // (least-squares fit to the two sweeps: 4 % rms)
    auto cost_of = [&](int R) {
        const int occ = pk_occ(R, 4);
        const int64_t tiles = (n + R - 1) / R, slots = (int64_t)cus * occ;
        const double W = R * 0.6 / 16.0 + 0.346, L = 1.27;
        const int64_t full = tiles / slots, rem = tiles - full * slots;
        double cost = (double)full * (L + occ * W * tau(occ));
        if (rem) { const int c = (int)((rem + cus - 1) / cus); cost += L + c * W * tau(c); }
        return cost;
    };
    double best_cost = 1e300;
    int best = PK_RMAX;
    for (int R = PK_RMAX; R >= PK_RMIN; R -= 2)
        if (cost_of(R) < best_cost) { best_cost = cost_of(R); best = R; }
    // The model is flat to within its own error (4 % rms) over wide ranges of R — 149 856 rows: 260.5 at R = 50, 264.4 at 60, where the
    // measured sweep has 298 and 288 us (profiles/r04_conv_packed.md) — so among the sizes within 2 % of its minimum the LARGEST is taken
    // larger tiles pack better than the model's fixed + 1/2 tile per offset credits them with (round 5: conv0 picks 60 instead of 50).
    // (only among tiles of the minimum's own occupancy: across an occupancy step the model's error is not a few per cent)
    for (int R = PK_RMAX; R >= PK_RMIN; R -= 2)
        if (cost_of(R) <= 1.02 * best_cost && pk_occ(R, 4) == pk_occ(best, 4)) return R;
    return best;
}
// a forced tile size (pcgc_set_packed_tuning) the kernel supports: 0 = chosen per launch, or an even R in PK_RMIN .. PK_RMAX
static inline bool pk_rows_allowed(int R) { return R == 0 || (R >= PK_RMIN && R <= PK_RMAX && (R & 1) == 0); }
// rows per workgroup and workgroups of a launch of n rows
static inline int pk_launch_rows(int64_t n, int cus, int forced) { return forced > 0 ? forced : pk_rows(n, cus); }
static inline unsigned pk_launch_grid(int64_t n, int R) { return (unsigned)((n + R - 1) / R); }
