// Batch collation out of the data loader's device-resident arena (pcgcv2_amd/data_loader.py): the clouds of a batch lie in
// one uint8 arena as their file's rows, three values of 1, 2 or 4 bytes each; one launch writes the batch's (item, x, y, z) rows and its
// column of ones.  Nothing here is on the encode/decode path.
//
// The <= 16 items travel by value in the kernel arguments, so a batch costs no host-to-device copy and the kernel reads no table from
// memory.  One thread per output row: it finds its item among the row prefixes, reads its three packed values (lanes read consecutive
// addresses), applies the item's symmetry of the cube and stores the row as one 16-byte vector.
#include "pcgc_common.h"

constexpr int COLLATE_BLOCK = 256;

struct CollateArgs { pcgc_collate_item it[PCGC_COLLATE_MAX_ITEMS]; };

// itertools.permutations(range(3)) in its own order, 2 bits per entry: out[a] = w[perm[a]]
__device__ static inline int perm_entry(int p, int a) {
    constexpr uint64_t T = (0ull | 1ull << 2 | 2ull << 4) | (0ull | 2ull << 2 | 1ull << 4) << 6 | (1ull | 0ull << 2 | 2ull << 4) << 12 |
                           (1ull | 2ull << 2 | 0ull << 4) << 18 | (2ull | 0ull << 2 | 1ull << 4) << 24 | (2ull | 1ull << 2 | 0ull << 4) << 30;
    return (int)((T >> (6 * p + 2 * a)) & 3);
}
__device__ static inline int32_t pick(int32_t w0, int32_t w1, int32_t w2, int a) { return a == 0 ? w0 : (a == 1 ? w1 : w2); }

__global__ void __launch_bounds__(COLLATE_BLOCK) k_collate_rows(const uint8_t* __restrict__ arena, const CollateArgs args, int32_t n,
                                                                int4* __restrict__ coords, float* __restrict__ feats) {
    const int32_t i = (int32_t)(blockIdx.x * COLLATE_BLOCK + threadIdx.x);
    if (i >= n) return;
    // the last item whose first row is <= i (an item without rows shares its first row with its successor, which wins; the unused
    // tail of the table starts at INT32_MAX).  Unrolled selects: the table stays in scalar registers, nothing is indexed in memory.
    pcgc_collate_item it = args.it[0];
    int32_t b = 0;
#pragma unroll
    for (int k = 1; k < PCGC_COLLATE_MAX_ITEMS; ++k)
        if (i >= args.it[k].first_row) { it = args.it[k]; b = k; }
    const int64_t r = i - it.first_row;
    const uint8_t* src = arena + it.offset + r * 3 * it.width;
    int32_t w0, w1, w2;
    if (it.width == 1) {
        w0 = src[0]; w1 = src[1]; w2 = src[2];
    } else if (it.width == 2) {
        const uint16_t* s = (const uint16_t*)src;
        w0 = s[0]; w1 = s[1]; w2 = s[2];
    } else {
        const int32_t* s = (const int32_t*)src;
        w0 = s[0]; w1 = s[1]; w2 = s[2];
    }
    const int p = it.symmetry % 6, flips = it.symmetry / 6;
    if (flips & 1) w0 = it.extent - w0;
    if (flips & 2) w1 = it.extent - w1;
    if (flips & 4) w2 = it.extent - w2;
    coords[i] = make_int4(b, pick(w0, w1, w2, perm_entry(p, 0)), pick(w0, w1, w2, perm_entry(p, 1)), pick(w0, w1, w2, perm_entry(p, 2)));
    feats[i] = 1.0f;
}

extern "C" int pcgc_collate_rows(const uint8_t* arena, const pcgc_collate_item* items, int n_items, int32_t* coords_out, float* feats_out,
                                 void* stream) {
    PCGC_REQUIRE(n_items >= 0 && n_items <= PCGC_COLLATE_MAX_ITEMS, "0 to 16 items");
    if (n_items == 0) return 0;
    PCGC_REQUIRE(items, "null argument");
    CollateArgs args;
    int64_t n = 0;
    for (int k = 0; k < n_items; ++k) {
        const pcgc_collate_item& it = items[k];
        PCGC_REQUIRE(it.width == 1 || it.width == 2 || it.width == 4, "width must be 1, 2 or 4 bytes");
        PCGC_REQUIRE(it.offset >= 0 && (it.offset & 15) == 0, "a cloud starts on a 16-byte boundary of the arena");
        PCGC_REQUIRE(it.rows >= 0 && it.first_row == n, "first_row must be the sum of the rows before the item");
        PCGC_REQUIRE(it.symmetry >= 0 && it.symmetry < 48, "symmetry code must be 0..47");
        n += it.rows;
        PCGC_REQUIRE(n < INT32_MAX, "too many rows");
        args.it[k] = it;
    }
    for (int k = n_items; k < PCGC_COLLATE_MAX_ITEMS; ++k) {
        args.it[k] = pcgc_collate_item{0, INT32_MAX, 0, 1, 0, 0, 0};
    }
    if (n == 0) return 0;
    PCGC_REQUIRE(arena && coords_out && feats_out, "null argument");
    PCGC_REQUIRE(((uintptr_t)arena & 15) == 0 && ((uintptr_t)coords_out & 15) == 0, "arena and coords_out must be 16-byte aligned");
    hipLaunchKernelGGL(k_collate_rows, dim3(grid_for(n, COLLATE_BLOCK)), dim3(COLLATE_BLOCK), 0, S(stream), arena, args, (int32_t)n,
                       (int4*)coords_out, feats_out);
    PCGC_CHECK_LAUNCH("collate_rows");
    return 0;
}
