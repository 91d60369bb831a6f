// Colour transform of the attribute stream `_A.bin`: the region-adaptive hierarchical transform (RAHT) in integer lifting form on YCoCg-R.
// The format is stated in tests/raht_reference.py and DESIGN.md 8j; everything here is integer arithmetic and is held to equality with it.
//
//   pcgc_raht_keys        Morton keys (bit 3 i + 0 / 1 / 2 of the key = bit i of x / y / z) of the rows, sorted (rocPRIM), the permutation,
//                         the number of adjacent equal keys, and whether a row lies outside [0, 2^20)^3 or carries a batch index
//   pcgc_raht_tree        gap i between sorted leaves i and i + 1 is one merge.  One thread per gap: split bit d = msb(key_i ^ key_{i+1}); the
//                         range [lo, hi] and the two children by binary search on the common prefix (Karras 2012): the keys that share
//                         key_i's bits above d are a run of the sorted array, so its ends are found in log n probes.  A stable radix
//                         sort of the gaps by frame * 64 + 63 - d is the coding order (frame, d descending, gap ascending: 6 bits for one
//                         frame); a second one by 63 - d with the bit "range lies inside one tile" on top lists the gaps that cross a
//                         tile boundary first, in the same order.
//   pcgc_raht_forward     node values live in place: the value of a node stands at the first leaf of its range, so a merge reads val[lo]
//   pcgc_raht_inverse     and val[i + 1] and writes val[lo] (and H[i]); ranges of one split bit are disjoint.  A node depends on nodes of
//                         lower split bit only.  NOTHING is handed from one workgroup to another inside a launch (no tickets, flags,
//                         spins, fences): dependent nodes are ordered by a launch boundary or by __syncthreads() in one workgroup.
//                           form 0: one launch per populated split bit over the coding order (ascending forward, descending inverse)
//                           form 1: a tile kernel, one workgroup per RAHT_TILE consecutive leaves, orders its gaps by split bit in LDS and
//                                   does every node whose range lies in the tile there, bit by bit; the nodes that cross a tile boundary
//                                   (the ancestors of the tile-boundary gaps: about 1 % of the gaps of a surface at 2^10 voxels a side)
//                                   are done by ONE workgroup, bit by bit, with __syncthreads() between bits
//                         The three channels travel as one int32 x 3.
//   pcgc_raht_quantize    levels, tokens, contexts, escape remainders (compacted behind pcgc_mask_scan) and the [48, 64] histogram
//   pcgc_raht_dequantize  tokens and escapes -> H^ per gap
//
// A SINGLE FRAME IS THE BATCH OF ONE: every step has one kernel and one host body that take `frames`; pcgc_raht_X and pcgc_raht_X_batch are
// thin entries around it that differ in their argument lists and refusals, and the single ones pass frames = 1 (frame 0 everywhere, no
// frame boundary, `keys` not read by the quantiser).  Work that exists only for batches sits behind a uniform run-time test.
// A BATCH of up to RAHT_MAX_FRAMES frames goes through the same steps once (pcgc_raht_*_batch): the frame index is bits
// 60 .. 63 of the key, so after ONE sort frame b is a run of leaves and every gap with d < 60 lies inside one frame, with the lo / hi /
// children it has in that frame alone (shifted by the run's start): the searches above compare whole keys.  The B - 1 gaps with d >= 60
// are frame boundaries: no merge, no token; they get lo = hi = -1, which every transform kernel already leaves alone.  The coding order
// is frame, then d descending, then gap ascending, the boundaries behind it; each frame's DC is the value at the start of its run.
#include <cstring>
#include "pcgc_common.h"
#include <rocprim/rocprim.hpp>

#define RAHT_MAX_POINTS (1ll << 24)
#define RAHT_TILE 1024                       // leaves per workgroup of the tile kernel (12 KiB of LDS)
#define RAHT_THREADS 256
#define RAHT_GAPS_PER_THREAD (RAHT_TILE / RAHT_THREADS)
#define RAHT_SPINE_THREADS 1024
#define RAHT_CONTEXTS 48
#define RAHT_ESCAPE 63
#define RAHT_MAX_FRAMES 16                   // the batch index is a 4-bit field everywhere (pcgc_common.h); here key bits 60 .. 63
#define RAHT_FRAME_BIT 60

struct i3 { int32_t a, b, c; };              // (Y, Co, Cg), or the three H of a gap

static size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

extern "C" int64_t pcgc_raht_tile_leaves(void) { return RAHT_TILE; }

// ------------------------------------------------------------------------------------------------------------------ keys
__host__ __device__ static inline uint64_t spread3(uint32_t x) {
    uint64_t v = x & 0x1FFFFFu;
    v = (v | (v << 32)) & 0x1F00000000FFFFull;
    v = (v | (v << 16)) & 0x1F0000FF0000FFull;
    v = (v | (v << 8)) & 0x100F00F00F00F00Full;
    v = (v | (v << 4)) & 0x10C30C30C30C30C3ull;
    v = (v | (v << 2)) & 0x1249249249249249ull;
    return v;
}
// One frame is the batch of one: with frames == 1 every row is frame 0 and bits 60 .. 63 of its key are 0.  A row whose batch column lies
// outside 0 .. frames - 1 raises bit 1 of the flag word and is keyed as frame 0: it neither enters the key nor indexes a counter.
// dups [frames]: adjacent equal keys per frame (k_raht_dups); rows [frames]: rows per frame, or null where nobody asks (a single frame);
// flags: bit 0 = a coordinate outside [0, 2^20), bit 1 = a batch index outside 0 .. frames - 1
__global__ void __launch_bounds__(256) k_raht_keys(const int4* __restrict__ coords, int64_t n, int frames, uint64_t* __restrict__ keys,
                                                   int32_t* __restrict__ idx, int32_t* rows, int32_t* flags) {
    __shared__ int32_t cnt[RAHT_MAX_FRAMES];
    if (rows) {                                                // (uniform)
        if (threadIdx.x < RAHT_MAX_FRAMES) cnt[threadIdx.x] = 0;
        __syncthreads();
    }
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const int4 c = coords[i];
        const int bad = ((((uint32_t)c.y | (uint32_t)c.z | (uint32_t)c.w) >> 20) ? 1 : 0) | ((uint32_t)c.x >= (uint32_t)frames ? 2 : 0);
        if (bad) atomicOr(flags, bad);
        const uint32_t f = (bad & 2) ? 0u : (uint32_t)c.x;
        const uint64_t m = spread3((uint32_t)c.y) | (spread3((uint32_t)c.z) << 1) | (spread3((uint32_t)c.w) << 2);
        keys[i] = (m & ((1ull << RAHT_FRAME_BIT) - 1)) | ((uint64_t)f << RAHT_FRAME_BIT);
        idx[i] = (int32_t)i;
        if (rows && !(bad & 2)) atomicAdd(&cnt[f], 1);
    }
    if (rows) {
        __syncthreads();
        if (threadIdx.x < RAHT_MAX_FRAMES && cnt[threadIdx.x]) atomicAdd(rows + threadIdx.x, cnt[threadIdx.x]);
    }
}
__global__ void __launch_bounds__(256) k_raht_dups(const uint64_t* __restrict__ keys, int64_t n, int32_t* dups) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i + 1 < n && keys[i] == keys[i + 1]) atomicAdd(dups + (int)(keys[i] >> RAHT_FRAME_BIT), 1);      // (< frames: k_raht_keys wrote the key)
}

template <typename K>
static size_t sort_temp_bytes(int64_t n, int bits) {
    size_t tmp = 0;
    (void)rocprim::radix_sort_pairs((void*)nullptr, tmp, (K*)nullptr, (K*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr, (size_t)n, 0, bits,
                                    (hipStream_t)0);
    return tmp;
}

// The entries below are thin: each checks what is its own to check under its own name (`who`, as PCGC_REQUIRE would print it), then calls
// the one implementation of its step, which takes `frames`.  who + 5 is the name without "pcgc_", as the launch errors print it.
#define RAHT_REQUIRE(who, cond, msg) do { if (!(cond)) { pcgc_set_error("%s: %s", who, msg); return -2; } } while (0)
#define RAHT_CHECK_HIP(who, e) do { if ((e) != hipSuccess) { pcgc_set_error("%s: %s", (who) + 5, hipGetErrorString(e)); return -1; } } while (0)

// sort_bits: the sort's end bit, 60 for the single entry and 64 for the batch's (unsigned: frames 8 .. 15 set bit 63)
static size_t keys_workspace_bytes(int64_t n, int sort_bits) {
    if (n < 1) n = 1;
    return align256((size_t)n * 8) + align256((size_t)n * 4) + align256(sort_temp_bytes<uint64_t>(n, sort_bits));
}
// status: status_ints ints, zeroed here; dups = status [frames], rows and flags point into it
static int raht_keys(const char* who, const int32_t* coords, int64_t n, int frames, int sort_bits, uint64_t* keys, int32_t* perm, int32_t* status,
                     int status_ints, int32_t* rows, int32_t* flags, void* workspace, size_t workspace_bytes, hipStream_t s) {
    RAHT_REQUIRE(who, n >= 1 && n <= RAHT_MAX_POINTS, "1 to 2^24 points");
    RAHT_REQUIRE(who, frames >= 1 && frames <= RAHT_MAX_FRAMES, "1 to 16 frames");
    RAHT_REQUIRE(who, coords && keys && perm && status && workspace, "null argument");
    RAHT_REQUIRE(who, workspace_bytes >= keys_workspace_bytes(n, sort_bits), "workspace too small");
    char* ws = (char*)workspace;
    uint64_t* kin = (uint64_t*)ws; ws += align256((size_t)n * 8);
    int32_t* idx = (int32_t*)ws; ws += align256((size_t)n * 4);
    size_t tmp = sort_temp_bytes<uint64_t>(n, sort_bits);
    hipError_t e = hipMemsetAsync(status, 0, status_ints * sizeof(int32_t), s);
    RAHT_CHECK_HIP(who, e);
    hipLaunchKernelGGL(k_raht_keys, dim3(grid_for(n, 256)), dim3(256), 0, s, (const int4*)coords, n, frames, kin, idx, rows, flags);
    PCGC_CHECK_LAUNCH(who + 5);
    e = rocprim::radix_sort_pairs((void*)ws, tmp, kin, keys, idx, perm, (size_t)n, 0, sort_bits, s);
    RAHT_CHECK_HIP(who, e);
    hipLaunchKernelGGL(k_raht_dups, dim3(grid_for(n, 256)), dim3(256), 0, s, keys, n, status);
    PCGC_CHECK_LAUNCH(who + 5);
    return 0;
}
// status [2]: adjacent equal keys, then the flag word (bit 1: a non-zero batch column)
extern "C" size_t pcgc_raht_keys_workspace_bytes(int64_t n) { return keys_workspace_bytes(n, RAHT_FRAME_BIT); }
extern "C" int pcgc_raht_keys(const int32_t* coords, int64_t n, uint64_t* keys, int32_t* perm, int32_t* status, void* workspace,
                              size_t workspace_bytes, void* stream) {
    return raht_keys(__func__, coords, n, 1, RAHT_FRAME_BIT, keys, perm, status, 2, nullptr, status ? status + 1 : nullptr, workspace, workspace_bytes,
                     S(stream));
}
// status [34]: [0 .. 15] adjacent equal keys per frame, [16 .. 31] rows per frame, [32] the flag word
extern "C" int64_t pcgc_raht_keys_batch_workspace_bytes(int64_t n) { return (int64_t)keys_workspace_bytes(n, 64); }
extern "C" int pcgc_raht_keys_batch(const int32_t* coords, int64_t n, int frames, uint64_t* keys, int32_t* perm, int32_t* status, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    return raht_keys(__func__, coords, n, frames, 64, keys, perm, status, 34, status ? status + RAHT_MAX_FRAMES : nullptr,
                     status ? status + 2 * RAHT_MAX_FRAMES : nullptr, workspace, workspace_bytes, S(stream));
}

// ------------------------------------------------------------------------------------------------------------------ tree
__device__ static inline int msb64(uint64_t v) { return 63 - __clzll((long long)v); }

// gap g of split bit d = msb(key_g ^ key_{g+1}): the range [lo, hi] of the merged node and its two children (a gap, or ~leaf)
__device__ static inline void tree_gap(const uint64_t* __restrict__ keys, int64_t n, int64_t g, int d, int64_t& lo, int64_t& hi, int32_t& left,
                                   int32_t& right) {
    const uint64_t ki = keys[g], kj = keys[g + 1];
    int64_t a = 0, b = g;                                  // lo: the first leaf that shares key_i's bits above d
    while (a < b) { const int64_t m = (a + b) >> 1; if (((keys[m] ^ ki) >> (d + 1)) == 0) b = m; else a = m + 1; }
    lo = a;
    a = g + 1; b = n - 1;                                  // hi: the last one
    while (a < b) { const int64_t m = (a + b + 1) >> 1; if (((keys[m] ^ kj) >> (d + 1)) == 0) a = m; else b = m - 1; }
    hi = a;
    left = ~(int32_t)g; right = ~(int32_t)(g + 1);
    if (lo < g) {                                          // the split of [lo, g]: the last leaf whose bit dl is key_lo's
        const uint64_t kl = keys[lo];
        const int dl = msb64((kl ^ ki) | 1ull);
        a = lo; b = g - 1;
        while (a < b) { const int64_t m = (a + b + 1) >> 1; if (((keys[m] ^ kl) >> dl) == 0) a = m; else b = m - 1; }
        left = (int32_t)a;
    }
    if (hi > g + 1) {
        const int dr = msb64((kj ^ keys[hi]) | 1ull);
        a = g + 1; b = hi - 1;
        while (a < b) { const int64_t m = (a + b + 1) >> 1; if (((keys[m] ^ kj) >> dr) == 0) a = m; else b = m - 1; }
        right = (int32_t)a;
    }
}

// cnt [(frames + 1) x 64]: gaps per frame and split bit, then (row `frames`) those of all frames whose range crosses a tile boundary.  The LDS
// array has the size of the largest batch; only the used rows are zeroed and flushed (128 counters for a single frame).
// A frame boundary (frames > 1 and d >= 60) is no merge: lo = hi = -1, no children, counted nowhere, sorted behind everything.
// K: the type of the coding order's sort key, frame * 64 + 63 - d: uint8_t holds it for a single frame, a batch needs uint16_t.
#define RAHT_CNT_MAX ((RAHT_MAX_FRAMES + 1) * 64)
template <typename K>
__global__ void __launch_bounds__(256) k_raht_tree(const uint64_t* __restrict__ keys, int64_t n, int frames, int32_t tile, uint8_t* __restrict__ d8,
                                                   int32_t* __restrict__ lo_o, int32_t* __restrict__ hi_o, int32_t* __restrict__ left_o,
                                                   int32_t* __restrict__ right_o, K* __restrict__ skey, uint8_t* __restrict__ skey_cross,
                                                   int32_t* __restrict__ idx, int32_t* cnt) {
    __shared__ int32_t h[RAHT_CNT_MAX];
    const int used = (frames + 1) * 64;
    for (int j = threadIdx.x; j < used; j += 256) h[j] = 0;
    __syncthreads();
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g < n - 1) {
        const int d = msb64((keys[g] ^ keys[g + 1]) | 1ull);   // (| 1: equal keys are refused by the caller; this keeps the shifts defined)
        idx[g] = (int32_t)g;
        d8[g] = (uint8_t)d;
        if (frames > 1 && d >= RAHT_FRAME_BIT) {
            lo_o[g] = -1; hi_o[g] = -1; left_o[g] = ~(int32_t)g; right_o[g] = ~(int32_t)(g + 1);
            skey[g] = (K)(RAHT_MAX_FRAMES * 64); skey_cross[g] = 128;
        } else {
            int64_t lo, hi;
            int32_t left, right;
            tree_gap(keys, n, g, d, lo, hi, left, right);
            const int cross = (lo / tile) != (hi / tile);
            const int f = frames > 1 ? (int)(keys[g] >> RAHT_FRAME_BIT) : 0;
            lo_o[g] = (int32_t)lo; hi_o[g] = (int32_t)hi; left_o[g] = left; right_o[g] = right;
            skey[g] = (K)(f * 64 + 63 - d); skey_cross[g] = (uint8_t)((63 - d) | (cross ? 0 : 64));
            if (f < frames) {                                  // (always, for keys pcgc_raht_keys wrote)
                atomicAdd(&h[f * 64 + d], 1);
                if (cross) atomicAdd(&h[frames * 64 + d], 1);
            }
        }
    }
    __syncthreads();
    for (int j = threadIdx.x; j < used; j += 256) if (h[j]) atomicAdd(cnt + j, h[j]);
}
// offsets [(frames + 1) x 65]: bucket [65] of every frame (counted from the frame's own first gap), then cross [65] of all frames; the gaps
// of split bit d are list[off[63 - d] .. off[64 - d]).  A single frame: bucket [65], then cross [65].
__global__ void k_raht_offsets(const int32_t* __restrict__ cnt, int frames, int32_t* __restrict__ offsets) {
    if ((int)threadIdx.x <= frames) {
        const int32_t* c = cnt + 64 * threadIdx.x;
        int32_t* o = offsets + 65 * threadIdx.x;
        int32_t acc = 0;
        for (int b = 0; b < 64; ++b) { o[b] = acc; acc += c[63 - b]; }
        o[64] = acc;
    }
}

// the two sorts run one after the other and share their temporary storage
template <typename K>
static size_t tree_sort_temp_bytes(size_t g, int order_bits, int cross_bits) {
    const size_t a = sort_temp_bytes<K>((int64_t)g, order_bits), b = sort_temp_bytes<uint8_t>((int64_t)g, cross_bits);
    return a > b ? a : b;
}
template <typename K>
static size_t tree_workspace_bytes(int64_t n, int frames, int order_bits, int cross_bits) {
    const size_t g = (size_t)(n < 2 ? 1 : n - 1);
    return 2 * align256(g * sizeof(K)) + 2 * align256(g) + align256(g * 4) + align256((size_t)(frames + 1) * 64 * 4) +
           align256(tree_sort_temp_bytes<K>(g, order_bits, cross_bits));
}
// order_bits, cross_bits: the end bits of the two sorts (6 and 7 for the single entry, 11 and 8 for the batch's); sized: what the entry's own
// sizing call answers, at least tree_workspace_bytes<K>(n, frames, ..)
template <typename K>
static int raht_tree(const char* who, const uint64_t* keys, int64_t n, int frames, int order_bits, int cross_bits, uint8_t* d, int32_t* lo,
                     int32_t* hi, int32_t* left, int32_t* right, int32_t* order, int32_t* cross_order, int32_t* offsets, void* workspace,
                     size_t workspace_bytes, size_t sized, hipStream_t s) {
    RAHT_REQUIRE(who, n >= 1 && n <= RAHT_MAX_POINTS, "1 to 2^24 points");
    RAHT_REQUIRE(who, frames >= 1 && frames <= RAHT_MAX_FRAMES && (frames == 1 || sizeof(K) > 1), "1 to 16 frames");
    RAHT_REQUIRE(who, offsets && workspace, "null argument");
    RAHT_REQUIRE(who, workspace_bytes >= sized, "workspace too small");
    const int64_t g = n - 1;
    const size_t g1 = (size_t)(g < 1 ? 1 : g), cnt_bytes = (size_t)(frames + 1) * 64 * 4;
    char* ws = (char*)workspace;
    K* skey = (K*)ws; ws += align256(g1 * sizeof(K));
    K* sorted = (K*)ws; ws += align256(g1 * sizeof(K));
    uint8_t* skey_cross = (uint8_t*)ws; ws += align256(g1);
    uint8_t* sorted_cross = (uint8_t*)ws; ws += align256(g1);
    int32_t* idx = (int32_t*)ws; ws += align256(g1 * 4);
    int32_t* cnt = (int32_t*)ws; ws += align256(cnt_bytes);
    hipError_t e = hipMemsetAsync(cnt, 0, cnt_bytes, s);
    RAHT_CHECK_HIP(who, e);
    if (g > 0) {
        RAHT_REQUIRE(who, keys && d && lo && hi && left && right && order && cross_order, "null argument");
        hipLaunchKernelGGL(k_raht_tree<K>, dim3(grid_for(g, 256)), dim3(256), 0, s, keys, n, frames, (int32_t)RAHT_TILE, d, lo, hi, left, right, skey,
                           skey_cross, idx, cnt);
        PCGC_CHECK_LAUNCH(who + 5);
        size_t tmp = tree_sort_temp_bytes<K>(g1, order_bits, cross_bits);
        e = rocprim::radix_sort_pairs((void*)ws, tmp, skey, sorted, idx, order, (size_t)g, 0, order_bits, s);
        if (e == hipSuccess) e = rocprim::radix_sort_pairs((void*)ws, tmp, skey_cross, sorted_cross, idx, cross_order, (size_t)g, 0, cross_bits, s);
        RAHT_CHECK_HIP(who, e);
    }
    hipLaunchKernelGGL(k_raht_offsets, dim3(1), dim3(64), 0, s, (const int32_t*)cnt, frames, offsets);
    PCGC_CHECK_LAUNCH(who + 5);
    return 0;
}
extern "C" size_t pcgc_raht_tree_workspace_bytes(int64_t n) { return tree_workspace_bytes<uint8_t>(n, 1, 6, 7); }
extern "C" int pcgc_raht_tree(const uint64_t* keys, int64_t n, uint8_t* d, int32_t* lo, int32_t* hi, int32_t* left, int32_t* right,
                              int32_t* order, int32_t* cross_order, int32_t* offsets, void* workspace, size_t workspace_bytes, void* stream) {
    return raht_tree<uint8_t>(__func__, keys, n, 1, 6, 7, d, lo, hi, left, right, order, cross_order, offsets, workspace, workspace_bytes,
                              pcgc_raht_tree_workspace_bytes(n), S(stream));
}
extern "C" int64_t pcgc_raht_tree_batch_workspace_bytes(int64_t n) { return (int64_t)tree_workspace_bytes<uint16_t>(n, RAHT_MAX_FRAMES, 11, 8); }
extern "C" int pcgc_raht_tree_batch(const uint64_t* keys, int64_t n, int frames, uint8_t* d, int32_t* lo, int32_t* hi, int32_t* left, int32_t* right,
                                    int32_t* order, int32_t* cross_order, int32_t* offsets, void* workspace, size_t workspace_bytes,
                                    void* stream) {
    return raht_tree<uint16_t>(__func__, keys, n, frames, 11, 8, d, lo, hi, left, right, order, cross_order, offsets, workspace, workspace_bytes,
                               (size_t)pcgc_raht_tree_batch_workspace_bytes(n), S(stream));
}


// ------------------------------------------------------------------------------------------------------------------ colour space, lifting
__device__ static inline i3 ycocg_fwd(const uint8_t* __restrict__ rgb, int64_t row) {
    const int32_t r = rgb[3 * row], g = rgb[3 * row + 1], b = rgb[3 * row + 2];
    const int32_t co = r - b, t = b + (co >> 1), cg = g - t;
    return i3{t + (cg >> 1), co, cg};
}
__device__ static inline int32_t clamp255(int32_t v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
__device__ static inline void ycocg_inv(i3 v, uint8_t* __restrict__ rgb, int64_t row) {
    // (wrapping 32-bit sums, as the definition's int32 node values give them; a sound stream stays far inside)
    const int32_t t = (int32_t)((uint32_t)v.a - (uint32_t)(v.c >> 1)), g = (int32_t)((uint32_t)v.c + (uint32_t)t);
    const int32_t b = (int32_t)((uint32_t)t - (uint32_t)(v.b >> 1)), r = (int32_t)((uint32_t)b + (uint32_t)v.b);
    rgb[3 * row] = (uint8_t)clamp255(r); rgb[3 * row + 1] = (uint8_t)clamp255(g); rgb[3 * row + 2] = (uint8_t)clamp255(b);
}
__device__ static inline int64_t floor_div(int64_t num, int64_t den) {          // 0 < den <= 2^25
    if (num == (int64_t)(int32_t)num) {                        // (nearly always: |H| <= 510 forward, a 64-bit division costs several times more)
        const int32_t n32 = (int32_t)num, d32 = (int32_t)den, q = n32 / d32;
        return q - ((n32 % d32) < 0 ? 1 : 0);
    }
    const int64_t q = num / den;
    return q - ((num % den) < 0 ? 1 : 0);
}
// H = a2 - a1; L = a1 + floor(w2 H / (w1 + w2))
__device__ static inline void lift_fwd(i3 a1, i3 a2, int64_t w1, int64_t w2, i3& L, i3& H) {
    H = i3{a2.a - a1.a, a2.b - a1.b, a2.c - a1.c};
    const int64_t w = w1 + w2;
    L = i3{a1.a + (int32_t)floor_div(w2 * H.a, w), a1.b + (int32_t)floor_div(w2 * H.b, w), a1.c + (int32_t)floor_div(w2 * H.c, w)};
}
// a1 = L - floor(w2 H^ / (w1 + w2)); a2 = a1 + H^   (64-bit products, values stored as int32)
__device__ static inline void lift_inv(i3 L, i3 H, int64_t w1, int64_t w2, i3& a1, i3& a2) {
    const int64_t w = w1 + w2;
    a1 = i3{(int32_t)((int64_t)L.a - floor_div(w2 * H.a, w)), (int32_t)((int64_t)L.b - floor_div(w2 * H.b, w)),
            (int32_t)((int64_t)L.c - floor_div(w2 * H.c, w))};
    a2 = i3{(int32_t)((int64_t)a1.a + H.a), (int32_t)((int64_t)a1.b + H.b), (int32_t)((int64_t)a1.c + H.c)};
}

__global__ void __launch_bounds__(256) k_raht_load(const uint8_t* __restrict__ rgb, const int32_t* __restrict__ perm, int64_t n, i3* __restrict__ val) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) val[i] = ycocg_fwd(rgb, perm[i]);
}
__global__ void __launch_bounds__(256) k_raht_store(const i3* __restrict__ val, const int32_t* __restrict__ perm, int64_t n, uint8_t* __restrict__ rgb) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) ycocg_inv(val[i], rgb, perm[i]);
}
__global__ void k_raht_set_dc(i3* val, i3 dc) { if (threadIdx.x == 0 && blockIdx.x == 0) val[0] = dc; }

// the gaps list[begin .. end): all of one split bit, so their ranges are disjoint
template <bool FWD>
__device__ static inline void lift_node(int64_t n, int32_t g, int32_t l, int32_t h, i3* val, i3* H) {
    if (l < 0 || l > g || h <= g || h >= n) return;            // (never, for a tree pcgc_raht_tree built)
    const int64_t w1 = g - l + 1, w2 = h - g;
    if (FWD) {
        i3 L, Hg;
        lift_fwd(val[l], val[g + 1], w1, w2, L, Hg);
        H[g] = Hg; val[l] = L;
    } else {
        i3 a1, a2;
        lift_inv(val[l], H[g], w1, w2, a1, a2);
        val[l] = a1; val[g + 1] = a2;
    }
}
template <bool FWD>
__device__ static inline void lift_gap(int64_t n, int32_t g, const int32_t* __restrict__ lo, const int32_t* __restrict__ hi, i3* val, i3* H) {
    lift_node<FWD>(n, g, lo[g], hi[g], val, H);
}
template <bool FWD>
__global__ void __launch_bounds__(256) k_raht_bit(const int32_t* __restrict__ list, int64_t begin, int64_t end, int64_t n,
                                                  const int32_t* __restrict__ lo, const int32_t* __restrict__ hi, i3* val, i3* H) {
    const int64_t p = begin + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= end) return;
    const int32_t g = list[p];
    if (g < 0 || g >= n - 1) return;
    lift_gap<FWD>(n, g, lo, hi, val, H);
}
// The gaps whose range crosses a tile boundary, by ONE workgroup: split bits ascending (forward) or descending (inverse), a barrier
// between bits.  offsets: the cross half of pcgc_raht_tree's offsets.
template <bool FWD>
__global__ void __launch_bounds__(RAHT_SPINE_THREADS) k_raht_spine(const int32_t* __restrict__ list, const int32_t* __restrict__ offsets, int64_t n,
                                                                   const int32_t* __restrict__ lo, const int32_t* __restrict__ hi, i3* val, i3* H) {
    // A level costs a chain of dependent memory round trips; the gap index and its (lo, hi) do not depend on the values, so they are
    // fetched one and two levels ahead (the first RAHT_SPINE_THREADS gaps of a level: the levels of the spine are short), which leaves
    // values -> stores -> barrier on the chain.
    __shared__ int32_t off[65];
    __shared__ int seq[64];                                    // the populated buckets in processing order (bucket b holds split bit 63 - b)
    __shared__ int ns_s;
    if (threadIdx.x < 65) { const int64_t o = offsets[threadIdx.x]; off[threadIdx.x] = (int32_t)(o < 0 ? 0 : (o > n - 1 ? n - 1 : o)); }
    __syncthreads();
    if (threadIdx.x == 0) {
        int c = 0;
        for (int s = 0; s < 64; ++s) { const int b = FWD ? 63 - s : s; if (off[b + 1] > off[b]) seq[c++] = b; }
        ns_s = c;
    }
    __syncthreads();
    const int ns = ns_s;
    int32_t g0 = -1, l0 = 0, h0 = 0, g1 = -1;
    if (ns > 0) { const int32_t p = off[seq[0]] + (int32_t)threadIdx.x; if (p < off[seq[0] + 1]) g0 = list[p]; }
    if (ns > 1) { const int32_t p = off[seq[1]] + (int32_t)threadIdx.x; if (p < off[seq[1] + 1]) g1 = list[p]; }
    if (g0 >= 0 && g0 < n - 1) { l0 = lo[g0]; h0 = hi[g0]; } else g0 = -1;
    for (int i = 0; i < ns; ++i) {                             // (uniform: every thread reads the same offsets)
        int32_t l1 = 0, h1 = 0, g2 = -1;
        if (g1 >= 0 && g1 < n - 1) { l1 = lo[g1]; h1 = hi[g1]; } else g1 = -1;
        if (i + 2 < ns) { const int32_t p = off[seq[i + 2]] + (int32_t)threadIdx.x; if (p < off[seq[i + 2] + 1]) g2 = list[p]; }
        if (g0 >= 0) lift_node<FWD>(n, g0, l0, h0, val, H);
        for (int64_t p = (int64_t)off[seq[i]] + threadIdx.x + RAHT_SPINE_THREADS; p < off[seq[i] + 1]; p += RAHT_SPINE_THREADS) {
            const int32_t g = list[p];
            if (g >= 0 && g < n - 1) lift_gap<FWD>(n, g, lo, hi, val, H);
        }
        __syncthreads();                                       // (orders this workgroup's global writes before its later reads)
        g0 = g1; l0 = l1; h0 = h1; g1 = g2;
    }
}
// One workgroup per RAHT_TILE consecutive leaves: every gap whose range lies inside the tile, in LDS, one split bit after the other.
// Forward: reads the colours through perm, writes H of its gaps and the tile's node values to val.  Inverse: reads val (what the spine
// left there), H^ of its gaps, writes the colours through perm.
template <bool FWD>
__global__ void __launch_bounds__(RAHT_THREADS) k_raht_tile(const uint8_t* __restrict__ rgb_in, uint8_t* __restrict__ rgb_out,
                                                            const int32_t* __restrict__ perm, int64_t n, const uint8_t* __restrict__ d8,
                                                            const int32_t* __restrict__ lo, const int32_t* __restrict__ hi, i3* val, i3* H) {
    // The tile's gaps are first ordered by split bit in LDS (a counting sort; the order inside a bit does not matter: its ranges are
    // disjoint), so that every pass over a bit keeps whole waves busy instead of the few lanes whose own gap has that bit.
    __shared__ i3 sv[RAHT_TILE];
    __shared__ uint32_t node[RAHT_TILE];                       // j | (lo - s) << 10 | w2 << 20, by split bit
    __shared__ int cnt[64], off[65];
    const int64_t s = (int64_t)blockIdx.x * RAHT_TILE;
    const int m = (int)(n - s < RAHT_TILE ? n - s : RAHT_TILE);
    if (threadIdx.x < 64) cnt[threadIdx.x] = 0;
    for (int j = threadIdx.x; j < m; j += RAHT_THREADS) sv[j] = FWD ? ycocg_fwd(rgb_in, perm[s + j]) : val[s + j];
    __syncthreads();
    uint32_t packed[RAHT_GAPS_PER_THREAD];
    int gd[RAHT_GAPS_PER_THREAD], rank[RAHT_GAPS_PER_THREAD];  // d (-1: not this tile's), place among the tile's gaps of that bit
#pragma unroll
    for (int k = 0; k < RAHT_GAPS_PER_THREAD; ++k) {
        const int j = threadIdx.x + k * RAHT_THREADS;          // the gap behind leaf s + j
        gd[k] = -1; rank[k] = 0; packed[k] = 0;
        if (j + 1 < m) {
            const int64_t g = s + j;
            const int64_t l = lo[g], h = hi[g];
            if (l >= s && l <= g && h > g && h < s + m) {
                gd[k] = d8[g] & 63;
                packed[k] = (uint32_t)j | ((uint32_t)(l - s) << 10) | ((uint32_t)(h - g) << 20);
                rank[k] = atomicAdd(&cnt[gd[k]], 1);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int acc = 0;
        for (int b = 0; b < 64; ++b) { off[b] = acc; acc += cnt[b]; }
        off[64] = acc;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < RAHT_GAPS_PER_THREAD; ++k)
        if (gd[k] >= 0) node[off[gd[k]] + rank[k]] = packed[k];
    __syncthreads();
    for (int t = 0; t < 64; ++t) {
        const int b = FWD ? t : 63 - t;
        const int begin = off[b], end = off[b + 1];
        if (begin == end) continue;                            // (uniform)
        for (int i = begin + (int)threadIdx.x; i < end; i += RAHT_THREADS) {
            const uint32_t v = node[i];
            const int j = (int)(v & 1023u), l = (int)((v >> 10) & 1023u);
            const int64_t w1 = j - l + 1, w2 = (int64_t)(v >> 20);
            if (FWD) {
                i3 L, Hg;
                lift_fwd(sv[l], sv[j + 1], w1, w2, L, Hg);
                H[s + j] = Hg; sv[l] = L;
            } else {
                i3 a1, a2;
                lift_inv(sv[l], H[s + j], w1, w2, a1, a2);
                sv[l] = a1; sv[j + 1] = a2;
            }
        }
        __syncthreads();
    }
    for (int j = threadIdx.x; j < m; j += RAHT_THREADS) {
        if (FWD) val[s + j] = sv[j];
        else ycocg_inv(sv[j], rgb_out, perm[s + j]);
    }
}

// `sets` groups of 65 offsets on the HOST, one behind the other in one list: each ascending, each starting where the one before ends, all
// within [0, n - 1]
static bool offsets_sound(const int32_t* off, int sets, int64_t n) {
    int32_t at = 0;
    for (int set = 0; set < sets; ++set) {
        if (off[65 * set] != at) return false;
        for (int b = 0; b < 64; ++b) if (off[65 * set + b + 1] < off[65 * set + b]) return false;
        at = off[65 * set + 64];
    }
    return at <= n - 1;
}

// One transform for one frame or a batch: a frame boundary has lo = hi = -1, so the tile kernel does not take it (l >= s fails), it is in no
// list the other two walk, and ranges of one split bit are disjoint across frames as they are inside one.  Form 0 walks `list` by `sets`
// groups of 65 host offsets per split bit: a single frame's coding order under its bucket offsets (one group), or a batch's cross_order,
// which lists every split bit twice (the crossing gaps, then the others: two groups).  The DCs of the inverse are set by the caller.
template <bool FWD>
static void raht_run(const uint8_t* rgb_in, uint8_t* rgb_out, const int32_t* perm, int64_t n, const uint8_t* d, const int32_t* lo, const int32_t* hi,
                     const int32_t* list, const int32_t* off, int sets, const int32_t* cross_order, const int32_t* cross_off_dev, int form, i3* val,
                     i3* H, hipStream_t s) {
    const unsigned tiles = grid_for(n, RAHT_TILE);
    if (form == 0) {
        if (FWD) hipLaunchKernelGGL(k_raht_load, dim3(grid_for(n, 256)), dim3(256), 0, s, rgb_in, perm, n, val);
        for (int k = 0; k < 64; ++k) {
            const int b = FWD ? 63 - k : k;
            for (int set = 0; set < sets; ++set) {
                const int64_t begin = off[65 * set + b], end = off[65 * set + b + 1];
                if (begin < end)
                    hipLaunchKernelGGL(k_raht_bit<FWD>, dim3(grid_for(end - begin, 256)), dim3(256), 0, s, list, begin, end, n, lo, hi, val, H);
            }
        }
        if (!FWD) hipLaunchKernelGGL(k_raht_store, dim3(grid_for(n, 256)), dim3(256), 0, s, val, perm, n, rgb_out);
    } else {
        if (FWD) hipLaunchKernelGGL(k_raht_tile<true>, dim3(tiles), dim3(RAHT_THREADS), 0, s, rgb_in, rgb_out, perm, n, d, lo, hi, val, H);
        if (tiles > 1)
            hipLaunchKernelGGL(k_raht_spine<FWD>, dim3(1), dim3(RAHT_SPINE_THREADS), 0, s, cross_order, cross_off_dev, n, lo, hi, val, H);
        if (!FWD) hipLaunchKernelGGL(k_raht_tile<false>, dim3(tiles), dim3(RAHT_THREADS), 0, s, rgb_in, rgb_out, perm, n, d, lo, hi, val, H);
    }
}
// what the four entries share; `list`, `off`, `sets` as raht_run takes them; other: the entry's own pointers, all of them non-null
static int raht_run_args(const char* who, int64_t n, int form, bool other, const void* rgb, const int32_t* perm, const int32_t* val,
                         const uint8_t* d, const int32_t* lo, const int32_t* hi, const int32_t* list, const int32_t* off, int sets,
                         const int32_t* cross_order, const int32_t* cross_off, const int32_t* H, const char* unsound) {
    RAHT_REQUIRE(who, form == 0 || form == 1, "form 0 (one launch per split bit) or 1 (tiles)");
    RAHT_REQUIRE(who, rgb && perm && val && off && cross_off && other, "null argument");
    RAHT_REQUIRE(who, n == 1 || (d && lo && hi && list && cross_order && H), "null argument");
    RAHT_REQUIRE(who, offsets_sound(off, sets, n), unsound);
    return 0;
}
static const char* const RAHT_BUCKET_UNSOUND = "bucket offsets are not those of a tree of n leaves";
static const char* const RAHT_BIT_UNSOUND = "bit offsets are not those of a batch tree of n leaves";

extern "C" int pcgc_raht_forward(const uint8_t* rgb, const int32_t* perm, int64_t n, const uint8_t* d, const int32_t* lo, const int32_t* hi,
                                 const int32_t* order, const int32_t* bucket_off, const int32_t* cross_order, const int32_t* cross_off, int form,
                                 int32_t* val, int32_t* H, void* stream) {
    PCGC_REQUIRE(n >= 1 && n <= RAHT_MAX_POINTS, "1 to 2^24 points");
    if (int r = raht_run_args(__func__, n, form, true, rgb, perm, val, d, lo, hi, order, bucket_off, 1, cross_order, cross_off, H, RAHT_BUCKET_UNSOUND))
        return r;
    raht_run<true>(rgb, nullptr, perm, n, d, lo, hi, order, bucket_off, 1, cross_order, cross_off, form, (i3*)val, (i3*)H, S(stream));
    PCGC_CHECK_LAUNCH("raht_forward");
    return 0;
}
extern "C" int pcgc_raht_inverse(const int32_t* Hhat, int32_t dc_y, int32_t dc_co, int32_t dc_cg, const int32_t* perm, int64_t n, const uint8_t* d,
                                 const int32_t* lo, const int32_t* hi, const int32_t* order, const int32_t* bucket_off,
                                 const int32_t* cross_order, const int32_t* cross_off, int form, int32_t* val, uint8_t* rgb, void* stream) {
    PCGC_REQUIRE(n >= 1 && n <= RAHT_MAX_POINTS, "1 to 2^24 points");
    if (int r = raht_run_args(__func__, n, form, true, rgb, perm, val, d, lo, hi, order, bucket_off, 1, cross_order, cross_off, Hhat, RAHT_BUCKET_UNSOUND))
        return r;
    hipLaunchKernelGGL(k_raht_set_dc, dim3(1), dim3(64), 0, S(stream), (i3*)val, i3{dc_y, dc_co, dc_cg});
    raht_run<false>(nullptr, rgb, perm, n, d, lo, hi, order, bucket_off, 1, cross_order, cross_off, form, (i3*)val, (i3*)const_cast<int32_t*>(Hhat),
                    S(stream));
    PCGC_CHECK_LAUNCH("raht_inverse");
    return 0;
}

// A batch: bit_off [130] on the HOST holds the two groups of 65 offsets into cross_order; every frame's DC stands at the start of its run.
__global__ void k_raht_set_dc_batch(i3* val, int64_t n, const int32_t* __restrict__ starts, const i3* __restrict__ dc, int frames) {
    const int b = threadIdx.x;
    if (b < frames && starts[b] >= 0 && starts[b] < n) val[starts[b]] = dc[b];
}
extern "C" int pcgc_raht_forward_batch(const uint8_t* rgb, const int32_t* perm, int64_t n, const uint8_t* d, const int32_t* lo, const int32_t* hi,
                                       const int32_t* cross_order, const int32_t* bit_off, const int32_t* cross_off, int form, int32_t* val,
                                       int32_t* H, void* stream) {
    PCGC_REQUIRE(n >= 1 && n <= RAHT_MAX_POINTS, "1 to 2^24 points");
    if (int r = raht_run_args(__func__, n, form, true, rgb, perm, val, d, lo, hi, cross_order, bit_off, 2, cross_order, cross_off, H, RAHT_BIT_UNSOUND))
        return r;
    raht_run<true>(rgb, nullptr, perm, n, d, lo, hi, cross_order, bit_off, 2, cross_order, cross_off, form, (i3*)val, (i3*)H, S(stream));
    PCGC_CHECK_LAUNCH("raht_forward_batch");
    return 0;
}
extern "C" int pcgc_raht_inverse_batch(const int32_t* Hhat, const int32_t* dc, const int32_t* starts, int frames, const int32_t* perm, int64_t n,
                                       const uint8_t* d, const int32_t* lo, const int32_t* hi, const int32_t* cross_order, const int32_t* bit_off,
                                       const int32_t* cross_off, int form, int32_t* val, uint8_t* rgb, void* stream) {
    PCGC_REQUIRE(n >= 1 && n <= RAHT_MAX_POINTS, "1 to 2^24 points");
    PCGC_REQUIRE(frames >= 1 && frames <= RAHT_MAX_FRAMES, "1 to 16 frames");
    if (int r = raht_run_args(__func__, n, form, dc && starts, rgb, perm, val, d, lo, hi, cross_order, bit_off, 2, cross_order, cross_off, Hhat,
                              RAHT_BIT_UNSOUND))
        return r;
    hipLaunchKernelGGL(k_raht_set_dc_batch, dim3(1), dim3(64), 0, S(stream), (i3*)val, n, starts, (const i3*)dc, frames);
    raht_run<false>(nullptr, rgb, perm, n, d, lo, hi, cross_order, bit_off, 2, cross_order, cross_off, form, (i3*)val,
                    (i3*)const_cast<int32_t*>(Hhat), S(stream));
    PCGC_CHECK_LAUNCH("raht_inverse_batch");
    return 0;
}


// ------------------------------------------------------------------------------------------------------------------ quantiser
__device__ static inline uint32_t isqrt64(uint64_t v) {       // v < 2^52
    uint64_t r = 0;
#pragma unroll
    for (int b = 25; b >= 0; --b) { const uint64_t t = r | (1ull << b); if (t * t <= v) r = t; }
    return (uint32_t)r;
}
// the step in sixteenths: Q sqrt((w1 + w2) / (w1 w2)), at least 1
__device__ static inline int64_t delta16(int Q, int64_t w1, int64_t w2) {
    if (Q == 0) return 16;
    const uint32_t r = isqrt64((uint64_t)(256ll * Q * Q * (w1 + w2)) / (uint64_t)(w1 * w2));
    return r < 16 ? 16 : (int64_t)r;
}
__device__ static inline int32_t level_z(int32_t H, int64_t D) {               // z = 2 k (k >= 0), -2 k - 1 (k < 0)
    const int64_t a = H < 0 ? -(int64_t)H : (int64_t)H;
    const int64_t k = (32 * a + D) / (2 * D);
    const int64_t z = (H < 0 && k > 0) ? 2 * k - 1 : 2 * k;
    return (int32_t)(z > 63 + 1023 ? 63 + 1023 : z);           // (|H| <= 510 gives z <= 1020; an escape has 10 bits)
}

// The steps of every frame, passed by value.  coded = n - frames positions of the coding order (a batch's frame boundaries lie behind them).
// The frame of a position is bits 60 .. 63 of its gap's key; with one frame it is 0 and `keys` is not read (the single entries pass null).
struct RahtSteps { uint8_t luma[RAHT_MAX_FRAMES], chroma[RAHT_MAX_FRAMES]; };

// the frame of gap g, -1 for a gap that is no merge of frames 0 .. frames - 1 (never, for a tree pcgc_raht_tree built)
__device__ static inline int frame_of_gap(const uint64_t* __restrict__ keys, int frames, int64_t gaps, int32_t g, const int32_t* __restrict__ lo) {
    if (g < 0 || g >= gaps || lo[g] < 0) return -1;
    const int f = frames > 1 ? (int)(keys[g] >> RAHT_FRAME_BIT) : 0;
    return f < frames ? f : -1;
}
// frame f's steps.  A lane's own index into the by-value table is a load from the kernel's arguments in memory; a single frame reads
// entry 0, which is a scalar register like the two ints it stands for
__device__ static inline void steps_at(const RahtSteps& q, int frames, int f, int& q_luma, int& q_chroma) {
    q_luma = frames > 1 ? q.luma[f] : q.luma[0];
    q_chroma = frames > 1 ? q.chroma[f] : q.chroma[0];
}
// one thread per position of the coding order; hist [frames, 48, 64]
__global__ void __launch_bounds__(256) k_raht_quantize(const i3* __restrict__ H, int64_t coded, int64_t gaps, int frames, const uint64_t* __restrict__ keys,
                                                       const uint8_t* __restrict__ d8, const int32_t* __restrict__ lo, const int32_t* __restrict__ hi,
                                                       const int32_t* __restrict__ order, RahtSteps q, int16_t* __restrict__ tokens,
                                                       uint16_t* __restrict__ ctx, uint8_t* __restrict__ escmask, uint16_t* __restrict__ rem,
                                                       int32_t* hist) {
    // the block's LDS histogram is that of the frame of its first position; the few positions of a block that belong to a later frame go
    // to the global histogram directly (integer atomics either way: the sums do not depend on the order)
    __shared__ int32_t h[RAHT_CONTEXTS * 64];
    __shared__ int f0_s;
    for (int j = threadIdx.x; j < RAHT_CONTEXTS * 64; j += 256) h[j] = 0;
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int32_t g = p < coded ? order[p] : -1;
    const int f = frame_of_gap(keys, frames, gaps, g, lo);
    if (threadIdx.x == 0) f0_s = f;
    __syncthreads();
    const int f0 = f0_s;
    if (f >= 0) {
        const int64_t w1 = g - lo[g] + 1, w2 = hi[g] - g;
        const i3 v = H[g];
        int q_luma, q_chroma;
        steps_at(q, frames, f, q_luma, q_chroma);
        const int64_t dl = delta16(q_luma, w1, w2), dc = delta16(q_chroma, w1, w2);
        const int row = (d8[g] & 63) / 3 < 15 ? (d8[g] & 63) / 3 : 15;
        const int32_t z[3] = {level_z(v.a, dl), level_z(v.b, dc), level_z(v.c, dc)};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int t = z[c] < RAHT_ESCAPE ? z[c] : RAHT_ESCAPE;
            tokens[3 * p + c] = (int16_t)t;
            ctx[3 * p + c] = (uint16_t)(16 * c + row);
            escmask[3 * p + c] = t == RAHT_ESCAPE;
            rem[3 * p + c] = (uint16_t)(t == RAHT_ESCAPE ? z[c] - RAHT_ESCAPE : 0);
            if (f == f0) atomicAdd(&h[(16 * c + row) * 64 + t], 1);
            else atomicAdd(hist + ((int64_t)f * RAHT_CONTEXTS + 16 * c + row) * 64 + t, 1);
        }
    } else if (p < coded) {                                    // (never, see frame_of_gap)
#pragma unroll
        for (int c = 0; c < 3; ++c) { tokens[3 * p + c] = 0; ctx[3 * p + c] = (uint16_t)(16 * c); escmask[3 * p + c] = 0; rem[3 * p + c] = 0; }
    }
    __syncthreads();
    if (f0 >= 0)
        for (int j = threadIdx.x; j < RAHT_CONTEXTS * 64; j += 256) if (h[j]) atomicAdd(hist + (int64_t)f0 * RAHT_CONTEXTS * 64 + j, h[j]);
}
__global__ void __launch_bounds__(256) k_raht_compact_esc(const uint8_t* __restrict__ escmask, const int32_t* __restrict__ prefix,
                                                          const uint16_t* __restrict__ rem, int64_t n, uint16_t* __restrict__ esc) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && escmask[i]) esc[prefix[i]] = rem[i];
}

static bool steps_of(const int32_t* q_luma, const int32_t* q_chroma, int frames, RahtSteps& q) {
    memset(&q, 0, sizeof(q));
    for (int b = 0; b < frames; ++b) {
        if (q_luma[b] < 0 || q_luma[b] > 255 || q_chroma[b] < 0 || q_chroma[b] > 255) return false;
        q.luma[b] = (uint8_t)q_luma[b]; q.chroma[b] = (uint8_t)q_chroma[b];
    }
    return true;
}
static size_t tokens_of(int64_t n, int frames) { return (size_t)(n - frames < 1 ? 1 : 3 * (n - frames)); }

static size_t quantize_workspace_bytes(int64_t n, int frames) {
    const size_t t = tokens_of(n, frames);
    return align256(t) + align256(t * 2) + align256(t * 4) + align256(pcgc_scan_workspace_bytes((int64_t)t));
}
static int raht_quantize(const char* who, const int32_t* H, int64_t n, int frames, const uint64_t* keys, const uint8_t* d, const int32_t* lo,
                         const int32_t* hi, const int32_t* order, const RahtSteps& q, int16_t* tokens, uint16_t* ctx, uint16_t* escapes,
                         int32_t* n_escapes, int32_t* hist, void* workspace, size_t workspace_bytes, void* stream) {
    RAHT_REQUIRE(who, n_escapes && hist && workspace, "null argument");
    RAHT_REQUIRE(who, workspace_bytes >= quantize_workspace_bytes(n, frames), "workspace too small");
    hipError_t e = hipMemsetAsync(hist, 0, (size_t)frames * RAHT_CONTEXTS * 64 * sizeof(int32_t), S(stream));
    if (e == hipSuccess) e = hipMemsetAsync(n_escapes, 0, sizeof(int32_t), S(stream));
    RAHT_CHECK_HIP(who, e);
    if (n == frames) return 0;
    RAHT_REQUIRE(who, H && (frames == 1 || keys) && d && lo && hi && order && tokens && ctx && escapes, "null argument");
    const int64_t coded = n - frames, t = 3 * coded;
    char* ws = (char*)workspace;
    uint8_t* escmask = (uint8_t*)ws; ws += align256((size_t)t);
    uint16_t* rem = (uint16_t*)ws; ws += align256((size_t)t * 2);
    int32_t* prefix = (int32_t*)ws; ws += align256((size_t)t * 4);
    hipLaunchKernelGGL(k_raht_quantize, dim3(grid_for(coded, 256)), dim3(256), 0, S(stream), (const i3*)H, coded, n - 1, frames, keys, d, lo, hi, order,
                       q, tokens, ctx, escmask, rem, hist);
    PCGC_CHECK_LAUNCH(who + 5);
    if (pcgc_mask_scan(escmask, t, prefix, n_escapes, ws, pcgc_scan_workspace_bytes(t), stream) != 0) return -1;
    hipLaunchKernelGGL(k_raht_compact_esc, dim3(grid_for(t, 256)), dim3(256), 0, S(stream), escmask, prefix, rem, t, escapes);
    PCGC_CHECK_LAUNCH(who + 5);
    return 0;
}
extern "C" size_t pcgc_raht_quantize_workspace_bytes(int64_t n) { return quantize_workspace_bytes(n, 1); }
extern "C" int pcgc_raht_quantize(const int32_t* H, int64_t n, const uint8_t* d, const int32_t* lo, const int32_t* hi, const int32_t* order,
                                  int q_luma, int q_chroma, int16_t* tokens, uint16_t* ctx, uint16_t* escapes, int32_t* n_escapes, int32_t* hist,
                                  void* workspace, size_t workspace_bytes, void* stream) {
    PCGC_REQUIRE(n >= 1 && n <= RAHT_MAX_POINTS, "1 to 2^24 points");
    RahtSteps q;
    PCGC_REQUIRE(steps_of(&q_luma, &q_chroma, 1, q), "quantiser 0 .. 255");
    return raht_quantize(__func__, H, n, 1, nullptr, d, lo, hi, order, q, tokens, ctx, escapes, n_escapes, hist, workspace, workspace_bytes, stream);
}
extern "C" int64_t pcgc_raht_quantize_batch_workspace_bytes(int64_t n, int frames) { return (int64_t)quantize_workspace_bytes(n, frames); }
extern "C" int pcgc_raht_quantize_batch(const int32_t* H, int64_t n, int frames, const uint64_t* keys, const uint8_t* d, const int32_t* lo,
                                        const int32_t* hi, const int32_t* order, const int32_t* q_luma, const int32_t* q_chroma, int16_t* tokens,
                                        uint16_t* ctx, uint16_t* escapes, int32_t* n_escapes, int32_t* hist, void* workspace,
                                        size_t workspace_bytes, void* stream) {
    PCGC_REQUIRE(n >= 1 && n <= RAHT_MAX_POINTS, "1 to 2^24 points");
    PCGC_REQUIRE(frames >= 1 && frames <= RAHT_MAX_FRAMES && frames <= n, "1 to 16 frames of at least one point");
    PCGC_REQUIRE(q_luma && q_chroma, "null argument");
    RahtSteps q;
    PCGC_REQUIRE(steps_of(q_luma, q_chroma, frames, q), "quantiser 0 .. 255");
    return raht_quantize(__func__, H, n, frames, keys, d, lo, hi, order, q, tokens, ctx, escapes, n_escapes, hist, workspace, workspace_bytes, stream);
}

// ------------------------------------------------------------------------------------------------------------------ dequantiser
// the mask of the tokens that are 63, and how many of them each frame has (counts [16], zeroed by the caller; null: nobody asks)
__global__ void __launch_bounds__(256) k_raht_escmask(const int16_t* __restrict__ tokens, int64_t n, const int32_t* __restrict__ order,
                                                      const uint64_t* __restrict__ keys, const int32_t* __restrict__ lo, int64_t gaps, int frames,
                                                      uint8_t* __restrict__ escmask, int32_t* counts) {
    __shared__ int32_t c[RAHT_MAX_FRAMES];
    if (counts) {                                              // (uniform)
        if (threadIdx.x < RAHT_MAX_FRAMES) c[threadIdx.x] = 0;
        __syncthreads();
    }
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const bool m = tokens[i] == RAHT_ESCAPE;
        escmask[i] = m;
        if (m && counts) { const int f = frame_of_gap(keys, frames, gaps, order[i / 3], lo); if (f >= 0) atomicAdd(&c[f], 1); }
    }
    if (counts) {
        __syncthreads();
        if (threadIdx.x < RAHT_MAX_FRAMES && c[threadIdx.x]) atomicAdd(counts + threadIdx.x, c[threadIdx.x]);
    }
}
__device__ static inline int32_t dequant(int32_t z, int64_t D) {
    const int64_t k = z >> 1;                                  // |k| of an even z; an odd z = -2 k - 1 has |k| = (z + 1) / 2
    const int64_t a = (z & 1) ? k + 1 : k;
    const int64_t v = (a * D + 8) / 16;
    return (int32_t)((z & 1) ? -v : v);
}
__global__ void __launch_bounds__(256) k_raht_dequantize(const int16_t* __restrict__ tokens, const int32_t* __restrict__ prefix,
                                                         const uint16_t* __restrict__ esc, int64_t n_esc, int64_t coded, int64_t gaps, int frames,
                                                         const uint64_t* __restrict__ keys, const int32_t* __restrict__ lo,
                                                         const int32_t* __restrict__ hi, const int32_t* __restrict__ order, RahtSteps q,
                                                         i3* __restrict__ Hhat) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= coded) return;
    const int32_t g = order[p];
    const int f = frame_of_gap(keys, frames, gaps, g, lo);
    if (f < 0) return;
    const int64_t w1 = g - lo[g] + 1, w2 = hi[g] - g;
    int32_t z[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        int32_t t = tokens[3 * p + c];
        t = t < 0 ? 0 : (t > RAHT_ESCAPE ? RAHT_ESCAPE : t);
        if (t == RAHT_ESCAPE) { const int64_t e = prefix[3 * p + c]; t += e < n_esc ? (esc[e] & 1023) : 0; }
        z[c] = t;
    }
    int q_luma, q_chroma;
    steps_at(q, frames, f, q_luma, q_chroma);
    const int64_t dl = delta16(q_luma, w1, w2), dc = delta16(q_chroma, w1, w2);
    Hhat[g] = i3{dequant(z[0], dl), dequant(z[1], dc), dequant(z[2], dc)};
}

static size_t dequantize_workspace_bytes(int64_t n, int frames) {
    const size_t t = tokens_of(n, frames);
    return align256(t) + align256(t * 4) + align256(pcgc_scan_workspace_bytes((int64_t)t));
}
// per_frame [16] (dev, null for a single frame) and total [1] (dev): the tokens equal to 63; the caller refuses a stream whose escape lists
// have other lengths
static int raht_dequantize(const char* who, const int16_t* tokens, const uint16_t* escapes, int64_t n_escapes, int64_t n, int frames,
                           const uint64_t* keys, const int32_t* lo, const int32_t* hi, const int32_t* order, const RahtSteps& q, int32_t* Hhat,
                           int32_t* per_frame, int32_t* total, void* workspace, size_t workspace_bytes, void* stream) {
    RAHT_REQUIRE(who, n_escapes >= 0 && total && workspace, "bad argument");
    RAHT_REQUIRE(who, workspace_bytes >= dequantize_workspace_bytes(n, frames), "workspace too small");
    hipError_t e = per_frame ? hipMemsetAsync(per_frame, 0, RAHT_MAX_FRAMES * sizeof(int32_t), S(stream)) : hipSuccess;
    if (e == hipSuccess && n == frames) e = hipMemsetAsync(total, 0, sizeof(int32_t), S(stream));      // (else pcgc_mask_scan writes it)
    RAHT_CHECK_HIP(who, e);
    if (n == frames) return 0;
    RAHT_REQUIRE(who, tokens && (frames == 1 || keys) && lo && hi && order && Hhat && (n_escapes == 0 || escapes), "null argument");
    const int64_t coded = n - frames, t = 3 * coded;
    char* ws = (char*)workspace;
    uint8_t* escmask = (uint8_t*)ws; ws += align256((size_t)t);
    int32_t* prefix = (int32_t*)ws; ws += align256((size_t)t * 4);
    hipLaunchKernelGGL(k_raht_escmask, dim3(grid_for(t, 256)), dim3(256), 0, S(stream), tokens, t, order, keys, lo, n - 1, frames, escmask, per_frame);
    PCGC_CHECK_LAUNCH(who + 5);
    if (pcgc_mask_scan(escmask, t, prefix, total, ws, pcgc_scan_workspace_bytes(t), stream) != 0) return -1;
    hipLaunchKernelGGL(k_raht_dequantize, dim3(grid_for(coded, 256)), dim3(256), 0, S(stream), tokens, (const int32_t*)prefix, escapes, n_escapes, coded,
                       n - 1, frames, keys, lo, hi, order, q, (i3*)Hhat);
    PCGC_CHECK_LAUNCH(who + 5);
    return 0;
}
extern "C" size_t pcgc_raht_dequantize_workspace_bytes(int64_t n) { return dequantize_workspace_bytes(n, 1); }
extern "C" int pcgc_raht_dequantize(const int16_t* tokens, const uint16_t* escapes, int64_t n_escapes, int64_t n, const int32_t* lo, const int32_t* hi,
                                    const int32_t* order, int q_luma, int q_chroma, int32_t* Hhat, int32_t* n_escape_tokens, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    PCGC_REQUIRE(n >= 1 && n <= RAHT_MAX_POINTS, "1 to 2^24 points");
    RahtSteps q;
    PCGC_REQUIRE(steps_of(&q_luma, &q_chroma, 1, q), "quantiser 0 .. 255");
    return raht_dequantize(__func__, tokens, escapes, n_escapes, n, 1, nullptr, lo, hi, order, q, Hhat, nullptr, n_escape_tokens, workspace,
                           workspace_bytes, stream);
}
// n_escape_tokens [17] (dev): the tokens that are 63 per frame, then [16] of all frames
extern "C" int64_t pcgc_raht_dequantize_batch_workspace_bytes(int64_t n, int frames) { return (int64_t)dequantize_workspace_bytes(n, frames); }
extern "C" int pcgc_raht_dequantize_batch(const int16_t* tokens, const uint16_t* escapes, int64_t n_escapes, int64_t n, int frames,
                                          const uint64_t* keys, const int32_t* lo, const int32_t* hi, const int32_t* order, const int32_t* q_luma,
                                          const int32_t* q_chroma, int32_t* Hhat, int32_t* n_escape_tokens, void* workspace,
                                          size_t workspace_bytes, void* stream) {
    PCGC_REQUIRE(n >= 1 && n <= RAHT_MAX_POINTS, "1 to 2^24 points");
    PCGC_REQUIRE(frames >= 1 && frames <= RAHT_MAX_FRAMES && frames <= n, "1 to 16 frames of at least one point");
    PCGC_REQUIRE(q_luma && q_chroma && n_escape_tokens, "bad argument");
    RahtSteps q;
    PCGC_REQUIRE(steps_of(q_luma, q_chroma, frames, q), "quantiser 0 .. 255");
    return raht_dequantize(__func__, tokens, escapes, n_escapes, n, frames, keys, lo, hi, order, q, Hhat, n_escape_tokens,
                           n_escape_tokens + RAHT_MAX_FRAMES, workspace, workspace_bytes, stream);
}

