// Cleaning a voxelised cloud (the definition is tests/clean_reference.py): radius counts for the density filter, connected
// components over the k3 map for the fragment filter, the selection of what stays.  The reference has no such stage: it assumes clouds
// that were cleaned elsewhere.  Integers only; every output is a function of the voxel set and the row order.
//
// Stage 1 (pcgc_clean_neighbours) reads the D2 index of the cloud (metric.hip) the way the normals' moment pass does (normals.hip): one
// thread per sorted row probes the (2 C + 1)^3 cells around its own and adds the popcounts of occupancy & ball mask; the voxel itself is
// one of those bits, so the count of OTHER voxels is the sum less one.  No atomics but the count of repeated rows.
//
// Stage 2 (pcgc_components) labels the rows of a k3 map [27][n]: parent[i] <= i is a forest over the rows; a round (one launch) takes
// every edge {i, j} of the 13 forward offsets once, lowers parent[i], parent[j] and parent[max(parent[i], parent[j])] to the smaller of the
// two parents (hooking), then follows the row's chain for at most CC_WALK links and lowers parent[i] to where it got (pointer jumping).
// All writes are atomicMin on int32, so parent only ever decreases, and every value written for a row is a row of its own component.
//
// Termination.  No launch waits on another workgroup and every device loop has a fixed trip count (13 offsets, CC_WALK links).  The host
// launches rounds and reads a change counter per round (a round adds to its counter only when an atomicMin lowered a value) after every
// CC_CHECK_EVERY rounds.  A round that changed nothing ran on a constant array: every edge has equal parents and every parent[i] is a root,
// so every row of a component holds the same root r, r is a row of the component with parent[r] = r, and the smallest row m of the
// component has parent[m] <= m inside the component, that is parent[m] = m = r: the labels are final.  Bound: let m be the smallest row of
// a component.  By induction every row at most t edges from m has parent = m after round t: such a row j has a neighbour i with parent[i]
// = m when round t starts, m is the floor of every value of the component so parent[i] is m whenever it is read, and the thread that owns
// edge {i, j} lowers parent[j] to it.  A component of k rows has no row farther than k - 1 edges from m, so after n - 1 rounds nothing can
// change and round n reads zero: at most n rounds (CC cap: n + 1).  When the cap is reached the entry returns an error; it never loops on.
// The hooking and jumping make it a few rounds in practice (a folded path of 4 097 rows in reversed order: DESIGN.md 8p).
#include <cstring>
#include "pcgc_common.h"
#include <rocprim/rocprim.hpp>

#define CLEAN_MAX_ROWS (1ll << 24)
#define CLEAN_MAX_R2 64
#define CC_WALK 8
#define CC_CHECK_EVERY 4

// ---- stage 1 -------------------------------------------------------------------------------------------------------------------------
static inline int clean_reach_cells(int r2) { int r = 0; while ((r + 1) * (r + 1) <= r2) ++r; return (r + 3) / 4; }

__global__ void __launch_bounds__(256) k_clean_neighbours(const int4* __restrict__ qs, const int32_t* __restrict__ perm,
                                                          const int32_t* __restrict__ runlen, int64_t n, const uint64_t* __restrict__ ckeys,
                                                          const int32_t* __restrict__ cvals, uint64_t cmask,
                                                          const unsigned long long* __restrict__ masks,
                                                          const unsigned long long* __restrict__ ball, int C, int32_t min_neighbours,
                                                          int32_t* __restrict__ neighbours, uint8_t* __restrict__ keep,
                                                          int32_t* __restrict__ repeated) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (runlen[i] == 0) atomicAdd(repeated, 1);                      // (a run of r equal rows: its r - 1 later rows have runlen 0)
    const int4 c = qs[i];
    const int X = c.y & ~3, Y = c.z & ~3, Z = c.w & ~3;
    const int pos = (c.y & 3) | ((c.z & 3) << 2) | ((c.w & 3) << 4);
    int k = 0, t = 0;
    for (int oz = -C; oz <= C; ++oz)
        for (int oy = -C; oy <= C; ++oy)
            for (int ox = -C; ox <= C; ++ox, ++t) {
                // (a cell at a negative or too large coordinate is out of the key's range: hash_lookup misses, nothing wraps)
                const int32_t row = hash_lookup(ckeys, cvals, cmask, c.x, X + 4 * ox, Y + 4 * oy, Z + 4 * oz);
                if (row >= 0) k += __builtin_popcountll(masks[row] & ball[(int64_t)t * 64 + pos]);
            }
    const int32_t row = perm[i];
    neighbours[row] = k - 1;
    keep[row] = k - 1 >= min_neighbours ? 1 : 0;
}

extern "C" int pcgc_clean_neighbours(const int32_t* qs, const int32_t* perm, int64_t n, const uint64_t* cell_keys, const int32_t* cell_vals,
                                     int64_t cell_cap, const uint64_t* masks, const int32_t* runlen, const uint64_t* ball, int32_t r2,
                                     int32_t min_neighbours, int32_t* neighbours, uint8_t* keep, int32_t* repeated, void* stream) {
    PCGC_REQUIRE(r2 >= 1 && r2 <= CLEAN_MAX_R2, "r2 outside 1 .. 64");
    PCGC_REQUIRE(min_neighbours >= 0, "min_neighbours is negative");
    PCGC_REQUIRE(n >= 0 && n <= CLEAN_MAX_ROWS, "row count outside 0 .. 2^24");
    PCGC_REQUIRE(cell_cap > 0 && (cell_cap & (cell_cap - 1)) == 0, "bad hash capacity");
    PCGC_REQUIRE(qs && perm && cell_keys && cell_vals && masks && runlen && ball && neighbours && keep && repeated, "null argument");
    hipError_t e = hipMemsetAsync(repeated, 0, sizeof(int32_t), S(stream));
    if (e != hipSuccess) { pcgc_set_error("clean_neighbours: %s", hipGetErrorString(e)); return -1; }
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_clean_neighbours, dim3(grid_for(n, 256)), dim3(256), 0, S(stream), (const int4*)qs, perm, runlen, n, cell_keys,
                       cell_vals, (uint64_t)(cell_cap - 1), (const unsigned long long*)masks, (const unsigned long long*)ball,
                       clean_reach_cells(r2), min_neighbours, neighbours, keep, repeated);
    PCGC_CHECK_LAUNCH("clean_neighbours");
    return 0;
}

// ---- stage 2: components ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_cc_init(int64_t n, int32_t* __restrict__ parent) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) parent[i] = (int32_t)i;
}

// parent is read while other workgroups lower it: relaxed atomic loads at device scope (vector loads that pass the CU's own cache)
__device__ static inline int32_t cc_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// atomicMin that reports whether it lowered the value.  A value that is low enough already is left alone (values only fall, so a read
// that is not above v settles it): most rows of a large component aim at the same few words, and the atomics on one word are served in turn
__device__ static inline int cc_lower(int32_t* p, int32_t v) {
    if (cc_load(p) <= v) return 0;
    return atomicMin(p, v) > v ? 1 : 0;
}

__global__ void __launch_bounds__(256) k_cc_round(const int32_t* __restrict__ nbr, int64_t n, int32_t* parent, int32_t* changes) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int changed = 0;
    if (i < n) {
#pragma unroll
        for (int k = 14; k < 27; ++k) {                               // the 13 offsets after the centre: every edge is met from one end
            const int32_t j = nbr[(int64_t)k * n + i];
            if ((uint32_t)j >= (uint32_t)n) continue;                 // (-1 = absent; an entry that is no row is never followed)
            const int32_t a = cc_load(parent + i), b = cc_load(parent + j);
            if (a == b) continue;
            const int32_t lo = a < b ? a : b, hi = a < b ? b : a;
            changed |= cc_lower(parent + i, lo) | cc_lower(parent + j, lo) | cc_lower(parent + hi, lo);
        }
        int32_t r = cc_load(parent + i);
#pragma unroll 1
        for (int s = 0; s < CC_WALK; ++s) {                           // parent[x] <= x: the chain descends and stays inside [0, n)
            const int32_t p = cc_load(parent + r);
            if (p == r) break;
            r = p;
        }
        changed |= cc_lower(parent + i, r);
    }
    if (__ballot(changed) && (threadIdx.x & 63) == 0) atomicAdd(changes, 1);
}

// the histogram of the final labels, and the number of roots.  The lanes of a wave that hold one label add it once (neighbouring rows
// mostly share their component, and a million atomics on one word are served in turn): at most 64 turns, one per distinct label
__global__ void __launch_bounds__(256) k_cc_histogram(const int32_t* __restrict__ labels, int64_t n, int32_t* __restrict__ hist,
                                                      int32_t* __restrict__ n_roots) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int32_t l = i < n ? labels[i] : -1;
    const bool valid = (uint32_t)l < (uint32_t)n;                     // (always, for i < n: parent[i] is a row; no index is followed unchecked)
    const unsigned long long roots = __ballot(valid && l == (int32_t)i);
    if (roots && lane == 0) atomicAdd(n_roots, __builtin_popcountll(roots));
    unsigned long long left = __ballot(valid);
#pragma unroll 1
    for (int turn = 0; turn < 64 && left; ++turn) {
        const int leader = __ffsll((long long)left) - 1;
        const int32_t l0 = __shfl(l, leader);
        const unsigned long long same = __ballot(valid && l == l0);
        if (lane == leader) atomicAdd(hist + l0, __builtin_popcountll(same));
        left &= ~same;
    }
}

__global__ void __launch_bounds__(256) k_cc_sizes(const int32_t* __restrict__ labels, const int32_t* __restrict__ hist, int64_t n,
                                                  int32_t* __restrict__ sizes) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) sizes[i] = (uint32_t)labels[i] < (uint32_t)n ? hist[labels[i]] : 0;
}

// workspace: int32 [16] counters (changes of CC_CHECK_EVERY rounds | roots) | int32 [n] histogram
#define CC_WS_HEAD 64
#define CC_ROOTS (CC_CHECK_EVERY + 0)
extern "C" int64_t pcgc_components_workspace_bytes(int64_t n) { return CC_WS_HEAD + (int64_t)(n < 1 ? 1 : n) * 4; }

extern "C" int pcgc_components(const int32_t* nbr, int64_t n, int32_t* labels, int32_t* sizes, int64_t* n_components, int32_t* rounds,
                               void* workspace, size_t workspace_bytes, void* stream) {
    PCGC_REQUIRE(n >= 0 && n <= CLEAN_MAX_ROWS, "row count outside 0 .. 2^24");
    PCGC_REQUIRE(workspace_bytes >= (size_t)pcgc_components_workspace_bytes(n), "workspace too small");
    PCGC_REQUIRE(nbr && labels && sizes && n_components && rounds && workspace, "null argument");
    *n_components = 0; *rounds = 0;
    if (n == 0) return 0;
    static thread_local int32_t* host = nullptr;
    if (!host && hipHostMalloc((void**)&host, CC_WS_HEAD, hipHostMallocDefault) != hipSuccess) {
        host = nullptr; pcgc_set_error("components: cannot allocate pinned memory"); return -1;
    }
    hipStream_t s = S(stream);
    int32_t* counters = (int32_t*)workspace;
    int32_t* hist = (int32_t*)((char*)workspace + CC_WS_HEAD);
    hipError_t e = hipMemsetAsync(workspace, 0, (size_t)pcgc_components_workspace_bytes(n), s);
    if (e != hipSuccess) { pcgc_set_error("components: %s", hipGetErrorString(e)); return -1; }
    hipLaunchKernelGGL(k_cc_init, dim3(grid_for(n, 256)), dim3(256), 0, s, n, labels);
    PCGC_CHECK_LAUNCH("components_init");
    const int64_t cap = n + 1;                                        // the bound of the argument at the head of this file
    int64_t done = 0;
    bool settled = false;
    while (!settled && done < cap) {
        const int batch = (int)(cap - done < CC_CHECK_EVERY ? cap - done : CC_CHECK_EVERY);
        if (done) {
            e = hipMemsetAsync(counters, 0, CC_CHECK_EVERY * sizeof(int32_t), s);
            if (e != hipSuccess) { pcgc_set_error("components: %s", hipGetErrorString(e)); return -1; }
        }
        for (int r = 0; r < batch; ++r) {
            hipLaunchKernelGGL(k_cc_round, dim3(grid_for(n, 256)), dim3(256), 0, s, nbr, n, labels, counters + r);
            PCGC_CHECK_LAUNCH("components_round");
        }
        e = hipMemcpyAsync(host, counters, CC_WS_HEAD, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) { pcgc_set_error("components: %s", hipGetErrorString(e)); return -1; }
        for (int r = 0; r < batch && !settled; ++r) {                 // the first round that changed nothing is the last one needed
            ++done;
            settled = host[r] == 0;
        }
    }
    *rounds = (int32_t)done;
    if (!settled) { pcgc_set_error("components: labels still changing after %lld rounds (the cap for %lld rows)", (long long)done, (long long)n); return -3; }
    hipLaunchKernelGGL(k_cc_histogram, dim3(grid_for(n, 256)), dim3(256), 0, s, labels, n, hist, counters + CC_ROOTS);
    PCGC_CHECK_LAUNCH("components_histogram");
    hipLaunchKernelGGL(k_cc_sizes, dim3(grid_for(n, 256)), dim3(256), 0, s, labels, hist, n, sizes);
    PCGC_CHECK_LAUNCH("components_sizes");
    e = hipMemcpyAsync(host, counters, CC_WS_HEAD, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) { pcgc_set_error("components: %s", hipGetErrorString(e)); return -1; }
    *n_components = host[CC_ROOTS];
    return 0;
}

// ---- labels of the survivors' compacted rows back on the input rows ---------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_clean_expand(const uint8_t* __restrict__ keep1, const int32_t* __restrict__ prefix,
                                                      const int32_t* __restrict__ orig, const int32_t* __restrict__ labels_c,
                                                      const int32_t* __restrict__ sizes_c, int64_t n, int64_t n_c,
                                                      int32_t* __restrict__ labels, int32_t* __restrict__ sizes) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int32_t l = -1, z = 0;
    if (keep1[i]) {
        const int32_t c = prefix[i];
        if ((uint32_t)c < (uint32_t)n_c) {
            const int32_t lc = labels_c[c];
            if ((uint32_t)lc < (uint32_t)n_c) { l = orig[lc]; z = sizes_c[c]; }       // (compaction keeps the order: the smallest compact row
        }                                                                             //  of a component is its smallest input row)
    }
    labels[i] = l; sizes[i] = z;
}

extern "C" int pcgc_clean_expand(const uint8_t* keep1, const int32_t* prefix, const int32_t* orig, const int32_t* labels_c,
                                 const int32_t* sizes_c, int64_t n, int64_t n_c, int32_t* labels, int32_t* sizes, void* stream) {
    PCGC_REQUIRE(n >= 0 && n <= CLEAN_MAX_ROWS && n_c >= 0 && n_c <= n, "row counts");
    PCGC_REQUIRE(keep1 && prefix && labels && sizes && (n_c == 0 || (orig && labels_c && sizes_c)), "null argument");
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_clean_expand, dim3(grid_for(n, 256)), dim3(256), 0, S(stream), keep1, prefix, orig, labels_c, sizes_c, n, n_c, labels,
                       sizes);
    PCGC_CHECK_LAUNCH("clean_expand");
    return 0;
}

// ---- what stays -------------------------------------------------------------------------------------------------------------------------
// a root's key: batch (4 bits) | 2^24 - size (25 bits) | label (24 bits): ascending = per batch item the largest component first, ties to
// the smaller label.  Every other row: all ones (sorted behind every root).
#define SEL_BATCH_SHIFT 49
__global__ void __launch_bounds__(256) k_sel_keys(const int4* __restrict__ coords, const int32_t* __restrict__ labels,
                                                  const int32_t* __restrict__ sizes, int64_t n, uint64_t* __restrict__ keys) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t key = ~0ull;
    if (labels[i] == (int32_t)i)
        key = ((uint64_t)(coords[i].x & 15) << SEL_BATCH_SHIFT) | ((uint64_t)((1 << 24) - sizes[i]) << 24) | (uint64_t)i;
    keys[i] = key;
}

// the rank of a root among the roots of its batch item = its place less the place of the item's first key (a binary search: at most 25 steps)
__global__ void __launch_bounds__(256) k_sel_rank(const uint64_t* __restrict__ sorted, int64_t n, int64_t keep_largest,
                                                  uint8_t* __restrict__ root_keep) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const uint64_t key = sorted[p];
    if (key == ~0ull) return;
    const uint64_t first_key = (key >> SEL_BATCH_SHIFT) << SEL_BATCH_SHIFT;
    int64_t lo = 0, hi = p;                                           // the first place whose key is not below first_key lies in [0, p]
#pragma unroll 1
    for (int step = 0; step < 25 && lo < hi; ++step) {
        const int64_t mid = (lo + hi) >> 1;
        if (sorted[mid] < first_key) lo = mid + 1; else hi = mid;
    }
    root_keep[key & 0xFFFFFF] = (p - lo) < keep_largest ? 1 : 0;
}

__global__ void __launch_bounds__(256) k_sel_keep(const int32_t* __restrict__ labels, const int32_t* __restrict__ sizes, int64_t n,
                                                  int32_t min_component, const uint8_t* __restrict__ root_keep, uint8_t* __restrict__ keep) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t l = labels[i];
    bool k = (uint32_t)l < (uint32_t)n && sizes[i] >= min_component;
    if (k && root_keep) k = root_keep[l] != 0;
    keep[i] = k ? 1 : 0;
}

static size_t sel_sort_temp(int64_t n) {
    size_t tmp = 0;
    (void)rocprim::radix_sort_keys((void*)nullptr, tmp, (uint64_t*)nullptr, (uint64_t*)nullptr, (size_t)n, 0, 64, (hipStream_t)0);
    return tmp;
}
static inline size_t a256(size_t v) { return (v + 255) & ~(size_t)255; }

// workspace: uint64 [n] keys | uint64 [n] sorted keys | uint8 [n] root_keep | rocPRIM's scratch
extern "C" int64_t pcgc_clean_select_workspace_bytes(int64_t n) {
    const int64_t m = n < 1 ? 1 : n;
    return (int64_t)(2 * a256((size_t)m * 8) + a256((size_t)m) + a256(sel_sort_temp(m)));
}

extern "C" int pcgc_clean_select(const int32_t* coords, const int32_t* labels, const int32_t* sizes, int64_t n, int32_t min_component,
                                 int64_t keep_largest, uint8_t* keep, void* workspace, size_t workspace_bytes, void* stream) {
    PCGC_REQUIRE(n >= 0 && n <= CLEAN_MAX_ROWS, "row count outside 0 .. 2^24");
    PCGC_REQUIRE(min_component >= 1 && keep_largest >= 0, "min_component below 1 or keep_largest below 0");
    PCGC_REQUIRE(workspace_bytes >= (size_t)pcgc_clean_select_workspace_bytes(n), "workspace too small");
    PCGC_REQUIRE(coords && labels && sizes && keep && workspace, "null argument");
    PCGC_REQUIRE(((uintptr_t)coords & 15) == 0 && ((uintptr_t)workspace & 7) == 0, "misaligned argument");
    if (n == 0) return 0;
    hipStream_t s = S(stream);
    uint8_t* root_keep = nullptr;
    if (keep_largest > 0) {
        uint64_t* keys = (uint64_t*)workspace;
        uint64_t* sorted = (uint64_t*)((char*)workspace + a256((size_t)n * 8));
        root_keep = (uint8_t*)workspace + 2 * a256((size_t)n * 8);
        void* tmp_at = (char*)root_keep + a256((size_t)n);
        size_t tmp = sel_sort_temp(n);
        hipLaunchKernelGGL(k_sel_keys, dim3(grid_for(n, 256)), dim3(256), 0, s, (const int4*)coords, labels, sizes, n, keys);
        PCGC_CHECK_LAUNCH("clean_select_keys");
        hipError_t e = rocprim::radix_sort_keys(tmp_at, tmp, keys, sorted, (size_t)n, 0, 64, s);
        if (e != hipSuccess) { pcgc_set_error("clean_select: sort: %s", hipGetErrorString(e)); return -1; }
        hipLaunchKernelGGL(k_sel_rank, dim3(grid_for(n, 256)), dim3(256), 0, s, sorted, n, keep_largest, root_keep);
        PCGC_CHECK_LAUNCH("clean_select_rank");
    }
    hipLaunchKernelGGL(k_sel_keep, dim3(grid_for(n, 256)), dim3(256), 0, s, labels, sizes, n, min_component, root_keep, keep);
    PCGC_CHECK_LAUNCH("clean_select_keep");
    return 0;
}

// colours [n,3] of the rows that stay, in input order (pcgc_compact_coords for three bytes a row)
__global__ void __launch_bounds__(256) k_clean_compact_colours(const uint8_t* __restrict__ in, const uint8_t* __restrict__ mask,
                                                               const int32_t* __restrict__ prefix, int64_t n, uint8_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !mask[i]) return;
    const int64_t o = prefix[i];
    out[3 * o] = in[3 * i]; out[3 * o + 1] = in[3 * i + 1]; out[3 * o + 2] = in[3 * i + 2];
}

extern "C" int pcgc_clean_compact_colours(const uint8_t* colours, const uint8_t* mask, const int32_t* prefix, int64_t n, uint8_t* out,
                                          void* stream) {
    PCGC_REQUIRE(n >= 0 && n <= CLEAN_MAX_ROWS, "row count outside 0 .. 2^24");
    PCGC_REQUIRE(colours && mask && prefix && out, "null argument");
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_clean_compact_colours, dim3(grid_for(n, 256)), dim3(256), 0, S(stream), colours, mask, prefix, n, out);
    PCGC_CHECK_LAUNCH("clean_compact_colours");
    return 0;
}
