// Partition of a large cloud into kd-tree blocks of at most max_num rows (the definition is tests/partition_reference.py).
// Integers only; every output is a function of the input rows and their order and EQUAL to the definition's.
//
// cell = coord >> log2(align).  A round (launched by the host) works on the blocks with more than max_num rows that are not known to lie in
// one cell:
//   bounds   min and max cell per axis and block: int32 atomicMin / atomicMax; the rows of a wave that share a block reduce in the wave first
//   plan     one thread per block: the axis of the largest extent (ties to x, then y), cmin, cmax and the bin width w = ceil((extent + 1) /
//            1024); a block of extent 0 on every axis is marked and never looked at again
//   coarse   per (block, bin) the row count and, where w > 1, the largest occupied cell of the bin
//   cut 1    one workgroup per block scans the 1 024 counts to the bin J in which the cumulative count reaches n / 2, and finds the last
//            occupied cell before bin J
//   fine     the counts of the at most 128 cells of bin J (w > 1; with w = 1 the bin is the cell and cut 1 has its count)
//   cut 2    one thread per block walks the cells of bin J to the crossing cell c* (the first cell with 2 C(c*) >= n, C = rows at or below),
//            and picks the plane.  |2 L(k) - n| over the monotone L is smallest at one of the two planes around the crossing, and the tie
//            rule takes the first plane of a run of equal L, which is "an occupied cell + 1": the candidates are c* + 1 (if c* < cmax) and
//            p + 1, p = the occupied cell before c* (if there is one), with L = C(c*) and C(c*) - count(c*); a tie goes to p + 1.
//            Then an exclusive scan of the split flags renumbers the blocks (children take the parent's place: the in-order of the tree).
//   assign   every row of a split block takes its side and every row its block's new number
// and the host reads one record (blocks split, blocks now, blocks still too large).
//
// Termination.  No workgroup waits on another: no tickets, flags or spins.  Every device loop has a fixed trip count (4 bins a thread, 8 or
// 10 scan steps, 128 cells, 4 aggregation turns, 6 shuffle steps).  A round that is followed by another has split at least one block and
// both children of a split are non-empty, so the block count grows every round and cannot pass 1 024: at most 1 023 splitting rounds.  The
// host stops at the first record that names no split, no block left to look at, or a block count above 1 024 (the refusal; the caller's
// outputs have not been touched: the rounds work on a copy of block_of in the workspace).
//
// Workspace: O(n) (block_of, sort keys, row numbers, rocPRIM's scratch) + 1 024 x (1 024 counts + 1 024 cells + 128 counts + 20 words): it
// does not depend on any block's extent.
#include <chrono>
#include <cstring>
#include "pcgc_common.h"
#include <rocprim/rocprim.hpp>

#define PART_MAX_BLOCKS 1024
#define PART_BINS 1024
#define PART_FINE 128
#define PART_MAX_ROWS (1ll << 27)
#define PART_COORD_BITS 20
#define PART_TURNS 4
#define PART_INT_MAX 0x7FFFFFFF

// per-block words of the workspace (each int32 [1024])
enum { PB_CNT_A, PB_CNT_B, PB_STUCK_A, PB_STUCK_B, PB_MIN, PB_MIN_Y, PB_MIN_Z, PB_MAX, PB_MAX_Y, PB_MAX_Z, PB_ACT, PB_AXIS, PB_CMIN, PB_CMAX, PB_W,
       PB_J, PB_CUMX, PB_PREV, PB_K, PB_NEWIDX, PB_WORDS };
// the record a round leaves for the host (int32 [16])
enum { PR_SPLIT, PR_BLOCKS, PR_OPEN, PR_ERROR, PR_OVERSIZE, PR_BAD_RANGE, PR_BAD_BATCH };

static inline size_t p256(size_t v) { return (v + 255) & ~(size_t)255; }
#define PART_HEAD 256
static inline size_t part_blocks_bytes() { return (size_t)PB_WORDS * PART_MAX_BLOCKS * 4; }
static inline size_t part_hist_bytes() { return (size_t)PART_MAX_BLOCKS * (2 * PART_BINS + PART_FINE) * 4; }
static size_t part_sort_temp(int64_t n) {
    size_t tmp = 0;
    (void)rocprim::radix_sort_pairs((void*)nullptr, tmp, (uint32_t*)nullptr, (uint32_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr, (size_t)n,
                                    0, 10, (hipStream_t)0);
    return tmp;
}

// workspace: record | per-block words | coarse counts, coarse cells, fine counts | block_of [n] | sorted keys [n] | row numbers [n] | scratch
extern "C" int64_t pcgc_partition_workspace_bytes(int64_t n) {
    const int64_t m = n < 1 ? 1 : (n > PART_MAX_ROWS ? PART_MAX_ROWS : n);
    return (int64_t)(PART_HEAD + p256(part_blocks_bytes()) + p256(part_hist_bytes()) + 3 * p256((size_t)m * 4) + p256(part_sort_temp(m)));
}

__device__ static inline int part_cell(const int32_t* __restrict__ coords, int64_t i, int cols, int axis, int shift) {
    return coords[i * cols + (cols - 3) + axis] >> shift;
}

// ---- the preconditions: rows with a coordinate outside [0, 2^20) and rows with a batch index other than 0 ----------------------------------
__global__ void __launch_bounds__(256) k_part_check(const int32_t* __restrict__ coords, int64_t n, int cols, int32_t* __restrict__ rec) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool range = false, batch = false;
    if (i < n) {
        const int32_t* r = coords + i * cols + (cols - 3);
        range = ((uint32_t)r[0] | (uint32_t)r[1] | (uint32_t)r[2]) >> PART_COORD_BITS;
        batch = cols == 4 && coords[i * cols] != 0;
    }
    const unsigned long long a = __ballot(range), b = __ballot(batch);
    if ((threadIdx.x & 63) == 0) {
        if (a) atomicAdd(rec + PR_BAD_RANGE, __builtin_popcountll(a));
        if (b) atomicAdd(rec + PR_BAD_BATCH, __builtin_popcountll(b));
    }
}

__global__ void __launch_bounds__(256) k_part_fill(int32_t* __restrict__ p, int64_t n, int32_t base, int32_t step) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = base + step * (int32_t)i;
}

// ---- bounds: lo[3] / hi[3] of block b at lo + b * lo_stride + axis * axis_stride (the rounds' per-block words, or the rows of the table) ----
// The lanes of a wave that hold one block reduce their six values over the wave and their first lane issues six atomics, for at most
// PART_TURNS distinct blocks a wave (raster input: one block, or the few that meet in 64 neighbouring rows); what is left issues its own.
// A bound that is good enough already is left alone: bounds only widen, so a read that is not above (below) the value settles it, and the
// atomics of a million rows on the six words of one block would be served in turn.
__device__ static inline int32_t part_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ static inline void part_lower(int32_t* p, int32_t v) { if (part_load(p) > v) atomicMin(p, v); }
__device__ static inline void part_raise(int32_t* p, int32_t v) { if (part_load(p) < v) atomicMax(p, v); }
__device__ static inline void part_bounds(bool valid, int b, int vx, int vy, int vz, int32_t* lo, int32_t* hi, int b_stride, int axis_stride) {
    unsigned long long left = __ballot(valid);
    const int lane = threadIdx.x & 63;
#pragma unroll 1
    for (int turn = 0; turn < PART_TURNS && left; ++turn) {           // (`left` is the same in every lane: the whole wave leaves together)
        const int leader = __ffsll((long long)left) - 1;
        const int b0 = __shfl(b, leader);
        const bool mine = valid && b == b0;                           // (the lanes of earlier turns hold other blocks)
        int mn[3] = {mine ? vx : PART_INT_MAX, mine ? vy : PART_INT_MAX, mine ? vz : PART_INT_MAX};
        int mx[3] = {mine ? vx : -1, mine ? vy : -1, mine ? vz : -1};
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1)
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const int o = __shfl_xor(mn[a], s), q = __shfl_xor(mx[a], s);
                mn[a] = o < mn[a] ? o : mn[a];
                mx[a] = q > mx[a] ? q : mx[a];
            }
        if (lane == leader) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                part_lower(lo + (int64_t)b0 * b_stride + a * axis_stride, mn[a]);
                part_raise(hi + (int64_t)b0 * b_stride + a * axis_stride, mx[a]);
            }
        }
        left &= ~__ballot(mine);
    }
    if (valid && ((left >> lane) & 1)) {
        const int v[3] = {vx, vy, vz};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            part_lower(lo + (int64_t)b * b_stride + a * axis_stride, v[a]);
            part_raise(hi + (int64_t)b * b_stride + a * axis_stride, v[a]);
        }
    }
}

__global__ void __launch_bounds__(1024) k_part_round_init(int32_t* __restrict__ pb, int32_t* __restrict__ rec) {
    const int b = threadIdx.x;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        pb[(PB_MIN + a) * PART_MAX_BLOCKS + b] = PART_INT_MAX;
        pb[(PB_MAX + a) * PART_MAX_BLOCKS + b] = -1;
    }
    pb[PB_ACT * PART_MAX_BLOCKS + b] = 0;
    pb[PB_J * PART_MAX_BLOCKS + b] = -1;
    if (b < 4) rec[b] = 0;
}

// open[b]: block b has more than max_num rows and is not known to lie in one cell
__device__ static inline bool part_open(const int32_t* __restrict__ cnt, const int32_t* __restrict__ stuck, int b, int64_t max_num) {
    return (int64_t)cnt[b] > max_num && !stuck[b];
}

__global__ void __launch_bounds__(256) k_part_bounds(const int32_t* __restrict__ coords, int64_t n, int cols, int shift,
                                                     const int32_t* __restrict__ block_of, const int32_t* __restrict__ cnt,
                                                     const int32_t* __restrict__ stuck, int64_t max_num, int32_t* __restrict__ pb) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int b = 0, x = 0, y = 0, z = 0;
    bool valid = false;
    if (i < n) {
        b = block_of[i];
        if ((uint32_t)b < PART_MAX_BLOCKS && part_open(cnt, stuck, b, max_num)) {
            valid = true;
            x = part_cell(coords, i, cols, 0, shift); y = part_cell(coords, i, cols, 1, shift); z = part_cell(coords, i, cols, 2, shift);
        }
    }
    part_bounds(valid, b, x, y, z, pb + PB_MIN * PART_MAX_BLOCKS, pb + PB_MAX * PART_MAX_BLOCKS, 1, PART_MAX_BLOCKS);
}

__global__ void __launch_bounds__(1024) k_part_plan(int blocks, const int32_t* __restrict__ cnt, int32_t* __restrict__ stuck, int64_t max_num,
                                                    int32_t* __restrict__ pb) {
    const int b = threadIdx.x;
    if (b >= blocks || !part_open(cnt, stuck, b, max_num)) return;
    int axis = 0, best = -1, lo = 0, hi = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {                                       // (a later axis wins only with a LARGER extent: ties to x, then y)
        const int mn = pb[(PB_MIN + a) * PART_MAX_BLOCKS + b], mx = pb[(PB_MAX + a) * PART_MAX_BLOCKS + b];
        if (mx - mn > best) { best = mx - mn; axis = a; lo = mn; hi = mx; }
    }
    if (best <= 0) { stuck[b] = 1; return; }                            // all rows in one cell: the block stays as it is
    pb[PB_ACT * PART_MAX_BLOCKS + b] = 1;
    pb[PB_AXIS * PART_MAX_BLOCKS + b] = axis;
    pb[PB_CMIN * PART_MAX_BLOCKS + b] = lo;
    pb[PB_CMAX * PART_MAX_BLOCKS + b] = hi;
    pb[PB_W * PART_MAX_BLOCKS + b] = (best + 1 + PART_BINS - 1) / PART_BINS;
}

// ---- coarse pass ---------------------------------------------------------------------------------------------------------------------------
// The lanes of a wave that hold one (block, bin) add it once, for at most PART_TURNS distinct keys a wave (raster input: neighbouring rows
// share their bin); what is left adds itself.
__global__ void __launch_bounds__(256) k_part_coarse(const int32_t* __restrict__ coords, int64_t n, int cols, int shift,
                                                     const int32_t* __restrict__ block_of, const int32_t* __restrict__ pb,
                                                     int32_t* __restrict__ ccnt, int32_t* __restrict__ cmaxcell) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int key = -1, cell = 0, w = 1;
    if (i < n) {
        const int b = block_of[i];
        if ((uint32_t)b < PART_MAX_BLOCKS && pb[PB_ACT * PART_MAX_BLOCKS + b]) {
            w = pb[PB_W * PART_MAX_BLOCKS + b];
            cell = part_cell(coords, i, cols, pb[PB_AXIS * PART_MAX_BLOCKS + b], shift);
            const int bin = (cell - pb[PB_CMIN * PART_MAX_BLOCKS + b]) / w;
            if ((uint32_t)bin < PART_BINS) key = b * PART_BINS + bin;   // (always: cmin <= cell <= cmax and w covers the extent in 1 024 bins)
        }
    }
    if (key >= 0 && w > 1) part_raise(cmaxcell + key, cell);
    unsigned long long left = __ballot(key >= 0);
#pragma unroll 1
    for (int turn = 0; turn < PART_TURNS && left; ++turn) {
        const int leader = __ffsll((long long)left) - 1;
        const int k0 = __shfl(key, leader);
        const unsigned long long same = __ballot(key >= 0 && key == k0);
        if (lane == leader) atomicAdd(ccnt + k0, __builtin_popcountll(same));
        if (key == k0) key = -1;
        left &= ~same;
    }
    if (key >= 0) atomicAdd(ccnt + key, 1);
}

// ---- cut 1: the bin of the crossing ----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_part_cut1(const int32_t* __restrict__ cnt, int32_t* __restrict__ pb, const int32_t* __restrict__ ccnt,
                                                   const int32_t* __restrict__ cmaxcell, int32_t* __restrict__ fine) {
    const int b = blockIdx.x, t = threadIdx.x;
    if (!pb[PB_ACT * PART_MAX_BLOCKS + b]) return;                      // (the whole workgroup)
    __shared__ int sc[2][256];
    __shared__ int sJ, sPrev;
    const int n = cnt[b], w = pb[PB_W * PART_MAX_BLOCKS + b];
    int c[4], sum = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) { c[j] = ccnt[b * PART_BINS + 4 * t + j]; sum += c[j]; }
    if (t == 0) { sJ = -1; sPrev = -1; }
    sc[0][t] = sum;
    __syncthreads();
    int cur = 0;
#pragma unroll
    for (int s = 1; s < 256; s <<= 1) {                                 // inclusive scan of the 256 partial sums
        sc[cur ^ 1][t] = sc[cur][t] + (t >= s ? sc[cur][t - s] : 0);
        cur ^= 1;
        __syncthreads();
    }
    int run = sc[cur][t] - sum;
#pragma unroll
    for (int j = 0; j < 4; ++j) {                                       // exactly one bin has 2 * rows before < n <= 2 * rows up to and with it
        const int incl = run + c[j];
        if (2 * run < n && 2 * incl >= n) {
            sJ = 4 * t + j;
            pb[PB_J * PART_MAX_BLOCKS + b] = 4 * t + j;
            pb[PB_CUMX * PART_MAX_BLOCKS + b] = run;
            if (w == 1) fine[b * PART_FINE] = c[j];
        }
        run = incl;
    }
    __syncthreads();
    const int J = sJ;
    int mine = -1;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (c[j] > 0 && 4 * t + j < J) mine = 4 * t + j;
    if (mine >= 0) atomicMax(&sPrev, mine);
    __syncthreads();
    if (t == 0) {
        int prev = -1;                                                  // the last occupied cell before bin J, or -1
        if (sPrev >= 0) prev = w == 1 ? pb[PB_CMIN * PART_MAX_BLOCKS + b] + sPrev : cmaxcell[b * PART_BINS + sPrev];
        pb[PB_PREV * PART_MAX_BLOCKS + b] = prev;
    }
}

// ---- fine pass: the cells of bin J (w > 1) -----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_part_fine(const int32_t* __restrict__ coords, int64_t n, int cols, int shift,
                                                   const int32_t* __restrict__ block_of, const int32_t* __restrict__ pb, int32_t* __restrict__ fine) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int b = block_of[i];
    if ((uint32_t)b >= PART_MAX_BLOCKS || !pb[PB_ACT * PART_MAX_BLOCKS + b]) return;
    const int w = pb[PB_W * PART_MAX_BLOCKS + b], J = pb[PB_J * PART_MAX_BLOCKS + b];
    if (w <= 1 || J < 0) return;
    const int cell = part_cell(coords, i, cols, pb[PB_AXIS * PART_MAX_BLOCKS + b], shift);
    const int f = cell - (pb[PB_CMIN * PART_MAX_BLOCKS + b] + J * w);
    if ((uint32_t)f < (uint32_t)w && f < PART_FINE) atomicAdd(fine + b * PART_FINE + f, 1);
}

// ---- cut 2: the plane of every block, the new numbering and the new counts ---------------------------------------------------------------------
__global__ void __launch_bounds__(1024) k_part_cut2(int blocks, const int32_t* __restrict__ cnt, const int32_t* __restrict__ stuck,
                                                    int32_t* __restrict__ cnt_new, int32_t* __restrict__ stuck_new, int64_t max_num,
                                                    int32_t* __restrict__ pb, const int32_t* __restrict__ fine, int32_t* __restrict__ rec) {
    const int b = threadIdx.x;
    __shared__ int sc[2][1024];
    __shared__ int sOpen, sErr;
    if (b == 0) { sOpen = 0; sErr = 0; }
    __syncthreads();
    int split = 0, k = 0, L = 0, n = 0;
    const bool act = b < blocks && pb[PB_ACT * PART_MAX_BLOCKS + b];
    if (b < blocks) n = cnt[b];
    if (act) {
        const int w = pb[PB_W * PART_MAX_BLOCKS + b], J = pb[PB_J * PART_MAX_BLOCKS + b], cmax = pb[PB_CMAX * PART_MAX_BLOCKS + b];
        const int base = pb[PB_CMIN * PART_MAX_BLOCKS + b] + (J < 0 ? 0 : J) * w;
        int run = pb[PB_CUMX * PART_MAX_BLOCKS + b], p = pb[PB_PREV * PART_MAX_BLOCKS + b];
        int cstar = -1, upto = 0, at = 0;
        bool found = false;
#pragma unroll 1
        for (int f = 0; f < PART_FINE; ++f) {
            const int c = (J >= 0 && f < w) ? fine[b * PART_FINE + f] : 0;
            if (c > 0 && !found) {
                if (2 * (run + c) >= n) { found = true; cstar = base + f; upto = run + c; at = c; }
                else { run += c; p = base + f; }
            }
        }
        if (found) {
            const bool hi_ok = cstar < cmax, lo_ok = p >= 0;
            const int d_lo = n - 2 * (upto - at), d_hi = 2 * upto - n;
            if (lo_ok && (!hi_ok || d_lo <= d_hi)) { k = p + 1; L = upto - at; split = 1; }
            else if (hi_ok) { k = cstar + 1; L = upto; split = 1; }
        }
        if (!split || L <= 0 || L >= n) { split = 0; atomicAdd(&sErr, 1); }   // (never: the counts of a block add up to its rows)
    }
    sc[0][b] = split;
    __syncthreads();
    int cur = 0;
#pragma unroll
    for (int s = 1; s < 1024; s <<= 1) {
        sc[cur ^ 1][b] = sc[cur][b] + (b >= s ? sc[cur][b - s] : 0);
        cur ^= 1;
        __syncthreads();
    }
    const int before = sc[cur][b] - split, total = sc[cur][1023];
    const int blocks_new = blocks + total;
    const bool write = blocks_new <= PART_MAX_BLOCKS && sErr == 0;
    if (b < blocks) {
        const int nb = b + before;
        pb[PB_NEWIDX * PART_MAX_BLOCKS + b] = nb;
        pb[PB_K * PART_MAX_BLOCKS + b] = k;
        pb[PB_ACT * PART_MAX_BLOCKS + b] = split;                       // from here on: this block is split at k
        if (write) {
            if (split) {
                cnt_new[nb] = L; cnt_new[nb + 1] = n - L;
                stuck_new[nb] = 0; stuck_new[nb + 1] = 0;
                const int open = ((int64_t)L > max_num) + ((int64_t)(n - L) > max_num);
                if (open) atomicAdd(&sOpen, open);
            } else {
                cnt_new[nb] = n; stuck_new[nb] = stuck[b];
            }
        }
    }
    __syncthreads();
    if (b == 0) { rec[PR_SPLIT] = total; rec[PR_BLOCKS] = blocks_new; rec[PR_OPEN] = sOpen; rec[PR_ERROR] = sErr; }
}

__global__ void __launch_bounds__(256) k_part_assign(const int32_t* __restrict__ coords, int64_t n, int cols, int shift, int32_t* __restrict__ block_of,
                                                     const int32_t* __restrict__ pb, const int32_t* __restrict__ rec) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || rec[PR_ERROR] || rec[PR_BLOCKS] > PART_MAX_BLOCKS || rec[PR_SPLIT] == 0) return;
    const int b = block_of[i];
    if ((uint32_t)b >= PART_MAX_BLOCKS) return;
    int nb = pb[PB_NEWIDX * PART_MAX_BLOCKS + b];
    if (pb[PB_ACT * PART_MAX_BLOCKS + b])
        nb += part_cell(coords, i, cols, pb[PB_AXIS * PART_MAX_BLOCKS + b], shift) >= pb[PB_K * PART_MAX_BLOCKS + b] ? 1 : 0;
    block_of[i] = nb;
}

// ---- after the last round: the table -------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(1024) k_part_table(int blocks, const int32_t* __restrict__ cnt, int64_t max_num, int32_t* __restrict__ table,
                                                     int32_t* __restrict__ rec) {
    const int b = threadIdx.x;
    __shared__ int sc[2][1024];
    __shared__ int sOver;
    if (b == 0) sOver = 0;
    const int n = b < blocks ? cnt[b] : 0;
    sc[0][b] = n;
    __syncthreads();
    int cur = 0;
#pragma unroll
    for (int s = 1; s < 1024; s <<= 1) {
        sc[cur ^ 1][b] = sc[cur][b] + (b >= s ? sc[cur][b - s] : 0);
        cur ^= 1;
        __syncthreads();
    }
    if (b < blocks) {
        table[b * 8] = sc[cur][b] - n; table[b * 8 + 1] = n;
#pragma unroll
        for (int a = 0; a < 3; ++a) { table[b * 8 + 2 + a] = PART_INT_MAX; table[b * 8 + 5 + a] = -1; }
        if ((int64_t)n > max_num) atomicAdd(&sOver, 1);
    }
    __syncthreads();
    if (b == 0) rec[PR_OVERSIZE] = sOver;
}

__global__ void __launch_bounds__(256) k_part_boxes(const int32_t* __restrict__ coords, int64_t n, int cols, const int32_t* __restrict__ block_of,
                                                    int blocks, int32_t* __restrict__ table) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int b = 0, x = 0, y = 0, z = 0;
    bool valid = false;
    if (i < n) {
        b = block_of[i];
        if ((uint32_t)b < (uint32_t)blocks) {
            valid = true;
            x = part_cell(coords, i, cols, 0, 0); y = part_cell(coords, i, cols, 1, 0); z = part_cell(coords, i, cols, 2, 0);
        }
    }
    part_bounds(valid, b, x, y, z, table + 2, table + 5, 8, 1);
}

#define PART_SYNC_ERR(e, what) do { if ((e) != hipSuccess) { pcgc_set_error("partition: %s: %s", what, hipGetErrorString(e)); return -1; } } while (0)

extern "C" int pcgc_partition(const int32_t* coords, int64_t n, int32_t cols, int64_t max_num, int32_t align, int32_t* block_of, int32_t* perm,
                              int32_t* table, int64_t* info, double* phase_seconds, void* workspace, size_t workspace_bytes, void* stream) {
    PCGC_REQUIRE(n >= 0 && n <= PART_MAX_ROWS, "row count outside 0 .. 2^27");
    PCGC_REQUIRE(cols == 3 || cols == 4, "rows of 3 or 4 columns");
    PCGC_REQUIRE(max_num >= 1, "max_num below 1");
    PCGC_REQUIRE(align >= 8 && align <= 1024 && (align & (align - 1)) == 0, "align is no power of two in 8 .. 1024");
    PCGC_REQUIRE(workspace_bytes >= (size_t)pcgc_partition_workspace_bytes(n), "workspace too small");
    PCGC_REQUIRE(coords && block_of && perm && table && info && workspace, "null argument");
    PCGC_REQUIRE(((uintptr_t)workspace & 255) == 0, "misaligned workspace");
    for (int j = 0; j < PARTITION_INFO_WORDS; ++j) info[j] = 0;
    if (n == 0) return 0;
    // (64 pinned bytes a host thread, allocated on its first call and kept for the thread's life; every read of it is followed by a wait for
    //  `stream` before the entry goes on, so calls of one thread on several devices or streams take their turns with it)
    static thread_local int32_t* host = nullptr;
    if (!host && hipHostMalloc((void**)&host, 64, hipHostMallocDefault) != hipSuccess) {
        host = nullptr; pcgc_set_error("partition: cannot allocate pinned memory"); return -1;
    }
    hipStream_t s = S(stream);
    int shift = 0;
    while ((1 << shift) < align) ++shift;
    char* at = (char*)workspace;
    int32_t* rec = (int32_t*)at;                                        at += PART_HEAD;
    int32_t* pb = (int32_t*)at;                                         at += p256(part_blocks_bytes());
    int32_t* ccnt = (int32_t*)at;
    int32_t* cmaxcell = ccnt + (size_t)PART_MAX_BLOCKS * PART_BINS;
    int32_t* fine = cmaxcell + (size_t)PART_MAX_BLOCKS * PART_BINS;    at += p256(part_hist_bytes());
    int32_t* work = (int32_t*)at;                                       at += p256((size_t)n * 4);
    uint32_t* keys_out = (uint32_t*)at;                                 at += p256((size_t)n * 4);
    int32_t* rows = (int32_t*)at;                                       at += p256((size_t)n * 4);
    void* sort_tmp = at;
    size_t sort_bytes = part_sort_temp(n);
    const unsigned grid = grid_for(n, 256);

    auto clock = std::chrono::steady_clock::now();
    hipError_t e = hipSuccess;
    auto tick = [&](int phase) -> hipError_t {                          // measurement hook: waits for the stream after every phase
        if (!phase_seconds) return hipSuccess;
        const hipError_t w = hipStreamSynchronize(s);
        const auto now = std::chrono::steady_clock::now();
        phase_seconds[phase] += std::chrono::duration<double>(now - clock).count();
        clock = now;
        return w;
    };
#define PART_TICK(phase) do { e = tick(phase); PART_SYNC_ERR(e, "phase timing"); } while (0)
    auto read_record = [&]() {
        hipError_t r = hipMemcpyAsync(host, rec, 64, hipMemcpyDeviceToHost, s);
        if (r == hipSuccess) r = hipStreamSynchronize(s);
        return r;
    };

    e = hipMemsetAsync(workspace, 0, PART_HEAD + p256(part_blocks_bytes()), s);
    PART_SYNC_ERR(e, "clear");
    hipLaunchKernelGGL(k_part_check, dim3(grid), dim3(256), 0, s, coords, n, (int)cols, rec);
    PCGC_CHECK_LAUNCH("partition_check");
    e = read_record();
    PART_SYNC_ERR(e, "check");
    PART_TICK(PARTITION_PHASE_COPIES);
    info[PARTITION_INFO_BAD_RANGE] = host[PR_BAD_RANGE]; info[PARTITION_INFO_BAD_BATCH] = host[PR_BAD_BATCH];
    if (host[PR_BAD_RANGE] || host[PR_BAD_BATCH]) {
        pcgc_set_error("partition: %d of %lld rows are outside 0 .. 2^20 - 1, %d have a batch index other than 0", host[PR_BAD_RANGE], (long long)n,
                       host[PR_BAD_BATCH]);
        return -3;
    }

    int32_t* cnt = pb + PB_CNT_A * PART_MAX_BLOCKS, *cnt_new = pb + PB_CNT_B * PART_MAX_BLOCKS;
    int32_t* stuck = pb + PB_STUCK_A * PART_MAX_BLOCKS, *stuck_new = pb + PB_STUCK_B * PART_MAX_BLOCKS;
    hipLaunchKernelGGL(k_part_fill, dim3(1), dim3(256), 0, s, cnt, (int64_t)1, (int32_t)n, 0);      // one block holds all rows
    PCGC_CHECK_LAUNCH("partition_first");
    e = hipMemsetAsync(work, 0, (size_t)n * 4, s);
    PART_SYNC_ERR(e, "clear");
    int blocks = 1, rounds = 0;
    bool open = n > max_num;
    while (open) {
        if (rounds >= PART_MAX_BLOCKS) { pcgc_set_error("partition: still splitting after %d rounds", rounds); return -1; }
        hipLaunchKernelGGL(k_part_round_init, dim3(1), dim3(1024), 0, s, pb, rec);
        PCGC_CHECK_LAUNCH("partition_round_init");
        e = hipMemsetAsync(ccnt, 0, part_hist_bytes(), s);
        PART_SYNC_ERR(e, "clear");
        hipLaunchKernelGGL(k_part_bounds, dim3(grid), dim3(256), 0, s, coords, n, (int)cols, shift, work, cnt, stuck, max_num, pb);
        PCGC_CHECK_LAUNCH("partition_bounds");
        hipLaunchKernelGGL(k_part_plan, dim3(1), dim3(1024), 0, s, blocks, cnt, stuck, max_num, pb);
        PCGC_CHECK_LAUNCH("partition_plan");
        PART_TICK(PARTITION_PHASE_BOUNDS);
        hipLaunchKernelGGL(k_part_coarse, dim3(grid), dim3(256), 0, s, coords, n, (int)cols, shift, work, pb, ccnt, cmaxcell);
        PCGC_CHECK_LAUNCH("partition_coarse");
        PART_TICK(PARTITION_PHASE_COARSE);
        hipLaunchKernelGGL(k_part_cut1, dim3(blocks), dim3(256), 0, s, cnt, pb, ccnt, cmaxcell, fine);
        PCGC_CHECK_LAUNCH("partition_cut1");
        PART_TICK(PARTITION_PHASE_CUT);
        hipLaunchKernelGGL(k_part_fine, dim3(grid), dim3(256), 0, s, coords, n, (int)cols, shift, work, pb, fine);
        PCGC_CHECK_LAUNCH("partition_fine");
        PART_TICK(PARTITION_PHASE_FINE);
        hipLaunchKernelGGL(k_part_cut2, dim3(1), dim3(1024), 0, s, blocks, cnt, stuck, cnt_new, stuck_new, max_num, pb, fine, rec);
        PCGC_CHECK_LAUNCH("partition_cut2");
        PART_TICK(PARTITION_PHASE_CUT);
        hipLaunchKernelGGL(k_part_assign, dim3(grid), dim3(256), 0, s, coords, n, (int)cols, shift, work, pb, rec);
        PCGC_CHECK_LAUNCH("partition_assign");
        PART_TICK(PARTITION_PHASE_ASSIGN);
        e = read_record();
        PART_SYNC_ERR(e, "round");
        PART_TICK(PARTITION_PHASE_COPIES);
        if (host[PR_ERROR]) { pcgc_set_error("partition: the counts of %d blocks do not add up to their rows", host[PR_ERROR]); return -1; }
        if (host[PR_SPLIT] == 0) break;                                 // the round that splits nothing is the end
        if (host[PR_BLOCKS] > PART_MAX_BLOCKS) {
            info[PARTITION_INFO_WOULD_BE] = host[PR_BLOCKS];
            pcgc_set_error("partition: %d blocks; at most %d (a larger max_num gives fewer)", host[PR_BLOCKS], PART_MAX_BLOCKS);
            return -4;
        }
        blocks = host[PR_BLOCKS];
        ++rounds;
        open = host[PR_OPEN] > 0;
        int32_t* t = cnt; cnt = cnt_new; cnt_new = t;
        t = stuck; stuck = stuck_new; stuck_new = t;
    }

    hipLaunchKernelGGL(k_part_table, dim3(1), dim3(1024), 0, s, blocks, cnt, max_num, table, rec);
    PCGC_CHECK_LAUNCH("partition_table");
    hipLaunchKernelGGL(k_part_boxes, dim3(grid), dim3(256), 0, s, coords, n, (int)cols, work, blocks, table);
    PCGC_CHECK_LAUNCH("partition_boxes");
    hipLaunchKernelGGL(k_part_fill, dim3(grid), dim3(256), 0, s, rows, n, 0, 1);
    PCGC_CHECK_LAUNCH("partition_rows");
    e = rocprim::radix_sort_pairs(sort_tmp, sort_bytes, (uint32_t*)work, keys_out, rows, perm, (size_t)n, 0, 10, s);   // stable: input order in a block
    PART_SYNC_ERR(e, "sort");
    e = hipMemcpyAsync(block_of, work, (size_t)n * 4, hipMemcpyDeviceToDevice, s);
    PART_SYNC_ERR(e, "copy");
    PART_TICK(PARTITION_PHASE_ORDER);
    e = read_record();
    PART_SYNC_ERR(e, "table");
    PART_TICK(PARTITION_PHASE_COPIES);
    info[PARTITION_INFO_ROUNDS] = rounds; info[PARTITION_INFO_BLOCKS] = blocks; info[PARTITION_INFO_OVERSIZE] = host[PR_OVERSIZE];
    return 0;
}

// ---- the collated rows of a run of blocks ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_part_gather(const int32_t* __restrict__ coords, int64_t n, int cols, const int32_t* __restrict__ perm,
                                                     const int32_t* __restrict__ block_of, int64_t first_row, int64_t rows, int32_t first_block,
                                                     int4* __restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= rows) return;
    const int32_t r = perm[first_row + j];
    int4 v = make_int4(-1, -1, -1, -1);                                 // (a row that is none: refused by every consumer's coordinate check)
    if ((uint32_t)r < (uint64_t)n) {
        const int32_t* c = coords + (int64_t)r * cols + (cols - 3);
        v = make_int4(block_of[r] - first_block, c[0], c[1], c[2]);
    }
    out[j] = v;
}

extern "C" int pcgc_partition_gather(const int32_t* coords, int64_t n, int32_t cols, const int32_t* perm, const int32_t* block_of, int64_t first_row,
                                     int64_t rows, int32_t first_block, int32_t* out, void* stream) {
    PCGC_REQUIRE(n >= 0 && n <= PART_MAX_ROWS, "row count outside 0 .. 2^27");
    PCGC_REQUIRE(cols == 3 || cols == 4, "rows of 3 or 4 columns");
    PCGC_REQUIRE(first_row >= 0 && rows >= 0 && first_row + rows <= n, "the run is outside the rows");
    PCGC_REQUIRE(first_block >= 0 && first_block < PART_MAX_BLOCKS, "first block outside 0 .. 1023");
    PCGC_REQUIRE(coords && perm && block_of && out, "null argument");
    PCGC_REQUIRE(((uintptr_t)out & 15) == 0, "misaligned output");
    if (rows == 0) return 0;
    hipLaunchKernelGGL(k_part_gather, dim3(grid_for(rows, 256)), dim3(256), 0, S(stream), coords, n, (int)cols, perm, block_of, first_row, rows,
                       first_block, (int4*)out);
    PCGC_CHECK_LAUNCH("partition_gather");
    return 0;
}
