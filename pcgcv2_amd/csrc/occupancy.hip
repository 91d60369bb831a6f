// Lossless mode (lossless.py, `_O.bin`): the occupancy bit of every candidate row of a decoder level is range-coded on the host under a
// probability that follows from the row's logit.  This file turns a level's logits into what the host coder reads: one uint16 per row,
// ctx << 1 | bit, in candidate-row order, plus (encoder side) the number of occupied rows and the ideal code length of the level.
//
//   ctx = clamp(rint(16 z), -176, 176) + 176        rint: ties to even; +-inf clamp; NaN gives ctx = 176 (p = 1/2)
//   cost += COST[ctx][bit]                           integers, units of 2^-16 bit (occupancy_tables.h; part of the format)
//
// One streaming pass, four consecutive rows per thread: 16 B of logits and 4 B of truth in, 8 B out per thread where the logits are dense
// and the pointers aligned, scalar accesses of the same rows otherwise.  The sums are integers: per-block partials in a slab, added by
// one block (loss.hip's scheme); the grid is a function of n alone.  pcgc_occ_symbols_segments is the same pass over the contiguous frames
// of a batch's level, with one pair of sums per frame (k_occ_symbols_segments below).
#include "pcgc_common.h"
#include "occupancy_tables.h"

constexpr int OCC_BLOCK = 256;
constexpr int OCC_ROWS = 4;                              // rows per thread; a block covers OCC_BLOCK * OCC_ROWS = 1024 rows

static const uint16_t h_occ_p1[PCGC_OCC_CONTEXTS] = {PCGC_OCC_P1_VALUES};
static const int32_t h_occ_cost[2 * PCGC_OCC_CONTEXTS] = {PCGC_OCC_COST_VALUES};
__device__ static const int32_t d_occ_cost[2 * PCGC_OCC_CONTEXTS] = {PCGC_OCC_COST_VALUES};

__device__ static inline int occ_context(float z) {
    const float s = 16.0f * z;                           // exact short of overflow, which gives +-inf and clamps
    if (!(s == s)) return PCGC_OCC_QMAX;                 // NaN
    const float c = fminf(fmaxf(s, -(float)PCGC_OCC_QMAX), (float)PCGC_OCC_QMAX);
    return (int)rintf(c) + PCGC_OCC_QMAX;                // the bounds are integers: clamping first rounds to the same integer
}

// A thread's OCC_ROWS consecutive rows from i0 (m of them exist): logits and truth in, ctx << 1 | bit out; ctx[] and bit[] stay with the caller
template <bool VEC>
__device__ static inline void occ_thread_rows(const float* __restrict__ logits, int64_t ld, const uint8_t* __restrict__ truth, uint16_t* __restrict__ packed,
                                              int64_t i0, int m, int (&ctx)[OCC_ROWS], int (&bit)[OCC_ROWS]) {
    float x[OCC_ROWS] = {0.f, 0.f, 0.f, 0.f};
    uint8_t y[OCC_ROWS] = {0, 0, 0, 0};
    if (VEC && m == OCC_ROWS) {
        const float4 v = *(const float4*)(logits + i0);
        x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
        if (truth) { const uchar4 t = *(const uchar4*)(truth + i0); y[0] = t.x; y[1] = t.y; y[2] = t.z; y[3] = t.w; }
    } else {
        for (int j = 0; j < m; ++j) {
            x[j] = logits[(i0 + j) * ld];
            if (truth) y[j] = truth[i0 + j];
        }
    }
    uint16_t w[OCC_ROWS] = {0, 0, 0, 0};
    for (int j = 0; j < m; ++j) {
        ctx[j] = occ_context(x[j]);
        bit[j] = y[j] != 0;
        w[j] = (uint16_t)((ctx[j] << 1) | bit[j]);
    }
    if (VEC && m == OCC_ROWS) {
        *(ushort4*)(packed + i0) = make_ushort4(w[0], w[1], w[2], w[3]);
    } else {
        for (int j = 0; j < m; ++j) packed[i0 + j] = w[j];
    }
}

template <bool VEC>
__global__ void __launch_bounds__(OCC_BLOCK) k_occ_symbols(const float* __restrict__ logits, int64_t ld, int64_t n, const uint8_t* __restrict__ truth,
                                                           uint16_t* __restrict__ packed,
                                                           uint32_t* __restrict__ cslab, unsigned long long* __restrict__ bslab) {
    __shared__ int32_t sh_cost[2 * PCGC_OCC_CONTEXTS];
    __shared__ unsigned cred[OCC_BLOCK / 64];
    __shared__ unsigned long long bred[OCC_BLOCK / 64];
    if (truth)                                           // (uniform across the grid)
        for (int i = threadIdx.x; i < 2 * PCGC_OCC_CONTEXTS; i += OCC_BLOCK) sh_cost[i] = d_occ_cost[i];
    __syncthreads();
    const int64_t i0 = ((int64_t)blockIdx.x * OCC_BLOCK + threadIdx.x) * OCC_ROWS;
    const int m = i0 >= n ? 0 : (int)(n - i0 < OCC_ROWS ? n - i0 : OCC_ROWS);
    int ctx[OCC_ROWS], bit[OCC_ROWS];
    occ_thread_rows<VEC>(logits, ld, truth, packed, i0, m, ctx, bit);
    if (!truth) return;                                  // decoder side: contexts only
    unsigned occupied = 0;
    unsigned long long bits = 0;
    for (int j = 0; j < m; ++j) { occupied += (unsigned)bit[j]; bits += (unsigned long long)sh_cost[2 * ctx[j] + bit[j]]; }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { occupied += __shfl_xor(occupied, d, 64); bits += __shfl_xor(bits, d, 64); }
    if ((threadIdx.x & 63) == 0) { cred[threadIdx.x >> 6] = occupied; bred[threadIdx.x >> 6] = bits; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned c = 0; unsigned long long b = 0;
        for (int k = 0; k < OCC_BLOCK / 64; ++k) { c += cred[k]; b += bred[k]; }
        cslab[blockIdx.x] = c; bslab[blockIdx.x] = b;
    }
}

// The same pass over nseg contiguous frames (a batch's level: frame f is rows row[f] .. row[f + 1]); the table travels by value.  packed is
// what k_occ_symbols writes (the grid and every thread's rows are the same: a context depends on its own logit only); the sums are per frame.
// A block of 1024 rows may hold the end of one frame, several whole small ones and the start of another: each block adds its rows into
// per-frame accumulators in LDS (a wave whose rows all lie in one frame reduces by shuffles first) and then adds them to sums [nseg, 2] with
// one integer atomic per frame it touches.  Integer sums: exact, whatever the order the blocks arrive in.  Nothing is read back in this launch.
constexpr int OCC_MAX_SEGMENTS = 16;
struct OccSegments {
    long long row[OCC_MAX_SEGMENTS + 1];                 // ascending from 0; row[f] = row[nseg] for f > nseg
    int nseg;
};
__device__ static inline int occ_segment_of(const OccSegments& sg, int64_t i) {       // the frame that holds row i < row[nseg] (frames may be empty)
    int f = 0;
    for (int b = 1; b < OCC_MAX_SEGMENTS; ++b) f += (b < sg.nseg && (int64_t)sg.row[b] <= i) ? 1 : 0;
    return f;
}

template <bool VEC>
__global__ void __launch_bounds__(OCC_BLOCK) k_occ_symbols_segments(const float* __restrict__ logits, int64_t ld, OccSegments sg, const uint8_t* __restrict__ truth,
                                                                    uint16_t* __restrict__ packed, unsigned long long* __restrict__ sums) {
    __shared__ int32_t sh_cost[2 * PCGC_OCC_CONTEXTS];
    __shared__ unsigned long long acc[OCC_MAX_SEGMENTS][2];
    for (int i = threadIdx.x; i < 2 * PCGC_OCC_CONTEXTS; i += OCC_BLOCK) sh_cost[i] = d_occ_cost[i];
    if (threadIdx.x < 2 * OCC_MAX_SEGMENTS) acc[threadIdx.x >> 1][threadIdx.x & 1] = 0ull;
    __syncthreads();
    const int64_t n = sg.row[OCC_MAX_SEGMENTS];
    const int64_t i0 =((int64_t)blockIdx.x * OCC_BLOCK + threadIdx.x) * OCC_ROWS;
    const int m = i0 >= n ? 0 : (int)(n - i0 < OCC_ROWS ? n - i0 : OCC_ROWS);
    int ctx[OCC_ROWS], bit[OCC_ROWS];
    occ_thread_rows<VEC>(logits, ld, truth, packed, i0, m, ctx, bit);
    // the frames of this thread's first and last row; a thread without rows sides with its wave's first lane
    const int f_lo = m ? occ_segment_of(sg, i0) : -1, f_hi = m ? occ_segment_of(sg, i0 + m - 1) : -1;
    const int f_wave = __shfl(f_lo, 0, 64);
    const bool one_frame = __all(m == 0 || (f_lo == f_wave && f_hi == f_wave));       // (lane 0 has rows whenever any lane of its wave has)
    if (one_frame) {
        unsigned long long occupied = 0, bits = 0;
        for (int j = 0; j < m; ++j) { occupied += (unsigned long long)bit[j]; bits += (unsigned long long)sh_cost[2 * ctx[j] + bit[j]]; }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) { occupied += __shfl_xor(occupied, d, 64); bits += __shfl_xor(bits, d, 64); }
        if ((threadIdx.x & 63) == 0 && f_wave >= 0) { atomicAdd(&acc[f_wave][0], occupied); atomicAdd(&acc[f_wave][1], bits); }
    } else {
        for (int j = 0; j < m; ++j) {
            const int f = occ_segment_of(sg, i0 + j);
            if (bit[j]) atomicAdd(&acc[f][0], 1ull);
            atomicAdd(&acc[f][1], (unsigned long long)sh_cost[2 * ctx[j] + bit[j]]);
        }
    }
    __syncthreads();
    // one global add per non-zero accumulator, i.e. per frame this block's rows lie in (integers: the order of arrival does not matter)
    if (threadIdx.x < 2 * OCC_MAX_SEGMENTS && acc[threadIdx.x >> 1][threadIdx.x & 1])
        atomicAdd(&sums[threadIdx.x], acc[threadIdx.x >> 1][threadIdx.x & 1]);
}
// second stage: one block; thread t adds slots t, t + 256, ... (integers: the order does not matter, the result is exact)
__global__ void __launch_bounds__(OCC_BLOCK) k_occ_final(const uint32_t* __restrict__ cslab, const unsigned long long* __restrict__ bslab, int64_t blocks,
                                                         long long* __restrict__ sums) {
    __shared__ long long sc[OCC_BLOCK / 64][2];
    long long c = 0, b = 0;
    for (int64_t i = threadIdx.x; i < blocks; i += OCC_BLOCK) { c += (long long)cslab[i]; b += (long long)bslab[i]; }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { c += __shfl_xor(c, d, 64); b += __shfl_xor(b, d, 64); }
    if ((threadIdx.x & 63) == 0) { sc[threadIdx.x >> 6][0] = c; sc[threadIdx.x >> 6][1] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        long long tc = 0, tb = 0;
        for (int k = 0; k < OCC_BLOCK / 64; ++k) { tc += sc[k][0]; tb += sc[k][1]; }
        sums[0] = tc; sums[1] = tb;
    }
}

static int64_t occ_blocks(int64_t n) { return (n + (int64_t)OCC_BLOCK * OCC_ROWS - 1) / ((int64_t)OCC_BLOCK * OCC_ROWS); }

extern "C" size_t pcgc_occ_workspace_bytes(int64_t n) {
    // one 64-bit and one 32-bit partial per block of the grid pcgc_occ_symbols launches for n rows
    const int64_t blocks = occ_blocks(n > 0 ? n : 1);
    return (size_t)blocks * (sizeof(unsigned long long) + sizeof(uint32_t)) + 64;
}

extern "C" int pcgc_occ_tables(uint16_t* p1, int32_t* cost) {
    if (p1) for (int i = 0; i < PCGC_OCC_CONTEXTS; ++i) p1[i] = h_occ_p1[i];
    if (cost) for (int i = 0; i < 2 * PCGC_OCC_CONTEXTS; ++i) cost[i] = h_occ_cost[i];
    return PCGC_OCC_CONTEXTS;
}

extern "C" int pcgc_occ_symbols(const float* logits, int64_t ld, int64_t n, const uint8_t* truth, uint16_t* packed, int64_t* sums,
                                void* workspace, size_t workspace_bytes, void* stream) {
    PCGC_REQUIRE(n >= 0 && ld >= 1, "bad arguments");
    if (n == 0) {                                        // (no rows: there may be no truth pointer to go with sums)
        if (sums) { hipError_t e = hipMemsetAsync(sums, 0, 2 * sizeof(int64_t), S(stream)); if (e != hipSuccess) { pcgc_set_error("occ_symbols: %s", hipGetErrorString(e)); return -1; } }
        return 0;
    }
    PCGC_REQUIRE(!truth == !sums, "truth and sums go together (both for the encoder, neither for the decoder)");
    PCGC_REQUIRE(n < ((int64_t)1 << 31) * OCC_ROWS, "too many rows");
    PCGC_REQUIRE(logits && packed, "null argument");
    const int64_t blocks = occ_blocks(n);
    unsigned long long* bslab = nullptr; uint32_t* cslab = nullptr;
    if (truth) {
        PCGC_REQUIRE(workspace && workspace_bytes >= pcgc_occ_workspace_bytes(n) && ((uintptr_t)workspace & 7) == 0, "workspace too small or misaligned");
        bslab = (unsigned long long*)workspace;
        cslab = (uint32_t*)(bslab + blocks);
    }
    const bool vec = ld == 1 && (((uintptr_t)logits) & 15) == 0 && (((uintptr_t)truth) & 3) == 0 && (((uintptr_t)packed) & 7) == 0;
    if (vec) hipLaunchKernelGGL(k_occ_symbols<true>, dim3((unsigned)blocks), dim3(OCC_BLOCK), 0, S(stream), logits, ld, n, truth, packed, cslab, bslab);
    else hipLaunchKernelGGL(k_occ_symbols<false>, dim3((unsigned)blocks), dim3(OCC_BLOCK), 0, S(stream), logits, ld, n, truth, packed, cslab, bslab);
    PCGC_CHECK_LAUNCH("occ_symbols");
    if (truth) {
        hipLaunchKernelGGL(k_occ_final, dim3(1), dim3(OCC_BLOCK), 0, S(stream), cslab, bslab, blocks, (long long*)sums);
        PCGC_CHECK_LAUNCH("occ_symbols");
    }
    return 0;
}

extern "C" int pcgc_occ_symbols_segments(const float* logits, int64_t ld, int nseg, const int64_t* seg_rows, const uint8_t* truth, uint16_t* packed,
                                         int64_t* sums, void* stream) {
    PCGC_REQUIRE(nseg >= 1 && nseg <= OCC_MAX_SEGMENTS && seg_rows && ld >= 1, "1 to 16 segments");
    OccSegments sg;
    sg.nseg = nseg;
    sg.row[0] = 0;
    for (int f = 0; f < OCC_MAX_SEGMENTS; ++f) {
        PCGC_REQUIRE(f >= nseg || seg_rows[f] >= 0, "negative row count");
        sg.row[f + 1] = sg.row[f] + (f < nseg ? seg_rows[f] : 0);
        PCGC_REQUIRE(sg.row[f + 1] < ((int64_t)1 << 31) * OCC_ROWS, "too many rows");
    }
    const int64_t n = sg.row[nseg];
    PCGC_REQUIRE(n == 0 || !truth == !sums, "truth and sums go together (both for the encoder, neither for the decoder)");
    if (!truth || n == 0) {                              // contexts only, or no rows (then there may be no truth pointer to go with sums)
        if (sums) { hipError_t e = hipMemsetAsync(sums, 0, 2 * nseg * sizeof(int64_t), S(stream)); if (e != hipSuccess) { pcgc_set_error("occ_symbols_segments: %s", hipGetErrorString(e)); return -1; } }
        return n ? pcgc_occ_symbols(logits, ld, n, nullptr, packed, nullptr, nullptr, 0, stream) : 0;
    }
    PCGC_REQUIRE(logits && packed, "null argument");
    hipError_t e = hipMemsetAsync(sums, 0, 2 * nseg * sizeof(int64_t), S(stream));
    if (e != hipSuccess) { pcgc_set_error("occ_symbols_segments: %s", hipGetErrorString(e)); return -1; }
    const int64_t blocks = occ_blocks(n);
    const bool vec = ld == 1 && (((uintptr_t)logits) & 15) == 0 && (((uintptr_t)truth) & 3) == 0 && (((uintptr_t)packed) & 7) == 0;
    if (vec) hipLaunchKernelGGL(k_occ_symbols_segments<true>, dim3((unsigned)blocks), dim3(OCC_BLOCK), 0, S(stream), logits, ld, sg, truth, packed, (unsigned long long*)sums);
    else hipLaunchKernelGGL(k_occ_symbols_segments<false>, dim3((unsigned)blocks), dim3(OCC_BLOCK), 0, S(stream), logits, ld, sg, truth, packed, (unsigned long long*)sums);
    PCGC_CHECK_LAUNCH("occ_symbols_segments");
    return 0;
}
