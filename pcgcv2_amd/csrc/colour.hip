// Per-point attributes (colours) carried between two clouds, and the colour distortion between them, over the kept nearest-distance tie sets
// that pcgc_d2_count / pcgc_d2_fill / pcgc_d2_segment_lowest produce (metric.hip).  Everything here is integer arithmetic: sums of integers
// do not depend on the order in which atomics or reduction trees add them, so every result is exact and bitwise reproducible.
//
//   pcgc_attr_transfer   attr(t) = mean, rounded half up, of the attributes of the sources whose tie set holds t, or, for a target that no
//                        source chose, of the sources of t's own tie set (the rule metric.hip's k_d2_normals applies to normals).
//                        pack:    the C bytes of a source row into one 32-bit word (a neighbour then costs one gather, not C byte loads)
//                        scatter: one thread per source adds its word, spread over 32-bit fields of 64-bit accumulators, to every target of
//                                 its tie set (2 atomics per pair for C <= 3, 3 for C = 4).  A field holds at most 255 * ns: the entry point
//                                 refuses ns for which that does not fit 32 bits, so no field carries into its neighbour.
//                        finish:  one thread per target divides, or averages over its own tie set
//   pcgc_colour_dist     per point of P: its colour against the rounded mean colour of its tie set in Q, as three squared BT.709 YUV
//                        differences (numerators with the coefficients x 10^4: integers below 2^43) and three squared RGB differences
//   pcgc_colour_reduce   sums of the YUV terms as two 64-bit sums each (low and high 32 bits: exact for any n < 2^31), maxima of the RGB terms
#include "pcgc_common.h"

#define ATTR_MAX_SOURCES ((int64_t)(0xFFFFFFFFu / 255u))        // 255 * ns <= 2^32 - 1

typedef unsigned long long u64;

__device__ static inline uint32_t pack_row(const uint8_t* __restrict__ a, int64_t i, int C) {
    uint32_t w = 0;
    for (int c = 0; c < C; ++c) w |= (uint32_t)a[i * C + c] << (8 * c);
    return w;
}

__global__ void __launch_bounds__(256) k_attr_pack(const uint8_t* __restrict__ attr, int64_t n, int C, uint32_t* __restrict__ packed) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) packed[i] = pack_row(attr, i, C);
}

// W = 2 (C <= 3): word 0 = c0 | c1 << 32, word 1 = c2 | count << 32.  W = 3 (C = 4): word 1 = c2 | c3 << 32, word 2 = count.
template <int W>
__global__ void __launch_bounds__(256) k_attr_scatter(const int64_t* __restrict__ seg, const int32_t* __restrict__ kept,
                                                      const int32_t* __restrict__ rows, int64_t ns, const uint32_t* __restrict__ packed,
                                                      int64_t nt, u64* __restrict__ acc) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= ns) return;
    const uint32_t w = packed[s];
    const u64 w0 = (u64)(w & 0xFFu) | ((u64)((w >> 8) & 0xFFu) << 32);
    const u64 w1 = W == 2 ? ((u64)((w >> 16) & 0xFFu) | (1ull << 32)) : ((u64)((w >> 16) & 0xFFu) | ((u64)(w >> 24) << 32));
    const int64_t b = seg[s];
    const int m = kept[s];
    for (int k = 0; k < m; ++k) {
        const int32_t t = rows[b + k];
        if ((uint32_t)t >= (uint64_t)nt) continue;                 // (a negative row is out of range too)
        u64* a = acc + (int64_t)t * W;
        atomicAdd(a, w0);
        atomicAdd(a + 1, w1);
        if (W == 3) atomicAdd(a + 2, 1ull);
    }
}

template <int W>
__global__ void __launch_bounds__(256) k_attr_finish(const u64* __restrict__ acc, int64_t nt, const int64_t* __restrict__ seg_ts,
                                                     const int32_t* __restrict__ kept_ts, const int32_t* __restrict__ rows_ts, int64_t ns,
                                                     const uint32_t* __restrict__ packed, int C, uint8_t* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt) return;
    const u64 a0 = acc[t * W], a1 = acc[t * W + 1];
    u64 sum[4] = {a0 & 0xFFFFFFFFull, a0 >> 32, a1 & 0xFFFFFFFFull, W == 3 ? a1 >> 32 : 0ull};
    u64 cnt = W == 3 ? acc[t * W + 2] : a1 >> 32;
    if (cnt == 0) {                                          // no source chose t: the sources t itself is nearest to
        const int64_t b = seg_ts[t];
        const int m = kept_ts[t];
        sum[0] = sum[1] = sum[2] = sum[3] = 0;
        for (int k = 0; k < m; ++k) {
            const int32_t s = rows_ts[b + k];
            if ((uint32_t)s >= (uint64_t)ns) continue;
            const uint32_t w = packed[s];
            sum[0] += w & 0xFFu; sum[1] += (w >> 8) & 0xFFu; sum[2] += (w >> 16) & 0xFFu; sum[3] += w >> 24;
            ++cnt;
        }
    }
    for (int c = 0; c < C; ++c) out[t * C + c] = cnt ? (uint8_t)((2 * sum[c] + cnt) / (2 * cnt)) : (uint8_t)0;
}

// p's colour against round_half_up(mean colour of its tie set): yuv2 [n,3] = (sum_c M[k][c] d_c)^2 with M the BT.709 matrix x 10^4 and
// d = own - mean in 8-bit units; rgb2 [n,3] = d_c^2
__global__ void __launch_bounds__(256) k_colour_dist(const uint8_t* __restrict__ cp, int64_t n, const uint8_t* __restrict__ cq, int64_t nq,
                                                     const int64_t* __restrict__ seg, const int32_t* __restrict__ kept,
                                                     const int32_t* __restrict__ rows, int64_t* __restrict__ yuv2, int32_t* __restrict__ rgb2) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t b = seg[i];
    const int m = kept[i];
    int32_t sr = 0, sg = 0, sb = 0, cnt = 0;
    for (int k = 0; k < m; ++k) {
        const int32_t r = rows[b + k];
        if ((uint32_t)r >= (uint64_t)nq) continue;
        sr += cq[3 * (int64_t)r]; sg += cq[3 * (int64_t)r + 1]; sb += cq[3 * (int64_t)r + 2];
        ++cnt;
    }
    int32_t dr = 0, dg = 0, db = 0;
    if (cnt) {
        dr = (int32_t)cp[3 * i] - (2 * sr + cnt) / (2 * cnt);
        dg = (int32_t)cp[3 * i + 1] - (2 * sg + cnt) / (2 * cnt);
        db = (int32_t)cp[3 * i + 2] - (2 * sb + cnt) / (2 * cnt);
    }
    const int64_t y = 2126 * dr + 7152 * dg + 722 * db;
    const int64_t u = -1146 * dr - 3854 * dg + 5000 * db;
    const int64_t v = 5000 * dr - 4542 * dg - 458 * db;
    yuv2[3 * i] = y * y; yuv2[3 * i + 1] = u * u; yuv2[3 * i + 2] = v * v;
    rgb2[3 * i] = dr * dr; rgb2[3 * i + 1] = dg * dg; rgb2[3 * i + 2] = db * db;
}

// 9 values per thread: low-word sums, high-word sums, maxima.  Reduced across the 64 lanes of a wave by shuffles, across the 4 waves of the
// block through LDS.
#define COLOUR_RED_BLOCKS 1024
__device__ static inline void block_reduce9(u64 (&v)[9], u64* __restrict__ dst) {
    __shared__ u64 part[4][9];
    for (int off = 32; off > 0; off >>= 1)
        for (int j = 0; j < 9; ++j) {
            const u64 o = __shfl_xor(v[j], off, 64);
            v[j] = j < 6 ? v[j] + o : (o > v[j] ? o : v[j]);
        }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
        for (int j = 0; j < 9; ++j) part[wave][j] = v[j];
    __syncthreads();
    if (threadIdx.x < 9) {
        const int j = threadIdx.x;
        u64 r = part[0][j];
        for (int w = 1; w < 4; ++w) r = j < 6 ? r + part[w][j] : (part[w][j] > r ? part[w][j] : r);
        dst[j] = r;
    }
}
__global__ void __launch_bounds__(256) k_colour_reduce(const int64_t* __restrict__ yuv2, const int32_t* __restrict__ rgb2, int64_t n,
                                                       int stride_blocks, u64* __restrict__ partial) {
    u64 v[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)stride_blocks * 256)
        for (int k = 0; k < 3; ++k) {
            const u64 q = (u64)yuv2[3 * i + k];
            const u64 m = (u64)(uint32_t)rgb2[3 * i + k];
            v[k] += q & 0xFFFFFFFFull; v[3 + k] += q >> 32; v[6 + k] = m > v[6 + k] ? m : v[6 + k];
        }
    block_reduce9(v, partial + (int64_t)blockIdx.x * 9);
}
__global__ void __launch_bounds__(256) k_colour_reduce_final(const u64* __restrict__ partial, int blocks, u64* __restrict__ out) {
    u64 v[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = threadIdx.x; i < blocks; i += 256)
        for (int j = 0; j < 9; ++j) {
            const u64 o = partial[(int64_t)i * 9 + j];
            v[j] = j < 6 ? v[j] + o : (o > v[j] ? o : v[j]);
        }
    block_reduce9(v, out);
}

static size_t attr_packed_bytes(int64_t ns) { return (((size_t)(ns < 1 ? 1 : ns) * 4) + 255) & ~(size_t)255; }

extern "C" size_t pcgc_attr_transfer_workspace_bytes(int64_t ns, int64_t nt, int channels) {
    return attr_packed_bytes(ns) + (size_t)(nt < 1 ? 1 : nt) * (channels == 4 ? 3 : 2) * 8;
}

extern "C" int pcgc_attr_transfer(const int64_t* seg_st, const int32_t* kept_st, const int32_t* rows_st, int64_t ns, const int64_t* seg_ts,
                                  const int32_t* kept_ts, const int32_t* rows_ts, int64_t nt, const uint8_t* attr_s, int channels,
                                  uint8_t* attr_t, void* workspace, size_t workspace_bytes, void* stream) {
    PCGC_REQUIRE(channels >= 1 && channels <= 4, "1 to 4 channels");
    PCGC_REQUIRE(ns >= 0 && nt >= 0 && nt <= 0x7FFFFFFFll, "bad row count");
    PCGC_REQUIRE(ns <= ATTR_MAX_SOURCES, "too many source rows for the 32-bit accumulator fields (255 * ns must stay below 2^32)");
    if (nt == 0) return 0;
    PCGC_REQUIRE(ns > 0, "no source rows");
    PCGC_REQUIRE(seg_st && kept_st && rows_st && seg_ts && kept_ts && rows_ts && attr_s && attr_t && workspace, "null argument");
    PCGC_REQUIRE(workspace_bytes >= pcgc_attr_transfer_workspace_bytes(ns, nt, channels), "workspace too small");
    const int W = channels == 4 ? 3 : 2;
    uint32_t* packed = (uint32_t*)workspace;
    u64* acc = (u64*)((char*)workspace + attr_packed_bytes(ns));
    hipError_t e = hipMemsetAsync(acc, 0, (size_t)nt * W * 8, S(stream));
    if (e != hipSuccess) { pcgc_set_error("attr_transfer: %s", hipGetErrorString(e)); return -1; }
    hipLaunchKernelGGL(k_attr_pack, dim3(grid_for(ns, 256)), dim3(256), 0, S(stream), attr_s, ns, channels, packed);
    PCGC_CHECK_LAUNCH("attr_pack");
    if (W == 2) {
        hipLaunchKernelGGL(k_attr_scatter<2>, dim3(grid_for(ns, 256)), dim3(256), 0, S(stream), seg_st, kept_st, rows_st, ns, packed, nt, acc);
        PCGC_CHECK_LAUNCH("attr_scatter");
        hipLaunchKernelGGL(k_attr_finish<2>, dim3(grid_for(nt, 256)), dim3(256), 0, S(stream), acc, nt, seg_ts, kept_ts, rows_ts, ns, packed,
                           channels, attr_t);
    } else {
        hipLaunchKernelGGL(k_attr_scatter<3>, dim3(grid_for(ns, 256)), dim3(256), 0, S(stream), seg_st, kept_st, rows_st, ns, packed, nt, acc);
        PCGC_CHECK_LAUNCH("attr_scatter");
        hipLaunchKernelGGL(k_attr_finish<3>, dim3(grid_for(nt, 256)), dim3(256), 0, S(stream), acc, nt, seg_ts, kept_ts, rows_ts, ns, packed,
                           channels, attr_t);
    }
    PCGC_CHECK_LAUNCH("attr_finish");
    return 0;
}

extern "C" int pcgc_colour_dist(const uint8_t* cp, int64_t n, const uint8_t* cq, int64_t nq, const int64_t* seg, const int32_t* kept,
                                const int32_t* rows, int64_t* yuv2, int32_t* rgb2, void* stream) {
    PCGC_REQUIRE(n >= 0 && n <= 0x7FFFFFFFll && nq >= 0 && nq <= 0x7FFFFFFFll, "bad row count");
    if (n == 0) return 0;
    PCGC_REQUIRE(nq > 0, "no rows in the other cloud");
    PCGC_REQUIRE(cp && cq && seg && kept && rows && yuv2 && rgb2, "null argument");
    hipLaunchKernelGGL(k_colour_dist, dim3(grid_for(n, 256)), dim3(256), 0, S(stream), cp, n, cq, nq, seg, kept, rows, yuv2, rgb2);
    PCGC_CHECK_LAUNCH("colour_dist");
    return 0;
}

extern "C" size_t pcgc_colour_reduce_workspace_bytes(void) { return (size_t)COLOUR_RED_BLOCKS * 9 * 8; }
extern "C" int pcgc_colour_reduce(const int64_t* yuv2, const int32_t* rgb2, int64_t n, int64_t* out, void* workspace, size_t workspace_bytes,
                                  void* stream) {
    PCGC_REQUIRE(n >= 0 && n <= 0x7FFFFFFFll, "bad row count");
    PCGC_REQUIRE(out && workspace && (n == 0 || (yuv2 && rgb2)), "null argument");
    PCGC_REQUIRE(workspace_bytes >= pcgc_colour_reduce_workspace_bytes(), "workspace too small");
    int blocks = (int)grid_for(n < 1 ? 1 : n, 256);
    blocks = blocks < COLOUR_RED_BLOCKS ? blocks : COLOUR_RED_BLOCKS;          // (a function of n only, like pcgc_d2_reduce)
    hipLaunchKernelGGL(k_colour_reduce, dim3(blocks), dim3(256), 0, S(stream), yuv2, rgb2, n, blocks, (u64*)workspace);
    PCGC_CHECK_LAUNCH("colour_reduce");
    hipLaunchKernelGGL(k_colour_reduce_final, dim3(1), dim3(256), 0, S(stream), (const u64*)workspace, blocks, (u64*)out);
    PCGC_CHECK_LAUNCH("colour_reduce");
    return 0;
}
