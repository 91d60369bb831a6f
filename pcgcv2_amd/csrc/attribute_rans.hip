// Colour codec, `_A.bin` version 2 (attributes.py): the tokens of the colour transform coded ON THE DEVICE by interleaved rANS, so that only
// the coded bytes cross the bus.  Input is what pcgc_raht_quantize writes (tokens and their contexts in coding order) and the stream's own
// frequency tables; the format is stated in include/pcgc_hip.h and, in plain Python integers, in tests/attr_rans_reference.py.  It is the
// occupancy stream's coder (occupancy_rans.hip) with a 64-ary token in place of a bit: one wave per chunk of 64 S tokens, lane j codes
// tokens base + 64 t + j, 64-bit state, 32-bit words, L = 2^31, 16-bit frequencies; which lanes renormalise at a step is a ballot, where
// each lane's word goes is the prefix popcount of that ballot.
//
// The tables live in LDS, one row of AR_ROW words per context, filled once per workgroup:
//     [0 .. 7]   pivots cdf[8], cdf[16], .., cdf[56], then 65536      [8 .. 72]  cdf[0 .. 64] with cdf[0] = 0, cdf[64] = 65536      (3 words pad)
// so that every group of eight entries cdf[8 g .. 8 g + 7] and the pivots are 16-byte aligned.
//
//   encoder  steps t = S - 1 .. 0.  c and f of a token are two LDS words that depend on the input alone, so they are off the chain.  f = 65536
//            (a token that owns its row) is taken out before the division: the update is the identity and the token never emits.  A token
//            outside 0 .. 63, a context outside 0 .. 47 or f <= 0 is counted and skipped: nothing is divided by 0.  Words are written
//            downwards from the end of the chunk's scratch, then an offsets scan and a compaction, as in occupancy_rans.hip.
//   decoder  steps t = 0 .. S - 1.  The symbol search is two 8-way levels.  Level 1, which group of eight holds s, compares s with the
//            seven pivots; they depend on the context alone and are in registers before the batch's chain starts.  Level 2 reads the
//            group's eight entries (the one table read on the chain) and counts those <= s; c is the largest entry <= s and c + f the
//            smallest entry > s, taken by max / min over the same sixteen registers, so no index formed from table bytes ever addresses
//            memory and the token is in 0 .. 63 whatever the table says.  Words are staged through a ring in LDS as in occupancy_rans.hip.
//            The contexts come from k_attr_rans_ctx, which derives them from the tree's bucket offsets: they are never uploaded.
//
// A batch of frames (pcgc_attr_rans_*_batch) is one launch of the chunks of all frames: the chunk bodies below are shared, a
// workgroup serves one frame's chunk with that frame's table, and every frame's payload is packed on its own.
//
// No workgroup reads what another wrote in the same launch.  All integer arithmetic: the bytes are a function of the input alone.
#include <cstring>
#include "pcgc_common.h"

constexpr int AR_LANES = 64;
constexpr int AR_BATCH = 8;                                   // steps whose contexts (and pivots) are fetched together
constexpr int AR_FILL = AR_BATCH * AR_LANES;                  // words a batch can consume at most = words staged at a time
constexpr int AR_RING = 2 * AR_FILL;
constexpr int AR_MAX_STEPS = 1 << 24;                         // 64 S tokens per chunk stay below 2^31
constexpr int AR_CONTEXTS = 48;
constexpr int AR_TOKENS = 64;
constexpr int AR_ROW = 76;                                    // LDS words per context
constexpr uint64_t AR_L = 1ull << 31;
constexpr uint64_t AR_STATE_END = 1ull << 63;
constexpr int AR_SCAN_BLOCK = 256;
constexpr uint32_t AR_NONE = 0xffffffffu;

// table [48][65] uint16 in rc_encode_ctx's convention (entry 0 and entry 64 are implied) -> the LDS rows described above
__device__ static inline void ar_load_table(uint32_t* sh, const uint16_t* __restrict__ table) {
    for (int i = threadIdx.x; i < AR_CONTEXTS * AR_ROW; i += AR_LANES) {
        const int c = i / AR_ROW, w = i - c * AR_ROW;
        int e = w < 7 ? 8 * (w + 1) : w == 7 ? 64 : w - 8;     // the cdf entry this word holds
        if (e > 64) e = 64;                                     // (pad)
        sh[i] = e == 0 ? 0u : e == 64 ? 65536u : (uint32_t)table[c * (AR_TOKENS + 1) + e];
    }
    __syncthreads();
}
__device__ static inline int ar_lanes_below(uint64_t m) {
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}
// exact x / f and x % f for x < f << 47, 1 <= f <= 65535: schoolbook division in base 2^16 below the top 32 bits (as in occupancy_rans.hip)
__device__ static inline void ar_divmod(uint64_t x, uint32_t f, uint64_t& q, uint32_t& r) {
    const uint32_t a = (uint32_t)(x >> 32), b = (uint32_t)x;
    const uint32_t q1 = a / f, r1 = a - q1 * f;
    const uint32_t d2 = (r1 << 16) | (b >> 16);
    const uint32_t q2 = d2 / f, r2 = d2 - q2 * f;
    const uint32_t d3 = (r2 << 16) | (b & 0xffffu);
    const uint32_t q3 = d3 / f;
    r = d3 - q3 * f;
    q = ((uint64_t)q1 << 32) | ((uint64_t)q2 << 16) | (uint64_t)q3;
}

static inline int64_t ar_chunks(int64_t n, int steps) { return (n + (int64_t)AR_LANES * steps - 1) / ((int64_t)AR_LANES * steps); }

// ---- encoder ---------------------------------------------------------------------------------------------------------------------------------
// one chunk of `rows` tokens by one wave: sh = the LDS rows of its table; out: rows words of scratch, of which [top, rows) are written;
// states: the chunk's 64, wcount: its word count, refused: the counter of the tokens that cannot be coded
__device__ __forceinline__ void ar_encode_chunk(const uint32_t* sh, const uint16_t* __restrict__ in_c, const int16_t* __restrict__ in_t, int rows,
                                                uint32_t* __restrict__ out, unsigned long long* __restrict__ states, uint32_t* __restrict__ wcount,
                                                unsigned long long* __restrict__ refused) {
    const int lane = threadIdx.x;
    const int steps = (rows + AR_LANES - 1) / AR_LANES;       // steps that hold a token at all
    int top = rows;
    uint64_t x = AR_L;
    unsigned bad = 0;
    uint32_t cur[AR_BATCH], nxt[AR_BATCH];
    // batch starting at step t0 holds steps t0, t0 - 1, ..; a word is ctx << 16 | token (both as stored); a step without a token for
    // this lane is told from its index, not from the word
#define AR_FETCH(dst, t0)                                                                                 \
    _Pragma("unroll") for (int i = 0; i < AR_BATCH; ++i) {                                                \
        const int r = ((t0) - i) * AR_LANES + lane;                                                       \
        dst[i] = ((t0) - i >= 0 && r < rows) ? ((uint32_t)in_c[r] << 16) | (uint16_t)in_t[r] : 0u;        \
    }
    AR_FETCH(cur, steps - 1)
    for (int t0 = steps - 1; t0 >= 0; t0 -= AR_BATCH) {
        AR_FETCH(nxt, t0 - AR_BATCH)
#pragma unroll
        for (int i = 0; i < AR_BATCH; ++i) {
            const bool here = t0 - i >= 0 && (t0 - i) * AR_LANES + lane < rows;
            const uint32_t cx = cur[i] >> 16, a = cur[i] & 0xffffu;
            const bool inside = cx < (uint32_t)AR_CONTEXTS && a < (uint32_t)AR_TOKENS;
            const uint32_t* row = sh + (inside ? cx : 0u) * AR_ROW + 8 + (inside ? a : 0u);
            const uint32_t c = row[0], e = row[1];
            const uint32_t f = e > c ? e - c : 0u;
            const bool act = here && inside && f != 0u;
            bad += (here && !act) ? 1u : 0u;
            const bool whole = f == 65536u;                                      // identity: x < 2^63 = f << 47 never emits
            const bool emit = act && !whole && x >= ((uint64_t)f << 47);
            const uint64_t m = __ballot(emit);
            const int total = __popcll(m);
            if (emit) {
                out[top - total + ar_lanes_below(m)] = (uint32_t)x;              // >= 0: a token emits one word at most
                x >>= 32;
            }
            top -= total;
            if (act && !whole) {
                uint64_t q; uint32_t r;
                ar_divmod(x, f, q, r);
                x = (q << 16) + r + c;
            }
        }
#pragma unroll
        for (int i = 0; i < AR_BATCH; ++i) cur[i] = nxt[i];
    }
#undef AR_FETCH
    states[lane] = x;
    if (lane == 0) *wcount = (uint32_t)(rows - top);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) bad += __shfl_xor(bad, d, 64);
    if (lane == 0 && bad) atomicAdd(refused, (unsigned long long)bad);           // (integer atomic: the sum does not depend on the order)
}
__global__ void __launch_bounds__(AR_LANES) k_attr_rans_encode(const uint16_t* __restrict__ table, const uint16_t* __restrict__ ctx,
                                                               const int16_t* __restrict__ tokens, int64_t n, int S, uint32_t* __restrict__ scratch,
                                                               unsigned long long* __restrict__ states, uint32_t* __restrict__ wcount,
                                                               unsigned long long* __restrict__ refused) {
    __shared__ __attribute__((aligned(16))) uint32_t sh[AR_CONTEXTS * AR_ROW];
    ar_load_table(sh, table);
    const int64_t k = blockIdx.x, base = k * AR_LANES * S;
    const int rows = (int)(n - base < (int64_t)AR_LANES * S ? n - base : (int64_t)AR_LANES * S);
    ar_encode_chunk(sh, ctx + base, tokens + base, rows, scratch + base, states + k * AR_LANES, wcount + k, refused);
}

// A batch of frames in ONE launch sequence (pcgc_attr_rans_*_batch): chunks never straddle frames, so a workgroup serves one frame and loads
// that frame's table.  The table below travels by value; chunk k of the launch belongs to the last frame f with chunk[f] <= k.
constexpr int AR_MAX_FRAMES = 16;
struct ArFrames {
    long long tok[AR_MAX_FRAMES + 1];          // first token of the frame in the batch's coding order; tok[frames] = all tokens
    long long pay[AR_MAX_FRAMES];              // byte offset of the frame's payload in the payload buffer, a multiple of 8
    long long words[AR_MAX_FRAMES];            // decoder: 32-bit words the frame's payload holds behind its tables
    int chunk[AR_MAX_FRAMES + 1];              // first chunk of the frame; chunk[frames] = all chunks (a frame may have none)
    int steps[AR_MAX_FRAMES];
    int frames;
};
__device__ static inline int ar_frame_of(const ArFrames& fr, int64_t k) {
    int f = 0;
    for (int b = 1; b < AR_MAX_FRAMES; ++b) f += (b < fr.frames && (int64_t)fr.chunk[b] <= k) ? 1 : 0;     // (chunk[] ascends)
    return f;
}
__global__ void __launch_bounds__(AR_LANES) k_attr_rans_encode_batch(const uint16_t* __restrict__ tables, const uint16_t* __restrict__ ctx,
                                                                     const int16_t* __restrict__ tokens, ArFrames fr, uint32_t* __restrict__ scratch,
                                                                     uint8_t* __restrict__ payload, unsigned long long* __restrict__ refused) {
    __shared__ __attribute__((aligned(16))) uint32_t sh[AR_CONTEXTS * AR_ROW];
    const int f = ar_frame_of(fr, blockIdx.x);
    ar_load_table(sh, tables + (size_t)f * AR_CONTEXTS * (AR_TOKENS + 1));
    const int S = fr.steps[f];
    const int64_t k = (int64_t)blockIdx.x - fr.chunk[f], K = fr.chunk[f + 1] - fr.chunk[f], n = fr.tok[f + 1] - fr.tok[f];
    const int64_t base = k * AR_LANES * S;
    const int rows = (int)(n - base < (int64_t)AR_LANES * S ? n - base : (int64_t)AR_LANES * S);
    uint8_t* mine = payload + fr.pay[f];
    ar_encode_chunk(sh, ctx + fr.tok[f] + base, tokens + fr.tok[f] + base, rows, scratch + fr.tok[f] + base,
                    (unsigned long long*)(mine + 8) + k * AR_LANES, (uint32_t*)(mine + 8 + 512 * K) + k, refused + f);
}

// exclusive scan of the chunks' word counts (one block; thread t owns a run of consecutive chunks) -> offs [K] (saturating: counts a decoder
// reads are not to be trusted), slot[0] = their sum.  Encoder side: also the payload's head.
__device__ __forceinline__ void ar_offsets(unsigned long long* part, const uint32_t* __restrict__ wcount, int64_t K, uint32_t* __restrict__ offs,
                                           long long* __restrict__ slot, uint32_t* __restrict__ head, uint32_t S) {
    const int64_t per = (K + AR_SCAN_BLOCK - 1) / AR_SCAN_BLOCK;
    const int64_t lo = (int64_t)threadIdx.x * per < K ? (int64_t)threadIdx.x * per : K, hi = lo + per < K ? lo + per : K;
    unsigned long long s = 0;
    for (int64_t i = lo; i < hi; ++i) s += wcount[i];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long run = 0;
        for (int i = 0; i < AR_SCAN_BLOCK; ++i) { const unsigned long long v = part[i]; part[i] = run; run += v; }
        slot[0] = (long long)run;
        if (head) { head[0] = S; head[1] = (uint32_t)K; }
    }
    __syncthreads();
    unsigned long long run = part[threadIdx.x];
    for (int64_t i = lo; i < hi; ++i) { offs[i] = run < 0xffffffffull ? (uint32_t)run : 0xffffffffu; run += wcount[i]; }
}
__global__ void __launch_bounds__(AR_SCAN_BLOCK) k_attr_rans_offsets(const uint32_t* __restrict__ wcount, int64_t K, uint32_t* __restrict__ offs,
                                                                     long long* __restrict__ slot, uint32_t* __restrict__ head, uint32_t S) {
    __shared__ unsigned long long part[AR_SCAN_BLOCK];
    ar_offsets(part, wcount, K, offs, slot, head, S);
}
// block f: frame f's chunks -> offs [chunk[f] ..) counted from the frame's own first word, slot[f] = the frame's words; a frame without
// chunks has no head (its payload is empty)
__global__ void __launch_bounds__(AR_SCAN_BLOCK) k_attr_rans_offsets_batch(ArFrames fr, uint8_t* payload, uint32_t* __restrict__ offs,
                                                                           long long* __restrict__ slot, int with_head) {
    __shared__ unsigned long long part[AR_SCAN_BLOCK];
    const int f = blockIdx.x;
    const int64_t K = fr.chunk[f + 1] - fr.chunk[f];
    if (K <= 0) { if (threadIdx.x == 0) slot[f] = 0; return; }      // (uniform)
    uint8_t* mine = payload + fr.pay[f];
    ar_offsets(part, (const uint32_t*)(mine + 8 + 512 * K), K, offs + fr.chunk[f], slot + f, with_head ? (uint32_t*)mine : (uint32_t*)nullptr,
               (uint32_t)fr.steps[f]);
}

// chunk k's words, from the end of its scratch to their place in the payload
__global__ void __launch_bounds__(AR_SCAN_BLOCK) k_attr_rans_compact(const uint32_t* __restrict__ scratch, int64_t n, int S, const uint32_t* __restrict__ wcount,
                                                                     const uint32_t* __restrict__ offs, uint32_t* __restrict__ words) {
    const int64_t k = blockIdx.x, base = k * AR_LANES * S;
    const int64_t rows = n - base < (int64_t)AR_LANES * S ? n - base : (int64_t)AR_LANES * S;
    const uint32_t W = wcount[k];                             // <= rows: the encoder wrote it
    const uint32_t* __restrict__ src = scratch + base + rows - W;
    uint32_t* __restrict__ dst = words + offs[k];
    for (uint32_t i = threadIdx.x; i < W; i += AR_SCAN_BLOCK) dst[i] = src[i];
}
__global__ void __launch_bounds__(AR_SCAN_BLOCK) k_attr_rans_compact_batch(const uint32_t* __restrict__ scratch, ArFrames fr, const uint32_t* __restrict__ offs,
                                                                           uint8_t* __restrict__ payload) {
    const int f = ar_frame_of(fr, blockIdx.x);
    const int S = fr.steps[f];
    const int64_t k = (int64_t)blockIdx.x - fr.chunk[f], K = fr.chunk[f + 1] - fr.chunk[f], n = fr.tok[f + 1] - fr.tok[f];
    const int64_t base = k * AR_LANES * S;
    const int64_t rows = n - base < (int64_t)AR_LANES * S ? n - base : (int64_t)AR_LANES * S;
    const uint32_t* wcount = (const uint32_t*)(payload + fr.pay[f] + 8 + 512 * K);
    const uint32_t W = wcount[k];                             // <= rows: the encoder wrote it
    const uint32_t* __restrict__ src = scratch + fr.tok[f] + base + rows - W;
    uint32_t* __restrict__ dst = (uint32_t*)(wcount + K) + offs[blockIdx.x];
    for (uint32_t i = threadIdx.x; i < W; i += AR_SCAN_BLOCK) dst[i] = src[i];
}

// ---- decoder ---------------------------------------------------------------------------------------------------------------------------------
// the context of every token in coding order from the tree's 65 bucket offsets: position p of the order (token 3 p + channel) has split bit
// d = 63 - b, where b is the last bucket with bucket[b] <= p; ctx = 16 channel + min(d / 3, 15)
__global__ void __launch_bounds__(AR_SCAN_BLOCK) k_attr_rans_ctx(const int32_t* __restrict__ bucket, int64_t n, uint16_t* __restrict__ ctx /*[n]*/) {
    __shared__ int32_t sh_b[AR_TOKENS + 1];
    if (threadIdx.x <= AR_TOKENS) sh_b[threadIdx.x] = bucket[threadIdx.x];
    __syncthreads();
    const int64_t p = (int64_t)blockIdx.x * AR_SCAN_BLOCK + threadIdx.x;
    if (3 * p >= n) return;
    int b = 0;
#pragma unroll
    for (int step = 32; step > 0; step >>= 1) b += (b + step <= 63 && (int64_t)sh_b[b + step] <= p) ? step : 0;        // b stays in 0 .. 63
    const int d = 63 - b;
    const uint16_t level = (uint16_t)(d / 3 < 15 ? d / 3 : 15);
    ctx[3 * p] = level;
    if (3 * p + 1 < n) ctx[3 * p + 1] = (uint16_t)(16 + level);
    if (3 * p + 2 < n) ctx[3 * p + 2] = (uint16_t)(32 + level);
}

// one chunk of `rows` tokens by one wave: sh = the LDS rows of its table, ring: AR_RING words of LDS; in / out: the chunk's contexts and
// tokens; states: its 64; W, off: its word count and where its words start among the words_total of `words`
__device__ __forceinline__ void ar_decode_chunk(const uint32_t* sh, uint32_t* ring, const uint16_t* __restrict__ in, int rows,
                                                const unsigned long long* __restrict__ states, uint32_t W, int64_t off,
                                                const uint32_t* __restrict__ words, int64_t words_total, int16_t* __restrict__ out,
                                                unsigned long long* __restrict__ result /*[0] tokens that are 63, [1] unsound chunks*/) {
    const int lane = threadIdx.x;
    const int steps = (rows + AR_LANES - 1) / AR_LANES;
    // the words this chunk may read: [0, avail) of src, inside both its own count and the payload
    const uint32_t avail = off >= words_total ? 0u : (uint32_t)((int64_t)W < words_total - off ? (int64_t)W : words_total - off);
    const uint32_t* __restrict__ src = words + (off < words_total ? off : 0);
    uint64_t x = states[lane];
    bool bad = x < AR_L || x >= AR_STATE_END || avail != W;
    uint32_t pos = 0, filled = 0;                             // stream indices: the ring holds [pos, filled)
    uint32_t stage[AR_BATCH];                                 // words [filled, filled + AR_FILL), on their way
#define AR_STAGE(from)                                                                        \
    _Pragma("unroll") for (int i = 0; i < AR_BATCH; ++i) {                                    \
        const uint32_t idx = (from) + (uint32_t)(i * AR_LANES + lane);                        \
        stage[i] = idx < avail ? src[idx] : 0u;                                               \
    }
#define AR_FETCH(dst, t0)                                                                     \
    _Pragma("unroll") for (int i = 0; i < AR_BATCH; ++i) {                                    \
        const int r = ((t0) + i) * AR_LANES + lane;                                           \
        dst[i] = r < rows ? (uint32_t)in[r] : AR_NONE;                                        \
    }
    AR_STAGE(0u)
    uint32_t cur[AR_BATCH], nxt[AR_BATCH];
    AR_FETCH(cur, 0)
    unsigned escapes = 0;
    for (int t0 = 0; t0 < steps; t0 += AR_BATCH) {
        AR_FETCH(nxt, t0 + AR_BATCH)
        if (filled - pos < (uint32_t)AR_FILL) {               // (uniform) the slots written held words below pos: filled - pos <= RING - FILL
#pragma unroll
            for (int i = 0; i < AR_BATCH; ++i) ring[(filled + (uint32_t)(i * AR_LANES + lane)) & (AR_RING - 1)] = stage[i];
            filled += AR_FILL;
            AR_STAGE(filled)
            __syncthreads();
        }
        // level 1 of the batch's searches: rows and pivots follow from the contexts alone
        uint32_t rowat[AR_BATCH];
        uint4 pa[AR_BATCH], pb[AR_BATCH];
#pragma unroll
        for (int i = 0; i < AR_BATCH; ++i) {
            const uint32_t cx = cur[i] < (uint32_t)AR_CONTEXTS ? cur[i] : 0u;    // (a context outside the table cannot come from k_attr_rans_ctx; clamp it all the same)
            rowat[i] = cx * AR_ROW;
            pa[i] = *(const uint4*)(sh + rowat[i]);
            pb[i] = *(const uint4*)(sh + rowat[i] + 4);
        }
#pragma unroll
        for (int i = 0; i < AR_BATCH; ++i) {
            const bool act = cur[i] != AR_NONE;
            const uint32_t s = (uint32_t)x & 0xffffu;
            const uint32_t piv[8] = {pa[i].x, pa[i].y, pa[i].z, pa[i].w, pb[i].x, pb[i].y, pb[i].z, pb[i].w};
            uint32_t g = 0, above = 65536u;                                      // group of eight; smallest pivot > s
#pragma unroll
            for (int j = 0; j < 7; ++j) {
                const bool le = piv[j] <= s;
                g += le ? 1u : 0u;
                above = min(above, le ? 65536u : piv[j]);
            }
            const uint4 ea = *(const uint4*)(sh + rowat[i] + 8 + 8 * g);         // g <= 7: inside the row
            const uint4 eb = *(const uint4*)(sh + rowat[i] + 12 + 8 * g);
            const uint32_t e[8] = {ea.x, ea.y, ea.z, ea.w, eb.x, eb.y, eb.z, eb.w};
            uint32_t r = 0, c = e[0] <= s ? e[0] : 0u;                           // e[0] = cdf[8 g] <= s in a monotone row
#pragma unroll
            for (int j = 1; j < 8; ++j) {
                const bool le = e[j] <= s;
                r += le ? 1u : 0u;
                c = max(c, le ? e[j] : 0u);
                above = min(above, le ? 65536u : e[j]);
            }
            const uint32_t a = 8 * g + r;                                        // 0 .. 63
            const uint32_t f = above - c;                                        // 1 .. 65536 in a monotone row
            if (act) x = (uint64_t)f * (x >> 16) + s - c;
            const bool need = act && x < AR_L;
            const uint64_t m = __ballot(need);
            if (need) x = (x << 32) | ring[(pos + (uint32_t)ar_lanes_below(m)) & (AR_RING - 1)];
            pos += (uint32_t)__popcll(m);
            if (act) { out[(t0 + i) * AR_LANES + lane] = (int16_t)a; escapes += a == 63u ? 1u : 0u; }
        }
#pragma unroll
        for (int i = 0; i < AR_BATCH; ++i) cur[i] = nxt[i];
    }
#undef AR_FETCH
#undef AR_STAGE
    bad = bad || x != AR_L || pos != W;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) escapes += __shfl_xor(escapes, d, 64);
    const bool any_bad = __ballot(bad) != 0;
    if (lane == 0) {                                          // (integer atomics: the sums do not depend on the order)
        atomicAdd(result, (unsigned long long)escapes);
        if (any_bad) atomicAdd(result + 1, 1ull);
    }
}
__global__ void __launch_bounds__(AR_LANES) k_attr_rans_decode(const uint16_t* __restrict__ table, const uint16_t* __restrict__ ctx, int64_t n, int S,
                                                               const unsigned long long* __restrict__ states, const uint32_t* __restrict__ wcount,
                                                               const uint32_t* __restrict__ offs, const uint32_t* __restrict__ words,
                                                               int64_t words_total, int16_t* __restrict__ tokens,
                                                               unsigned long long* __restrict__ result /*[0] tokens that are 63, [1] unsound chunks*/) {
    __shared__ __attribute__((aligned(16))) uint32_t sh[AR_CONTEXTS * AR_ROW];
    __shared__ uint32_t ring[AR_RING];
    ar_load_table(sh, table);
    const int64_t k = blockIdx.x, base = k * AR_LANES * S;
    const int rows = (int)(n - base < (int64_t)AR_LANES * S ? n - base : (int64_t)AR_LANES * S);
    ar_decode_chunk(sh, ring, ctx + base, rows, states + k * AR_LANES, wcount[k], (int64_t)offs[k], words, words_total, tokens + base, result);
}

// the contexts of a batch: position p of the batch's coding order lies in the last frame f with tok[f] <= 3 p, at position p - tok[f] / 3 of
// that frame's own order, whose 65 offsets are row f of bucket [frames, 65]
__global__ void __launch_bounds__(AR_SCAN_BLOCK) k_attr_rans_ctx_batch(const int32_t* __restrict__ bucket, ArFrames fr, uint16_t* __restrict__ ctx) {
    const int64_t p = (int64_t)blockIdx.x * AR_SCAN_BLOCK + threadIdx.x;
    if (3 * p >= fr.tok[fr.frames]) return;
    int f = 0;
    for (int b = 1; b < AR_MAX_FRAMES; ++b) f += (b < fr.frames && fr.tok[b] <= 3 * p) ? 1 : 0;
    const int32_t* __restrict__ row = bucket + f * (AR_TOKENS + 1);
    const int64_t q = p - fr.tok[f] / 3;
    int b = 0;
#pragma unroll
    for (int step = 32; step > 0; step >>= 1) b += (b + step <= 63 && (int64_t)row[b + step] <= q) ? step : 0;         // b stays in 0 .. 63
    const int d = 63 - b;
    const uint16_t level = (uint16_t)(d / 3 < 15 ? d / 3 : 15);
    ctx[3 * p] = level; ctx[3 * p + 1] = (uint16_t)(16 + level); ctx[3 * p + 2] = (uint16_t)(32 + level);          // (tok[] are multiples of 3)
}
// result [2 f], [2 f + 1]: frame f's tokens that are 63 and its unsound chunks
__global__ void __launch_bounds__(AR_LANES) k_attr_rans_decode_batch(const uint16_t* __restrict__ tables, const uint16_t* __restrict__ ctx, ArFrames fr,
                                                                     const uint8_t* __restrict__ payload, const uint32_t* __restrict__ offs,
                                                                     int16_t* __restrict__ tokens, unsigned long long* __restrict__ result) {
    __shared__ __attribute__((aligned(16))) uint32_t sh[AR_CONTEXTS * AR_ROW];
    __shared__ uint32_t ring[AR_RING];
    const int f = ar_frame_of(fr, blockIdx.x);
    ar_load_table(sh, tables + (size_t)f * AR_CONTEXTS * (AR_TOKENS + 1));
    const int S = fr.steps[f];
    const int64_t k = (int64_t)blockIdx.x - fr.chunk[f], K = fr.chunk[f + 1] - fr.chunk[f], n = fr.tok[f + 1] - fr.tok[f];
    const int64_t base = k * AR_LANES * S;
    const int rows = (int)(n - base < (int64_t)AR_LANES * S ? n - base : (int64_t)AR_LANES * S);
    const uint8_t* mine = payload + fr.pay[f];
    const uint32_t* wcount = (const uint32_t*)(mine + 8 + 512 * K);
    ar_decode_chunk(sh, ring, ctx + fr.tok[f] + base, rows, (const unsigned long long*)(mine + 8) + k * AR_LANES, wcount[k],
                    (int64_t)offs[blockIdx.x], wcount + K, fr.words[f], tokens + fr.tok[f] + base, result + 2 * f);
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------------
// workspace: [slot: 4 x int64][offs: K x u32, padded to 8 bytes][encoder: scratch, n x u32 | decoder: contexts, n x u16]
static size_t ar_offs_bytes(int64_t K) { return (size_t)((K * 4 + 7) / 8 * 8); }

extern "C" int64_t pcgc_attr_rans_workspace_bytes(int64_t n, int steps) {
    if (n < 0) n = 0;
    if (steps < 1) steps = 1;
    return 32 + (int64_t)ar_offs_bytes(ar_chunks(n, steps)) + n * 4 + 64;
}

static long long* ar_host_slot() {
    static thread_local long long* host = nullptr;
    if (!host && hipHostMalloc((void**)&host, 64, hipHostMallocDefault) != hipSuccess) host = nullptr;
    return host;
}

extern "C" int pcgc_attr_rans_encode(const uint16_t* table, const uint16_t* ctx, const int16_t* tokens, int64_t n, int steps, uint8_t* payload,
                                     size_t payload_capacity, int64_t* host2, void* workspace, size_t workspace_bytes, void* stream) {
    PCGC_REQUIRE(n >= 1 && n < ((int64_t)1 << 31), "bad token count");
    PCGC_REQUIRE(steps >= 1 && steps <= AR_MAX_STEPS, "steps per chunk outside 1 .. 2^24");
    PCGC_REQUIRE(table && ctx && tokens && payload && host2, "null argument");
    const int64_t K = ar_chunks(n, steps);
    PCGC_REQUIRE(payload_capacity >= (size_t)(8 + 516 * K + 4 * n) && ((uintptr_t)payload & 7) == 0, "payload buffer too small or misaligned");
    PCGC_REQUIRE(workspace && workspace_bytes >= (size_t)pcgc_attr_rans_workspace_bytes(n, steps) && ((uintptr_t)workspace & 7) == 0, "workspace too small or misaligned");
    long long* slot = (long long*)workspace;
    uint32_t* offs = (uint32_t*)((char*)workspace + 32);
    uint32_t* scratch = (uint32_t*)((char*)workspace + 32 + ar_offs_bytes(K));
    unsigned long long* states = (unsigned long long*)(payload + 8);
    uint32_t* wcount = (uint32_t*)(payload + 8 + 512 * K);
    uint32_t* words = wcount + K;
    long long* host = ar_host_slot();
    if (!host) { pcgc_set_error("attr_rans_encode: cannot allocate pinned memory"); return -1; }
    hipError_t e = hipMemsetAsync(slot, 0, 32, S(stream));
    if (e != hipSuccess) { pcgc_set_error("attr_rans_encode: %s", hipGetErrorString(e)); return -1; }
    hipLaunchKernelGGL(k_attr_rans_encode, dim3((unsigned)K), dim3(AR_LANES), 0, S(stream), table, ctx, tokens, n, steps, scratch, states, wcount,
                       (unsigned long long*)(slot + 1));
    PCGC_CHECK_LAUNCH("attr_rans_encode");
    hipLaunchKernelGGL(k_attr_rans_offsets, dim3(1), dim3(AR_SCAN_BLOCK), 0, S(stream), (const uint32_t*)wcount, K, offs, slot, (uint32_t*)payload, (uint32_t)steps);
    PCGC_CHECK_LAUNCH("attr_rans_encode");
    hipLaunchKernelGGL(k_attr_rans_compact, dim3((unsigned)K), dim3(AR_SCAN_BLOCK), 0, S(stream), (const uint32_t*)scratch, n, steps, (const uint32_t*)wcount,
                       (const uint32_t*)offs, words);
    PCGC_CHECK_LAUNCH("attr_rans_encode");
    e = hipMemcpyAsync(host, slot, 2 * sizeof(long long), hipMemcpyDeviceToHost, S(stream));
    if (e == hipSuccess) e = hipStreamSynchronize(S(stream));
    if (e != hipSuccess) { pcgc_set_error("attr_rans_encode: %s", hipGetErrorString(e)); return -1; }
    host2[0] = 8 + 516 * K + 4 * (int64_t)host[0];
    host2[1] = (int64_t)host[1];
    return 0;
}

extern "C" int pcgc_attr_rans_decode(const uint16_t* table, const int32_t* bucket, int64_t n, const uint8_t* payload, int64_t payload_bytes, int steps,
                                     int16_t* tokens, int64_t* host2, void* workspace, size_t workspace_bytes, void* stream) {
    PCGC_REQUIRE(n >= 1 && n < ((int64_t)1 << 31), "bad token count");
    PCGC_REQUIRE(table && bucket && tokens && payload && host2, "null argument");
    PCGC_REQUIRE(((uintptr_t)payload & 7) == 0, "payload misaligned");
    PCGC_REQUIRE(steps >= 1 && steps <= AR_MAX_STEPS, "steps per chunk outside 1 .. 2^24");
    long long* host = ar_host_slot();
    if (!host) { pcgc_set_error("attr_rans_decode: cannot allocate pinned memory"); return -1; }
    const int64_t K = ar_chunks(n, steps);            // (the head's own S and K are the caller's to compare: ops.attr_rans_decode)
    PCGC_REQUIRE(payload_bytes >= 8 + 516 * K && (payload_bytes - 8 - 516 * K) % 4 == 0, "payload cut inside its tables or not whole words");
    const int64_t words_total = (payload_bytes - 8 - 516 * K) / 4;
    PCGC_REQUIRE(workspace && workspace_bytes >= (size_t)pcgc_attr_rans_workspace_bytes(n, steps) && ((uintptr_t)workspace & 7) == 0, "workspace too small or misaligned");
    long long* slot = (long long*)workspace;
    uint32_t* offs = (uint32_t*)((char*)workspace + 32);
    uint16_t* ctx = (uint16_t*)((char*)workspace + 32 + ar_offs_bytes(K));
    const unsigned long long* states = (const unsigned long long*)(payload + 8);
    const uint32_t* wcount = (const uint32_t*)(payload + 8 + 512 * K);
    const uint32_t* words = wcount + K;
    hipError_t e = hipMemsetAsync(slot, 0, 32, S(stream));
    if (e != hipSuccess) { pcgc_set_error("attr_rans_decode: %s", hipGetErrorString(e)); return -1; }
    hipLaunchKernelGGL(k_attr_rans_ctx, dim3(grid_for((n + 2) / 3, AR_SCAN_BLOCK)), dim3(AR_SCAN_BLOCK), 0, S(stream), bucket, n, ctx);
    PCGC_CHECK_LAUNCH("attr_rans_decode");
    hipLaunchKernelGGL(k_attr_rans_offsets, dim3(1), dim3(AR_SCAN_BLOCK), 0, S(stream), wcount, K, offs, slot, (uint32_t*)nullptr, 0u);
    PCGC_CHECK_LAUNCH("attr_rans_decode");
    hipLaunchKernelGGL(k_attr_rans_decode, dim3((unsigned)K), dim3(AR_LANES), 0, S(stream), table, (const uint16_t*)ctx, n, steps, states, wcount,
                       (const uint32_t*)offs, words, words_total, tokens, (unsigned long long*)(slot + 1));
    PCGC_CHECK_LAUNCH("attr_rans_decode");
    e = hipMemcpyAsync(host, slot, 3 * sizeof(long long), hipMemcpyDeviceToHost, S(stream));
    if (e == hipSuccess) e = hipStreamSynchronize(S(stream));
    if (e != hipSuccess) { pcgc_set_error("attr_rans_decode: %s", hipGetErrorString(e)); return -1; }
    host2[0] = (int64_t)host[1];
    host2[1] = (int64_t)host[2] + (host[0] != words_total ? 1 : 0);      // unsound chunks (+ 1: the word counts do not add up to the payload)
    return 0;
}

// ---- a batch of frames ------------------------------------------------------------------------------------------------------------------------
// workspace: [slot: 64 x int64 = words per frame [16], then the encoder's refused tokens per frame [16] or the decoder's result [32]]
//            [offs: K x u32, padded to 8 bytes][encoder: scratch, n x u32 | decoder: contexts, n x u16]
extern "C" int64_t pcgc_attr_rans_batch_workspace_bytes(int64_t n, int64_t chunks) {
    if (n < 0) n = 0;
    if (chunks < 0) chunks = 0;
    return 512 + (int64_t)ar_offs_bytes(chunks) + n * 4 + 64;
}
static long long* ar_host_slot_batch() {
    static thread_local long long* host = nullptr;
    if (!host && hipHostMalloc((void**)&host, 512, hipHostMallocDefault) != hipSuccess) host = nullptr;
    return host;
}
// fills fr from the host arrays; false when they are not a batch: tok ascending multiples of 3 from 0, steps in range, K_f chunks each
static bool ar_frames_of(int frames, const int64_t* tok, const int32_t* steps, const int64_t* pay, ArFrames& fr, bool all) {
    memset(&fr, 0, sizeof(fr));
    if (frames < 1 || frames > AR_MAX_FRAMES || !tok || !steps || !pay || tok[0] != 0) return false;
    fr.frames = frames;
    int64_t K = 0;
    for (int f = 0; f < frames; ++f) {
        const int64_t n = tok[f + 1] - tok[f];
        if (n < 0 || n % 3 || tok[f + 1] >= ((int64_t)1 << 31) || steps[f] < 0 || steps[f] > AR_MAX_STEPS || (pay[f] & 7) || pay[f] < 0) return false;
        if (all && n > 0 && steps[f] < 1) return false;
        fr.tok[f] = tok[f]; fr.pay[f] = pay[f]; fr.steps[f] = steps[f]; fr.chunk[f] = (int)K;
        K += (n > 0 && steps[f] > 0) ? ar_chunks(n, steps[f]) : 0;
        if (K >= ((int64_t)1 << 31)) return false;
    }
    for (int f = frames; f <= AR_MAX_FRAMES; ++f) { fr.tok[f] = tok[frames]; fr.chunk[f] = (int)K; }
    return true;
}

extern "C" int pcgc_attr_rans_encode_batch(const uint16_t* tables, const uint16_t* ctx, const int16_t* tokens, int frames, const int64_t* tok,
                                           const int32_t* steps, uint8_t* payload, const int64_t* pay, int64_t* host, void* workspace,
                                           size_t workspace_bytes, void* stream) {
    ArFrames fr;
    PCGC_REQUIRE(ar_frames_of(frames, tok, steps, pay, fr, true), "1 to 16 frames; token offsets ascending multiples of 3 below 2^31; steps per chunk 1 .. 2^24; payload offsets multiples of 8");
    PCGC_REQUIRE(tables && ctx && tokens && payload && host && ((uintptr_t)payload & 7) == 0, "null or misaligned argument");
    const int64_t n = fr.tok[frames], K = fr.chunk[frames];
    PCGC_REQUIRE(n >= 1, "no token: nothing to launch");
    for (int f = 0; f < frames; ++f)
        PCGC_REQUIRE(pay[f + 1] - pay[f] >= (fr.chunk[f + 1] > fr.chunk[f] ? 8 + 516 * (int64_t)(fr.chunk[f + 1] - fr.chunk[f]) + 4 * (tok[f + 1] - tok[f]) : 0),
                     "payload room of a frame below 8 + 516 K + 4 n bytes");
    PCGC_REQUIRE(workspace && workspace_bytes >= (size_t)pcgc_attr_rans_batch_workspace_bytes(n, K) && ((uintptr_t)workspace & 7) == 0, "workspace too small or misaligned");
    long long* slot = (long long*)workspace;
    uint32_t* offs = (uint32_t*)((char*)workspace + 512);
    uint32_t* scratch = (uint32_t*)((char*)workspace + 512 + ar_offs_bytes(K));
    long long* hostslot = ar_host_slot_batch();
    if (!hostslot) { pcgc_set_error("attr_rans_encode_batch: cannot allocate pinned memory"); return -1; }
    hipError_t e = hipMemsetAsync(slot, 0, 512, S(stream));
    if (e != hipSuccess) { pcgc_set_error("attr_rans_encode_batch: %s", hipGetErrorString(e)); return -1; }
    hipLaunchKernelGGL(k_attr_rans_encode_batch, dim3((unsigned)K), dim3(AR_LANES), 0, S(stream), tables, ctx, tokens, fr, scratch, payload,
                       (unsigned long long*)(slot + AR_MAX_FRAMES));
    PCGC_CHECK_LAUNCH("attr_rans_encode_batch");
    hipLaunchKernelGGL(k_attr_rans_offsets_batch, dim3((unsigned)frames), dim3(AR_SCAN_BLOCK), 0, S(stream), fr, payload, offs, slot, 1);
    PCGC_CHECK_LAUNCH("attr_rans_encode_batch");
    hipLaunchKernelGGL(k_attr_rans_compact_batch, dim3((unsigned)K), dim3(AR_SCAN_BLOCK), 0, S(stream), (const uint32_t*)scratch, fr, (const uint32_t*)offs, payload);
    PCGC_CHECK_LAUNCH("attr_rans_encode_batch");
    e = hipMemcpyAsync(hostslot, slot, 2 * AR_MAX_FRAMES * sizeof(long long), hipMemcpyDeviceToHost, S(stream));
    if (e == hipSuccess) e = hipStreamSynchronize(S(stream));
    if (e != hipSuccess) { pcgc_set_error("attr_rans_encode_batch: %s", hipGetErrorString(e)); return -1; }
    for (int f = 0; f < frames; ++f) {
        const int64_t Kf = fr.chunk[f + 1] - fr.chunk[f];
        host[f] = Kf ? 8 + 516 * Kf + 4 * (int64_t)hostslot[f] : 0;
        host[frames + f] = (int64_t)hostslot[AR_MAX_FRAMES + f];
    }
    return 0;
}

extern "C" int pcgc_attr_rans_decode_batch(const uint16_t* tables, const int32_t* bucket, int frames, const int64_t* tok, const int32_t* steps,
                                           const uint8_t* payload, const int64_t* pay, const int64_t* pay_bytes, int16_t* tokens, int64_t* host,
                                           void* workspace, size_t workspace_bytes, void* stream) {
    ArFrames fr;
    PCGC_REQUIRE(ar_frames_of(frames, tok, steps, pay, fr, false), "1 to 16 frames; token offsets ascending multiples of 3 below 2^31; steps per chunk 0 .. 2^24; payload offsets multiples of 8");
    PCGC_REQUIRE(tables && bucket && tokens && payload && pay_bytes && host && ((uintptr_t)payload & 7) == 0, "null or misaligned argument");
    const int64_t n = fr.tok[frames], K = fr.chunk[frames];
    PCGC_REQUIRE(n >= 1 && K >= 1, "no chunk: nothing to launch");
    for (int f = 0; f < frames; ++f) {
        const int64_t Kf = fr.chunk[f + 1] - fr.chunk[f];
        if (!Kf) continue;
        PCGC_REQUIRE(pay_bytes[f] >= 8 + 516 * Kf && (pay_bytes[f] - 8 - 516 * Kf) % 4 == 0, "a payload cut inside its tables or not whole words");
        fr.words[f] = (pay_bytes[f] - 8 - 516 * Kf) / 4;
    }
    PCGC_REQUIRE(workspace && workspace_bytes >= (size_t)pcgc_attr_rans_batch_workspace_bytes(n, K) && ((uintptr_t)workspace & 7) == 0, "workspace too small or misaligned");
    long long* slot = (long long*)workspace;
    uint32_t* offs = (uint32_t*)((char*)workspace + 512);
    uint16_t* ctx = (uint16_t*)((char*)workspace + 512 + ar_offs_bytes(K));
    long long* hostslot = ar_host_slot_batch();
    if (!hostslot) { pcgc_set_error("attr_rans_decode_batch: cannot allocate pinned memory"); return -1; }
    hipError_t e = hipMemsetAsync(slot, 0, 512, S(stream));
    if (e != hipSuccess) { pcgc_set_error("attr_rans_decode_batch: %s", hipGetErrorString(e)); return -1; }
    hipLaunchKernelGGL(k_attr_rans_ctx_batch, dim3(grid_for(n / 3, AR_SCAN_BLOCK)), dim3(AR_SCAN_BLOCK), 0, S(stream), bucket, fr, ctx);
    PCGC_CHECK_LAUNCH("attr_rans_decode_batch");
    hipLaunchKernelGGL(k_attr_rans_offsets_batch, dim3((unsigned)frames), dim3(AR_SCAN_BLOCK), 0, S(stream), fr, const_cast<uint8_t*>(payload), offs, slot, 0);
    PCGC_CHECK_LAUNCH("attr_rans_decode_batch");
    hipLaunchKernelGGL(k_attr_rans_decode_batch, dim3((unsigned)K), dim3(AR_LANES), 0, S(stream), tables, (const uint16_t*)ctx, fr, payload,
                       (const uint32_t*)offs, tokens, (unsigned long long*)(slot + AR_MAX_FRAMES));
    PCGC_CHECK_LAUNCH("attr_rans_decode_batch");
    e = hipMemcpyAsync(hostslot, slot, 3 * AR_MAX_FRAMES * sizeof(long long), hipMemcpyDeviceToHost, S(stream));
    if (e == hipSuccess) e = hipStreamSynchronize(S(stream));
    if (e != hipSuccess) { pcgc_set_error("attr_rans_decode_batch: %s", hipGetErrorString(e)); return -1; }
    for (int f = 0; f < frames; ++f) {
        const bool here = fr.chunk[f + 1] > fr.chunk[f];
        host[f] = here ? (int64_t)hostslot[AR_MAX_FRAMES + 2 * f] : 0;
        host[frames + f] = here ? (int64_t)hostslot[AR_MAX_FRAMES + 2 * f + 1] + (hostslot[f] != fr.words[f] ? 1 : 0) : 0;
    }
    return 0;
}
