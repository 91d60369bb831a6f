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
// A batch of frames (pcgc_attr_rans_*_batch) is one launch of the chunks of all frames: a workgroup serves one frame's chunk
// with that frame's table, and every frame's payload is packed on its own.  A SINGLE FRAME IS THE BATCH OF ONE: there is one kernel per step
// (encode, offsets, compact, contexts, decode) over an ArFrames, one workspace layout and one pinned slot; pcgc_attr_rans_encode / _decode
// build the ArFrames of one frame (of any length: only the batch entries demand token counts in multiples of 3) and run the same bodies.
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
// A batch of frames in ONE launch sequence; a single frame is the batch of one (frames = 1, tok = {0, n}, pay = {0}).  Chunks never straddle
// frames, so a workgroup serves one frame and loads that frame's table.  The table below travels by value; chunk k of the launch belongs to
// the last frame f with chunk[f] <= k.
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
// chunk blockIdx.x of the launch: its frame f, the frame's S, K and tokens, the chunk's place k in the frame, its first token and its rows
struct ArChunk { int f, S, rows; int64_t k, K, base; };
__device__ static inline ArChunk ar_chunk_of(const ArFrames& fr) {
    ArChunk c;
    c.f = ar_frame_of(fr, blockIdx.x);
    c.S = fr.steps[c.f];
    c.k = (int64_t)blockIdx.x - fr.chunk[c.f];
    c.K = fr.chunk[c.f + 1] - fr.chunk[c.f];
    const int64_t n = fr.tok[c.f + 1] - fr.tok[c.f], in_frame = c.k * AR_LANES * c.S;
    c.rows = (int)(n - in_frame < (int64_t)AR_LANES * c.S ? n - in_frame : (int64_t)AR_LANES * c.S);
    c.base = fr.tok[c.f] + in_frame;
    return c;
}
// (a frame's payload: head [8 bytes], states [K x 64 x u64], word counts [K x u32], words)
__global__ void __launch_bounds__(AR_LANES) k_attr_rans_encode(const uint16_t* __restrict__ tables, const uint16_t* __restrict__ ctx,
                                                               const int16_t* __restrict__ tokens, ArFrames fr, uint32_t* __restrict__ scratch,
                                                               uint8_t* __restrict__ payload, unsigned long long* __restrict__ refused) {
    __shared__ __attribute__((aligned(16))) uint32_t sh[AR_CONTEXTS * AR_ROW];
    const ArChunk c = ar_chunk_of(fr);
    ar_load_table(sh, tables + (size_t)c.f * AR_CONTEXTS * (AR_TOKENS + 1));
    uint8_t* mine = payload + fr.pay[c.f];
    ar_encode_chunk(sh, ctx + c.base, tokens + c.base, c.rows, scratch + c.base, (unsigned long long*)(mine + 8) + c.k * AR_LANES,
                    (uint32_t*)(mine + 8 + 512 * c.K) + c.k, refused + c.f);
}

// block f: an exclusive scan of the word counts of frame f's chunks (thread t owns a run of consecutive chunks) -> offs [chunk[f] ..) counted
// from the frame's own first word (saturating: counts a decoder reads are not to be trusted), slot[f] = the frame's words.  Encoder side
// (with_head): also the payload's head; a frame without chunks has none (its payload is empty).
__global__ void __launch_bounds__(AR_SCAN_BLOCK) k_attr_rans_offsets(ArFrames fr, uint8_t* payload, uint32_t* __restrict__ offs,
                                                                     long long* __restrict__ slot, int with_head) {
    __shared__ unsigned long long part[AR_SCAN_BLOCK];
    const int f = blockIdx.x;
    const int64_t K = fr.chunk[f + 1] - fr.chunk[f];
    if (K <= 0) { if (threadIdx.x == 0) slot[f] = 0; return; }      // (uniform)
    uint8_t* mine = payload + fr.pay[f];
    const uint32_t* __restrict__ wcount = (const uint32_t*)(mine + 8 + 512 * K);
    offs += fr.chunk[f];
    const int64_t per = (K + AR_SCAN_BLOCK - 1) / AR_SCAN_BLOCK;
    const int64_t lo = (int64_t)threadIdx.x * per < K ? (int64_t)threadIdx.x * per : K, hi = lo + per < K ? lo + per : K;
    unsigned long long s = 0;
    for (int64_t i = lo; i < hi; ++i) s += wcount[i];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long run = 0;
        for (int i = 0; i < AR_SCAN_BLOCK; ++i) { const unsigned long long v = part[i]; part[i] = run; run += v; }
        slot[f] = (long long)run;
        if (with_head) { ((uint32_t*)mine)[0] = (uint32_t)fr.steps[f]; ((uint32_t*)mine)[1] = (uint32_t)K; }
    }
    __syncthreads();
    unsigned long long run = part[threadIdx.x];
    for (int64_t i = lo; i < hi; ++i) { offs[i] = run < 0xffffffffull ? (uint32_t)run : 0xffffffffu; run += wcount[i]; }
}

// a chunk's words, from the end of its scratch to their place in its frame's payload
__global__ void __launch_bounds__(AR_SCAN_BLOCK) k_attr_rans_compact(const uint32_t* __restrict__ scratch, ArFrames fr, const uint32_t* __restrict__ offs,
                                                                     uint8_t* __restrict__ payload) {
    const ArChunk c = ar_chunk_of(fr);
    const uint32_t* wcount = (const uint32_t*)(payload + fr.pay[c.f] + 8 + 512 * c.K);
    const uint32_t W = wcount[c.k];                           // <= rows: the encoder wrote it
    const uint32_t* __restrict__ src = scratch + c.base + c.rows - W;
    uint32_t* __restrict__ dst = (uint32_t*)(wcount + c.K) + offs[blockIdx.x];
    for (uint32_t i = threadIdx.x; i < W; i += AR_SCAN_BLOCK) dst[i] = src[i];
}

// ---- decoder ---------------------------------------------------------------------------------------------------------------------------------
// the context of every token in coding order from the trees' bucket offsets: position p of the coding order (token 3 p + channel) lies in
// the last frame f with tok[f] <= 3 p, at position q = p - tok[f] / 3 of that frame's own order, whose 65 offsets are row f of bucket
// [frames, 65]; its split bit is d = 63 - b, where b is the last bucket with row[b] <= q; ctx = 16 channel + min(d / 3, 15).  tok[] of the
// frames of a batch are multiples of 3; the last position of a single frame may hold fewer than three tokens, so the tail stores are guarded.
__global__ void __launch_bounds__(AR_SCAN_BLOCK) k_attr_rans_ctx(const int32_t* __restrict__ bucket, ArFrames fr, uint16_t* __restrict__ ctx) {
    const int64_t p = (int64_t)blockIdx.x * AR_SCAN_BLOCK + threadIdx.x, n = fr.tok[fr.frames];
    if (3 * p >= n) return;
    int f = 0;
    for (int b = 1; b < AR_MAX_FRAMES; ++b) f += (b < fr.frames && fr.tok[b] <= 3 * p) ? 1 : 0;
    const int32_t* __restrict__ row = bucket + f * (AR_TOKENS + 1);
    const int64_t q = p - fr.tok[f] / 3;
    int b = 0;
#pragma unroll
    for (int step = 32; step > 0; step >>= 1) b += (b + step <= 63 && (int64_t)row[b + step] <= q) ? step : 0;         // b stays in 0 .. 63
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
// result [2 f], [2 f + 1]: frame f's tokens that are 63 and its unsound chunks
__global__ void __launch_bounds__(AR_LANES) k_attr_rans_decode(const uint16_t* __restrict__ tables, const uint16_t* __restrict__ ctx, ArFrames fr,
                                                               const uint8_t* __restrict__ payload, const uint32_t* __restrict__ offs,
                                                               int16_t* __restrict__ tokens, unsigned long long* __restrict__ result) {
    __shared__ __attribute__((aligned(16))) uint32_t sh[AR_CONTEXTS * AR_ROW];
    __shared__ uint32_t ring[AR_RING];
    const ArChunk c = ar_chunk_of(fr);
    ar_load_table(sh, tables + (size_t)c.f * AR_CONTEXTS * (AR_TOKENS + 1));
    const uint8_t* mine = payload + fr.pay[c.f];
    const uint32_t* wcount = (const uint32_t*)(mine + 8 + 512 * c.K);
    ar_decode_chunk(sh, ring, ctx + c.base, c.rows, (const unsigned long long*)(mine + 8) + c.k * AR_LANES, wcount[c.k], (int64_t)offs[blockIdx.x],
                    wcount + c.K, fr.words[c.f], tokens + c.base, result + 2 * c.f);
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------------
// The batch entries and the single ones run the same two bodies below over an ArFrames; a single entry builds the ArFrames of one frame and
// translates the body's per-frame answers into its documented host2.
// workspace: [slot: 64 x int64 = words per frame [16], then the encoder's refused tokens per frame [16] or the decoder's result [32]]
//            [offs: K x u32, padded to 8 bytes][encoder: scratch, n x u32 | decoder: contexts, n x u16]
constexpr size_t AR_SLOT_BYTES = 4 * AR_MAX_FRAMES * sizeof(long long);
static size_t ar_offs_bytes(int64_t K) { return (size_t)((K * 4 + 7) / 8 * 8); }

extern "C" int64_t pcgc_attr_rans_batch_workspace_bytes(int64_t n, int64_t chunks) {
    if (n < 0) n = 0;
    if (chunks < 0) chunks = 0;
    return (int64_t)AR_SLOT_BYTES + (int64_t)ar_offs_bytes(chunks) + n * 4 + 64;
}
extern "C" int64_t pcgc_attr_rans_workspace_bytes(int64_t n, int steps) {
    if (n < 0) n = 0;
    if (steps < 1) steps = 1;
    return pcgc_attr_rans_batch_workspace_bytes(n, ar_chunks(n, steps));
}

#define AR_REQUIRE(who, cond, msg) do { if (!(cond)) { pcgc_set_error("%s: %s", who, msg); return -2; } } while (0)
#define AR_CHECK_HIP(who, e) do { if ((e) != hipSuccess) { pcgc_set_error("%s: %s", (who) + 5, hipGetErrorString(e)); return -1; } } while (0)

// fills fr from the host arrays; false when they are not a batch: tok ascending from 0 (thirds, the batch entries' own demand: in multiples
// of 3), steps in range, K_f chunks each
static bool ar_frames_of(int frames, const int64_t* tok, const int32_t* steps, const int64_t* pay, ArFrames& fr, bool all, bool thirds) {
    memset(&fr, 0, sizeof(fr));
    if (frames < 1 || frames > AR_MAX_FRAMES || !tok || !steps || !pay || tok[0] != 0) return false;
    fr.frames = frames;
    int64_t K = 0;
    for (int f = 0; f < frames; ++f) {
        const int64_t n = tok[f + 1] - tok[f];
        if (n < 0 || (thirds && n % 3) || tok[f + 1] >= ((int64_t)1 << 31) || steps[f] < 0 || steps[f] > AR_MAX_STEPS || (pay[f] & 7) || pay[f] < 0)
            return false;
        if (all && n > 0 && steps[f] < 1) return false;
        fr.tok[f] = tok[f]; fr.pay[f] = pay[f]; fr.steps[f] = steps[f]; fr.chunk[f] = (int)K;
        K += (n > 0 && steps[f] > 0) ? ar_chunks(n, steps[f]) : 0;
        if (K >= ((int64_t)1 << 31)) return false;
    }
    for (int f = frames; f <= AR_MAX_FRAMES; ++f) { fr.tok[f] = tok[frames]; fr.chunk[f] = (int)K; }
    return true;
}
static bool ar_frame_of_one(int64_t n, int steps, ArFrames& fr) {
    const int64_t tok[2] = {0, n}, pay = 0;
    const int32_t s = steps;
    return ar_frames_of(1, tok, &s, &pay, fr, true, false);
}

static long long* ar_host_slot() {
    static thread_local long long* host = nullptr;
    if (!host && hipHostMalloc((void**)&host, AR_SLOT_BYTES, hipHostMallocDefault) != hipSuccess) host = nullptr;
    return host;
}
// both bodies: the workspace is checked and carved and its slots are zeroed; rest: the encoder's scratch or the decoder's contexts
static int ar_begin(const char* who, const ArFrames& fr, void* workspace, size_t workspace_bytes, long long*& host, long long*& slot, uint32_t*& offs,
                    void*& rest, hipStream_t s) {
    const int64_t n = fr.tok[fr.frames], K = fr.chunk[fr.frames];
    AR_REQUIRE(who, workspace && workspace_bytes >= (size_t)pcgc_attr_rans_batch_workspace_bytes(n, K) && ((uintptr_t)workspace & 7) == 0,
               "workspace too small or misaligned");
    slot = (long long*)workspace;
    offs = (uint32_t*)((char*)workspace + AR_SLOT_BYTES);
    rest = (char*)workspace + AR_SLOT_BYTES + ar_offs_bytes(K);
    host = ar_host_slot();
    if (!host) { pcgc_set_error("%s: cannot allocate pinned memory", who + 5); return -1; }
    hipError_t e = hipMemsetAsync(slot, 0, AR_SLOT_BYTES, s);
    AR_CHECK_HIP(who, e);
    return 0;
}
// the first `count` slots brought down, the stream synchronised
static int ar_end(const char* who, long long* host, const long long* slot, int count, hipStream_t s) {
    hipError_t e = hipMemcpyAsync(host, slot, count * sizeof(long long), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    AR_CHECK_HIP(who, e);
    return 0;
}

// host [2 frames] = every frame's payload bytes (8 + 516 K_f + 4 words; 0 for a frame without chunks), then its refused tokens
static int ar_encode(const char* who, const uint16_t* tables, const uint16_t* ctx, const int16_t* tokens, const ArFrames& fr, uint8_t* payload,
                     int64_t* host, void* workspace, size_t workspace_bytes, hipStream_t s) {
    long long *hostslot, *slot;
    uint32_t* offs;
    void* scratch;
    if (int r = ar_begin(who, fr, workspace, workspace_bytes, hostslot, slot, offs, scratch, s)) return r;
    const int frames = fr.frames;
    const unsigned K = (unsigned)fr.chunk[frames];
    hipLaunchKernelGGL(k_attr_rans_encode, dim3(K), dim3(AR_LANES), 0, s, tables, ctx, tokens, fr, (uint32_t*)scratch, payload,
                       (unsigned long long*)(slot + AR_MAX_FRAMES));
    PCGC_CHECK_LAUNCH(who + 5);
    hipLaunchKernelGGL(k_attr_rans_offsets, dim3((unsigned)frames), dim3(AR_SCAN_BLOCK), 0, s, fr, payload, offs, slot, 1);
    PCGC_CHECK_LAUNCH(who + 5);
    hipLaunchKernelGGL(k_attr_rans_compact, dim3(K), dim3(AR_SCAN_BLOCK), 0, s, (const uint32_t*)scratch, fr, (const uint32_t*)offs, payload);
    PCGC_CHECK_LAUNCH(who + 5);
    if (int r = ar_end(who, hostslot, slot, 2 * AR_MAX_FRAMES, s)) return r;
    for (int f = 0; f < frames; ++f) {
        const int64_t Kf = fr.chunk[f + 1] - fr.chunk[f];
        host[f] = Kf ? 8 + 516 * Kf + 4 * (int64_t)hostslot[f] : 0;
        host[frames + f] = (int64_t)hostslot[AR_MAX_FRAMES + f];
    }
    return 0;
}
// fr.words[f]: the words of frame f's payload behind its tables.  host [2 frames] = every frame's tokens that are 63, then its unsound chunks
// (+ 1: the word counts do not add up to the payload); 0 and 0 for a frame without chunks
static int ar_decode(const char* who, const uint16_t* tables, const int32_t* bucket, const ArFrames& fr, const uint8_t* payload, int16_t* tokens,
                     int64_t* host, void* workspace, size_t workspace_bytes, hipStream_t s) {
    long long *hostslot, *slot;
    uint32_t* offs;
    void* ctx;
    if (int r = ar_begin(who, fr, workspace, workspace_bytes, hostslot, slot, offs, ctx, s)) return r;
    const int frames = fr.frames;
    const int64_t n = fr.tok[frames];
    hipLaunchKernelGGL(k_attr_rans_ctx, dim3(grid_for((n + 2) / 3, AR_SCAN_BLOCK)), dim3(AR_SCAN_BLOCK), 0, s, bucket, fr, (uint16_t*)ctx);
    PCGC_CHECK_LAUNCH(who + 5);
    hipLaunchKernelGGL(k_attr_rans_offsets, dim3((unsigned)frames), dim3(AR_SCAN_BLOCK), 0, s, fr, const_cast<uint8_t*>(payload), offs, slot, 0);
    PCGC_CHECK_LAUNCH(who + 5);
    hipLaunchKernelGGL(k_attr_rans_decode, dim3((unsigned)fr.chunk[frames]), dim3(AR_LANES), 0, s, tables, (const uint16_t*)ctx, fr, payload,
                       (const uint32_t*)offs, tokens, (unsigned long long*)(slot + AR_MAX_FRAMES));
    PCGC_CHECK_LAUNCH(who + 5);
    if (int r = ar_end(who, hostslot, slot, 3 * AR_MAX_FRAMES, s)) return r;
    for (int f = 0; f < frames; ++f) {
        const bool here = fr.chunk[f + 1] > fr.chunk[f];
        host[f] = here ? (int64_t)hostslot[AR_MAX_FRAMES + 2 * f] : 0;
        host[frames + f] = here ? (int64_t)hostslot[AR_MAX_FRAMES + 2 * f + 1] + (hostslot[f] != fr.words[f] ? 1 : 0) : 0;
    }
    return 0;
}

// ---- one frame: any n; host2 = {payload bytes, refused tokens} and {tokens that are 63, unsound chunks} are the body's answers for frame 0
extern "C" int pcgc_attr_rans_encode(const uint16_t* table, const uint16_t* ctx, const int16_t* tokens, int64_t n, int steps, uint8_t* payload,
                                     size_t payload_capacity, int64_t* host2, void* workspace, size_t workspace_bytes, void* stream) {
    PCGC_REQUIRE(n >= 1 && n < ((int64_t)1 << 31), "bad token count");
    PCGC_REQUIRE(steps >= 1 && steps <= AR_MAX_STEPS, "steps per chunk outside 1 .. 2^24");
    PCGC_REQUIRE(table && ctx && tokens && payload && host2, "null argument");
    ArFrames fr;
    PCGC_REQUIRE(ar_frame_of_one(n, steps, fr), "bad token count");
    PCGC_REQUIRE(payload_capacity >= (size_t)(8 + 516 * (int64_t)fr.chunk[1] + 4 * n) && ((uintptr_t)payload & 7) == 0,
                 "payload buffer too small or misaligned");
    return ar_encode(__func__, table, ctx, tokens, fr, payload, host2, workspace, workspace_bytes, S(stream));
}

extern "C" int pcgc_attr_rans_decode(const uint16_t* table, const int32_t* bucket, int64_t n, const uint8_t* payload, int64_t payload_bytes, int steps,
                                     int16_t* tokens, int64_t* host2, void* workspace, size_t workspace_bytes, void* stream) {
    PCGC_REQUIRE(n >= 1 && n < ((int64_t)1 << 31), "bad token count");
    PCGC_REQUIRE(table && bucket && tokens && payload && host2, "null argument");
    PCGC_REQUIRE(((uintptr_t)payload & 7) == 0, "payload misaligned");
    PCGC_REQUIRE(steps >= 1 && steps <= AR_MAX_STEPS, "steps per chunk outside 1 .. 2^24");
    ArFrames fr;
    PCGC_REQUIRE(ar_frame_of_one(n, steps, fr), "bad token count");
    const int64_t K = fr.chunk[1];                    // (the head's own S and K are the caller's to compare: ops.attr_rans_decode)
    PCGC_REQUIRE(payload_bytes >= 8 + 516 * K && (payload_bytes - 8 - 516 * K) % 4 == 0, "payload cut inside its tables or not whole words");
    fr.words[0] = (payload_bytes - 8 - 516 * K) / 4;
    return ar_decode(__func__, table, bucket, fr, payload, tokens, host2, workspace, workspace_bytes, S(stream));
}

// ---- a batch of frames: per-frame token counts in multiples of 3
extern "C" int pcgc_attr_rans_encode_batch(const uint16_t* tables, const uint16_t* ctx, const int16_t* tokens, int frames, const int64_t* tok,
                                           const int32_t* steps, uint8_t* payload, const int64_t* pay, int64_t* host, void* workspace,
                                           size_t workspace_bytes, void* stream) {
    ArFrames fr;
    PCGC_REQUIRE(ar_frames_of(frames, tok, steps, pay, fr, true, true), "1 to 16 frames; token offsets ascending multiples of 3 below 2^31; steps per chunk 1 .. 2^24; payload offsets multiples of 8");
    PCGC_REQUIRE(tables && ctx && tokens && payload && host && ((uintptr_t)payload & 7) == 0, "null or misaligned argument");
    PCGC_REQUIRE(fr.tok[frames] >= 1, "no token: nothing to launch");
    for (int f = 0; f < frames; ++f)
        PCGC_REQUIRE(pay[f + 1] - pay[f] >= (fr.chunk[f + 1] > fr.chunk[f] ? 8 + 516 * (int64_t)(fr.chunk[f + 1] - fr.chunk[f]) + 4 * (tok[f + 1] - tok[f]) : 0),
                     "payload room of a frame below 8 + 516 K + 4 n bytes");
    return ar_encode(__func__, tables, ctx, tokens, fr, payload, host, workspace, workspace_bytes, S(stream));
}

extern "C" int pcgc_attr_rans_decode_batch(const uint16_t* tables, const int32_t* bucket, int frames, const int64_t* tok, const int32_t* steps,
                                           const uint8_t* payload, const int64_t* pay, const int64_t* pay_bytes, int16_t* tokens, int64_t* host,
                                           void* workspace, size_t workspace_bytes, void* stream) {
    ArFrames fr;
    PCGC_REQUIRE(ar_frames_of(frames, tok, steps, pay, fr, false, true), "1 to 16 frames; token offsets ascending multiples of 3 below 2^31; steps per chunk 0 .. 2^24; payload offsets multiples of 8");
    PCGC_REQUIRE(tables && bucket && tokens && payload && pay_bytes && host && ((uintptr_t)payload & 7) == 0, "null or misaligned argument");
    PCGC_REQUIRE(fr.tok[frames] >= 1 && fr.chunk[frames] >= 1, "no chunk: nothing to launch");
    for (int f = 0; f < frames; ++f) {
        const int64_t Kf = fr.chunk[f + 1] - fr.chunk[f];
        if (!Kf) continue;
        PCGC_REQUIRE(pay_bytes[f] >= 8 + 516 * Kf && (pay_bytes[f] - 8 - 516 * Kf) % 4 == 0, "a payload cut inside its tables or not whole words");
        fr.words[f] = (pay_bytes[f] - 8 - 516 * Kf) / 4;
    }
    return ar_decode(__func__, tables, bucket, fr, payload, tokens, host, workspace, workspace_bytes, S(stream));
}

