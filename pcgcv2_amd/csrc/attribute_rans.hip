// Colour codec, `_A.bin` version 2 (attributes.py): the tokens of the colour transform coded ON THE DEVICE by interleaved rANS, so that only
// the coded bytes cross the bus.  Input is what pcgc_raht_quantize writes (tokens and their contexts in coding order) and the stream's own
// frequency tables; the format is stated in include/pcgc_hip.h and, in plain Python integers, in tests/attr_rans_reference.py.
//
// The coder itself is rans_core.h (chunks, frames, the encoder's emit step, the decoder's word ring and its soundness argument, offsets and
// compaction, the host side).  This file is the symbol model: a 64-ary token under one of 48 contexts, 16-bit frequencies.
//
// The tables live in LDS, one row of AR_ROW words per context, filled once per workgroup:
//     [0 .. 7]   pivots cdf[8], cdf[16], .., cdf[56], then 65536      [8 .. 72]  cdf[0 .. 64] with cdf[0] = 0, cdf[64] = 65536      (3 words pad)
// so that every group of eight entries cdf[8 g .. 8 g + 7] and the pivots are 16-byte aligned.
//
//   encoder  c and f of a token are two LDS words that depend on the input alone, so they are off the chain.  f = 65536 (a token that owns
//            its row) is taken out before the division: the update is the identity and the token never emits.  A token outside 0 .. 63, a
//            context outside 0 .. 47 or f <= 0 is counted and skipped: nothing is divided by 0.
//   decoder  The symbol search is two 8-way levels.  Level 1, which group of eight holds s, compares s with the seven pivots; they depend
//            on the context alone and are in registers before the batch's chain starts.  Level 2 reads the group's eight entries (the one
//            table read on the chain) and counts those <= s; c is the largest entry <= s and c + f the smallest entry > s, taken by max /
//            min over the same sixteen registers, so no index formed from table bytes ever addresses memory and the token is in 0 .. 63
//            whatever the table says.  The contexts come from k_attr_rans_ctx, which derives them from the tree's bucket offsets: they are
//            never uploaded.
//
// A batch of frames (pcgc_attr_rans_*_batch) is one launch of the chunks of all frames: a workgroup serves one frame's chunk
// with that frame's table, and every frame's payload is packed on its own.  A SINGLE FRAME IS THE BATCH OF ONE: pcgc_attr_rans_encode /
// _decode build the RansFrames of one frame (of any length: only the batch entries demand token counts in multiples of 3) and run the same
// bodies.  No workgroup reads what another wrote in the same launch.
#include "rans_core.h"

constexpr int AR_CONTEXTS = 48;
constexpr int AR_TOKENS = 64;
constexpr int AR_ROW = 76;                                    // LDS words per context

// table [48][65] uint16 in rc_encode_ctx's convention (entry 0 and entry 64 are implied) -> the LDS rows described above
__device__ static inline void ar_load_table(uint32_t* sh, const uint16_t* __restrict__ table) {
    for (int i = threadIdx.x; i < AR_CONTEXTS * AR_ROW; i += RANS_LANES) {
        const int c = i / AR_ROW, w = i - c * AR_ROW;
        int e = w < 7 ? 8 * (w + 1) : w == 7 ? 64 : w - 8;     // the cdf entry this word holds
        if (e > 64) e = 64;                                     // (pad)
        sh[i] = e == 0 ? 0u : e == 64 ? 65536u : (uint32_t)table[c * (AR_TOKENS + 1) + e];
    }
    __syncthreads();
}

// ---- encoder ---------------------------------------------------------------------------------------------------------------------------------
// refused [f]: frame f's tokens that cannot be coded
__global__ void __launch_bounds__(RANS_LANES) k_attr_rans_encode(const uint16_t* __restrict__ tables, const uint16_t* __restrict__ ctx,
                                                                 const int16_t* __restrict__ tokens, RansFrames fr, uint32_t* __restrict__ scratch,
                                                                 uint8_t* __restrict__ payload, unsigned long long* __restrict__ refused) {
    __shared__ __attribute__((aligned(16))) uint32_t sh[AR_CONTEXTS * AR_ROW];
    const RansChunk c = rans_chunk_of(fr);
    ar_load_table(sh, tables + (size_t)c.f * AR_CONTEXTS * (AR_TOKENS + 1));
    const int lane = threadIdx.x, rows = c.rows;
    const uint16_t* __restrict__ in_c = ctx + c.base;
    const int16_t* __restrict__ in_t = tokens + c.base;
    uint32_t* __restrict__ out = scratch + c.base;            // rows words: [top, rows) are written
    const int steps = (rows + RANS_LANES - 1) / RANS_LANES;   // steps that hold a token at all
    int top = rows;
    uint64_t x = RANS_L;
    unsigned bad = 0;
    uint32_t cur[RANS_BATCH], nxt[RANS_BATCH];
    // batch starting at step t0 holds steps t0, t0 - 1, ..; a word is ctx << 16 | token (both as stored); a step without a token for
    // this lane is told from its index, not from the word
#define AR_FETCH(dst, t0)                                                                                 \
    _Pragma("unroll") for (int i = 0; i < RANS_BATCH; ++i) {                                              \
        const int r = ((t0) - i) * RANS_LANES + lane;                                                     \
        dst[i] = ((t0) - i >= 0 && r < rows) ? ((uint32_t)in_c[r] << 16) | (uint16_t)in_t[r] : 0u;        \
    }
    AR_FETCH(cur, steps - 1)
    for (int t0 = steps - 1; t0 >= 0; t0 -= RANS_BATCH) {
        AR_FETCH(nxt, t0 - RANS_BATCH)
#pragma unroll
        for (int i = 0; i < RANS_BATCH; ++i) {
            const bool here = t0 - i >= 0 && (t0 - i) * RANS_LANES + lane < rows;
            const uint32_t cx = cur[i] >> 16, a = cur[i] & 0xffffu;
            const bool inside = cx < (uint32_t)AR_CONTEXTS && a < (uint32_t)AR_TOKENS;
            const uint32_t* row = sh + (inside ? cx : 0u) * AR_ROW + 8 + (inside ? a : 0u);
            const uint32_t cum = row[0], e = row[1];
            const uint32_t f = e > cum ? e - cum : 0u;
            const bool act = here && inside && f != 0u;
            bad += (here && !act) ? 1u : 0u;
            rans_put(x, top, out, act && f != 65536u, f, cum);                   // f = 65536 is the identity: x < 2^63 = f << 47 never emits
        }
#pragma unroll
        for (int i = 0; i < RANS_BATCH; ++i) cur[i] = nxt[i];
    }
#undef AR_FETCH
    rans_put_end(payload + fr.pay[c.f], c, x, top);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) bad += __shfl_xor(bad, d, 64);
    if (lane == 0 && bad) atomicAdd(refused + c.f, (unsigned long long)bad);      // (integer atomic: the sum does not depend on the order)
}

// ---- decoder ---------------------------------------------------------------------------------------------------------------------------------
// the context of every token in coding order from the trees' bucket offsets: position p of the coding order (token 3 p + channel) lies in
// the last frame f with first[f] <= 3 p, at position q = p - first[f] / 3 of that frame's own order, whose 65 offsets are row f of bucket
// [frames, 65]; its split bit is d = 63 - b, where b is the last bucket with row[b] <= q; ctx = 16 channel + min(d / 3, 15).  first[] of the
// frames of a batch are multiples of 3; the last position of a single frame may hold fewer than three tokens, so the tail stores are guarded.
__global__ void __launch_bounds__(RANS_SCAN_BLOCK) k_attr_rans_ctx(const int32_t* __restrict__ bucket, RansFrames fr, uint16_t* __restrict__ ctx) {
    const int64_t p = (int64_t)blockIdx.x * RANS_SCAN_BLOCK + threadIdx.x, n = fr.first[fr.frames];
    if (3 * p >= n) return;
    int f = 0;
    for (int b = 1; b < RANS_MAX_FRAMES; ++b) f += (b < fr.frames && fr.first[b] <= 3 * p) ? 1 : 0;
    const int32_t* __restrict__ row = bucket + f * (AR_TOKENS + 1);
    const int64_t q = p - fr.first[f] / 3;
    int b = 0;
#pragma unroll
    for (int step = 32; step > 0; step >>= 1) b += (b + step <= 63 && (int64_t)row[b + step] <= q) ? step : 0;         // b stays in 0 .. 63
    const int d = 63 - b;
    const uint16_t level = (uint16_t)(d / 3 < 15 ? d / 3 : 15);
    ctx[3 * p] = level;
    if (3 * p + 1 < n) ctx[3 * p + 1] = (uint16_t)(16 + level);
    if (3 * p + 2 < n) ctx[3 * p + 2] = (uint16_t)(32 + level);
}

// result [2 f], [2 f + 1]: frame f's tokens that are 63 and its unsound chunks
__global__ void __launch_bounds__(RANS_LANES) k_attr_rans_decode(const uint16_t* __restrict__ tables, const uint16_t* __restrict__ ctx, RansFrames fr,
                                                                 const uint8_t* __restrict__ payload, const uint32_t* __restrict__ offs,
                                                                 int16_t* __restrict__ tokens, unsigned long long* __restrict__ result) {
    __shared__ __attribute__((aligned(16))) uint32_t sh[AR_CONTEXTS * AR_ROW];
    __shared__ uint32_t ring[RANS_RING];
    const RansChunk c = rans_chunk_of(fr);
    ar_load_table(sh, tables + (size_t)c.f * AR_CONTEXTS * (AR_TOKENS + 1));
    const int lane = threadIdx.x, rows = c.rows;
    const int steps = (rows + RANS_LANES - 1) / RANS_LANES;
    const uint16_t* __restrict__ in = ctx + c.base;
    int16_t* __restrict__ out = tokens + c.base;
    RansReader rd;
    uint64_t x = rd.open(fr, c, payload, offs, ring);
#define AR_FETCH(dst, t0)                                                                     \
    _Pragma("unroll") for (int i = 0; i < RANS_BATCH; ++i) {                                  \
        const int r = ((t0) + i) * RANS_LANES + lane;                                         \
        dst[i] = r < rows ? (uint32_t)in[r] : RANS_NONE;                                      \
    }
    uint32_t cur[RANS_BATCH], nxt[RANS_BATCH];
    AR_FETCH(cur, 0)
    unsigned escapes = 0;
    for (int t0 = 0; t0 < steps; t0 += RANS_BATCH) {
        AR_FETCH(nxt, t0 + RANS_BATCH)
        rd.refill();
        // level 1 of the batch's searches: rows and pivots follow from the contexts alone
        uint32_t rowat[RANS_BATCH];
        uint4 pa[RANS_BATCH], pb[RANS_BATCH];
#pragma unroll
        for (int i = 0; i < RANS_BATCH; ++i) {
            const uint32_t cx = cur[i] < (uint32_t)AR_CONTEXTS ? cur[i] : 0u;    // (a context outside the table cannot come from k_attr_rans_ctx; clamp it all the same)
            rowat[i] = cx * AR_ROW;
            pa[i] = *(const uint4*)(sh + rowat[i]);
            pb[i] = *(const uint4*)(sh + rowat[i] + 4);
        }
#pragma unroll
        for (int i = 0; i < RANS_BATCH; ++i) {
            const bool act = cur[i] != RANS_NONE;
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
            uint32_t r = 0, cum = e[0] <= s ? e[0] : 0u;                         // e[0] = cdf[8 g] <= s in a monotone row
#pragma unroll
            for (int j = 1; j < 8; ++j) {
                const bool le = e[j] <= s;
                r += le ? 1u : 0u;
                cum = max(cum, le ? e[j] : 0u);
                above = min(above, le ? 65536u : e[j]);
            }
            const uint32_t a = 8 * g + r;                                        // 0 .. 63
            const uint32_t f = above - cum;                                      // 1 .. 65536 in a monotone row
            if (act) x = (uint64_t)f * (x >> 16) + s - cum;
            rd.take(x, act);
            if (act) { out[(t0 + i) * RANS_LANES + lane] = (int16_t)a; escapes += a == 63u ? 1u : 0u; }
        }
#pragma unroll
        for (int i = 0; i < RANS_BATCH; ++i) cur[i] = nxt[i];
    }
#undef AR_FETCH
    rd.close(x, escapes, result + 2 * c.f);
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------------
// The batch entries and the single ones run the same two bodies below over a RansFrames; a single entry builds the RansFrames of one frame.
// slot, 4 x 16 x int64: words per frame [16] | the encoder's refused tokens per frame [16] or the decoder's result [16][2]
// rest: the encoder's scratch, n x u32, or the decoder's contexts, n x u16
constexpr size_t AR_SLOT_BYTES = 4 * RANS_MAX_FRAMES * sizeof(long long);
static_assert(AR_SLOT_BYTES <= RANS_SLOT_MAX, "the pinned host slot holds every coder's slot");

extern "C" int64_t pcgc_attr_rans_batch_workspace_bytes(int64_t n, int64_t chunks) {
    if (n < 0) n = 0;
    if (chunks < 0) chunks = 0;
    return (int64_t)AR_SLOT_BYTES + (int64_t)rans_offs_bytes(chunks) + n * 4 + 64;
}
extern "C" int64_t pcgc_attr_rans_workspace_bytes(int64_t n, int steps) {
    if (n < 0) n = 0;
    if (steps < 1) steps = 1;
    return pcgc_attr_rans_batch_workspace_bytes(n, rans_chunks(n, steps));
}

// host [2 frames] = every frame's payload bytes (8 + 516 K_f + 4 words; 0 for a frame without chunks), then its refused tokens
static int ar_encode(const char* who, const uint16_t* tables, const uint16_t* ctx, const int16_t* tokens, const RansFrames& fr, uint8_t* payload,
                     int64_t* host, void* workspace, size_t workspace_bytes, hipStream_t s) {
    const int frames = fr.frames;
    RansWork w;
    if (int r = rans_begin(who, fr, workspace, workspace_bytes, AR_SLOT_BYTES, (size_t)fr.first[frames] * 4 + 64, w, s)) return r;
    hipLaunchKernelGGL(k_attr_rans_encode, dim3((unsigned)fr.chunk[frames]), dim3(RANS_LANES), 0, s, tables, ctx, tokens, fr, (uint32_t*)w.rest, payload,
                       (unsigned long long*)(w.slot + RANS_MAX_FRAMES));
    PCGC_CHECK_LAUNCH(who + 5);
    if (int r = rans_pack(who, fr, w, payload, 0, nullptr, s)) return r;
    if (int r = rans_end(who, w, 2 * RANS_MAX_FRAMES, s)) return r;
    for (int f = 0; f < frames; ++f) {
        host[f] = rans_payload_bytes(fr, f, w.host[f], 0);
        host[frames + f] = (int64_t)w.host[RANS_MAX_FRAMES + f];
    }
    return 0;
}
// fr.words[f]: the words of frame f's payload behind its tables.  host [2 frames] = every frame's tokens that are 63, then its unsound chunks
// (+ 1: the word counts do not add up to the payload); 0 and 0 for a frame without chunks
static int ar_decode(const char* who, const uint16_t* tables, const int32_t* bucket, const RansFrames& fr, const uint8_t* payload, int16_t* tokens,
                     int64_t* host, void* workspace, size_t workspace_bytes, hipStream_t s) {
    const int frames = fr.frames;
    const int64_t n = fr.first[frames];
    RansWork w;
    if (int r = rans_begin(who, fr, workspace, workspace_bytes, AR_SLOT_BYTES, (size_t)n * 4 + 64, w, s)) return r;
    hipLaunchKernelGGL(k_attr_rans_ctx, dim3(grid_for((n + 2) / 3, RANS_SCAN_BLOCK)), dim3(RANS_SCAN_BLOCK), 0, s, bucket, fr, (uint16_t*)w.rest);
    PCGC_CHECK_LAUNCH(who + 5);
    if (int r = rans_offsets(who, fr, w, payload, s)) return r;
    hipLaunchKernelGGL(k_attr_rans_decode, dim3((unsigned)fr.chunk[frames]), dim3(RANS_LANES), 0, s, tables, (const uint16_t*)w.rest, fr, payload,
                       (const uint32_t*)w.offs, tokens, (unsigned long long*)(w.slot + RANS_MAX_FRAMES));
    PCGC_CHECK_LAUNCH(who + 5);
    if (int r = rans_end(who, w, 3 * RANS_MAX_FRAMES, s)) return r;
    for (int f = 0; f < frames; ++f) {
        const bool here = fr.chunk[f + 1] > fr.chunk[f];
        host[f] = here ? (int64_t)w.host[RANS_MAX_FRAMES + 2 * f] : 0;
        host[frames + f] = here ? (int64_t)w.host[RANS_MAX_FRAMES + 2 * f + 1] + (w.host[f] != fr.words[f] ? 1 : 0) : 0;
    }
    return 0;
}

// ---- one frame: any n; host2 = {payload bytes, refused tokens} and {tokens that are 63, unsound chunks} are the body's answers for frame 0
extern "C" int pcgc_attr_rans_encode(const uint16_t* table, const uint16_t* ctx, const int16_t* tokens, int64_t n, int steps, uint8_t* payload,
                                     size_t payload_capacity, int64_t* host2, void* workspace, size_t workspace_bytes, void* stream) {
    PCGC_REQUIRE(n >= 1 && n < ((int64_t)1 << 31), "bad token count");
    PCGC_REQUIRE(steps >= 1 && steps <= RANS_MAX_STEPS, "steps per chunk outside 1 .. 2^24");
    PCGC_REQUIRE(table && ctx && tokens && payload && host2, "null argument");
    RansFrames fr;
    PCGC_REQUIRE(rans_frame_of_one(n, steps, fr), "bad token count");
    PCGC_REQUIRE(payload_capacity >= (size_t)rans_room(fr.chunk[1], n) && ((uintptr_t)payload & 7) == 0, "payload buffer too small or misaligned");
    return ar_encode(__func__, table, ctx, tokens, fr, payload, host2, workspace, workspace_bytes, S(stream));
}

extern "C" int pcgc_attr_rans_decode(const uint16_t* table, const int32_t* bucket, int64_t n, const uint8_t* payload, int64_t payload_bytes, int steps,
                                     int16_t* tokens, int64_t* host2, void* workspace, size_t workspace_bytes, void* stream) {
    PCGC_REQUIRE(n >= 1 && n < ((int64_t)1 << 31), "bad token count");
    PCGC_REQUIRE(table && bucket && tokens && payload && host2, "null argument");
    PCGC_REQUIRE(((uintptr_t)payload & 7) == 0, "payload misaligned");
    PCGC_REQUIRE(steps >= 1 && steps <= RANS_MAX_STEPS, "steps per chunk outside 1 .. 2^24");
    RansFrames fr;
    PCGC_REQUIRE(rans_frame_of_one(n, steps, fr), "bad token count");
    // (the head's own S and K are the caller's to compare: ops.attr_rans_decode)
    PCGC_REQUIRE(rans_words_of(fr, 0, payload_bytes), "payload cut inside its tables or not whole words");
    return ar_decode(__func__, table, bucket, fr, payload, tokens, host2, workspace, workspace_bytes, S(stream));
}

// ---- a batch of frames: per-frame token counts in multiples of 3
extern "C" int pcgc_attr_rans_encode_batch(const uint16_t* tables, const uint16_t* ctx, const int16_t* tokens, int frames, const int64_t* tok,
                                           const int32_t* steps, uint8_t* payload, const int64_t* pay, int64_t* host, void* workspace,
                                           size_t workspace_bytes, void* stream) {
    RansFrames fr;
    PCGC_REQUIRE(rans_frames_of(frames, tok, steps, pay, fr, RANS_NEED_STEPS | RANS_THIRDS), "1 to 16 frames; token offsets ascending multiples of 3 below 2^31; steps per chunk 1 .. 2^24; payload offsets multiples of 8");
    PCGC_REQUIRE(tables && ctx && tokens && payload && host && ((uintptr_t)payload & 7) == 0, "null or misaligned argument");
    PCGC_REQUIRE(fr.first[frames] >= 1, "no token: nothing to launch");
    for (int f = 0; f < frames; ++f)
        PCGC_REQUIRE(pay[f + 1] - pay[f] >= rans_payload_bytes(fr, f, tok[f + 1] - tok[f], 0), "payload room of a frame below 8 + 516 K + 4 n bytes");
    return ar_encode(__func__, tables, ctx, tokens, fr, payload, host, workspace, workspace_bytes, S(stream));
}

extern "C" int pcgc_attr_rans_decode_batch(const uint16_t* tables, const int32_t* bucket, int frames, const int64_t* tok, const int32_t* steps,
                                           const uint8_t* payload, const int64_t* pay, const int64_t* pay_bytes, int16_t* tokens, int64_t* host,
                                           void* workspace, size_t workspace_bytes, void* stream) {
    RansFrames fr;
    PCGC_REQUIRE(rans_frames_of(frames, tok, steps, pay, fr, RANS_THIRDS), "1 to 16 frames; token offsets ascending multiples of 3 below 2^31; steps per chunk 0 .. 2^24; payload offsets multiples of 8");
    PCGC_REQUIRE(tables && bucket && tokens && payload && pay_bytes && host && ((uintptr_t)payload & 7) == 0, "null or misaligned argument");
    PCGC_REQUIRE(fr.first[frames] >= 1 && fr.chunk[frames] >= 1, "no chunk: nothing to launch");
    for (int f = 0; f < frames; ++f)
        PCGC_REQUIRE(fr.chunk[f + 1] == fr.chunk[f] || rans_words_of(fr, f, pay_bytes[f]), "a payload cut inside its tables or not whole words");
    return ar_decode(__func__, tables, bucket, fr, payload, tokens, host, workspace, workspace_bytes, S(stream));
}
