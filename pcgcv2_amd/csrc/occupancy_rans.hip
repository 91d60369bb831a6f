// Lossless mode, `_O.bin` version 2 (lossless.py): the occupancy bits of a decoder level coded ON THE DEVICE by interleaved rANS, so that
// only the coded bytes cross the bus.  Input is what pcgc_occ_symbols writes (packed[i] = ctx << 1 | bit); the format is stated in
// include/pcgc_hip.h and, in plain Python integers, in tests/rans_reference.py.
//
// The coder itself is rans_core.h (chunks, frames, the encoder's emit step, the decoder's word ring and its soundness argument, offsets and
// compaction, the host side).  This file is the symbol model: a bit under the 16-bit probability P1[ctx] (occupancy_tables.h), the table
// in LDS; lane j codes rows base + 64 t + j, so a step's loads of `packed` are one coalesced 128-byte access.  The chain of a decoder step
// is table lookup, multiply, compare, ballot, LDS read.  The contexts of the next RANS_BATCH steps are loaded while the current ones are
// coded.
//
// A batch of frames (the items of a collated batch at one decoder level) goes through ONE launch sequence;
// pcgc_occ_rans_encode / _decode are the batch of one, on the same slot layout.
#include "rans_core.h"
#include "occupancy_tables.h"

__device__ static const uint16_t d_rans_p1[PCGC_OCC_CONTEXTS] = {PCGC_OCC_P1_VALUES};

__device__ static inline void rans_load_p1(uint32_t* sh) {
    for (int i = threadIdx.x; i < PCGC_OCC_CONTEXTS; i += RANS_LANES) sh[i] = d_rans_p1[i];
    __syncthreads();
}
__device__ static inline uint32_t rans_p1(const uint32_t* sh, uint32_t word) {
    const uint32_t ctx = word >> 1;                          // (a context outside the table cannot come from pcgc_occ_symbols; clamp it all the same)
    return sh[ctx < PCGC_OCC_CONTEXTS ? ctx : PCGC_OCC_CONTEXTS - 1];
}

// ---- encoder ---------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(RANS_LANES) k_occ_rans_encode(const uint16_t* __restrict__ packed, RansFrames fr, uint32_t* __restrict__ scratch,
                                                                uint8_t* __restrict__ payload) {
    __shared__ uint32_t sh_p1[PCGC_OCC_CONTEXTS];
    rans_load_p1(sh_p1);
    const int lane = threadIdx.x;
    const RansChunk c = rans_chunk_of(fr);
    const int rows = c.rows;
    const uint16_t* __restrict__ in = packed + c.base;
    uint32_t* __restrict__ out = scratch + c.base;            // rows words: [top, rows) are written
    const int steps = (rows + RANS_LANES - 1) / RANS_LANES;   // steps that hold a row at all
    int top = rows;
    uint64_t x = RANS_L;
    uint32_t cur[RANS_BATCH], nxt[RANS_BATCH];
    // batch starting at step t0 holds steps t0, t0 - 1, ..; a word of RANS_NONE marks "no row"
#define OCC_FETCH(dst, t0)                                                                    \
    _Pragma("unroll") for (int i = 0; i < RANS_BATCH; ++i) {                                  \
        const int r = ((t0) - i) * RANS_LANES + lane;                                         \
        dst[i] = ((t0) - i >= 0 && r < rows) ? (uint32_t)in[r] : RANS_NONE;                   \
    }
    OCC_FETCH(cur, steps - 1)
    for (int t0 = steps - 1; t0 >= 0; t0 -= RANS_BATCH) {
        OCC_FETCH(nxt, t0 - RANS_BATCH)
#pragma unroll
        for (int i = 0; i < RANS_BATCH; ++i) {
            const bool act = cur[i] != RANS_NONE;
            const uint32_t p = rans_p1(sh_p1, act ? cur[i] : 0u), b = cur[i] & 1u;
            rans_put(x, top, out, act, b ? p : 65536u - p, b ? 65536u - p : 0u);
        }
#pragma unroll
        for (int i = 0; i < RANS_BATCH; ++i) cur[i] = nxt[i];
    }
#undef OCC_FETCH
    rans_put_end(payload + fr.pay[c.f], c, x, top);
}

// ---- decoder ---------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(RANS_LANES) k_occ_rans_decode(const uint16_t* __restrict__ packed, RansFrames fr, const uint8_t* __restrict__ payload,
                                                                const uint32_t* __restrict__ offs, uint8_t* __restrict__ mask,
                                                                unsigned long long* __restrict__ result /*per frame: occupied rows, unsound chunks*/) {
    __shared__ uint32_t sh_p1[PCGC_OCC_CONTEXTS];
    __shared__ uint32_t ring[RANS_RING];
    rans_load_p1(sh_p1);
    const int lane = threadIdx.x;
    const RansChunk c = rans_chunk_of(fr);
    const int rows = c.rows;
    const int steps = (rows + RANS_LANES - 1) / RANS_LANES;
    const uint16_t* __restrict__ in = packed + c.base;
    uint8_t* __restrict__ out = mask + c.base;
    RansReader rd;
    uint64_t x = rd.open(fr, c, payload, offs, ring);
#define OCC_FETCH(dst, t0)                                                                    \
    _Pragma("unroll") for (int i = 0; i < RANS_BATCH; ++i) {                                  \
        const int r = ((t0) + i) * RANS_LANES + lane;                                         \
        dst[i] = r < rows ? (uint32_t)in[r] : RANS_NONE;                                      \
    }
    uint32_t cur[RANS_BATCH], nxt[RANS_BATCH];
    OCC_FETCH(cur, 0)
    unsigned occupied = 0;
    for (int t0 = 0; t0 < steps; t0 += RANS_BATCH) {
        OCC_FETCH(nxt, t0 + RANS_BATCH)
        rd.refill();
#pragma unroll
        for (int i = 0; i < RANS_BATCH; ++i) {
            const bool act = cur[i] != RANS_NONE;
            const uint32_t p = rans_p1(sh_p1, act ? cur[i] : 0u);
            const uint32_t s = (uint32_t)x & 0xffffu;
            const uint32_t b = s >= 65536u - p ? 1u : 0u;
            const uint32_t f = b ? p : 65536u - p, cum = b ? 65536u - p : 0u;
            if (act) x = (uint64_t)f * (x >> 16) + s - cum;
            rd.take(x, act);
            if (act) { out[(t0 + i) * RANS_LANES + lane] = (uint8_t)b; occupied += b; }
        }
#pragma unroll
        for (int i = 0; i < RANS_BATCH; ++i) cur[i] = nxt[i];
    }
#undef OCC_FETCH
    rd.close(x, occupied, result + 2 * c.f);
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------------
// The batch entries and the single ones run the same two bodies below over a RansFrames; a single entry builds the RansFrames of one frame.
// slot, 3 x 16 x int64: words per frame [16] | per frame the encoder's sums[0], sums[1] or the decoder's occupied rows, unsound chunks [16][2]
// rest: the encoder's scratch, n x u32 (+ 64 bytes); the decoder has none
constexpr size_t OCC_SLOT_BYTES = 3 * RANS_MAX_FRAMES * sizeof(long long);
constexpr int OCC_OPTS = RANS_EMPTY_HEAD;
static_assert(OCC_SLOT_BYTES <= RANS_SLOT_MAX, "the pinned host slot holds every coder's slot");

extern "C" int64_t pcgc_occ_rans_batch_workspace_bytes(int64_t n, int64_t chunks) {
    if (n < 0) n = 0;
    if (chunks < 0) chunks = 0;
    return (int64_t)OCC_SLOT_BYTES + (int64_t)rans_offs_bytes(chunks) + n * 4 + 64;
}
extern "C" size_t pcgc_occ_rans_workspace_bytes(int64_t n, int steps) {
    if (n < 0) n = 0;
    if (steps < 1) steps = 1;
    return (size_t)pcgc_occ_rans_batch_workspace_bytes(n, rans_chunks(n, steps));
}

// host [3 frames] = every frame's payload bytes (8 + 516 K_f + 4 words), then every frame's sums[0], then every frame's sums[1] (0 without sums)
static int occ_encode(const char* who, const uint16_t* packed, const RansFrames& fr, const int64_t* sums, uint8_t* payload, int64_t* host, void* workspace,
                      size_t workspace_bytes, hipStream_t s) {
    const int frames = fr.frames;
    RansWork w;
    if (int r = rans_begin(who, fr, workspace, workspace_bytes, OCC_SLOT_BYTES, (size_t)fr.first[frames] * 4 + 64, w, s)) return r;
    if (fr.chunk[frames]) {
        hipLaunchKernelGGL(k_occ_rans_encode, dim3((unsigned)fr.chunk[frames]), dim3(RANS_LANES), 0, s, packed, fr, (uint32_t*)w.rest, payload);
        PCGC_CHECK_LAUNCH(who + 5);
    }
    if (int r = rans_pack(who, fr, w, payload, OCC_OPTS, (const long long*)sums, s)) return r;
    if (int r = rans_end(who, w, (size_t)RANS_MAX_FRAMES + 2 * frames, s)) return r;
    for (int f = 0; f < frames; ++f) {
        host[f] = rans_payload_bytes(fr, f, w.host[f], OCC_OPTS);
        host[frames + f] = sums ? (int64_t)w.host[RANS_MAX_FRAMES + 2 * f] : 0;
        host[2 * frames + f] = sums ? (int64_t)w.host[RANS_MAX_FRAMES + 2 * f + 1] : 0;
    }
    return 0;
}
// fr.words[f]: the words of frame f's payload behind its tables.  host [2 frames] = every frame's occupied rows, then its unsound chunks (+ 1:
// the word counts do not add up to the payload); 0 and 0 for a frame that is not decoded here
static int occ_decode(const char* who, const uint16_t* packed, const RansFrames& fr, const uint8_t* payload, uint8_t* mask, int64_t* host, void* workspace,
                      size_t workspace_bytes, hipStream_t s) {
    const int frames = fr.frames;
    RansWork w;
    if (int r = rans_begin(who, fr, workspace, workspace_bytes, OCC_SLOT_BYTES, 0, w, s)) return r;
    if (int r = rans_offsets(who, fr, w, payload, s)) return r;
    if (fr.chunk[frames]) {
        hipLaunchKernelGGL(k_occ_rans_decode, dim3((unsigned)fr.chunk[frames]), dim3(RANS_LANES), 0, s, packed, fr, payload, (const uint32_t*)w.offs, mask,
                           (unsigned long long*)(w.slot + RANS_MAX_FRAMES));
        PCGC_CHECK_LAUNCH(who + 5);
    }
    if (int r = rans_end(who, w, (size_t)RANS_MAX_FRAMES + 2 * frames, s)) return r;
    for (int f = 0; f < frames; ++f) {
        const bool here = fr.steps[f] > 0;
        host[f] = here ? (int64_t)w.host[RANS_MAX_FRAMES + 2 * f] : 0;
        host[frames + f] = here ? (int64_t)w.host[RANS_MAX_FRAMES + 2 * f + 1] + (w.host[f] != fr.words[f] ? 1 : 0) : 0;
    }
    return 0;
}

// ---- one level: host3 = {payload bytes, sums[0], sums[1]} and host2 = {occupied rows, unsound chunks} are the bodies' answers for frame 0
extern "C" int pcgc_occ_rans_encode(const uint16_t* packed, int64_t n, int steps, const int64_t* sums, uint8_t* payload, size_t payload_capacity,
                                    int64_t* host3, void* workspace, size_t workspace_bytes, void* stream) {
    PCGC_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "bad row count");
    PCGC_REQUIRE(steps >= 1 && steps <= RANS_MAX_STEPS, "steps per chunk outside 1 .. 2^24");
    PCGC_REQUIRE((n == 0 || packed) && payload && host3, "null argument");
    RansFrames fr;
    PCGC_REQUIRE(rans_frame_of_one(n, steps, fr), "bad row count");
    PCGC_REQUIRE(payload_capacity >= (size_t)rans_room(fr.chunk[1], n) && ((uintptr_t)payload & 7) == 0, "payload buffer too small or misaligned");
    return occ_encode(__func__, packed, fr, sums, payload, host3, workspace, workspace_bytes, S(stream));
}

extern "C" int pcgc_occ_rans_decode(const uint16_t* packed, int64_t n, const uint8_t* payload, int64_t payload_bytes, int steps, uint8_t* mask,
                                    int64_t* host2, void* workspace, size_t workspace_bytes, void* stream) {
    PCGC_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "bad row count");
    PCGC_REQUIRE((n == 0 || (packed && mask)) && payload && host2, "null argument");
    PCGC_REQUIRE(((uintptr_t)payload & 7) == 0, "payload misaligned");
    PCGC_REQUIRE(steps >= 1 && steps <= RANS_MAX_STEPS, "steps per chunk outside 1 .. 2^24");
    RansFrames fr;
    PCGC_REQUIRE(rans_frame_of_one(n, steps, fr), "bad row count");
    // (the head's own S and K are the caller's to compare: ops.occ_rans_decode)
    PCGC_REQUIRE(rans_words_of(fr, 0, payload_bytes), "payload cut inside its tables or not whole words");
    return occ_decode(__func__, packed, fr, payload, mask, host2, workspace, workspace_bytes, S(stream));
}

// ---- a batch of frames
extern "C" int pcgc_occ_rans_encode_batch(const uint16_t* packed, int frames, const int64_t* row, const int32_t* steps, const int64_t* sums, uint8_t* payload,
                                          const int64_t* pay, int64_t* host, void* workspace, size_t workspace_bytes, void* stream) {
    RansFrames fr;
    PCGC_REQUIRE(rans_frames_of(frames, row, steps, pay, fr, OCC_OPTS | RANS_NEED_STEPS), "1 to 16 frames; row offsets ascending from 0 and below 2^31; steps per chunk 1 .. 2^24; payload offsets multiples of 8");
    PCGC_REQUIRE((fr.first[frames] == 0 || packed) && payload && host && ((uintptr_t)payload & 7) == 0, "null argument or payload misaligned");
    for (int f = 0; f < frames; ++f)
        PCGC_REQUIRE(pay[f + 1] - pay[f] >= rans_room(fr.chunk[f + 1] - fr.chunk[f], row[f + 1] - row[f]), "payload room of a frame too small (below 8 + 516 K + 4 n bytes)");
    return occ_encode(__func__, packed, fr, sums, payload, host, workspace, workspace_bytes, S(stream));
}

extern "C" int pcgc_occ_rans_decode_batch(const uint16_t* packed, int frames, const int64_t* row, const int32_t* steps, const uint8_t* payload, const int64_t* pay,
                                          const int64_t* pay_bytes, uint8_t* mask, int64_t* host, void* workspace, size_t workspace_bytes, void* stream) {
    RansFrames fr;
    PCGC_REQUIRE(rans_frames_of(frames, row, steps, pay, fr, OCC_OPTS), "1 to 16 frames; row offsets ascending from 0 and below 2^31; steps per chunk 0 .. 2^24; payload offsets multiples of 8");
    PCGC_REQUIRE((fr.chunk[frames] == 0 || (packed && mask && payload)) && pay_bytes && host && ((uintptr_t)payload & 7) == 0, "null argument or payload misaligned");
    for (int f = 0; f < frames; ++f)
        PCGC_REQUIRE(!steps[f] || rans_words_of(fr, f, pay_bytes[f]), "a payload cut inside its tables or not whole words");
    return occ_decode(__func__, packed, fr, payload, mask, host, workspace, workspace_bytes, S(stream));
}
