// The interleaved rANS core that the occupancy stream's coder (occupancy_rans.hip, `_O.bin` version 2) and the colour stream's coder
// (attribute_rans.hip, `_A.bin` version 2) share; DESIGN.md 8n.  A coder supplies its symbol model only: which unit (a row, a token) a
// lane codes at a step, and that unit's frequency f and cumulative c in 16 bits.  Everything else is here, once:
//
//   geometry  one wave per chunk of 64 S units; lane j codes units base + 64 t + j.  64-bit state, 32-bit words, L = 2^31.  A batch of
//             frames goes through ONE launch sequence: every kernel takes a frames table (RansFrames) and a workgroup serves a chunk of one
//             frame; a single frame is the batch of one.  A frame's payload: head S | K [8 bytes], states [K x 64 x u64], W_k [K x u32], words.
//   encoder   steps t = S - 1 .. 0.  Which lanes renormalise at a step is a ballot, where each lane's word goes is the prefix popcount of
//             that ballot (rans_put).  The emitting lanes write their words, in ascending lane order, just below the words of the later
//             steps, downwards from the end of the chunk's scratch (one word per unit at most: `rows` words is the capacity).  Memory then
//             holds the stream in the decoder's order; an offsets scan and a compaction (rans_pack) move each chunk's words to their place.
//   decoder   steps t = 0 .. S - 1.  The stream is consumed strictly in order, so the chunk's words are staged through a ring in LDS, 512 at
//             a time, the next 512 already on their way in registers (RansReader).  A word index at or past W_k reads as 0; the chunk is
//             sound iff its states were in [2^31, 2^63), exactly W_k words were consumed and every lane ends at L.
//
// SOUNDNESS, read here and nowhere else: no read leaves the chunk's words, whatever the bytes say.  The only addresses formed from payload
// bytes are a chunk's word offset and count.  k_rans_offsets saturates the offsets it sums from the W_k; RansReader::open clamps offset and
// count into the frame's words (`avail`), whose number the host derived from the payload's own length (rans_words_of); every later index
// is compared with `avail` before it is used.  All integer arithmetic: the bytes are a function of the input alone.
#pragma once
#include <type_traits>
#include "pcgc_common.h"

constexpr int RANS_LANES = 64;
constexpr int RANS_BATCH = 8;                                 // steps whose units are fetched together
constexpr int RANS_FILL = RANS_BATCH * RANS_LANES;            // words a batch can consume at most = words staged at a time
constexpr int RANS_RING = 2 * RANS_FILL;
constexpr int RANS_MAX_STEPS = 1 << 24;                       // 64 S units per chunk stay below 2^31
constexpr uint64_t RANS_L = 1ull << 31;
constexpr uint64_t RANS_STATE_END = 1ull << 63;
constexpr int RANS_SCAN_BLOCK = 256;
constexpr uint32_t RANS_NONE = 0xffffffffu;                   // a fetched word that stands for "no unit for this lane at this step"

// Frame f is the contiguous units first[f] .. first[f + 1] of the coder's input and output, cut into K_f chunks of 64 S_f units from its own
// first unit, so chunks never straddle frames; its payload stands at byte pay[f] of the payload buffer.  The table travels by value; chunk
// k of the launch belongs to the last frame f with chunk[f] <= k.  A frame without chunks (no units, or steps = 0: "not decoded here") is
// served by no workgroup.
constexpr int RANS_MAX_FRAMES = 16;
struct RansFrames {
    long long first[RANS_MAX_FRAMES + 1];      // first unit of the frame; first[f] = all units for f >= frames
    long long pay[RANS_MAX_FRAMES];            // byte offset of the frame's payload in the payload buffer, a multiple of 8
    long long words[RANS_MAX_FRAMES];          // decoder: 32-bit words the frame's payload holds behind its tables
    int chunk[RANS_MAX_FRAMES + 1];            // first chunk of the frame; chunk[f] = all chunks for f >= frames
    int steps[RANS_MAX_FRAMES];
    int frames;
};
// chunk blockIdx.x of the launch: its frame f, the frame's S and K, the chunk's place k in the frame, its first unit and its units
struct RansChunk { int f, S, rows; int64_t k, K, base; };
__device__ static inline RansChunk rans_chunk_of(const RansFrames& fr) {
    RansChunk c;
    c.f = 0;
    for (int b = 1; b < RANS_MAX_FRAMES; ++b) c.f += (b < fr.frames && (int64_t)fr.chunk[b] <= (int64_t)blockIdx.x) ? 1 : 0;     // (chunk[] ascends)
    c.S = fr.steps[c.f];
    c.k = (int64_t)blockIdx.x - fr.chunk[c.f];
    c.K = fr.chunk[c.f + 1] - fr.chunk[c.f];
    const int64_t n = fr.first[c.f + 1] - fr.first[c.f], in_frame = c.k * RANS_LANES * c.S;
    c.rows = (int)(n - in_frame < (int64_t)RANS_LANES * c.S ? n - in_frame : (int64_t)RANS_LANES * c.S);
    c.base = fr.first[c.f] + in_frame;
    return c;
}
// the parts of a frame's payload behind its head (B: uint8_t or const uint8_t; what comes back is const with it)
template <class B, class T> using rans_cv = std::conditional_t<std::is_const<B>::value, const T, T>;
template <class B> __device__ static inline auto rans_states(B* mine) { return (rans_cv<B, unsigned long long>*)(mine + 8); }
template <class B> __device__ static inline auto rans_wcount(B* mine, int64_t K) { return (rans_cv<B, uint32_t>*)(mine + 8 + 512 * K); }
template <class B> __device__ static inline auto rans_words(B* mine, int64_t K) { return (rans_cv<B, uint32_t>*)(mine + 8 + 516 * K); }

__device__ static inline int rans_lanes_below(uint64_t m) {
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}
// exact x / f and x % f for x < f << 47, 1 <= f <= 65535: schoolbook division in base 2^16 below the top 32 bits.  Each remainder is < f,
// so every partial dividend r << 16 | digit is < 2^32 and every partial quotient after the first is < 2^16.
__device__ static inline void rans_divmod(uint64_t x, uint32_t f, uint64_t& q, uint32_t& r) {
    const uint32_t a = (uint32_t)(x >> 32), b = (uint32_t)x;
    const uint32_t q1 = a / f, r1 = a - q1 * f;
    const uint32_t d2 = (r1 << 16) | (b >> 16);
    const uint32_t q2 = d2 / f, r2 = d2 - q2 * f;
    const uint32_t d3 = (r2 << 16) | (b & 0xffffu);
    const uint32_t q3 = d3 / f;
    r = d3 - q3 * f;
    q = ((uint64_t)q1 << 32) | ((uint64_t)q2 << 16) | (uint64_t)q3;
}

// ---- encoder: one step of one lane.  act (1 <= f <= 65535 then): the lane codes a unit of frequency f and cumulative c at this step.
// out: the chunk's scratch, of which [top, rows) are written; top stays >= 0, a unit emits one word at most.
__device__ __forceinline__ void rans_put(uint64_t& x, int& top, uint32_t* __restrict__ out, bool act, uint32_t f, uint32_t c) {
    const bool emit = act && x >= ((uint64_t)f << 47);
    const uint64_t m = __ballot(emit);
    const int total = __popcll(m);
    if (emit) {
        out[top - total + rans_lanes_below(m)] = (uint32_t)x;
        x >>= 32;
    }
    top -= total;
    if (act) {
        uint64_t q; uint32_t r;
        rans_divmod(x, f, q, r);
        x = (q << 16) + r + c;
    }
}
// the chunk's 64 final states and its word count, into its frame's payload
__device__ __forceinline__ void rans_put_end(uint8_t* mine, const RansChunk& c, uint64_t x, int top) {
    rans_states(mine)[c.k * RANS_LANES + threadIdx.x] = x;
    if (threadIdx.x == 0) rans_wcount(mine, c.K)[c.k] = (uint32_t)(c.rows - top);
}

// ---- decoder: the words of one chunk, in stream order, for the lanes of one wave
struct RansReader {
    const uint32_t* __restrict__ src;          // the chunk's words: [0, avail) may be read
    uint32_t* ring;                            // RANS_RING words of LDS; holds stream indices [pos, filled)
    uint32_t W, avail, pos, filled;
    uint32_t stage[RANS_BATCH];                // words [filled, filled + RANS_FILL), on their way
    bool bad;

    __device__ __forceinline__ void stage_from(uint32_t from) {
#pragma unroll
        for (int i = 0; i < RANS_BATCH; ++i) {
            const uint32_t idx = from + (uint32_t)(i * RANS_LANES + threadIdx.x);
            stage[i] = idx < avail ? src[idx] : 0u;
        }
    }
    // -> this lane's initial state.  The words this chunk may read lie inside both its own count and its frame's payload.
    __device__ __forceinline__ uint64_t open(const RansFrames& fr, const RansChunk& c, const uint8_t* __restrict__ payload,
                                             const uint32_t* __restrict__ offs, uint32_t* ring_) {
        const uint8_t* mine = payload + fr.pay[c.f];
        const int64_t words_total = fr.words[c.f];
        W = rans_wcount(mine, c.K)[c.k];
        const int64_t off = (int64_t)offs[blockIdx.x];
        avail = off >= words_total ? 0u : (uint32_t)((int64_t)W < words_total - off ? (int64_t)W : words_total - off);
        src = rans_words(mine, c.K) + (off < words_total ? off : 0);
        ring = ring_;
        const uint64_t x = rans_states(mine)[c.k * RANS_LANES + threadIdx.x];
        bad = x < RANS_L || x >= RANS_STATE_END || avail != W;
        pos = filled = 0;
        stage_from(0u);
        return x;
    }
    // before every batch of RANS_BATCH steps: the ring then holds what the batch can consume
    __device__ __forceinline__ void refill() {
        if (filled - pos < (uint32_t)RANS_FILL) {             // (uniform) the slots written held words below pos: filled - pos <= RING - FILL
#pragma unroll
            for (int i = 0; i < RANS_BATCH; ++i) ring[(filled + (uint32_t)(i * RANS_LANES + threadIdx.x)) & (RANS_RING - 1)] = stage[i];
            filled += RANS_FILL;
            stage_from(filled);
            __syncthreads();
        }
    }
    // after a step's state update: the lanes below L take the next words in ascending lane order
    __device__ __forceinline__ void take(uint64_t& x, bool act) {
        const bool need = act && x < RANS_L;
        const uint64_t m = __ballot(need);
        if (need) x = (x << 32) | ring[(pos + (uint32_t)rans_lanes_below(m)) & (RANS_RING - 1)];
        pos += (uint32_t)__popcll(m);
    }
    // the verdict, and the model's count of this lane summed over the wave: result[0] += counts, result[1] += 1 for an unsound chunk
    __device__ __forceinline__ void close(uint64_t x, unsigned count, unsigned long long* __restrict__ result) {
        bad = bad || x != RANS_L || pos != W;
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) count += __shfl_xor(count, d, 64);
        const bool any_bad = __ballot(bad) != 0;
        if (threadIdx.x == 0) {                               // (integer atomics: the sums do not depend on the order)
            atomicAdd(result, (unsigned long long)count);
            if (any_bad) atomicAdd(result + 1, 1ull);
        }
    }
};

// ---- host side (rans_core.hip) ---------------------------------------------------------------------------------------------------------------
// workspace of every entry: [slot: words per frame [16], then the coder's own per-frame numbers][offs: K x u32, padded to 8 bytes][rest]
static inline int64_t rans_chunks(int64_t n, int steps) { return (n + (int64_t)RANS_LANES * steps - 1) / ((int64_t)RANS_LANES * steps); }
static inline size_t rans_offs_bytes(int64_t K) { return (size_t)((K * 4 + 7) / 8 * 8); }
static inline int64_t rans_room(int64_t K, int64_t n) { return 8 + 516 * K + 4 * n; }       // a frame's payload at most
constexpr size_t RANS_SLOT_MAX = 4 * RANS_MAX_FRAMES * sizeof(long long);                     // the pinned host slot; no coder's slot is longer

#define RANS_REQUIRE(who, cond, msg) do { if (!(cond)) { pcgc_set_error("%s: %s", who, msg); return -2; } } while (0)
#define RANS_CHECK_HIP(who, e) do { if ((e) != hipSuccess) { pcgc_set_error("%s: %s", (who) + 5, hipGetErrorString(e)); return -1; } } while (0)

enum {
    RANS_NEED_STEPS = 1,       // a frame that has a payload has steps >= 1 (the encoders' demand; else 0 = "not decoded here")
    RANS_THIRDS = 2,           // unit counts in multiples of 3 (the colour batch entries' demand)
    RANS_EMPTY_HEAD = 4,       // a frame without units still has its 8-byte head S | 0 (occupancy); else its payload is empty (colour)
};
// fills fr from the host arrays; false when they are not a batch: 1 to 16 frames, first ascending from 0 and below 2^31, steps in 0 .. 2^24,
// payload offsets non-negative multiples of 8, fewer than 2^31 chunks in all
bool rans_frames_of(int frames, const int64_t* first, const int32_t* steps, const int64_t* pay, RansFrames& fr, int opts);
bool rans_frame_of_one(int64_t n, int steps, RansFrames& fr);
// fr.words[f] from the byte length of frame f's payload; false when it is cut inside its tables or not whole words
bool rans_words_of(RansFrames& fr, int f, int64_t bytes);
// bytes of frame f's finished payload, given its words
int64_t rans_payload_bytes(const RansFrames& fr, int f, long long words, int opts);

struct RansWork { long long *host, *slot; uint32_t* offs; void* rest; };
// the workspace checked (slot_bytes + offsets of all chunks + rest_bytes, 8-byte aligned) and carved, its slot zeroed
int rans_begin(const char* who, const RansFrames& fr, void* workspace, size_t workspace_bytes, size_t slot_bytes, size_t rest_bytes, RansWork& w, hipStream_t s);
// encoder, after its step kernel (rest = the scratch): heads, offsets, compaction.  sums: NULL or [frames][2] to copy behind the words
int rans_pack(const char* who, const RansFrames& fr, const RansWork& w, uint8_t* payload, int opts, const long long* sums, hipStream_t s);
// decoder, before its step kernel: the offsets of the chunks' words and slot[f] = the words the counts of frame f add up to
int rans_offsets(const char* who, const RansFrames& fr, const RansWork& w, const uint8_t* payload, hipStream_t s);
// the first `count` slots brought down to w.host, the stream synchronised
int rans_end(const char* who, const RansWork& w, size_t count, hipStream_t s);
