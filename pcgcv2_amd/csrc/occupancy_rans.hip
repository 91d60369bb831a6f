// Lossless mode, `_O.bin` version 2 (lossless.py): the occupancy bits of a decoder level coded ON THE DEVICE by interleaved rANS, so that
// only the coded bytes cross the bus.  Input is what pcgc_occ_symbols writes (packed[i] = ctx << 1 | bit); the format is stated in
// include/pcgc_hip.h and, in plain Python integers, in tests/rans_reference.py.
//
// One wave per chunk of 64 S rows; lane j codes rows base + 64 t + j, so a step's loads of `packed` are one coalesced 128-byte access.
// 64-bit state, 32-bit words, L = 2^31, 16-bit probabilities straight from P1 (occupancy_tables.h).  Which lanes renormalise at a step is a
// ballot, where each lane's word goes is the prefix popcount of that ballot.
//
//   encoder  steps t = S - 1 .. 0.  The emitting lanes of a step write their words, in ascending lane order, just below the words of the later
//            steps, downwards from the end of the chunk's scratch (one word per row at most: `rows` words is the capacity).  Memory then
//            holds the stream in the decoder's order, and a second small pass moves each chunk's words to their final offset.
//   decoder  steps t = 0 .. S - 1.  The stream is consumed strictly in order, so the chunk's words are staged through a ring in LDS, 512 at
//            a time, the next 512 already on their way in registers: the chain of a step is table lookup, multiply, compare, ballot, LDS read.
//            A word index at or past W_k reads as 0; the chunk is sound iff its states were in [2^31, 2^63), exactly W_k words were consumed
//            and every lane ends at L.  No read leaves the chunk's words, whatever the bytes say.
//
// The contexts of the next RANS_BATCH steps are loaded while the current ones are coded.  All integer arithmetic: the bytes are a function
// of the input alone.
//
// A batch of frames (the items of a collated batch at one decoder level) goes through ONE launch sequence: every kernel
// takes a frames table (OrFrames) and a workgroup serves a chunk of one frame; pcgc_occ_rans_encode / _decode are the batch of one.
#include <cstring>
#include "pcgc_common.h"
#include "occupancy_tables.h"

constexpr int RANS_LANES = 64;
constexpr int RANS_BATCH = 8;                                 // steps whose contexts are fetched together
constexpr int RANS_FILL = RANS_BATCH * RANS_LANES;            // words a batch can consume at most = words staged at a time
constexpr int RANS_RING = 2 * RANS_FILL;
constexpr int RANS_MAX_STEPS = 1 << 24;                       // 64 S rows per chunk stay below 2^31
constexpr uint64_t RANS_L = 1ull << 31;
constexpr uint64_t RANS_STATE_END = 1ull << 63;
constexpr int RANS_SCAN_BLOCK = 256;

__device__ static const uint16_t d_rans_p1[PCGC_OCC_CONTEXTS] = {PCGC_OCC_P1_VALUES};

__device__ static inline void rans_load_p1(uint32_t* sh) {
    for (int i = threadIdx.x; i < PCGC_OCC_CONTEXTS; i += RANS_LANES) sh[i] = d_rans_p1[i];
    __syncthreads();
}
__device__ static inline uint32_t rans_p1(const uint32_t* sh, uint32_t word) {
    const uint32_t ctx = word >> 1;                          // (a context outside the table cannot come from pcgc_occ_symbols; clamp it all the same)
    return sh[ctx < PCGC_OCC_CONTEXTS ? ctx : PCGC_OCC_CONTEXTS - 1];
}
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

static inline int64_t rans_chunks(int64_t n, int steps) { return (n + (int64_t)RANS_LANES * steps - 1) / ((int64_t)RANS_LANES * steps); }

// A batch of frames in ONE launch sequence; a single level is the batch of one (frames = 1, row = {0, n}, pay = {0}).  Frame f is the
// contiguous rows row[f] .. row[f + 1] of `packed` and of `mask`, cut into K_f chunks of 64 S_f rows from its own first row, so chunks never
// straddle frames; its payload, in the layout of one level, stands at byte pay[f] of the payload buffer.  The table below travels by value;
// chunk k of the launch belongs to the last frame f with chunk[f] <= k.  A frame without chunks (no rows, or on the decoder steps = 0: "not
// decoded here") is served by no workgroup.
constexpr int RANS_MAX_FRAMES = 16;
struct OrFrames {
    long long row[RANS_MAX_FRAMES + 1];        // first row of the frame; row[f] = all rows for f >= frames
    long long pay[RANS_MAX_FRAMES];            // byte offset of the frame's payload in the payload buffer, a multiple of 8
    long long words[RANS_MAX_FRAMES];          // decoder: 32-bit words the frame's payload holds behind its tables
    int chunk[RANS_MAX_FRAMES + 1];            // first chunk of the frame; chunk[f] = all chunks for f >= frames
    int steps[RANS_MAX_FRAMES];
    int frames;
};
// chunk blockIdx.x of the launch: its frame f, the frame's S and K, the chunk's place k in the frame, its first row and its rows
struct OrChunk { int f, S, rows; int64_t k, K, base; };
__device__ static inline OrChunk rans_chunk_of(const OrFrames& fr) {
    OrChunk c;
    c.f = 0;
    for (int b = 1; b < RANS_MAX_FRAMES; ++b) c.f += (b < fr.frames && (int64_t)fr.chunk[b] <= (int64_t)blockIdx.x) ? 1 : 0;     // (chunk[] ascends)
    c.S = fr.steps[c.f];
    c.k = (int64_t)blockIdx.x - fr.chunk[c.f];
    c.K = fr.chunk[c.f + 1] - fr.chunk[c.f];
    const int64_t n = fr.row[c.f + 1] - fr.row[c.f], in_frame = c.k * RANS_LANES * c.S;
    c.rows = (int)(n - in_frame < (int64_t)RANS_LANES * c.S ? n - in_frame : (int64_t)RANS_LANES * c.S);
    c.base = fr.row[c.f] + in_frame;
    return c;
}
// (a frame's payload: head [8 bytes], states [K x 64 x u64], word counts [K x u32], words)
__device__ static inline uint32_t* rans_wcount(uint8_t* mine, int64_t K) { return (uint32_t*)(mine + 8 + 512 * K); }
__device__ static inline const uint32_t* rans_wcount(const uint8_t* mine, int64_t K) { return (const uint32_t*)(mine + 8 + 512 * K); }

// ---- encoder ---------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(RANS_LANES) k_occ_rans_encode(const uint16_t* __restrict__ packed, OrFrames fr, uint32_t* __restrict__ scratch,
                                                                uint8_t* __restrict__ payload) {
    __shared__ uint32_t sh_p1[PCGC_OCC_CONTEXTS];
    rans_load_p1(sh_p1);
    const int lane = threadIdx.x;
    const OrChunk c = rans_chunk_of(fr);
    const int rows = c.rows;
    const uint16_t* __restrict__ in = packed + c.base;
    uint32_t* __restrict__ out = scratch + c.base;            // rows words: [top, rows) are written
    const int steps = (rows + RANS_LANES - 1) / RANS_LANES;   // steps that hold a row at all
    int top = rows;
    uint64_t x = RANS_L;
    uint32_t cur[RANS_BATCH], nxt[RANS_BATCH];
    // batch starting at step t0 holds steps t0, t0 - 1, ..; a word of 0xffffffff marks "no row"
#define RANS_FETCH(dst, t0)                                                                   \
    _Pragma("unroll") for (int i = 0; i < RANS_BATCH; ++i) {                                  \
        const int r = ((t0) - i) * RANS_LANES + lane;                                         \
        dst[i] = ((t0) - i >= 0 && r < rows) ? (uint32_t)in[r] : 0xffffffffu;                 \
    }
    RANS_FETCH(cur, steps - 1)
    for (int t0 = steps - 1; t0 >= 0; t0 -= RANS_BATCH) {
        RANS_FETCH(nxt, t0 - RANS_BATCH)
#pragma unroll
        for (int i = 0; i < RANS_BATCH; ++i) {
            const bool act = cur[i] != 0xffffffffu;
            const uint32_t p = rans_p1(sh_p1, act ? cur[i] : 0u), b = cur[i] & 1u;
            const uint32_t f = b ? p : 65536u - p, cum = b ? 65536u - p : 0u;
            const bool emit = act && x >= ((uint64_t)f << 47);
            const uint64_t m = __ballot(emit);
            const int total = __popcll(m);
            if (emit) {
                out[top - total + rans_lanes_below(m)] = (uint32_t)x;        // >= 0: a row emits one word at most
                x >>= 32;
            }
            top -= total;
            if (act) {
                uint64_t q; uint32_t r;
                rans_divmod(x, f, q, r);
                x = (q << 16) + r + cum;
            }
        }
#pragma unroll
        for (int i = 0; i < RANS_BATCH; ++i) cur[i] = nxt[i];
    }
#undef RANS_FETCH
    uint8_t* mine = payload + fr.pay[c.f];
    ((unsigned long long*)(mine + 8))[c.k * RANS_LANES + lane] = x;
    if (lane == 0) rans_wcount(mine, c.K)[c.k] = (uint32_t)(rows - top);
}

// block f: an exclusive scan of the word counts of frame f's chunks (thread t owns a run of consecutive chunks) -> offs [chunk[f] ..) counted
// from the frame's own first word (saturating: counts a decoder reads are not to be trusted), slot[f] = the frame's words.  Encoder side
// (with_head): also the payload's head — a frame without rows has the head S | 0 and nothing else — and, with sums (pcgc_occ_symbols' pair,
// or pcgc_occ_symbols_segments' pair per frame), aux[2 f ..] = sums[2 f ..], so that one small copy brings lengths and sums to the host.
__global__ void __launch_bounds__(RANS_SCAN_BLOCK) k_occ_rans_offsets(OrFrames fr, uint8_t* payload, uint32_t* __restrict__ offs, long long* __restrict__ slot,
                                                                      int with_head, const long long* __restrict__ sums, long long* __restrict__ aux) {
    __shared__ unsigned long long part[RANS_SCAN_BLOCK];
    const int f = blockIdx.x;
    const int64_t K = fr.chunk[f + 1] - fr.chunk[f];
    if (threadIdx.x == 0 && sums) { aux[2 * f] = sums[2 * f]; aux[2 * f + 1] = sums[2 * f + 1]; }
    if (K <= 0) {                                             // (uniform)
        if (threadIdx.x == 0) {
            slot[f] = 0;
            if (with_head) { ((uint32_t*)(payload + fr.pay[f]))[0] = (uint32_t)fr.steps[f]; ((uint32_t*)(payload + fr.pay[f]))[1] = 0u; }
        }
        return;
    }
    uint8_t* mine = payload + fr.pay[f];
    const uint32_t* __restrict__ wcount = rans_wcount(mine, K);
    offs += fr.chunk[f];
    const int64_t per = (K + RANS_SCAN_BLOCK - 1) / RANS_SCAN_BLOCK;
    const int64_t lo = (int64_t)threadIdx.x * per < K ? (int64_t)threadIdx.x * per : K, hi = lo + per < K ? lo + per : K;
    unsigned long long s = 0;
    for (int64_t i = lo; i < hi; ++i) s += wcount[i];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long run = 0;
        for (int i = 0; i < RANS_SCAN_BLOCK; ++i) { const unsigned long long v = part[i]; part[i] = run; run += v; }
        slot[f] = (long long)run;
        if (with_head) { ((uint32_t*)mine)[0] = (uint32_t)fr.steps[f]; ((uint32_t*)mine)[1] = (uint32_t)K; }
    }
    __syncthreads();
    unsigned long long run = part[threadIdx.x];
    for (int64_t i = lo; i < hi; ++i) { offs[i] = run < 0xffffffffull ? (uint32_t)run : 0xffffffffu; run += wcount[i]; }
}

// a chunk's words, from the end of its scratch to their place in its frame's payload
__global__ void __launch_bounds__(RANS_SCAN_BLOCK) k_occ_rans_compact(const uint32_t* __restrict__ scratch, OrFrames fr, const uint32_t* __restrict__ offs,
                                                                      uint8_t* __restrict__ payload) {
    const OrChunk c = rans_chunk_of(fr);
    const uint32_t* wcount = rans_wcount(payload + fr.pay[c.f], c.K);
    const uint32_t W = wcount[c.k];                           // <= rows: the encoder wrote it
    const uint32_t* __restrict__ src = scratch + c.base + c.rows - W;
    uint32_t* __restrict__ dst = (uint32_t*)(wcount + c.K) + offs[blockIdx.x];
    for (uint32_t i = threadIdx.x; i < W; i += RANS_SCAN_BLOCK) dst[i] = src[i];
}

// ---- decoder ---------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(RANS_LANES) k_occ_rans_decode(const uint16_t* __restrict__ packed, OrFrames fr, const uint8_t* __restrict__ payload,
                                                                const uint32_t* __restrict__ offs, uint8_t* __restrict__ mask,
                                                                unsigned long long* __restrict__ result /*per frame: occupied rows, unsound chunks*/) {
    __shared__ uint32_t sh_p1[PCGC_OCC_CONTEXTS];
    __shared__ uint32_t ring[RANS_RING];
    rans_load_p1(sh_p1);
    const int lane = threadIdx.x;
    const OrChunk c = rans_chunk_of(fr);
    const int rows = c.rows;
    const int steps = (rows + RANS_LANES - 1) / RANS_LANES;
    const uint16_t* __restrict__ in = packed + c.base;
    uint8_t* __restrict__ out = mask + c.base;
    const uint8_t* mine = payload + fr.pay[c.f];
    const uint32_t* wcount = rans_wcount(mine, c.K);
    const uint32_t* __restrict__ words = wcount + c.K;
    const int64_t words_total = fr.words[c.f];
    const uint32_t W = wcount[c.k];
    const int64_t off = (int64_t)offs[blockIdx.x];
    // the words this chunk may read: [0, avail) of src, inside both its own count and its frame's payload
    const uint32_t avail = off >= words_total ? 0u : (uint32_t)((int64_t)W < words_total - off ? (int64_t)W : words_total - off);
    const uint32_t* __restrict__ src = words + (off < words_total ? off : 0);
    uint64_t x = ((const unsigned long long*)(mine + 8))[c.k * RANS_LANES + lane];
    bool bad = x < RANS_L || x >= RANS_STATE_END || avail != W;
    uint32_t pos = 0, filled = 0;                             // stream indices: the ring holds [pos, filled)
    uint32_t stage[RANS_BATCH];                               // words [filled, filled + RANS_FILL), on their way
#define RANS_STAGE(from)                                                                      \
    _Pragma("unroll") for (int i = 0; i < RANS_BATCH; ++i) {                                  \
        const uint32_t idx = (from) + (uint32_t)(i * RANS_LANES + lane);                      \
        stage[i] = idx < avail ? src[idx] : 0u;                                               \
    }
#define RANS_FETCH(dst, t0)                                                                   \
    _Pragma("unroll") for (int i = 0; i < RANS_BATCH; ++i) {                                  \
        const int r = ((t0) + i) * RANS_LANES + lane;                                         \
        dst[i] = r < rows ? (uint32_t)in[r] : 0xffffffffu;                                    \
    }
    RANS_STAGE(0u)
    uint32_t cur[RANS_BATCH], nxt[RANS_BATCH];
    RANS_FETCH(cur, 0)
    unsigned occupied = 0;
    for (int t0 = 0; t0 < steps; t0 += RANS_BATCH) {
        RANS_FETCH(nxt, t0 + RANS_BATCH)
        if (filled - pos < (uint32_t)RANS_FILL) {             // (uniform) the slots written held words below pos: filled - pos <= RING - FILL
#pragma unroll
            for (int i = 0; i < RANS_BATCH; ++i) ring[(filled + (uint32_t)(i * RANS_LANES + lane)) & (RANS_RING - 1)] = stage[i];
            filled += RANS_FILL;
            RANS_STAGE(filled)
            __syncthreads();
        }
#pragma unroll
        for (int i = 0; i < RANS_BATCH; ++i) {
            const bool act = cur[i] != 0xffffffffu;
            const uint32_t p = rans_p1(sh_p1, act ? cur[i] : 0u);
            const uint32_t s = (uint32_t)x & 0xffffu;
            const uint32_t b = s >= 65536u - p ? 1u : 0u;
            const uint32_t f = b ? p : 65536u - p, cum = b ? 65536u - p : 0u;
            if (act) x = (uint64_t)f * (x >> 16) + s - cum;
            const bool need = act && x < RANS_L;
            const uint64_t m = __ballot(need);
            if (need) x = (x << 32) | ring[(pos + (uint32_t)rans_lanes_below(m)) & (RANS_RING - 1)];
            pos += (uint32_t)__popcll(m);
            if (act) { out[(t0 + i) * RANS_LANES + lane] = (uint8_t)b; occupied += b; }
        }
#pragma unroll
        for (int i = 0; i < RANS_BATCH; ++i) cur[i] = nxt[i];
    }
#undef RANS_FETCH
#undef RANS_STAGE
    bad = bad || x != RANS_L || pos != W;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) occupied += __shfl_xor(occupied, d, 64);
    const bool any_bad = __ballot(bad) != 0;
    if (lane == 0) {                                          // (integer atomics: the sums do not depend on the order)
        atomicAdd(result + 2 * c.f, (unsigned long long)occupied);
        if (any_bad) atomicAdd(result + 2 * c.f + 1, 1ull);
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------------
// The batch entries and the single ones run the same two bodies below over an OrFrames; a single entry builds the OrFrames of one frame.
// workspace: [slot][offs: K x u32, padded to 8 bytes][encoder only: scratch, n x u32]
//   slot of a single level, 4 x int64:   words | encoder: sums[0], sums[1]; decoder: occupied rows, unsound chunks
//   slot of a batch, 3 x 16 x int64:     words per frame [16] | the same pair per frame [16][2]
// i.e. the pairs stand `lead` int64 behind the words, lead = 1 for a single level and 16 for a batch.
constexpr size_t RANS_SLOT_ONE = 32, RANS_SLOT_BATCH = 3 * RANS_MAX_FRAMES * sizeof(long long);
static size_t rans_offs_bytes(int64_t K) { return (size_t)((K * 4 + 7) / 8 * 8); }

extern "C" size_t pcgc_occ_rans_workspace_bytes(int64_t n, int steps) {
    if (n < 0) n = 0;
    if (steps < 1) steps = 1;
    return RANS_SLOT_ONE + rans_offs_bytes(rans_chunks(n, steps)) + (size_t)n * 4 + 64;
}
extern "C" int64_t pcgc_occ_rans_batch_workspace_bytes(int64_t n, int64_t chunks) {
    if (n < 0) n = 0;
    if (chunks < 0) chunks = 0;
    return (int64_t)RANS_SLOT_BATCH + (int64_t)rans_offs_bytes(chunks) + n * 4 + 64;
}

static long long* rans_host_slot() {
    static thread_local long long* host = nullptr;
    if (!host && hipHostMalloc((void**)&host, RANS_SLOT_BATCH, hipHostMallocDefault) != hipSuccess) host = nullptr;
    return host;
}

#define RANS_REQUIRE(who, cond, msg) do { if (!(cond)) { pcgc_set_error("%s: %s", who, msg); return -2; } } while (0)
#define RANS_CHECK_HIP(who, e) do { if ((e) != hipSuccess) { pcgc_set_error("%s: %s", (who) + 5, hipGetErrorString(e)); return -1; } } while (0)

// fills fr from the host arrays; false when they are not a batch: 1 to 16 frames, row ascending from 0 and below 2^31, steps in range (all:
// at least 1 for every frame, the encoder's demand; else 0 = "not decoded here"), payload offsets non-negative multiples of 8
static bool rans_frames_of(int frames, const int64_t* row, const int32_t* steps, const int64_t* pay, OrFrames& fr, bool all) {
    memset(&fr, 0, sizeof(fr));
    if (frames < 1 || frames > RANS_MAX_FRAMES || !row || !steps || !pay || row[0] != 0) return false;
    fr.frames = frames;
    int64_t K = 0;
    for (int f = 0; f < frames; ++f) {
        const int64_t n = row[f + 1] - row[f];
        if (n < 0 || row[f + 1] >= ((int64_t)1 << 31) || steps[f] < (all ? 1 : 0) || steps[f] > RANS_MAX_STEPS || (pay[f] & 7) || pay[f] < 0) return false;
        fr.row[f] = row[f]; fr.pay[f] = pay[f]; fr.steps[f] = steps[f]; fr.chunk[f] = (int)K;
        K += steps[f] > 0 ? rans_chunks(n, steps[f]) : 0;
    }
    for (int f = frames; f <= RANS_MAX_FRAMES; ++f) { fr.row[f] = row[frames]; fr.chunk[f] = (int)K; }      // (K <= rows / 64 + frames: an int)
    return true;
}
static bool rans_frame_of_one(int64_t n, int steps, OrFrames& fr) {
    const int64_t row[2] = {0, n}, pay = 0;
    const int32_t s = steps;
    return rans_frames_of(1, row, &s, &pay, fr, true);
}
// the first `count` slots brought down, the stream synchronised
static int rans_end(const char* who, long long* host, const long long* slot, size_t count, hipStream_t s) {
    hipError_t e = hipMemcpyAsync(host, slot, count * sizeof(long long), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    RANS_CHECK_HIP(who, e);
    return 0;
}

// host [3 frames] = every frame's payload bytes (8 + 516 K_f + 4 words), then every frame's sums[0], then every frame's sums[1] (0 without sums)
static int rans_encode(const char* who, const uint16_t* packed, const OrFrames& fr, const int64_t* sums, uint8_t* payload, int64_t* host, void* workspace,
                       size_t workspace_bytes, size_t slot_bytes, hipStream_t s) {
    const int frames = fr.frames, lead = slot_bytes == RANS_SLOT_ONE ? 1 : RANS_MAX_FRAMES;
    const int64_t n = fr.row[frames], K = fr.chunk[frames];
    RANS_REQUIRE(who, workspace && workspace_bytes >= slot_bytes + rans_offs_bytes(K) + (size_t)n * 4 + 64 && ((uintptr_t)workspace & 7) == 0,
                 "workspace too small or misaligned");
    long long* slot = (long long*)workspace;
    uint32_t* offs = (uint32_t*)((char*)workspace + slot_bytes);
    uint32_t* scratch = (uint32_t*)((char*)workspace + slot_bytes + rans_offs_bytes(K));
    long long* hostslot = rans_host_slot();
    if (!hostslot) { pcgc_set_error("%s: cannot allocate pinned memory", who + 5); return -1; }
    if (K) {
        hipLaunchKernelGGL(k_occ_rans_encode, dim3((unsigned)K), dim3(RANS_LANES), 0, s, packed, fr, scratch, payload);
        PCGC_CHECK_LAUNCH(who + 5);
    }
    hipLaunchKernelGGL(k_occ_rans_offsets, dim3((unsigned)frames), dim3(RANS_SCAN_BLOCK), 0, s, fr, payload, offs, slot, 1, (const long long*)sums, slot + lead);
    PCGC_CHECK_LAUNCH(who + 5);
    if (K) {
        hipLaunchKernelGGL(k_occ_rans_compact, dim3((unsigned)K), dim3(RANS_SCAN_BLOCK), 0, s, (const uint32_t*)scratch, fr, (const uint32_t*)offs, payload);
        PCGC_CHECK_LAUNCH(who + 5);
    }
    if (int r = rans_end(who, hostslot, slot, (size_t)lead + 2 * frames, s)) return r;
    for (int f = 0; f < frames; ++f) {
        host[f] = 8 + 516 * (int64_t)(fr.chunk[f + 1] - fr.chunk[f]) + 4 * (int64_t)hostslot[f];
        host[frames + f] = sums ? (int64_t)hostslot[lead + 2 * f] : 0;
        host[2 * frames + f] = sums ? (int64_t)hostslot[lead + 2 * f + 1] : 0;
    }
    return 0;
}
// fr.words[f]: the words of frame f's payload behind its tables.  host [2 frames] = every frame's occupied rows, then its unsound chunks (+ 1:
// the word counts do not add up to the payload); 0 and 0 for a frame that is not decoded here
static int rans_decode(const char* who, const uint16_t* packed, const OrFrames& fr, const uint8_t* payload, uint8_t* mask, int64_t* host, void* workspace,
                       size_t workspace_bytes, size_t slot_bytes, hipStream_t s) {
    const int frames = fr.frames, lead = slot_bytes == RANS_SLOT_ONE ? 1 : RANS_MAX_FRAMES;
    const int64_t K = fr.chunk[frames];
    RANS_REQUIRE(who, workspace && workspace_bytes >= slot_bytes + rans_offs_bytes(K) && ((uintptr_t)workspace & 7) == 0, "workspace too small or misaligned");
    long long* slot = (long long*)workspace;
    uint32_t* offs = (uint32_t*)((char*)workspace + slot_bytes);
    long long* hostslot = rans_host_slot();
    if (!hostslot) { pcgc_set_error("%s: cannot allocate pinned memory", who + 5); return -1; }
    hipError_t e = hipMemsetAsync(slot, 0, slot_bytes, s);
    RANS_CHECK_HIP(who, e);
    hipLaunchKernelGGL(k_occ_rans_offsets, dim3((unsigned)frames), dim3(RANS_SCAN_BLOCK), 0, s, fr, const_cast<uint8_t*>(payload), offs, slot, 0,
                       (const long long*)nullptr, (long long*)nullptr);
    PCGC_CHECK_LAUNCH(who + 5);
    if (K) {
        hipLaunchKernelGGL(k_occ_rans_decode, dim3((unsigned)K), dim3(RANS_LANES), 0, s, packed, fr, payload, (const uint32_t*)offs, mask,
                           (unsigned long long*)(slot + lead));
        PCGC_CHECK_LAUNCH(who + 5);
    }
    if (int r = rans_end(who, hostslot, slot, (size_t)lead + 2 * frames, s)) return r;
    for (int f = 0; f < frames; ++f) {
        const bool here = fr.steps[f] > 0;
        host[f] = here ? (int64_t)hostslot[lead + 2 * f] : 0;
        host[frames + f] = here ? (int64_t)hostslot[lead + 2 * f + 1] + (hostslot[f] != fr.words[f] ? 1 : 0) : 0;
    }
    return 0;
}

// ---- one level: host3 = {payload bytes, sums[0], sums[1]} and host2 = {occupied rows, unsound chunks} are the bodies' answers for frame 0
extern "C" int pcgc_occ_rans_encode(const uint16_t* packed, int64_t n, int steps, const int64_t* sums, uint8_t* payload, size_t payload_capacity,
                                    int64_t* host3, void* workspace, size_t workspace_bytes, void* stream) {
    PCGC_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "bad row count");
    PCGC_REQUIRE(steps >= 1 && steps <= RANS_MAX_STEPS, "steps per chunk outside 1 .. 2^24");
    PCGC_REQUIRE((n == 0 || packed) && payload && host3, "null argument");
    OrFrames fr;
    PCGC_REQUIRE(rans_frame_of_one(n, steps, fr), "bad row count");
    PCGC_REQUIRE(payload_capacity >= (size_t)(8 + 516 * (int64_t)fr.chunk[1] + 4 * n) && ((uintptr_t)payload & 7) == 0, "payload buffer too small or misaligned");
    return rans_encode(__func__, packed, fr, sums, payload, host3, workspace, workspace_bytes, RANS_SLOT_ONE, S(stream));
}

extern "C" int pcgc_occ_rans_decode(const uint16_t* packed, int64_t n, const uint8_t* payload, int64_t payload_bytes, int steps, uint8_t* mask,
                                    int64_t* host2, void* workspace, size_t workspace_bytes, void* stream) {
    PCGC_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "bad row count");
    PCGC_REQUIRE((n == 0 || (packed && mask)) && payload && host2, "null argument");
    PCGC_REQUIRE(((uintptr_t)payload & 7) == 0, "payload misaligned");
    PCGC_REQUIRE(steps >= 1 && steps <= RANS_MAX_STEPS, "steps per chunk outside 1 .. 2^24");
    OrFrames fr;
    PCGC_REQUIRE(rans_frame_of_one(n, steps, fr), "bad row count");
    const int64_t K = fr.chunk[1];                    // (the head's own S and K are the caller's to compare: ops.occ_rans_decode)
    PCGC_REQUIRE(payload_bytes >= 8 + 516 * K && (payload_bytes - 8 - 516 * K) % 4 == 0, "payload cut inside its tables or not whole words");
    fr.words[0] = (payload_bytes - 8 - 516 * K) / 4;
    return rans_decode(__func__, packed, fr, payload, mask, host2, workspace, workspace_bytes, RANS_SLOT_ONE, S(stream));
}

// ---- a batch of frames
extern "C" int pcgc_occ_rans_encode_batch(const uint16_t* packed, int frames, const int64_t* row, const int32_t* steps, const int64_t* sums, uint8_t* payload,
                                          const int64_t* pay, int64_t* host, void* workspace, size_t workspace_bytes, void* stream) {
    OrFrames fr;
    PCGC_REQUIRE(rans_frames_of(frames, row, steps, pay, fr, true), "1 to 16 frames; row offsets ascending from 0 and below 2^31; steps per chunk 1 .. 2^24; payload offsets multiples of 8");
    PCGC_REQUIRE((fr.row[frames] == 0 || packed) && payload && host && ((uintptr_t)payload & 7) == 0, "null argument or payload misaligned");
    for (int f = 0; f < frames; ++f)
        PCGC_REQUIRE(pay[f + 1] - pay[f] >= 8 + 516 * (int64_t)(fr.chunk[f + 1] - fr.chunk[f]) + 4 * (row[f + 1] - row[f]), "payload room of a frame too small (below 8 + 516 K + 4 n bytes)");
    return rans_encode(__func__, packed, fr, sums, payload, host, workspace, workspace_bytes, RANS_SLOT_BATCH, S(stream));
}

extern "C" int pcgc_occ_rans_decode_batch(const uint16_t* packed, int frames, const int64_t* row, const int32_t* steps, const uint8_t* payload, const int64_t* pay,
                                          const int64_t* pay_bytes, uint8_t* mask, int64_t* host, void* workspace, size_t workspace_bytes, void* stream) {
    OrFrames fr;
    PCGC_REQUIRE(rans_frames_of(frames, row, steps, pay, fr, false), "1 to 16 frames; row offsets ascending from 0 and below 2^31; steps per chunk 0 .. 2^24; payload offsets multiples of 8");
    PCGC_REQUIRE((fr.chunk[frames] == 0 || (packed && mask && payload)) && pay_bytes && host && ((uintptr_t)payload & 7) == 0, "null argument or payload misaligned");
    for (int f = 0; f < frames; ++f) {
        if (!steps[f]) continue;
        const int64_t Kf = fr.chunk[f + 1] - fr.chunk[f];
        PCGC_REQUIRE(pay_bytes[f] >= 8 + 516 * Kf && (pay_bytes[f] - 8 - 516 * Kf) % 4 == 0, "a payload cut inside its tables or not whole words");
        fr.words[f] = (pay_bytes[f] - 8 - 516 * Kf) / 4;
    }
    return rans_decode(__func__, packed, fr, payload, mask, host, workspace, workspace_bytes, RANS_SLOT_BATCH, S(stream));
}
