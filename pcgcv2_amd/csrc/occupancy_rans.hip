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

// ---- encoder ---------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(RANS_LANES) k_occ_rans_encode(const uint16_t* __restrict__ packed, int64_t n, int S, uint32_t* __restrict__ scratch,
                                                                unsigned long long* __restrict__ states, uint32_t* __restrict__ wcount) {
    __shared__ uint32_t sh_p1[PCGC_OCC_CONTEXTS];
    rans_load_p1(sh_p1);
    const int lane = threadIdx.x;
    const int64_t k = blockIdx.x, base = k * RANS_LANES * S;
    const int rows = (int)(n - base < (int64_t)RANS_LANES * S ? n - base : (int64_t)RANS_LANES * S);
    const uint16_t* __restrict__ in = packed + base;
    uint32_t* __restrict__ out = scratch + base;              // rows words: [top, rows) are written
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
            const uint32_t f = b ? p : 65536u - p, c = b ? 65536u - p : 0u;
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
                x = (q << 16) + r + c;
            }
        }
#pragma unroll
        for (int i = 0; i < RANS_BATCH; ++i) cur[i] = nxt[i];
    }
#undef RANS_FETCH
    states[k * RANS_LANES + lane] = x;
    if (lane == 0) wcount[k] = (uint32_t)(rows - top);
}

// exclusive scan of the chunks' word counts (one block; thread t owns a run of consecutive chunks) -> offs [K] (saturating: counts a decoder
// reads are not to be trusted), slot[0] = their sum.  Encoder side: also the payload's head and, with sums, slot[1..2] = sums[0..1], so that
// one small copy brings the length and pcgc_occ_symbols' sums to the host.
__global__ void __launch_bounds__(RANS_SCAN_BLOCK) k_occ_rans_offsets(const uint32_t* __restrict__ wcount, int64_t K, uint32_t* __restrict__ offs,
                                                                      long long* __restrict__ slot, uint32_t* __restrict__ head, uint32_t S,
                                                                      const long long* __restrict__ sums) {
    __shared__ unsigned long long part[RANS_SCAN_BLOCK];
    const int64_t per = (K + RANS_SCAN_BLOCK - 1) / RANS_SCAN_BLOCK;
    const int64_t lo = (int64_t)threadIdx.x * per < K ? (int64_t)threadIdx.x * per : K, hi = lo + per < K ? lo + per : K;
    unsigned long long s = 0;
    for (int64_t i = lo; i < hi; ++i) s += wcount[i];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long run = 0;
        for (int i = 0; i < RANS_SCAN_BLOCK; ++i) { const unsigned long long v = part[i]; part[i] = run; run += v; }
        slot[0] = (long long)run;
        if (head) { head[0] = S; head[1] = (uint32_t)K; }
        if (sums) { slot[1] = sums[0]; slot[2] = sums[1]; }
    }
    __syncthreads();
    unsigned long long run = part[threadIdx.x];
    for (int64_t i = lo; i < hi; ++i) { offs[i] = run < 0xffffffffull ? (uint32_t)run : 0xffffffffu; run += wcount[i]; }
}

// chunk k's words, from the end of its scratch to their place in the payload
__global__ void __launch_bounds__(RANS_SCAN_BLOCK) k_occ_rans_compact(const uint32_t* __restrict__ scratch, int64_t n, int S, const uint32_t* __restrict__ wcount,
                                                                      const uint32_t* __restrict__ offs, uint32_t* __restrict__ words) {
    const int64_t k = blockIdx.x, base = k * RANS_LANES * S;
    const int64_t rows = n - base < (int64_t)RANS_LANES * S ? n - base : (int64_t)RANS_LANES * S;
    const uint32_t W = wcount[k];                             // <= rows: the encoder wrote it
    const uint32_t* __restrict__ src = scratch + base + rows - W;
    uint32_t* __restrict__ dst = words + offs[k];
    for (uint32_t i = threadIdx.x; i < W; i += RANS_SCAN_BLOCK) dst[i] = src[i];
}

// ---- decoder ---------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(RANS_LANES) k_occ_rans_decode(const uint16_t* __restrict__ packed, int64_t n, int S, const unsigned long long* __restrict__ states,
                                                                const uint32_t* __restrict__ wcount, const uint32_t* __restrict__ offs,
                                                                const uint32_t* __restrict__ words, int64_t words_total, uint8_t* __restrict__ mask,
                                                                unsigned long long* __restrict__ result /*[0] occupied rows, [1] unsound chunks*/) {
    __shared__ uint32_t sh_p1[PCGC_OCC_CONTEXTS];
    __shared__ uint32_t ring[RANS_RING];
    rans_load_p1(sh_p1);
    const int lane = threadIdx.x;
    const int64_t k = blockIdx.x, base = k * RANS_LANES * S;
    const int rows = (int)(n - base < (int64_t)RANS_LANES * S ? n - base : (int64_t)RANS_LANES * S);
    const int steps = (rows + RANS_LANES - 1) / RANS_LANES;
    const uint16_t* __restrict__ in = packed + base;
    uint8_t* __restrict__ out = mask + base;
    const uint32_t W = wcount[k];
    const int64_t off = (int64_t)offs[k];
    // the words this chunk may read: [0, avail) of src, inside both its own count and the payload
    const uint32_t avail = off >= words_total ? 0u : (uint32_t)((int64_t)W < words_total - off ? (int64_t)W : words_total - off);
    const uint32_t* __restrict__ src = words + (off < words_total ? off : 0);
    uint64_t x = states[k * RANS_LANES + lane];
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
            const uint32_t f = b ? p : 65536u - p, c = b ? 65536u - p : 0u;
            if (act) x = (uint64_t)f * (x >> 16) + s - c;
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
        atomicAdd(result, (unsigned long long)occupied);
        if (any_bad) atomicAdd(result + 1, 1ull);
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------------
// workspace: [slot: 4 x int64][offs: K x u32, padded to 8 bytes][encoder only: scratch, n x u32]
static size_t rans_offs_bytes(int64_t K) { return (size_t)((K * 4 + 7) / 8 * 8); }

extern "C" size_t pcgc_occ_rans_workspace_bytes(int64_t n, int steps) {
    if (n < 0) n = 0;
    if (steps < 1) steps = 1;
    return 32 + rans_offs_bytes(rans_chunks(n, steps)) + (size_t)n * 4 + 64;
}

static long long* rans_host_slot() {
    static thread_local long long* host = nullptr;
    if (!host && hipHostMalloc((void**)&host, 64, hipHostMallocDefault) != hipSuccess) host = nullptr;
    return host;
}

extern "C" int pcgc_occ_rans_encode(const uint16_t* packed, int64_t n, int steps, const int64_t* sums, uint8_t* payload, size_t payload_capacity,
                                    int64_t* host3, void* workspace, size_t workspace_bytes, void* stream) {
    PCGC_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "bad row count");
    PCGC_REQUIRE(steps >= 1 && steps <= RANS_MAX_STEPS, "steps per chunk outside 1 .. 2^24");
    PCGC_REQUIRE((n == 0 || packed) && payload && host3, "null argument");
    const int64_t K = rans_chunks(n, steps);
    PCGC_REQUIRE(payload_capacity >= (size_t)(8 + 516 * K + 4 * n) && ((uintptr_t)payload & 7) == 0, "payload buffer too small or misaligned");
    PCGC_REQUIRE(workspace && workspace_bytes >= pcgc_occ_rans_workspace_bytes(n, steps) && ((uintptr_t)workspace & 7) == 0, "workspace too small or misaligned");
    long long* slot = (long long*)workspace;
    uint32_t* offs = (uint32_t*)((char*)workspace + 32);
    uint32_t* scratch = (uint32_t*)((char*)workspace + 32 + rans_offs_bytes(K));
    unsigned long long* states = (unsigned long long*)(payload + 8);
    uint32_t* wcount = (uint32_t*)(payload + 8 + 512 * K);
    uint32_t* words = wcount + K;
    long long* host = rans_host_slot();
    if (!host) { pcgc_set_error("occ_rans_encode: cannot allocate pinned memory"); return -1; }
    if (K) {
        hipLaunchKernelGGL(k_occ_rans_encode, dim3((unsigned)K), dim3(RANS_LANES), 0, S(stream), packed, n, steps, scratch, states, wcount);
        PCGC_CHECK_LAUNCH("occ_rans_encode");
    }
    hipLaunchKernelGGL(k_occ_rans_offsets, dim3(1), dim3(RANS_SCAN_BLOCK), 0, S(stream), (const uint32_t*)wcount, K, offs, slot, (uint32_t*)payload,
                       (uint32_t)steps, (const long long*)sums);
    PCGC_CHECK_LAUNCH("occ_rans_encode");
    if (K) {
        hipLaunchKernelGGL(k_occ_rans_compact, dim3((unsigned)K), dim3(RANS_SCAN_BLOCK), 0, S(stream), (const uint32_t*)scratch, n, steps,
                           (const uint32_t*)wcount, (const uint32_t*)offs, words);
        PCGC_CHECK_LAUNCH("occ_rans_encode");
    }
    hipError_t e = hipMemcpyAsync(host, slot, 3 * sizeof(long long), hipMemcpyDeviceToHost, S(stream));
    if (e == hipSuccess) e = hipStreamSynchronize(S(stream));
    if (e != hipSuccess) { pcgc_set_error("occ_rans_encode: %s", hipGetErrorString(e)); return -1; }
    host3[0] = 8 + 516 * K + 4 * (int64_t)host[0];
    host3[1] = sums ? (int64_t)host[1] : 0;
    host3[2] = sums ? (int64_t)host[2] : 0;
    return 0;
}

extern "C" int pcgc_occ_rans_decode(const uint16_t* packed, int64_t n, const uint8_t* payload, int64_t payload_bytes, int steps, uint8_t* mask,
                                    int64_t* host2, void* workspace, size_t workspace_bytes, void* stream) {
    PCGC_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "bad row count");
    PCGC_REQUIRE((n == 0 || (packed && mask)) && payload && host2, "null argument");
    PCGC_REQUIRE(((uintptr_t)payload & 7) == 0, "payload misaligned");
    PCGC_REQUIRE(steps >= 1 && steps <= RANS_MAX_STEPS, "steps per chunk outside 1 .. 2^24");
    long long* host = rans_host_slot();
    if (!host) { pcgc_set_error("occ_rans_decode: cannot allocate pinned memory"); return -1; }
    hipError_t e;
    const int64_t K = rans_chunks(n, steps);          // (the head's own S and K are the caller's to compare: ops.occ_rans_decode)
    PCGC_REQUIRE(payload_bytes >= 8 + 516 * K && (payload_bytes - 8 - 516 * K) % 4 == 0, "payload cut inside its tables or not whole words");
    const int64_t words_total = (payload_bytes - 8 - 516 * K) / 4;
    PCGC_REQUIRE(workspace && workspace_bytes >= 32 + rans_offs_bytes(K) && ((uintptr_t)workspace & 7) == 0, "workspace too small or misaligned");
    long long* slot = (long long*)workspace;
    uint32_t* offs = (uint32_t*)((char*)workspace + 32);
    const unsigned long long* states = (const unsigned long long*)(payload + 8);
    const uint32_t* wcount = (const uint32_t*)(payload + 8 + 512 * K);
    const uint32_t* words = wcount + K;
    e = hipMemsetAsync(slot, 0, 32, S(stream));
    if (e != hipSuccess) { pcgc_set_error("occ_rans_decode: %s", hipGetErrorString(e)); return -1; }
    hipLaunchKernelGGL(k_occ_rans_offsets, dim3(1), dim3(RANS_SCAN_BLOCK), 0, S(stream), wcount, K, offs, slot, (uint32_t*)nullptr, 0u, (const long long*)nullptr);
    PCGC_CHECK_LAUNCH("occ_rans_decode");
    if (K) {
        hipLaunchKernelGGL(k_occ_rans_decode, dim3((unsigned)K), dim3(RANS_LANES), 0, S(stream), packed, n, steps, states, wcount, (const uint32_t*)offs, words,
                           words_total, mask, (unsigned long long*)(slot + 1));
        PCGC_CHECK_LAUNCH("occ_rans_decode");
    }
    e = hipMemcpyAsync(host, slot, 3 * sizeof(long long), hipMemcpyDeviceToHost, S(stream));
    if (e == hipSuccess) e = hipStreamSynchronize(S(stream));
    if (e != hipSuccess) { pcgc_set_error("occ_rans_decode: %s", hipGetErrorString(e)); return -1; }
    host2[0] = (int64_t)host[1];
    host2[1] = (int64_t)host[2] + (host[0] != words_total ? 1 : 0);      // unsound chunks (+ 1: the word counts do not add up to the payload)
    return 0;
}
