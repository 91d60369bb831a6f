// The kernels and the host side of the interleaved rANS core (rans_core.h): what the occupancy and the colour coders run
// around their own step kernels.
#include <cstring>
#include "rans_core.h"

// block f: an exclusive scan of the word counts of frame f's chunks (thread t owns a run of consecutive chunks) -> offs [chunk[f] ..) counted
// from the frame's own first word (saturating: counts a decoder reads are not to be trusted), slot[f] = the frame's words.  Encoder side
// (head != 0): also the payload's head; a frame without chunks has the head S | 0 and nothing else (head == 2) or no payload at all.  With
// sums (a pair per frame), aux[2 f ..] = sums[2 f ..], so that one small copy brings lengths and sums to the host.
__global__ void __launch_bounds__(RANS_SCAN_BLOCK) k_rans_offsets(RansFrames fr, uint8_t* payload, uint32_t* __restrict__ offs, long long* __restrict__ slot,
                                                                  int head, const long long* __restrict__ sums, long long* __restrict__ aux) {
    __shared__ unsigned long long part[RANS_SCAN_BLOCK];
    const int f = blockIdx.x;
    const int64_t K = fr.chunk[f + 1] - fr.chunk[f];
    if (threadIdx.x == 0 && sums) { aux[2 * f] = sums[2 * f]; aux[2 * f + 1] = sums[2 * f + 1]; }
    if (K <= 0) {                                             // (uniform)
        if (threadIdx.x == 0) {
            slot[f] = 0;
            if (head == 2) { ((uint32_t*)(payload + fr.pay[f]))[0] = (uint32_t)fr.steps[f]; ((uint32_t*)(payload + fr.pay[f]))[1] = 0u; }
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
        if (head) { ((uint32_t*)mine)[0] = (uint32_t)fr.steps[f]; ((uint32_t*)mine)[1] = (uint32_t)K; }
    }
    __syncthreads();
    unsigned long long run = part[threadIdx.x];
    for (int64_t i = lo; i < hi; ++i) { offs[i] = run < 0xffffffffull ? (uint32_t)run : 0xffffffffu; run += wcount[i]; }
}

// a chunk's words, from the end of its scratch to their place in its frame's payload
__global__ void __launch_bounds__(RANS_SCAN_BLOCK) k_rans_compact(const uint32_t* __restrict__ scratch, RansFrames fr, const uint32_t* __restrict__ offs,
                                                                  uint8_t* __restrict__ payload) {
    const RansChunk c = rans_chunk_of(fr);
    uint8_t* mine = payload + fr.pay[c.f];
    const uint32_t W = rans_wcount(mine, c.K)[c.k];           // <= rows: the encoder wrote it
    const uint32_t* __restrict__ src = scratch + c.base + c.rows - W;
    uint32_t* __restrict__ dst = rans_words(mine, c.K) + offs[blockIdx.x];
    for (uint32_t i = threadIdx.x; i < W; i += RANS_SCAN_BLOCK) dst[i] = src[i];
}

bool rans_frames_of(int frames, const int64_t* first, const int32_t* steps, const int64_t* pay, RansFrames& fr, int opts) {
    memset(&fr, 0, sizeof(fr));
    if (frames < 1 || frames > RANS_MAX_FRAMES || !first || !steps || !pay || first[0] != 0) return false;
    fr.frames = frames;
    int64_t K = 0;
    for (int f = 0; f < frames; ++f) {
        const int64_t n = first[f + 1] - first[f];
        if (n < 0 || ((opts & RANS_THIRDS) && n % 3) || first[f + 1] >= ((int64_t)1 << 31) || steps[f] < 0 || steps[f] > RANS_MAX_STEPS || (pay[f] & 7) || pay[f] < 0)
            return false;
        if ((opts & RANS_NEED_STEPS) && (n > 0 || (opts & RANS_EMPTY_HEAD)) && steps[f] < 1) return false;
        fr.first[f] = first[f]; fr.pay[f] = pay[f]; fr.steps[f] = steps[f]; fr.chunk[f] = (int)K;
        K += steps[f] > 0 ? rans_chunks(n, steps[f]) : 0;
        if (K >= ((int64_t)1 << 31)) return false;
    }
    for (int f = frames; f <= RANS_MAX_FRAMES; ++f) { fr.first[f] = first[frames]; fr.chunk[f] = (int)K; }
    return true;
}
bool rans_frame_of_one(int64_t n, int steps, RansFrames& fr) {
    const int64_t first[2] = {0, n}, pay = 0;
    const int32_t s = steps;
    return rans_frames_of(1, first, &s, &pay, fr, RANS_NEED_STEPS);
}
bool rans_words_of(RansFrames& fr, int f, int64_t bytes) {
    const int64_t tables = rans_room(fr.chunk[f + 1] - fr.chunk[f], 0);
    if (bytes < tables || (bytes - tables) % 4) return false;
    fr.words[f] = (bytes - tables) / 4;
    return true;
}
int64_t rans_payload_bytes(const RansFrames& fr, int f, long long words, int opts) {
    const int64_t K = fr.chunk[f + 1] - fr.chunk[f];
    return K || (opts & RANS_EMPTY_HEAD) ? rans_room(K, words) : 0;
}

static long long* rans_host_slot() {
    static thread_local long long* host = nullptr;
    if (!host && hipHostMalloc((void**)&host, RANS_SLOT_MAX, hipHostMallocDefault) != hipSuccess) host = nullptr;
    return host;
}
int rans_begin(const char* who, const RansFrames& fr, void* workspace, size_t workspace_bytes, size_t slot_bytes, size_t rest_bytes, RansWork& w, hipStream_t s) {
    const int64_t K = fr.chunk[fr.frames];
    RANS_REQUIRE(who, workspace && workspace_bytes >= slot_bytes + rans_offs_bytes(K) + rest_bytes && ((uintptr_t)workspace & 7) == 0,
                 "workspace too small or misaligned");
    w.slot = (long long*)workspace;
    w.offs = (uint32_t*)((char*)workspace + slot_bytes);
    w.rest = (char*)workspace + slot_bytes + rans_offs_bytes(K);
    w.host = rans_host_slot();
    if (!w.host) { pcgc_set_error("%s: cannot allocate pinned memory", who + 5); return -1; }
    hipError_t e = hipMemsetAsync(w.slot, 0, slot_bytes, s);
    RANS_CHECK_HIP(who, e);
    return 0;
}
int rans_pack(const char* who, const RansFrames& fr, const RansWork& w, uint8_t* payload, int opts, const long long* sums, hipStream_t s) {
    hipLaunchKernelGGL(k_rans_offsets, dim3((unsigned)fr.frames), dim3(RANS_SCAN_BLOCK), 0, s, fr, payload, w.offs, w.slot, (opts & RANS_EMPTY_HEAD) ? 2 : 1,
                       sums, w.slot + RANS_MAX_FRAMES);
    PCGC_CHECK_LAUNCH(who + 5);
    if (fr.chunk[fr.frames]) {
        hipLaunchKernelGGL(k_rans_compact, dim3((unsigned)fr.chunk[fr.frames]), dim3(RANS_SCAN_BLOCK), 0, s, (const uint32_t*)w.rest, fr, (const uint32_t*)w.offs, payload);
        PCGC_CHECK_LAUNCH(who + 5);
    }
    return 0;
}
int rans_offsets(const char* who, const RansFrames& fr, const RansWork& w, const uint8_t* payload, hipStream_t s) {
    hipLaunchKernelGGL(k_rans_offsets, dim3((unsigned)fr.frames), dim3(RANS_SCAN_BLOCK), 0, s, fr, const_cast<uint8_t*>(payload), w.offs, w.slot, 0,
                       (const long long*)nullptr, (long long*)nullptr);
    PCGC_CHECK_LAUNCH(who + 5);
    return 0;
}
int rans_end(const char* who, const RansWork& w, size_t count, hipStream_t s) {
    hipError_t e = hipMemcpyAsync(w.host, w.slot, count * sizeof(long long), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    RANS_CHECK_HIP(who, e);
    return 0;
}
