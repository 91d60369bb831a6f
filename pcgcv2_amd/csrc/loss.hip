// The forward half of the training graph's losses on device (reference loss.py:8-40, data_utils.py:63-75, entropy_model.py:112-140):
// coordinate membership (isin), the bottleneck's per-element likelihood with the rate estimate, and the classification BCE with the
// confusion counts.  Nothing here is on the encode/decode path.
//
// Reductions follow metric.hip's rules: no floating-point atomics; every block reduces its elements in a fixed order (thread -> wave
// shuffles -> LDS across the waves) into one slot of a slab, and ONE block then adds the slots in a fixed order.  The grid is a function
// of the element count alone, so a sum is bitwise reproducible run to run, stream to stream.
#include "pcgc_common.h"
#include "eb_logits.h"

constexpr int LOSS_BLOCK = 256;

// ---- isin: mask[i] = row i of coords is a key of the table (| or_mask[i]) -----------------------------------------------------------
__global__ void __launch_bounds__(LOSS_BLOCK) k_hash_contains(const int4* __restrict__ coords, int64_t n, const uint64_t* __restrict__ keys,
                                                              const int32_t* __restrict__ vals, uint64_t cap_mask,
                                                              const uint8_t* __restrict__ or_mask, uint8_t* __restrict__ mask) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int4 c = coords[i];                            // (b, x, y, z); a row the key cannot hold is in no table
    bool in = keys != nullptr && hash_lookup(keys, vals, cap_mask, c.x, c.y, c.z, c.w) >= 0;
    if (or_mask) in = in || or_mask[i] != 0;
    mask[i] = in ? 1 : 0;
}
extern "C" int pcgc_hash_contains(const int32_t* coords, int64_t n, const uint64_t* keys, const int32_t* vals, int64_t cap,
                                  const uint8_t* or_mask, uint8_t* mask, void* stream) {
    PCGC_REQUIRE(cap == 0 || (keys && vals && (cap & (cap - 1)) == 0), "capacity must be a power of two (0 = empty table)");
    if (n == 0) return 0;
    PCGC_REQUIRE(coords && mask, "null argument");
    hipLaunchKernelGGL(k_hash_contains, dim3(grid_for(n, LOSS_BLOCK)), dim3(LOSS_BLOCK), 0, S(stream), (const int4*)coords, n,
                       cap ? keys : nullptr, vals, (uint64_t)(cap - 1), or_mask, mask);
    PCGC_CHECK_LAUNCH("hash_contains");
    return 0;
}

// ---- fixed-order block reduction: lanes of a wave by shuffles (the same butterfly in every wave), then the waves in ascending order ----
__device__ static inline double block_sum(double v, double* sh /*[LOSS_BLOCK / 64]*/) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < LOSS_BLOCK / 64; ++w) s += sh[w];
    __syncthreads();
    return s;                                           // (valid in thread 0)
}
__device__ static inline unsigned block_count(unsigned v, unsigned* sh /*[LOSS_BLOCK / 64]*/) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned s = 0;
    if (threadIdx.x == 0)
        for (int w = 0; w < LOSS_BLOCK / 64; ++w) s += sh[w];
    __syncthreads();
    return s;
}
// second stage: one block; thread t adds slots t, t + 256, ... in ascending order, then the block reduction above
__global__ void __launch_bounds__(LOSS_BLOCK) k_slab_sum(const double* __restrict__ slab, int64_t blocks, double* __restrict__ out) {
    __shared__ double sh[LOSS_BLOCK / 64];
    double v = 0.0;
    for (int64_t i = threadIdx.x; i < blocks; i += LOSS_BLOCK) v += slab[i];
    const double s = block_sum(v, sh);
    if (threadIdx.x == 0) out[0] = s;
}

// ---- bottleneck likelihood + bits (entropy_model.py:112-140, loss.py:17-20) -----------------------------------------------------------
// One element (row, channel) per thread, evaluated as k_cdf_likelihood evaluates a table entry: logits at v -+ 0.5 in fp64 from the fp32
// parameters, the sign trick, |sigmoid - sigmoid|, ONE rounding to fp32, then the lower bound on the fp32 value (Low_bound).  The bits are
// -log2 of that fp32 value, accumulated in fp64: what loss.get_bits computes from the stored tensor.
__global__ void __launch_bounds__(LOSS_BLOCK) k_eb_likelihood(const float* __restrict__ feats, int ld, int64_t n, int C, const float* __restrict__ P,
                                                              float bound, float* __restrict__ lik, double* __restrict__ slab) {
    __shared__ EbShared sh;
    __shared__ double red[LOSS_BLOCK / 64];
    eb_prepare(P, C, sh);
    __syncthreads();
    const int64_t t = (int64_t)blockIdx.x * LOSS_BLOCK + threadIdx.x;
    double term = 0.0;
    if (t < n * C) {
        const int64_t row = t / C;
        const int c = (int)(t - row * C);
        const double v = (double)feats[row * ld + c];
        const double lo = eb_logits(P, C, c, v - 0.5, sh), up = eb_logits(P, C, c, v + 0.5, sh);
        const double sum = lo + up, sign = sum > 0 ? -1.0 : (sum < 0 ? 1.0 : 0.0);
        float p = (float)fabs(eb_sigmoid(sign * up) - eb_sigmoid(sign * lo));
        if (p < bound) p = bound;
        if (lik) lik[t] = p;
        term = -log2((double)p);
    }
    if (slab) {                                          // (uniform across the grid)
        const double s = block_sum(term, red);
        if (threadIdx.x == 0) slab[blockIdx.x] = s;
    }
}
extern "C" size_t pcgc_loss_workspace_bytes(int64_t count) {
    // one fp64 slot and four 32-bit counters per block of the widest grid any of the calls below launches for `count` elements
    return (size_t)(grid_for(count > 0 ? count : 1, LOSS_BLOCK)) * (sizeof(double) + 4 * sizeof(uint32_t)) + 64;
}
extern "C" int pcgc_eb_likelihood(const float* feats, int ld, int64_t n, int C, const float* params, float bound, float* likelihood,
                                  double* bits, void* workspace, size_t workspace_bytes, void* stream) {
    PCGC_REQUIRE(C >= 1 && C <= EB_MAX_C, "entropy bottleneck: at most 16 channels");
    PCGC_REQUIRE(n >= 0 && ld >= C && params, "bad arguments");
    PCGC_REQUIRE(n * (int64_t)C < ((int64_t)1 << 31) * LOSS_BLOCK, "too many elements");
    PCGC_REQUIRE(likelihood || bits, "nothing to compute");
    const int64_t count = n * C;
    if (count == 0) {
        if (bits) { hipError_t e = hipMemsetAsync(bits, 0, sizeof(double), S(stream)); if (e != hipSuccess) { pcgc_set_error("eb_likelihood: %s", hipGetErrorString(e)); return -1; } }
        return 0;
    }
    PCGC_REQUIRE(feats, "null features");
    double* slab = nullptr;
    if (bits) {
        PCGC_REQUIRE(workspace && workspace_bytes >= pcgc_loss_workspace_bytes(count) && ((uintptr_t)workspace & 7) == 0, "workspace too small or misaligned");
        slab = (double*)workspace;
    }
    const unsigned blocks = grid_for(count, LOSS_BLOCK);
    hipLaunchKernelGGL(k_eb_likelihood, dim3(blocks), dim3(LOSS_BLOCK), 0, S(stream), feats, ld, n, C, params, bound, likelihood, slab);
    PCGC_CHECK_LAUNCH("eb_likelihood");
    if (bits) {
        hipLaunchKernelGGL(k_slab_sum, dim3(1), dim3(LOSS_BLOCK), 0, S(stream), slab, (int64_t)blocks, bits);
        PCGC_CHECK_LAUNCH("eb_likelihood");
    }
    return 0;
}

// bits of a likelihood tensor somebody holds already (loss.get_bits on its own): the same terms, the same partition, the same order as
// the fused form above, hence the same double
__global__ void __launch_bounds__(LOSS_BLOCK) k_neg_log2(const float* __restrict__ x, int ld, int64_t n, int C, double* __restrict__ slab) {
    __shared__ double red[LOSS_BLOCK / 64];
    const int64_t t = (int64_t)blockIdx.x * LOSS_BLOCK + threadIdx.x;
    double term = 0.0;
    if (t < n * C) {
        const int64_t row = t / C;
        term = -log2((double)x[row * ld + (t - row * C)]);
    }
    const double s = block_sum(term, red);
    if (threadIdx.x == 0) slab[blockIdx.x] = s;
}
extern "C" int pcgc_neg_log2_sum(const float* x, int ld, int64_t n, int C, double* bits, void* workspace, size_t workspace_bytes, void* stream) {
    PCGC_REQUIRE(n >= 0 && C >= 1 && ld >= C && bits, "bad arguments");
    PCGC_REQUIRE(n * (int64_t)C < ((int64_t)1 << 31) * LOSS_BLOCK, "too many elements");
    const int64_t count = n * C;
    if (count == 0) {
        hipError_t e = hipMemsetAsync(bits, 0, sizeof(double), S(stream));
        if (e != hipSuccess) { pcgc_set_error("neg_log2_sum: %s", hipGetErrorString(e)); return -1; }
        return 0;
    }
    PCGC_REQUIRE(x && workspace && workspace_bytes >= pcgc_loss_workspace_bytes(count) && ((uintptr_t)workspace & 7) == 0, "workspace too small or misaligned");
    double* slab = (double*)workspace;
    const unsigned blocks = grid_for(count, LOSS_BLOCK);
    hipLaunchKernelGGL(k_neg_log2, dim3(blocks), dim3(LOSS_BLOCK), 0, S(stream), x, ld, n, C, slab);
    hipLaunchKernelGGL(k_slab_sum, dim3(1), dim3(LOSS_BLOCK), 0, S(stream), slab, (int64_t)blocks, bits);
    PCGC_CHECK_LAUNCH("neg_log2_sum");
    return 0;
}

// ---- BCE with logits + confusion counts (loss.py:8-15, 31-40) ---------------------------------------------------------------------------
// A streaming pass: four consecutive rows per thread — one 16-byte load of the logits and one 4-byte load of each mask where the logits are
// dense (ld == 1) and the pointers aligned, scalar loads of the same four rows otherwise, so both forms add the same terms in the same order.
// term = max(x, 0) - x y + log1p(exp(-|x|)) in fp64 (torch.nn.BCEWithLogitsLoss's stable form); counts: TP, FN, FP, TN of (pred, truth).
constexpr int BCE_ROWS = 4;
template <bool VEC>
__global__ void __launch_bounds__(LOSS_BLOCK) k_bce_logits(const float* __restrict__ logits, int64_t ld, int64_t n, const uint8_t* __restrict__ truth,
                                                           const uint8_t* __restrict__ pred, double* __restrict__ slab, uint32_t* __restrict__ cslab) {
    __shared__ double red[LOSS_BLOCK / 64];
    __shared__ unsigned cred[LOSS_BLOCK / 64];
    const int64_t i0 = ((int64_t)blockIdx.x * LOSS_BLOCK + threadIdx.x) * BCE_ROWS;
    float x[BCE_ROWS] = {0.f, 0.f, 0.f, 0.f};
    uint8_t y[BCE_ROWS] = {0, 0, 0, 0}, p[BCE_ROWS] = {0, 0, 0, 0};
    const int m = i0 >= n ? 0 : (int)(n - i0 < BCE_ROWS ? n - i0 : BCE_ROWS);
    if (VEC && m == BCE_ROWS) {
        if (logits) { const float4 v = *(const float4*)(logits + i0); x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w; }
        const uchar4 t = *(const uchar4*)(truth + i0);
        y[0] = t.x; y[1] = t.y; y[2] = t.z; y[3] = t.w;
        if (pred) { const uchar4 q = *(const uchar4*)(pred + i0); p[0] = q.x; p[1] = q.y; p[2] = q.z; p[3] = q.w; }
    } else {
        for (int j = 0; j < m; ++j) {
            if (logits) x[j] = logits[(i0 + j) * ld];
            y[j] = truth[i0 + j];
            if (pred) p[j] = pred[i0 + j];
        }
    }
    double s = 0.0;
    unsigned tp = 0, fn = 0, fp = 0, tn = 0;
    for (int j = 0; j < m; ++j) {
        const bool yt = y[j] != 0, pt = p[j] != 0;
        if (logits) {
            const double v = (double)x[j];
            s += (v > 0 ? v : 0.0) - (yt ? v : 0.0) + log1p(exp(-fabs(v)));
        }
        tp += pt && yt; fn += !pt && yt; fp += pt && !yt; tn += !pt && !yt;
    }
    const double bs = block_sum(s, red);
    const unsigned btp = block_count(tp, cred), bfn = block_count(fn, cred), bfp = block_count(fp, cred), btn = block_count(tn, cred);
    if (threadIdx.x == 0) {
        slab[blockIdx.x] = bs;
        uint32_t* c = cslab + 4 * (int64_t)blockIdx.x;
        c[0] = btp; c[1] = bfn; c[2] = bfp; c[3] = btn;
    }
}
__global__ void __launch_bounds__(LOSS_BLOCK) k_bce_final(const double* __restrict__ slab, const uint32_t* __restrict__ cslab, int64_t blocks,
                                                          double divisor, double* __restrict__ bce, long long* __restrict__ counts) {
    __shared__ double sh[LOSS_BLOCK / 64];
    __shared__ long long sc[LOSS_BLOCK / 64][4];
    double v = 0.0;
    long long c[4] = {0, 0, 0, 0};
    for (int64_t i = threadIdx.x; i < blocks; i += LOSS_BLOCK) {
        v += slab[i];
        for (int k = 0; k < 4; ++k) c[k] += cslab[4 * i + k];
    }
    const double s = block_sum(v, sh);
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) c[k] += __shfl_xor(c[k], d, 64);
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < 4; ++k) sc[threadIdx.x >> 6][k] = c[k];
    __syncthreads();
    if (threadIdx.x == 0) {
        bce[0] = s / divisor;
        for (int k = 0; k < 4; ++k) {
            long long a = 0;
            for (int w = 0; w < LOSS_BLOCK / 64; ++w) a += sc[w][k];
            counts[k] = a;
        }
    }
}
extern "C" int pcgc_bce_logits(const float* logits, int64_t ld, int64_t n, const uint8_t* truth, const uint8_t* pred, double* bce,
                               int64_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
    PCGC_REQUIRE(n >= 0 && ld >= 1 && bce && counts, "bad arguments");
    if (n == 0) {
        hipError_t e = hipMemsetAsync(bce, 0, sizeof(double), S(stream));
        if (e == hipSuccess) e = hipMemsetAsync(counts, 0, 4 * sizeof(int64_t), S(stream));
        if (e != hipSuccess) { pcgc_set_error("bce_logits: %s", hipGetErrorString(e)); return -1; }
        return 0;
    }
    PCGC_REQUIRE(truth, "null truth mask");
    const int64_t threads = (n + BCE_ROWS - 1) / BCE_ROWS;
    PCGC_REQUIRE(workspace && workspace_bytes >= pcgc_loss_workspace_bytes(threads) && ((uintptr_t)workspace & 7) == 0, "workspace too small or misaligned");
    const unsigned blocks = grid_for(threads, LOSS_BLOCK);
    double* slab = (double*)workspace;
    uint32_t* cslab = (uint32_t*)(slab + blocks);
    const bool vec = ld == 1 && (((uintptr_t)logits) & 15) == 0 && (((uintptr_t)truth) & 3) == 0 && (((uintptr_t)pred) & 3) == 0;
    if (vec) hipLaunchKernelGGL(k_bce_logits<true>, dim3(blocks), dim3(LOSS_BLOCK), 0, S(stream), logits, ld, n, truth, pred, slab, cslab);
    else hipLaunchKernelGGL(k_bce_logits<false>, dim3(blocks), dim3(LOSS_BLOCK), 0, S(stream), logits, ld, n, truth, pred, slab, cslab);
    PCGC_CHECK_LAUNCH("bce_logits");
    // sum of the terms / ln 2 = loss.get_bce's "mean BCE / log(2) * n"
    hipLaunchKernelGGL(k_bce_final, dim3(1), dim3(LOSS_BLOCK), 0, S(stream), slab, cslab, (int64_t)blocks, 0.693147180559945309417232121458, bce, (long long*)counts);
    PCGC_CHECK_LAUNCH("bce_logits");
    return 0;
}
