// The backward half of the training graph on device (reference trainer.py:127-134 `sum_loss.backward()`): the weight gradient of every
// sparse convolution, the transposed kernel map, the small adjoints (ReLU, row gather) and the two leaf gradients (BCE, bottleneck rate).
// Nothing here is on the encode/decode path.  The input gradient of a convolution needs no kernel of its own: it is a forward gather
// convolution through a transposed map (pcgc_conv_gather; see pcgc_kmap_invert).
//
// Reductions follow loss.hip's rules: no floating-point atomics; a workgroup reduces its rows in a fixed order into one slot of a slab
// and a second stage adds the slots in ascending workgroup order.  Grids are functions of the shapes alone: bitwise reproducible.
#include "pcgc_common.h"
#include "mfma_util.h"
#include "eb_logits.h"

constexpr int GRAD_BLOCK = 256;

// ---- weight gradient -------------------------------------------------------------------------------------------------------------------
// gW[k][a][b] = sum over rows r of x[xrow(k, r)][a] * gy[grow(k, r)][b]:
//   gather form (pcgc_conv_wgrad):   xrow = nbr[k][r] (NULL: r; -1 = absent pair), grow = r          (k3, k1, k2 s2 down)
//   transpose form (pcgc_conv_up2_wgrad): xrow = rows ? rows[r] : r,                grow = 8 r + k    (generative transpose k2 s2)
// As a GEMM per offset k it is C[Cin x Cout] = A^T B over the row dimension: `v_mfma_f32_16x16x4_f32` with A[m = channel a][kk = row] the
// gathered, transposed x rows and B[kk = row][n = channel b] the gy rows — lane l holds A[l & 15][l >> 4] and B[l >> 4][l & 15], so the
// 16 lanes of a quarter read 16 consecutive floats of ONE row (64 bytes) of x and of gy: both operands come straight from global memory
// in fragment order, no LDS staging, no transpose.  A step covers 4 rows; MT x NT accumulator tiles cover the whole [Cin, Cout] slice of
// one offset, so every loaded fragment feeds NT (A) or MT (B) MFMAs.  Channels beyond Cin / Cout (8, 4 and 1 inside a 16-wide tile) and
// absent pairs load zeros: fma(0, 0, acc) leaves the chain exact.  A step whose 4 pairs are all absent is skipped.
// Rows are split over workgroups (wgrad_rows_per_group), the K offsets of a group over its waves (wave w: k = w, w + waves, ...); each
// wave writes its [Cin, Cout] partial of (group, k) to the slab, wave 0.. also the bias partial (column sums of gy over the group's rows).
__host__ __device__ static inline int64_t wgrad_rows_per_group(int K, int64_t n_rows, int Cin, int Cout) {
    // at most `cap` groups (the slab holds cap * K * Cin * Cout floats: <= 64 MiB, but never fewer than 128 groups); at least 128 rows
    // (K = 1: one wave per group) or 512 rows per group; a multiple of 16
    int64_t cap = ((int64_t)1 << 24) / ((int64_t)K * Cin * Cout);
    cap = cap < 128 ? 128 : (cap > 1024 ? 1024 : cap);
    const int64_t lo = K == 1 ? 128 : 512;
    int64_t r = (n_rows + cap - 1) / cap;
    r = r < lo ? lo : r;
    return (r + 15) / 16 * 16;
}
static inline int64_t wgrad_groups(int K, int64_t n_rows, int Cin, int Cout) {
    const int64_t r = wgrad_rows_per_group(K, n_rows, Cin, Cout);
    return n_rows > 0 ? (n_rows + r - 1) / r : 0;
}
extern "C" int64_t pcgc_conv_wgrad_rows_per_group(int K, int64_t n_rows, int Cin, int Cout) {
    if (K < 1 || Cin < 1 || Cout < 1 || n_rows < 0) return -1;
    return wgrad_rows_per_group(K, n_rows, Cin, Cout);
}
extern "C" size_t pcgc_conv_wgrad_workspace_bytes(int K, int64_t n_rows, int Cin, int Cout) {
    if (K < 1 || Cin < 1 || Cout < 1 || n_rows < 0) return 0;
    return (size_t)wgrad_groups(K, n_rows, Cin, Cout) * ((size_t)K * Cin * Cout + Cout) * sizeof(float) + 64;
}

template <int MT, int NT, bool UP>
__global__ void __launch_bounds__(GRAD_BLOCK) k_conv_wgrad(const int32_t* __restrict__ nbr, int K, int64_t n_rows, int64_t rows_per_group,
                                                           const float* __restrict__ x, int64_t n_in, int Cin, int x_ld,
                                                           const float* __restrict__ gy, int Cout, int gy_ld,
                                                           float* __restrict__ slab_w, float* __restrict__ slab_b) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const int col = lane & 15, q = lane >> 4;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_group;
    const int64_t r1 = r0 + rows_per_group < n_rows ? r0 + rows_per_group : n_rows;
    float* out_g = slab_w + (int64_t)blockIdx.x * K * Cin * Cout;
    for (int k = wave; k < K; k += waves) {
        f32x4 acc[MT][NT];
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int n = 0; n < NT; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
        // UP: nbr is the optional row list of a pruned input level (the same for every k)
        const int32_t* map = nbr ? (UP ? nbr : nbr + (int64_t)k * n_rows) : nullptr;
#pragma unroll 2
        for (int64_t r = r0 + q; r < r1 + q; r += 4) {         // (r - q uniform across the wave: every lane runs the same steps)
            int64_t xi = -1;
            if (r < r1) xi = map ? (int64_t)map[r] : r;
            if (xi >= n_in) xi = -1;
            if (__ballot(xi >= 0) == 0) continue;
            const int64_t gi = UP ? 8 * r + k : r;
            float a[MT], b[NT];
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const int c = 16 * m + col;
                a[m] = (xi >= 0 && c < Cin) ? x[xi * x_ld + c] : 0.f;
            }
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                const int c = 16 * n + col;
                b[n] = (xi >= 0 && c < Cout) ? gy[gi * gy_ld + c] : 0.f;
            }
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int n = 0; n < NT; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m], b[n], acc[m][n], 0, 0, 0);
        }
        // D[row = 4 q + i][col]: gW[k][a = 16 m + 4 q + i][b = 16 n + col]
        float* out_k = out_g + (int64_t)k * Cin * Cout;
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int n = 0; n < NT; ++n)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int ca = 16 * m + 4 * q + i, cb = 16 * n + col;
                    if (ca < Cin && cb < Cout) out_k[ca * Cout + cb] = acc[m][n][i];
                }
    }
    if (slab_b) {
        // bias partial: column sums of gy over the group's rows (UP: all 8 children of every row), thread = (column, row subset), rows
        // ascending within a subset, then the subsets in ascending order
        __shared__ float sh[GRAD_BLOCK];
        const int c = threadIdx.x & 63, sub = threadIdx.x >> 6;
        float s = 0.f;
        if (c < Cout) {
            const int64_t g0 = UP ? 8 * r0 : r0, g1 = UP ? 8 * r1 : r1;
            for (int64_t r = g0 + sub; r < g1; r += waves) s += gy[r * gy_ld + c];
        }
        sh[threadIdx.x] = s;
        __syncthreads();
        if (sub == 0 && c < Cout) {
            float t = 0.f;
            for (int w = 0; w < waves; ++w) t += sh[w * 64 + c];
            slab_b[(int64_t)blockIdx.x * Cout + c] = t;
        }
    }
}
// second stage: element e of gW (then of gb) = its slots added in ascending workgroup order
__global__ void __launch_bounds__(GRAD_BLOCK) k_wgrad_sum(const float* __restrict__ slab_w, const float* __restrict__ slab_b, int64_t groups,
                                                          int64_t n_w, int n_b, float* __restrict__ gW, float* __restrict__ gb) {
    const int64_t e = (int64_t)blockIdx.x * GRAD_BLOCK + threadIdx.x;
    if (e < n_w) {
        float s = 0.f;
        for (int64_t g = 0; g < groups; ++g) s += slab_w[g * n_w + e];
        gW[e] = s;
    } else if (e < n_w + n_b && gb) {
        const int64_t c = e - n_w;
        float s = 0.f;
        for (int64_t g = 0; g < groups; ++g) s += slab_b[g * n_b + c];
        gb[c] = s;
    }
}

template <bool UP>
static int wgrad_launch(const int32_t* nbr, int K, int64_t n_rows, const float* x, int64_t n_in, int Cin, int x_ld, const float* gy,
                        int Cout, int gy_ld, float* gW, float* gb, void* workspace, size_t workspace_bytes, void* stream, const char* name) {
    const int64_t n_w = (int64_t)K * Cin * Cout;
    if (n_rows == 0) {
        hipError_t e = hipMemsetAsync(gW, 0, n_w * sizeof(float), S(stream));
        if (e == hipSuccess && gb) e = hipMemsetAsync(gb, 0, Cout * sizeof(float), S(stream));
        if (e != hipSuccess) { pcgc_set_error("%s: %s", name, hipGetErrorString(e)); return -1; }
        return 0;
    }
    const int64_t rpg = wgrad_rows_per_group(K, n_rows, Cin, Cout), groups = wgrad_groups(K, n_rows, Cin, Cout);
    float* slab_w = (float*)workspace;
    float* slab_b = gb ? slab_w + groups * n_w : nullptr;
    const int waves = K >= 4 ? 4 : K;
    const int mt = (Cin + 15) / 16, nt = (Cout + 15) / 16;
    const dim3 grid((unsigned)groups), block(64 * waves);
#define WGRAD_CASE(M, N)                                                                                                          \
    if (mt <= M && nt <= N) {                                                                                                     \
        hipLaunchKernelGGL((k_conv_wgrad<M, N, UP>), grid, block, 0, S(stream), nbr, K, n_rows, rpg, x, n_in, Cin, x_ld, gy, Cout, \
                           gy_ld, slab_w, slab_b);                                                                                \
    } else
    WGRAD_CASE(1, 1) WGRAD_CASE(1, 2) WGRAD_CASE(2, 1) WGRAD_CASE(2, 2) WGRAD_CASE(1, 4) WGRAD_CASE(4, 1) WGRAD_CASE(2, 4) WGRAD_CASE(4, 2)
    WGRAD_CASE(4, 4) { pcgc_set_error("%s: at most 64 channels", name); return -2; }
#undef WGRAD_CASE
    PCGC_CHECK_LAUNCH(name);
    hipLaunchKernelGGL(k_wgrad_sum, dim3(grid_for(n_w + Cout, GRAD_BLOCK)), dim3(GRAD_BLOCK), 0, S(stream), slab_w, slab_b, groups, n_w, Cout, gW, gb);
    PCGC_CHECK_LAUNCH(name);
    return 0;
}
extern "C" int pcgc_conv_wgrad(const int32_t* nbr, int K, int64_t n_out, const float* x, int64_t n_in, int Cin, int x_ld, const float* gy,
                               int Cout, int gy_ld, float* gW, float* gb, void* workspace, size_t workspace_bytes, void* stream) {
    PCGC_REQUIRE(K >= 1 && K <= 27 && n_out >= 0 && n_in >= 0, "bad sizes");
    PCGC_REQUIRE(Cin >= 1 && Cin <= 64 && Cout >= 1 && Cout <= 64 && x_ld >= Cin && gy_ld >= Cout, "channels must be 1 .. 64 and fit the leading dimensions");
    PCGC_REQUIRE(nbr || (K == 1 && n_in >= n_out), "a NULL map is the identity of a k1 convolution");
    PCGC_REQUIRE(gW && (n_out == 0 || (x && gy)), "null argument");
    PCGC_REQUIRE(n_out == 0 || (workspace && workspace_bytes >= pcgc_conv_wgrad_workspace_bytes(K, n_out, Cin, Cout) && ((uintptr_t)workspace & 3) == 0),
                 "workspace too small or misaligned");
    return wgrad_launch<false>(nbr, K, n_out, x, n_in, Cin, x_ld, gy, Cout, gy_ld, gW, gb, workspace, workspace_bytes, stream, "conv_wgrad");
}
extern "C" int pcgc_conv_up2_wgrad(int64_t n_in, const float* x, int64_t x_rows, int Cin, int x_ld, const int32_t* rows, const float* gy,
                                   int Cout, int gy_ld, float* gW, float* gb, void* workspace, size_t workspace_bytes, void* stream) {
    PCGC_REQUIRE(n_in >= 0 && x_rows >= 0 && (rows || x_rows >= n_in), "bad sizes");
    PCGC_REQUIRE(Cin >= 1 && Cin <= 64 && Cout >= 1 && Cout <= 64 && x_ld >= Cin && gy_ld >= Cout, "channels must be 1 .. 64 and fit the leading dimensions");
    PCGC_REQUIRE(gW && (n_in == 0 || (x && gy)), "null argument");
    PCGC_REQUIRE(n_in == 0 || (workspace && workspace_bytes >= pcgc_conv_wgrad_workspace_bytes(8, n_in, Cin, Cout) && ((uintptr_t)workspace & 3) == 0),
                 "workspace too small or misaligned");
    return wgrad_launch<true>(rows, 8, n_in, x, x_rows, Cin, x_ld, gy, Cout, gy_ld, gW, gb, workspace, workspace_bytes, stream, "conv_up2_wgrad");
}

// ---- transposed kernel map ---------------------------------------------------------------------------------------------------------------
// inv[k][nbr[k][o]] = o, -1 elsewhere.  For a fixed k the map o -> nbr[k][o] is injective (k3: a translation; k2 s2 down: a fine row has one
// parent; generative up: a child has one parent), so every slot has at most one writer.
__global__ void __launch_bounds__(GRAD_BLOCK) k_kmap_invert(const int32_t* __restrict__ nbr, int64_t total, int64_t n_out, int64_t n_in,
                                                            int32_t* __restrict__ inv) {
    const int64_t t = (int64_t)blockIdx.x * GRAD_BLOCK + threadIdx.x;
    if (t >= total) return;
    const int64_t k = t / n_out, o = t - k * n_out;
    const int32_t i = nbr[t];
    if (i >= 0 && i < n_in) inv[k * n_in + i] = (int32_t)o;
}
extern "C" int pcgc_kmap_invert(const int32_t* nbr, int K, int64_t n_out, int64_t n_in, int32_t* inv, void* stream) {
    PCGC_REQUIRE(K >= 1 && n_out >= 0 && n_in >= 0 && n_out < ((int64_t)1 << 31) && n_in < ((int64_t)1 << 31), "bad sizes");
    if (n_in == 0) return 0;
    PCGC_REQUIRE(inv && (n_out == 0 || nbr), "null argument");
    hipError_t e = hipMemsetAsync(inv, 0xFF, (size_t)K * n_in * sizeof(int32_t), S(stream));
    if (e != hipSuccess) { pcgc_set_error("kmap_invert: %s", hipGetErrorString(e)); return -1; }
    if (n_out == 0) return 0;
    const int64_t total = (int64_t)K * n_out;
    hipLaunchKernelGGL(k_kmap_invert, dim3(grid_for(total, GRAD_BLOCK)), dim3(GRAD_BLOCK), 0, S(stream), nbr, total, n_out, n_in, inv);
    PCGC_CHECK_LAUNCH("kmap_invert");
    return 0;
}

// ---- small adjoints ----------------------------------------------------------------------------------------------------------------------
// ReLU: gx = g where y > 0 (decided on the bit pattern: +denormals pass, -0.0 / NaN do not, whatever the denormal mode), else +0
__global__ void __launch_bounds__(GRAD_BLOCK) k_relu_bwd(const float* __restrict__ g, int g_ld, const float* __restrict__ y, int y_ld,
                                                         int64_t n, int C, float* __restrict__ out, int out_ld) {
    const int64_t t = (int64_t)blockIdx.x * GRAD_BLOCK + threadIdx.x;
    if (t >= n * C) return;
    const int64_t r = t / C;
    const int c = (int)(t - r * C);
    const int32_t bits = __float_as_int(y[r * y_ld + c]);
    out[r * out_ld + c] = (bits > 0 && bits <= 0x7f800000) ? g[r * g_ld + c] : 0.f;
}
extern "C" int pcgc_relu_bwd(const float* g, int g_ld, const float* y, int y_ld, int64_t n, int C, float* out, int out_ld, void* stream) {
    PCGC_REQUIRE(n >= 0 && C >= 1 && g_ld >= C && y_ld >= C && out_ld >= C, "bad arguments");
    if (n == 0) return 0;
    PCGC_REQUIRE(g && y && out, "null argument");
    hipLaunchKernelGGL(k_relu_bwd, dim3(grid_for(n * C, GRAD_BLOCK)), dim3(GRAD_BLOCK), 0, S(stream), g, g_ld, y, y_ld, n, C, out, out_ld);
    PCGC_CHECK_LAUNCH("relu_bwd");
    return 0;
}
// adjoint of a row gather (pcgc_gather_rows_f32_ld, pcgc_compact_feats): gx = 0, then gx[orig[r]] = gy[r]; orig is unique
__global__ void __launch_bounds__(GRAD_BLOCK) k_scatter_rows(const float* __restrict__ gy, int gy_ld, const int32_t* __restrict__ orig,
                                                             int64_t n_rows, int C, int64_t n_out, float* __restrict__ gx, int gx_ld) {
    const int64_t t = (int64_t)blockIdx.x * GRAD_BLOCK + threadIdx.x;
    if (t >= n_rows * C) return;
    const int64_t r = t / C;
    const int c = (int)(t - r * C);
    const int64_t o = orig[r];
    if (o >= 0 && o < n_out) gx[o * gx_ld + c] = gy[r * gy_ld + c];
}
extern "C" int pcgc_scatter_rows(const float* gy, int C, int gy_ld, const int32_t* orig, int64_t n_rows, float* gx, int64_t n_out, int gx_ld,
                                 void* stream) {
    PCGC_REQUIRE(n_rows >= 0 && n_out >= 0 && C >= 1 && gy_ld >= C && gx_ld >= C, "bad arguments");
    if (n_out == 0) return 0;
    PCGC_REQUIRE(gx && (n_rows == 0 || (gy && orig)), "null argument");
    hipError_t e = gx_ld == C ? hipMemsetAsync(gx, 0, (size_t)n_out * C * sizeof(float), S(stream))
                              : hipMemset2DAsync(gx, (size_t)gx_ld * sizeof(float), 0, (size_t)C * sizeof(float), (size_t)n_out, S(stream));
    if (e != hipSuccess) { pcgc_set_error("scatter_rows: %s", hipGetErrorString(e)); return -1; }
    if (n_rows == 0) return 0;
    hipLaunchKernelGGL(k_scatter_rows, dim3(grid_for(n_rows * C, GRAD_BLOCK)), dim3(GRAD_BLOCK), 0, S(stream), gy, gy_ld, orig, n_rows, C, n_out, gx, gx_ld);
    PCGC_CHECK_LAUNCH("scatter_rows");
    return 0;
}

// ---- BCE-with-logits gradient (loss.py:8-15): d(sum of the terms / ln 2) / dz_i = (sigmoid(z_i) - t_i) / ln 2, times `scale`; fp64, one rounding
__global__ void __launch_bounds__(GRAD_BLOCK) k_bce_bwd(const float* __restrict__ z, int64_t ld, int64_t n, const uint8_t* __restrict__ truth,
                                                        double scale, float* __restrict__ g) {
    const int64_t i = (int64_t)blockIdx.x * GRAD_BLOCK + threadIdx.x;
    if (i >= n) return;
    const double v = (double)z[i * ld];
    const double d = truth[i] ? -eb_sigmoid(-v) : eb_sigmoid(v);       // sigmoid(v) - 1 = -sigmoid(-v): no cancellation where sigmoid saturates
    g[i] = (float)(scale * d / 0.693147180559945309417232121458);
}
extern "C" int pcgc_bce_logits_bwd(const float* logits, int64_t ld, int64_t n, const uint8_t* truth, double scale, float* g, void* stream) {
    PCGC_REQUIRE(n >= 0 && ld >= 1, "bad arguments");
    if (n == 0) return 0;
    PCGC_REQUIRE(logits && truth && g, "null argument");
    hipLaunchKernelGGL(k_bce_bwd, dim3(grid_for(n, GRAD_BLOCK)), dim3(GRAD_BLOCK), 0, S(stream), logits, ld, n, truth, scale, g);
    PCGC_CHECK_LAUNCH("bce_logits_bwd");
    return 0;
}

// ---- bottleneck rate gradient: reverse mode of eb_logits.h's chain for bits = -sum log2 max(lik, bound) --------------------------------------
// Per element (row, channel c) at v: lo = L(v - 0.5), up = L(v + 0.5), d = sigmoid(s up) - sigmoid(s lo) (s = the sign trick, a constant),
// term = -log2 |d|.  Where the fp32 likelihood the forward kernel stores is below the bound the element contributes nothing (Low_bound).
// Layer i of L: s_r = sum_q sp[r][q] h_q + b_r, t_r = s_r + tf_r tanh(s_r), sp = softplus(matrix), tf = tanh(factor); the tape keeps each
// layer's inputs h and tanh(s_r).  A thread accumulates the 44 parameter gradients of its channel over its rows (ascending) in fp64; the
// block adds its threads of one channel in ascending order into the slab; k_eb_bwd_final adds the blocks in ascending order, applies
// softplus' = sigmoid and tanh' = 1 - tanh^2 of the raw parameters, scales and rounds once.
struct EbTape { double h[4][3]; double th[4][3]; };
__device__ static double eb_logits_tape(const float* __restrict__ P, int C, int c, double v, const EbShared& sh, EbTape& tp) {
    constexpr int F[5] = {1, 3, 3, 3, 1}, LOFF[4] = {0, 3, 12, 21}, FOFF[4] = {0, 3, 6, 9};
    const float* B = P + 24 * C;
    const double* sp = sh.sp + c * 24; const double* tf = sh.tf + c * 10;
    double h[3] = {v, 0, 0}, t[3] = {0, 0, 0};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int fi = F[i], fo = F[i + 1];
#pragma unroll
        for (int q = 0; q < 3; ++q) tp.h[i][q] = q < fi ? h[q] : 0.0;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            if (r >= fo) continue;
            double s = 0;
#pragma unroll
            for (int q = 0; q < 3; ++q) if (q < fi) s += sp[LOFF[i] + r * fi + q] * h[q];
            s += (double)B[C * FOFF[i] + c * fo + r];
            const double th = tanh(s);
            tp.th[i][r] = th;
            t[r] = s + tf[FOFF[i] + r] * th;
        }
#pragma unroll
        for (int r = 0; r < 3; ++r) if (r < fo) h[r] = t[r];
    }
    return h[0];
}
// acc[0..23] += d/d sp, acc[24..33] += d/d bias, acc[34..43] += d/d tf; -> d/dv
__device__ static double eb_logits_bwd(int c, const EbShared& sh, const EbTape& tp, double gout, double* acc) {
    constexpr int F[5] = {1, 3, 3, 3, 1}, LOFF[4] = {0, 3, 12, 21}, FOFF[4] = {0, 3, 6, 9};
    const double* sp = sh.sp + c * 24; const double* tf = sh.tf + c * 10;
    double gt[3] = {gout, 0, 0};
#pragma unroll
    for (int i = 3; i >= 0; --i) {
        const int fi = F[i], fo = F[i + 1];
        double gh[3] = {0, 0, 0};
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            if (r >= fo) continue;
            const double th = tp.th[i][r];
            const double ds = gt[r] * (1.0 + tf[FOFF[i] + r] * (1.0 - th * th));
            acc[34 + FOFF[i] + r] += gt[r] * th;
            acc[24 + FOFF[i] + r] += ds;
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                if (q >= fi) continue;
                acc[LOFF[i] + r * fi + q] += ds * tp.h[i][q];
                gh[q] += ds * sp[LOFF[i] + r * fi + q];
            }
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) gt[q] = gh[q];
    }
    return gt[0];
}
constexpr int EB_BWD_PASSES = 8;                         // rows per thread
__global__ void __launch_bounds__(GRAD_BLOCK) k_eb_bwd(const float* __restrict__ feats, int ld, int64_t n, int C, const float* __restrict__ P,
                                                       float bound, double scale, float* __restrict__ gy, double* __restrict__ slab) {
    __shared__ EbShared sh;
    __shared__ double red[GRAD_BLOCK];
    eb_prepare(P, C, sh);
    __syncthreads();
    const int rows_pass = GRAD_BLOCK / C;
    const int c = threadIdx.x % C, sub = threadIdx.x / C;
    const bool active = sub < rows_pass;
    const int64_t row0 = (int64_t)blockIdx.x * rows_pass * EB_BWD_PASSES;
    double acc[44];
#pragma unroll
    for (int j = 0; j < 44; ++j) acc[j] = 0.0;
    if (active) {
        for (int p = 0; p < EB_BWD_PASSES; ++p) {
            const int64_t row = row0 + (int64_t)p * rows_pass + sub;
            if (row >= n) break;
            const double v = (double)feats[row * ld + c];
            EbTape tlo, tup;
            const double lo = eb_logits_tape(P, C, c, v - 0.5, sh, tlo), up = eb_logits_tape(P, C, c, v + 0.5, sh, tup);
            const double sum = lo + up, sign = sum > 0 ? -1.0 : (sum < 0 ? 1.0 : 0.0);
            const double su = eb_sigmoid(sign * up), sl = eb_sigmoid(sign * lo);
            const double d = su - sl, pd = fabs(d);
            double gv = 0.0;
            if (!((float)pd < bound) && pd > 0.0) {
                // d term / d d = -sgn(d) / (|d| ln 2); d d / d up = s su (1 - su), d d / d lo = -s sl (1 - sl)
                const double gd = -(d > 0 ? 1.0 : -1.0) / (pd * 0.693147180559945309417232121458);
                const double gup = gd * sign * su * eb_sigmoid(-sign * up), glo = -gd * sign * sl * eb_sigmoid(-sign * lo);
                gv = eb_logits_bwd(c, sh, tup, gup, acc) + eb_logits_bwd(c, sh, tlo, glo, acc);
            }
            gy[row * C + c] = (float)(scale * gv);
        }
    }
    // per parameter: the block's threads of one channel, row subsets ascending
    double* out = slab + (int64_t)blockIdx.x * 44 * C;
#pragma unroll
    for (int j = 0; j < 44; ++j) {
        red[threadIdx.x] = active ? acc[j] : 0.0;
        __syncthreads();
        if (threadIdx.x < C) {
            double s = 0.0;
            for (int u = 0; u < rows_pass; ++u) s += red[u * C + threadIdx.x];
            out[j * C + threadIdx.x] = s;
        }
        __syncthreads();
    }
}
// thread = one of the 44 C packed parameters (matrices | biases | factors, eb_logits.h)
__global__ void __launch_bounds__(GRAD_BLOCK) k_eb_bwd_final(const double* __restrict__ slab, int64_t blocks, int C, const float* __restrict__ P,
                                                             double scale, float* __restrict__ gP) {
    const int e = blockIdx.x * GRAD_BLOCK + threadIdx.x;
    if (e >= 44 * C) return;
    constexpr int F[5] = {1, 3, 3, 3, 1}, LOFF[4] = {0, 3, 12, 21}, FOFF[4] = {0, 3, 6, 9};
    int j, c;                                            // j: index inside the channel's 44 accumulators
    double chain;
    if (e < 24 * C) {
        int i = 3;
        while (C * LOFF[i] > e) --i;
        const int sz = F[i + 1] * F[i], w = e - C * LOFF[i];
        c = w / sz; j = LOFF[i] + w % sz;
        chain = eb_sigmoid((double)P[e]);                // softplus'
    } else {
        const bool fac = e >= 34 * C;
        const int w0 = e - (fac ? 34 : 24) * C;
        int i = 3;
        while (C * FOFF[i] > w0) --i;
        const int fo = F[i + 1], w = w0 - C * FOFF[i];
        c = w / fo; j = (fac ? 34 : 24) + FOFF[i] + w % fo;
        const double t = fac ? tanh((double)P[e]) : 0.0;
        chain = fac ? 1.0 - t * t : 1.0;
    }
    double s = 0.0;
    for (int64_t b = 0; b < blocks; ++b) s += slab[(b * 44 + j) * C + c];
    gP[e] = (float)(scale * s * chain);
}
static inline int64_t eb_bwd_blocks(int64_t n, int C) {
    const int64_t rows_block = (int64_t)(GRAD_BLOCK / C) * EB_BWD_PASSES;
    return n > 0 ? (n + rows_block - 1) / rows_block : 0;
}
extern "C" size_t pcgc_eb_bwd_workspace_bytes(int64_t n, int C) {
    if (C < 1 || C > EB_MAX_C || n < 0) return 0;
    return (size_t)eb_bwd_blocks(n, C) * 44 * C * sizeof(double) + 64;
}
extern "C" int pcgc_eb_likelihood_bwd(const float* feats, int ld, int64_t n, int C, const float* params, float bound, double scale,
                                      float* gy, float* gparams, void* workspace, size_t workspace_bytes, void* stream) {
    PCGC_REQUIRE(C >= 1 && C <= EB_MAX_C, "entropy bottleneck: at most 16 channels");
    PCGC_REQUIRE(n >= 0 && ld >= C && params && gparams, "bad arguments");
    const int64_t blocks = eb_bwd_blocks(n, C);
    PCGC_REQUIRE(blocks < ((int64_t)1 << 31), "too many elements");
    if (n > 0) {
        PCGC_REQUIRE(feats && gy, "null argument");
        PCGC_REQUIRE(workspace && workspace_bytes >= pcgc_eb_bwd_workspace_bytes(n, C) && ((uintptr_t)workspace & 7) == 0, "workspace too small or misaligned");
        hipLaunchKernelGGL(k_eb_bwd, dim3((unsigned)blocks), dim3(GRAD_BLOCK), 0, S(stream), feats, ld, n, C, params, bound, scale, gy, (double*)workspace);
        PCGC_CHECK_LAUNCH("eb_likelihood_bwd");
    }
    hipLaunchKernelGGL(k_eb_bwd_final, dim3(grid_for(44 * C, GRAD_BLOCK)), dim3(GRAD_BLOCK), 0, S(stream), (const double*)workspace, blocks, C, params, scale, gparams);
    PCGC_CHECK_LAUNCH("eb_likelihood_bwd");
    return 0;
}
