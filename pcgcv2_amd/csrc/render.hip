// Rendering a cloud into views (the definition is tests/render_reference.py): a z-buffer splat of the rows of up to 64
// (batch item, view) pairs, the pictures read out of it, and the integer sums of the projection metrics of two renderings.  The reference
// has no renderer.  Integers only; every output is a function of the rows, their order and the matrices.
//
// Transform.  A view is a 3x4 integer matrix M in Q16 (int64, built and range-checked by the host: pcgcv2_amd/render.py).  For a row
// (b, x, y, z): (u, v, d) = (M[:, :3] . (x, y, z) + M[:, 3]) >> 16, the products and sums in 64 bits, the shift arithmetic (a floor).
// With |M[:, :3]| <= 2^20, coordinates below 2^21 and |M[:, 3]| <= 2^60 nothing leaves int64; u and v are compared with the image in 64
// bits, so no matrix can place a pixel outside it; d is the host's to keep inside int32.
//
// Order.  The z-buffer holds one 64-bit word per (item, view, pixel): all ones = background, else (d + 2^31) << 32 | row.  A row covers
// the pixels [u - r, u + r] x [v - r, v + r] clipped to the image and lowers each word with an unsigned 64-bit atomic minimum: the
// smallest d wins, among equal d the smallest row, whatever order the threads arrive in.  A row's word is never all ones (row < 2^31).
// A plain read comes first (as coords.hip does for its hash): words only fall, so a word that is not above the row's is settled.
//
// No workgroup waits on another, every loop has a fixed trip count, and the only atomics are 64-bit integer minima and additions.
#include "pcgc_common.h"

#define RENDER_MAX_SLICES 64                    // batch items x views
#define RENDER_MAX_SIDE 4096
#define RENDER_MAX_R 4
#define RENDER_SPLAT_ROWS 256                   // rows per workgroup of the splat
#define RENDER_COORD_LIMIT (1u << 21)
#define RENDER_EMPTY 0xFFFFFFFFFFFFFFFFull
#define RENDER_SHADE_SPAN 200                   // the depth shade runs from 255 (near) down to 255 - RENDER_SHADE_SPAN (far)
#define RENDER_DEPTH_DIFF_LIMIT (1ll << 19)     // |depth_a - depth_b| the depth SSE takes in: 2^38 x 2^24 pixels stays below 2^63
#define RENDER_METRIC_SUMS 8                    // U, I, SSE R, G, B, Y, SSE depth, pixels of I at or past the limit

typedef unsigned long long u64;

// ---- clear -----------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_render_clear(u64* __restrict__ zbuf, int64_t words) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += stride) zbuf[i] = RENDER_EMPTY;
}

// ---- splat -----------------------------------------------------------------------------------------------------------------------------
__device__ static inline u64 zb_load(const u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// grid (rows / RENDER_SPLAT_ROWS, V): the matrix is uniform over a workgroup.  bad [1]: rows whose batch item or coordinates are out of
// range (counted by view 0 only; such a row touches nothing).  issued (null in the product; tools/render_time.py): the atomics sent, that is
// the covered pixels less the early-outs
__global__ void __launch_bounds__(RENDER_SPLAT_ROWS) k_render_splat(const int4* __restrict__ coords, int64_t n, int B, int V, int H, int W,
                                                                     int r, const long long* __restrict__ matrices, u64* zbuf,
                                                                     int32_t* __restrict__ bad, u64* __restrict__ issued) {
    const int64_t row = (int64_t)blockIdx.x * RENDER_SPLAT_ROWS + threadIdx.x;
    const int view = blockIdx.y;
    if (row >= n) return;
    const int4 c = coords[row];
    if ((uint32_t)c.x >= (uint32_t)B || (uint32_t)c.y >= RENDER_COORD_LIMIT || (uint32_t)c.z >= RENDER_COORD_LIMIT ||
        (uint32_t)c.w >= RENDER_COORD_LIMIT) {
        if (view == 0) atomicAdd(bad, 1);
        return;
    }
    const long long* m = matrices + 12 * view;
    const long long x = c.y, y = c.z, z = c.w;
    const long long u = (m[0] * x + m[1] * y + m[2] * z + m[3]) >> 16;
    const long long v = (m[4] * x + m[5] * y + m[6] * z + m[7]) >> 16;
    const long long d = (m[8] * x + m[9] * y + m[10] * z + m[11]) >> 16;
    if (u + r < 0 || u - r >= W || v + r < 0 || v - r >= H) return;    // (64-bit comparisons: u and v may be anywhere)
    const int u0 = (int)(u - r < 0 ? 0 : u - r), u1 = (int)(u + r > W - 1 ? W - 1 : u + r);
    const int v0 = (int)(v - r < 0 ? 0 : v - r), v1 = (int)(v + r > H - 1 ? H - 1 : v + r);
    const u64 word = ((u64)(uint32_t)((uint32_t)(int32_t)d + 0x80000000u) << 32) | (u64)(uint32_t)row;
    u64* slice = zbuf +((int64_t)c.x * V + view) * ((int64_t)H * W);
    int sent = 0;
    for (int py = v0; py <= v1; ++py)                                   // at most (2 r + 1)^2 = 81 pixels, all inside [0, H) x [0, W)
        for (int px = u0; px <= u1; ++px) {
            u64* p = slice + (int64_t)py * W + px;
            if (zb_load(p) <= word) continue;
            atomicMin(p, word);
            ++sent;
        }
    if (issued && sent) atomicAdd(issued, (u64)sent);
}

// ---- resolve ---------------------------------------------------------------------------------------------------------------------------
// grid (pixels / 256, B V).  Without colours the picture is the depth shade of DESIGN.md 8q between the view's near and far planes
__global__ void __launch_bounds__(256) k_render_resolve(const u64* __restrict__ zbuf, int64_t pixels, int V, int64_t n,
                                                        const uint8_t* __restrict__ colours, const int32_t* __restrict__ planes, uint32_t bg,
                                                        int32_t* __restrict__ index, int32_t* __restrict__ depth, uint8_t* __restrict__ mask,
                                                        uint8_t* __restrict__ image) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= pixels) return;
    const int slice = blockIdx.y;
    const int64_t at = (int64_t)slice * pixels + p;
    const u64 word = zbuf[at];
    int32_t row = -1, d = 0;
    uint8_t R = (uint8_t)(bg & 255), G = (uint8_t)((bg >> 8) & 255), Bl = (uint8_t)((bg >> 16) & 255), m = 0;
    const uint32_t lo = (uint32_t)word;
    if (word != RENDER_EMPTY && (int64_t)lo < n) {                      // (a word the splat wrote names a row; nothing else is followed)
        row = (int32_t)lo;
        d = (int32_t)((uint32_t)(word >> 32) - 0x80000000u);
        m = 1;
        if (colours) {
            R = colours[3 * (int64_t)row]; G = colours[3 * (int64_t)row + 1]; Bl = colours[3 * (int64_t)row + 2];
        } else {
            const int view = slice % V;
            const long long near = planes[2 * view], far = planes[2 * view + 1];
            const long long span = far > near ? far - near : 1;
            long long t = (long long)d - near;
            t = t < 0 ? 0 : (t > span ? span : t);
            R = G = Bl = (uint8_t)(255 - (RENDER_SHADE_SPAN * t) / span);
        }
    }
    index[at] = row; depth[at] = d; mask[at] = m;
    image[3 * at] = R; image[3 * at + 1] = G; image[3 * at + 2] = Bl;
}

// ---- metric ----------------------------------------------------------------------------------------------------------------------------
__device__ static inline int luma_q16(int R, int G, int B) { return (13933 * R + 46871 * G + 4732 * B + 32768) >> 16; }

// grid (workgroups per slice, B V): a workgroup sums its pixels in registers, across its lanes and waves, then adds once per sum
__global__ void __launch_bounds__(256) k_render_metric(const uint8_t* __restrict__ mask_a, const uint8_t* __restrict__ mask_b,
                                                       const uint8_t* __restrict__ image_a, const uint8_t* __restrict__ image_b,
                                                       const int32_t* __restrict__ depth_a, const int32_t* __restrict__ depth_b, int64_t pixels,
                                                       u64* __restrict__ sums) {
    __shared__ u64 part[4][RENDER_METRIC_SUMS];
    const int slice = blockIdx.y;
    const int64_t base = (int64_t)slice * pixels;
    u64 acc[RENDER_METRIC_SUMS];
#pragma unroll
    for (int k = 0; k < RENDER_METRIC_SUMS; ++k) acc[k] = 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < pixels; p += stride) {
        const int64_t at = base + p;
        const bool a = mask_a[at] != 0, b = mask_b[at] != 0;
        if (!(a || b)) continue;
        acc[0] += 1;
        const int ra = image_a[3 * at], ga = image_a[3 * at + 1], ba = image_a[3 * at + 2];
        const int rb = image_b[3 * at], gb = image_b[3 * at + 1], bb = image_b[3 * at + 2];
        const int dy = luma_q16(ra, ga, ba) - luma_q16(rb, gb, bb);
        acc[2] += (u64)((ra - rb) * (ra - rb)); acc[3] += (u64)((ga - gb) * (ga - gb)); acc[4] += (u64)((ba - bb) * (ba - bb));
        acc[5] += (u64)(dy * dy);
        if (a && b) {
            acc[1] += 1;
            long long dd = (long long)depth_a[at] - (long long)depth_b[at];
            dd = dd < 0 ? -dd : dd;
            if (dd >= RENDER_DEPTH_DIFF_LIMIT) acc[7] += 1; else acc[6] += (u64)(dd * dd);
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < RENDER_METRIC_SUMS; ++k) {
        u64 s = acc[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
        if (lane == 0) part[wave][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < RENDER_METRIC_SUMS) {
        const u64 s = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
        if (s) atomicAdd(sums + (int64_t)slice * RENDER_METRIC_SUMS + threadIdx.x, s);
    }
}

// ---- entries ---------------------------------------------------------------------------------------------------------------------------
extern "C" int64_t pcgc_render_splat_rows(void) { return RENDER_SPLAT_ROWS; }

static bool render_shape_ok(int B, int V, int H, int W) {
    return B >= 1 && V >= 1 && (int64_t)B * V <= RENDER_MAX_SLICES && H >= 1 && H <= RENDER_MAX_SIDE && W >= 1 && W <= RENDER_MAX_SIDE;
}

extern "C" int64_t pcgc_render_workspace_bytes(int B, int V, int H, int W) {
    if (!render_shape_ok(B, V, H, W)) return -1;
    return (int64_t)B * V * H * W * 8;
}

extern "C" int pcgc_render(const int32_t* coords, const uint8_t* colours, int64_t n, int B, int V, int H, int W, int r, const int64_t* matrices,
                           const int32_t* planes, uint32_t background, int32_t* index, int32_t* depth, uint8_t* mask, uint8_t* image,
                           int32_t* bad, uint64_t* issued, int phases, void* workspace, size_t workspace_bytes, void* stream) {
    PCGC_REQUIRE(render_shape_ok(B, V, H, W), "B V outside 1 .. 64 or a side outside 1 .. 4096");
    PCGC_REQUIRE(r >= 0 && r <= RENDER_MAX_R, "r outside 0 .. 4");
    PCGC_REQUIRE(n >= 0 && n < (1ll << 31), "row count outside 0 .. 2^31 - 1");
    PCGC_REQUIRE(background <= 0xFFFFFFu, "background is not 24 bits");
    PCGC_REQUIRE(phases >= 1 && phases <= 7, "phases outside 1 .. 7");
    PCGC_REQUIRE(workspace_bytes >= (size_t)pcgc_render_workspace_bytes(B, V, H, W), "workspace too small");
    PCGC_REQUIRE(matrices && planes && index && depth && mask && image && bad && workspace && (n == 0 || coords), "null argument");
    PCGC_REQUIRE(((uintptr_t)coords & 15) == 0 && ((uintptr_t)workspace & 7) == 0 && ((uintptr_t)matrices & 7) == 0, "misaligned argument");
    hipStream_t s = S(stream);
    const int64_t pixels = (int64_t)H * W, words = pixels * B * V;
    u64* zbuf = (u64*)workspace;
    hipError_t e = hipMemsetAsync(bad, 0, sizeof(int32_t), s);
    if (e == hipSuccess && issued) e = hipMemsetAsync(issued, 0, sizeof(uint64_t), s);
    if (e != hipSuccess) { pcgc_set_error("render: %s", hipGetErrorString(e)); return -1; }
    const int64_t clear_groups = (words + 255) / 256;
    if (phases & 1) {
        hipLaunchKernelGGL(k_render_clear, dim3((unsigned)(clear_groups < 16384 ? clear_groups : 16384)), dim3(256), 0, s, zbuf, words);
        PCGC_CHECK_LAUNCH("render_clear");
    }
    if (n > 0 && (phases & 2)) {
        hipLaunchKernelGGL(k_render_splat, dim3(grid_for(n, RENDER_SPLAT_ROWS), (unsigned)V), dim3(RENDER_SPLAT_ROWS), 0, s, (const int4*)coords,
                           n, B, V, H, W, r, (const long long*)matrices, zbuf, bad, (u64*)issued);
        PCGC_CHECK_LAUNCH("render_splat");
    }
    if (phases & 4) {
        hipLaunchKernelGGL(k_render_resolve, dim3(grid_for(pixels, 256), (unsigned)(B * V)), dim3(256), 0, s, zbuf, pixels, V, n, colours, planes,
                           background, index, depth, mask, image);
        PCGC_CHECK_LAUNCH("render_resolve");
    }
    return 0;
}

extern "C" int pcgc_render_metric(const uint8_t* mask_a, const uint8_t* mask_b, const uint8_t* image_a, const uint8_t* image_b,
                                  const int32_t* depth_a, const int32_t* depth_b, int slices, int64_t pixels, uint64_t* sums, void* stream) {
    PCGC_REQUIRE(slices >= 1 && slices <= RENDER_MAX_SLICES, "slices outside 1 .. 64");
    PCGC_REQUIRE(pixels >= 1 && pixels <= (int64_t)RENDER_MAX_SIDE * RENDER_MAX_SIDE, "pixels outside 1 .. 4096^2");
    PCGC_REQUIRE(mask_a && mask_b && image_a && image_b && depth_a && depth_b && sums, "null argument");
    hipStream_t s = S(stream);
    hipError_t e = hipMemsetAsync(sums, 0, (size_t)slices * RENDER_METRIC_SUMS * sizeof(uint64_t), s);
    if (e != hipSuccess) { pcgc_set_error("render_metric: %s", hipGetErrorString(e)); return -1; }
    const int64_t groups = (pixels + 1023) / 1024;                      // about four pixels a thread
    hipLaunchKernelGGL(k_render_metric, dim3((unsigned)(groups < 256 ? groups : 256), (unsigned)slices), dim3(256), 0, s, mask_a, mask_b, image_a,
                       image_b, depth_a, depth_b, pixels, (u64*)sums);
    PCGC_CHECK_LAUNCH("render_metric");
    return 0;
}
