// Voxelising a raw point cloud (the definition is tests/voxelize_reference.py): float or double rows in the caller's
// units -> the distinct voxels of a B-bit lattice in the codec's (z, y, x) order, with the number of rows merged into each, the voxel of
// every row and one colour per voxel.  Four steps, each its own launches on the caller's stream:
//   bounds    per-axis minimum and maximum of the finite rows in fp64 and the number of rows with a NaN or an infinity
//   quantise  q = rint((double(p) - origin) * scale), the key z << 40 | y << 20 | x, the number of rows outside [0, 2^B - 1]
//   heads     a stable sort of (key, row) and the scan of the run heads: the rank of every sorted row's voxel
//   merge     coordinates, counts, voxel_of and the colours: the rows of a voxel are adjacent, a workgroup reduces each of its runs in
//             LDS and adds one record per run that leaves it (64-bit integer atomics), or stores the record of a run that does not
// Nothing is handed from one workgroup to another inside a launch (the rule of DESIGN.md 8j): what a launch adds up is read by the next
// launch.  Integer sums and minima / maxima do not depend on the order they are taken in, so every output is the same on every run.
#include <cstring>
#include "pcgc_common.h"
#include <rocprim/rocprim.hpp>

#define VOX_BLOCK 256
#define VOX_TILE_ROWS 256                     // sorted rows per workgroup of the merge kernel: one per thread
#define VOX_BOUNDS_BLOCKS 1024                // the bounds kernel's largest grid; its partials are reduced by one workgroup
#define VOX_MAX_ROWS 2147483647ll

static size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

extern "C" int64_t pcgc_voxelize_tile_rows(void) { return VOX_TILE_ROWS; }

// ---- the exact widening: a float32 row read as the doubles of the same values.  A float32 denormal is man x 2^-149, built from the
// integer so that it does not depend on the denormal mode float conversions run under.
__device__ static inline double widen(float f) {
    const uint32_t u = __float_as_uint(f);
    if (((u >> 23) & 0xFFu) != 0) return (double)f;
    const double m = (double)(int32_t)(u & 0x7FFFFFu) * 0x1p-149;
    return (u >> 31) ? -m : m;
}
template <typename T> __device__ static inline void load_row(const T* __restrict__ p, int64_t i, double& x, double& y, double& z);
template <> __device__ inline void load_row<float>(const float* __restrict__ p, int64_t i, double& x, double& y, double& z) {
    x = widen(p[3 * i]); y = widen(p[3 * i + 1]); z = widen(p[3 * i + 2]);
}
template <> __device__ inline void load_row<double>(const double* __restrict__ p, int64_t i, double& x, double& y, double& z) {
    x = p[3 * i]; y = p[3 * i + 1]; z = p[3 * i + 2];
}
__device__ static inline bool finite3(double x, double y, double z) {
    const uint64_t inf = 0x7FF0000000000000ull;
    return ((uint64_t)__double_as_longlong(x) & inf) != inf && ((uint64_t)__double_as_longlong(y) & inf) != inf &&
           ((uint64_t)__double_as_longlong(z) & inf) != inf;
}

// ------------------------------------------------------------------------------------------------ bounds
// partial record of a workgroup: min x, y, z, max x, y, z (the identities +inf / -inf when it saw no finite row), then the bad rows
struct VoxPartial { double v[6]; unsigned long long bad; };

__device__ static inline void block_reduce_partial(double (&v)[6], unsigned long long& bad) {
    // 256 threads -> thread 0 holds the result.  Minima and maxima of finite doubles and an integer sum: no order dependence.
    __shared__ VoxPartial s[VOX_BLOCK / 64];
    for (int o = 32; o > 0; o >>= 1) {
        for (int k = 0; k < 3; ++k) {
            v[k] = fmin(v[k], __shfl_down(v[k], o, 64));
            v[3 + k] = fmax(v[3 + k], __shfl_down(v[3 + k], o, 64));
        }
        bad += __shfl_down(bad, o, 64);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { for (int k = 0; k < 6; ++k) s[wave].v[k] = v[k]; s[wave].bad = bad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < VOX_BLOCK / 64; ++w) {
            for (int k = 0; k < 3; ++k) { v[k] = fmin(v[k], s[w].v[k]); v[3 + k] = fmax(v[3 + k], s[w].v[3 + k]); }
            bad += s[w].bad;
        }
    }
}

template <typename T>
__global__ void __launch_bounds__(VOX_BLOCK) k_vox_bounds(const T* __restrict__ points, int64_t n, VoxPartial* __restrict__ partial) {
    const double inf = __longlong_as_double(0x7FF0000000000000ll);
    double v[6] = {inf, inf, inf, -inf, -inf, -inf};
    unsigned long long bad = 0;
    const int64_t step = (int64_t)gridDim.x * VOX_BLOCK;
    for (int64_t i = (int64_t)blockIdx.x * VOX_BLOCK + threadIdx.x; i < n; i += step) {
        double x, y, z;
        load_row<T>(points, i, x, y, z);
        if (finite3(x, y, z)) {
            v[0] = fmin(v[0], x); v[1] = fmin(v[1], y); v[2] = fmin(v[2], z);
            v[3] = fmax(v[3], x); v[4] = fmax(v[4], y); v[5] = fmax(v[5], z);
        } else {
            ++bad;
        }
    }
    block_reduce_partial(v, bad);
    if (threadIdx.x == 0) { for (int k = 0; k < 6; ++k) partial[blockIdx.x].v[k] = v[k]; partial[blockIdx.x].bad = bad; }
}

// one workgroup: the partials of the first launch -> bounds [6] (a zero comes out as +0) and the number of bad rows
__global__ void __launch_bounds__(VOX_BLOCK) k_vox_bounds_finish(const VoxPartial* __restrict__ partial, int blocks, double* __restrict__ bounds,
                                                                 int64_t* __restrict__ bad_rows) {
    const double inf = __longlong_as_double(0x7FF0000000000000ll);
    double v[6] = {inf, inf, inf, -inf, -inf, -inf};
    unsigned long long bad = 0;
    for (int b = threadIdx.x; b < blocks; b += VOX_BLOCK) {
        for (int k = 0; k < 3; ++k) { v[k] = fmin(v[k], partial[b].v[k]); v[3 + k] = fmax(v[3 + k], partial[b].v[3 + k]); }
        bad += partial[b].bad;
    }
    block_reduce_partial(v, bad);
    if (threadIdx.x == 0) {
        for (int k = 0; k < 6; ++k) bounds[k] = v[k] + 0.0;
        *bad_rows = (int64_t)bad;
    }
}

static unsigned bounds_blocks(int64_t n) {
    int64_t b = (n + VOX_BLOCK - 1) / VOX_BLOCK;
    return (unsigned)(b < 1 ? 1 : (b > VOX_BOUNDS_BLOCKS ? VOX_BOUNDS_BLOCKS : b));
}

extern "C" int64_t pcgc_voxelize_bounds_workspace_bytes(int64_t n) {
    (void)n;
    return (int64_t)align256(sizeof(VoxPartial) * VOX_BOUNDS_BLOCKS);
}

extern "C" int pcgc_voxelize_bounds(const void* points, int is_f64, int64_t n, double* bounds, int64_t* bad_rows, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    PCGC_REQUIRE(n >= 1 && n <= VOX_MAX_ROWS, "1 .. 2^31 - 1 rows");
    PCGC_REQUIRE(points && bounds && bad_rows && workspace, "null argument");
    PCGC_REQUIRE(is_f64 == 0 || is_f64 == 1, "is_f64 is 0 (float32 rows) or 1 (float64 rows)");
    PCGC_REQUIRE(workspace_bytes >= (size_t)pcgc_voxelize_bounds_workspace_bytes(n), "workspace too small");
    VoxPartial* partial = (VoxPartial*)workspace;
    const unsigned blocks = bounds_blocks(n);
    if (is_f64) hipLaunchKernelGGL(k_vox_bounds<double>, dim3(blocks), dim3(VOX_BLOCK), 0, S(stream), (const double*)points, n, partial);
    else hipLaunchKernelGGL(k_vox_bounds<float>, dim3(blocks), dim3(VOX_BLOCK), 0, S(stream), (const float*)points, n, partial);
    PCGC_CHECK_LAUNCH("voxelize_bounds");
    hipLaunchKernelGGL(k_vox_bounds_finish, dim3(1), dim3(VOX_BLOCK), 0, S(stream), (const VoxPartial*)partial, (int)blocks, bounds, bad_rows);
    PCGC_CHECK_LAUNCH("voxelize_bounds");
    return 0;
}

// ------------------------------------------------------------------------------------------------ quantise and key
// The subtraction and the product are two fp64 operations, each rounded once (the library is built with -ffp-contract=off); rint rounds
// ties to even.  A row whose q leaves [0, qmax] on any axis (a NaN does too) is counted and gets key 0: the caller refuses the cloud.
template <typename T>
__global__ void __launch_bounds__(VOX_BLOCK) k_vox_quantize(const T* __restrict__ points, int64_t n, double ox, double oy, double oz, double scale,
                                                            double qmax, uint64_t* __restrict__ keys, int32_t* __restrict__ rows,
                                                            unsigned long long* __restrict__ outside) {
    const int64_t i = (int64_t)blockIdx.x * VOX_BLOCK + threadIdx.x;
    int bad = 0;
    if (i < n) {
        double x, y, z;
        load_row<T>(points, i, x, y, z);
        const double dx = x - ox, dy = y - oy, dz = z - oz;
        const double qx = rint(dx * scale), qy = rint(dy * scale), qz = rint(dz * scale);
        bad = !(qx >= 0.0 && qx <= qmax && qy >= 0.0 && qy <= qmax && qz >= 0.0 && qz <= qmax);
        keys[i] = bad ? 0ull : (((uint64_t)(int64_t)qz << 40) | ((uint64_t)(int64_t)qy << 20) | (uint64_t)(int64_t)qx);
        rows[i] = (int32_t)i;
    }
    const int total = __syncthreads_count(bad);
    if (threadIdx.x == 0 && total) atomicAdd(outside, (unsigned long long)total);
}

extern "C" int pcgc_voxelize_quantize(const void* points, int is_f64, int64_t n, int bits, double ox, double oy, double oz, double scale,
                                      uint64_t* keys, int32_t* rows, int64_t* outside, void* stream) {
    PCGC_REQUIRE(n >= 1 && n <= VOX_MAX_ROWS, "1 .. 2^31 - 1 rows");
    PCGC_REQUIRE(bits >= 1 && bits <= 20, "bits in 1 .. 20");
    PCGC_REQUIRE(points && keys && rows && outside, "null argument");
    PCGC_REQUIRE(is_f64 == 0 || is_f64 == 1, "is_f64 is 0 (float32 rows) or 1 (float64 rows)");
    if (hipMemsetAsync(outside, 0, sizeof(int64_t), S(stream)) != hipSuccess) { pcgc_set_error("voxelize_quantize: memset failed"); return -1; }
    const double qmax = (double)((1 << bits) - 1);
    const unsigned grid = grid_for(n, VOX_BLOCK);
    if (is_f64) hipLaunchKernelGGL(k_vox_quantize<double>, dim3(grid), dim3(VOX_BLOCK), 0, S(stream), (const double*)points, n, ox, oy, oz, scale,
                                   qmax, keys, rows, (unsigned long long*)outside);
    else hipLaunchKernelGGL(k_vox_quantize<float>, dim3(grid), dim3(VOX_BLOCK), 0, S(stream), (const float*)points, n, ox, oy, oz, scale, qmax,
                            keys, rows, (unsigned long long*)outside);
    PCGC_CHECK_LAUNCH("voxelize_quantize");
    return 0;
}

// ------------------------------------------------------------------------------------------------ heads
// rocPRIM's radix sort is stable: inside a run of equal keys the rows ascend, so a run's head is the voxel's lowest input row.
struct VoxHead {
    const uint64_t* keys;
    __host__ __device__ int32_t operator()(size_t i) const { return (i == 0 || keys[i] != keys[i - 1]) ? 1 : 0; }
};
using VoxHeadIt = rocprim::transform_iterator<rocprim::counting_iterator<size_t>, VoxHead, int32_t>;

static size_t vox_sort_temp(int64_t n, int bits) {
    size_t tmp = 0;
    (void)rocprim::radix_sort_pairs((void*)nullptr, tmp, (uint64_t*)nullptr, (uint64_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr, (size_t)n,
                                    0, 40 + bits, (hipStream_t)0);
    return tmp;
}
static size_t vox_scan_temp(int64_t n) {
    size_t tmp = 0;
    VoxHeadIt in(rocprim::counting_iterator<size_t>(0), VoxHead{nullptr});
    (void)rocprim::inclusive_scan((void*)nullptr, tmp, in, (int32_t*)nullptr, (size_t)n, rocprim::plus<int32_t>(), (hipStream_t)0);
    return tmp;
}

extern "C" int64_t pcgc_voxelize_heads_workspace_bytes(int64_t n) {
    if (n < 1) n = 1;
    size_t a = vox_sort_temp(n, 20), b = vox_scan_temp(n);
    return (int64_t)align256(a > b ? a : b);
}

extern "C" int pcgc_voxelize_heads(const uint64_t* keys, const int32_t* rows, int64_t n, int bits, uint64_t* sorted_keys, int32_t* sorted_rows,
                                   int32_t* rank, void* workspace, size_t workspace_bytes, void* stream) {
    PCGC_REQUIRE(n >= 1 && n <= VOX_MAX_ROWS, "1 .. 2^31 - 1 rows");
    PCGC_REQUIRE(bits >= 1 && bits <= 20, "bits in 1 .. 20");
    PCGC_REQUIRE(keys && rows && sorted_keys && sorted_rows && rank && workspace, "null argument");
    PCGC_REQUIRE(workspace_bytes >= (size_t)pcgc_voxelize_heads_workspace_bytes(n), "workspace too small");
    size_t tmp = vox_sort_temp(n, bits);
    hipError_t e = rocprim::radix_sort_pairs(workspace, tmp, keys, sorted_keys, rows, sorted_rows, (size_t)n, 0, 40 + bits, S(stream));
    if (e != hipSuccess) { pcgc_set_error("voxelize_heads: sort: %s", hipGetErrorString(e)); return -1; }
    tmp = vox_scan_temp(n);
    VoxHeadIt in(rocprim::counting_iterator<size_t>(0), VoxHead{sorted_keys});
    e = rocprim::inclusive_scan(workspace, tmp, in, rank, (size_t)n, rocprim::plus<int32_t>(), S(stream));
    if (e != hipSuccess) { pcgc_set_error("voxelize_heads: scan: %s", hipGetErrorString(e)); return -1; }
    PCGC_CHECK_LAUNCH("voxelize_heads");
    return 0;
}

// ------------------------------------------------------------------------------------------------ merge
// acc [m][4] (uint64): rows, red, green and blue sums of every voxel.  One sorted row per thread; a segmented inclusive scan over the tile
// in LDS (the record of a row packs count << 48 | red << 32 | green << 16 | blue: 256 rows of 255 stay inside their 16 bits).  The last
// row of a run inside the tile holds the run's part of this tile: stored when the run neither began before the tile nor goes on behind it,
// added with integer atomics otherwise.  A cloud that is one voxel therefore issues one record per VOX_TILE_ROWS rows, not one per row.
__global__ void __launch_bounds__(VOX_TILE_ROWS) k_vox_merge(const uint64_t* __restrict__ keys, const int32_t* __restrict__ rows,
                                                             const int32_t* __restrict__ rank, int64_t n, const uint8_t* __restrict__ colours,
                                                             int first, int32_t* __restrict__ coords, int32_t* __restrict__ voxel_of,
                                                             uint8_t* __restrict__ colours_out, unsigned long long* __restrict__ acc) {
    __shared__ int32_t s_voxel[VOX_TILE_ROWS];
    __shared__ uint64_t s_rec[2][VOX_TILE_ROWS];
    const int t = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * VOX_TILE_ROWS, i = i0 + t;
    const bool live = i < n;
    int32_t v = -1, row = 0;
    uint64_t rec = 0;
    bool head = false;
    if (live) {
        v = rank[i] - 1;
        row = rows[i];
        head = i == 0 || rank[i - 1] != rank[i];
        voxel_of[row] = v;
        uint32_t r = 0, g = 0, b = 0;
        if (colours) { r = colours[3 * (int64_t)row]; g = colours[3 * (int64_t)row + 1]; b = colours[3 * (int64_t)row + 2]; }
        rec = (1ull << 48) | ((uint64_t)r << 32) | ((uint64_t)g << 16) | (uint64_t)b;
        if (head) {
            const uint64_t k = keys[i];
            ((int4*)coords)[v] = make_int4(0, (int32_t)(k & 0xFFFFF), (int32_t)((k >> 20) & 0xFFFFF), (int32_t)((k >> 40) & 0xFFFFF));
            if (first && colours) { colours_out[3 * (int64_t)v] = (uint8_t)r; colours_out[3 * (int64_t)v + 1] = (uint8_t)g; colours_out[3 * (int64_t)v + 2] = (uint8_t)b; }
        }
    }
    s_voxel[t] = v;
    s_rec[0][t] = rec;
    __syncthreads();
    int cur = 0;
    for (int d = 1; d < VOX_TILE_ROWS; d <<= 1) {
        uint64_t mine = s_rec[cur][t];
        if (t >= d && s_voxel[t - d] == v) mine += s_rec[cur][t - d];
        s_rec[cur ^ 1][t] = mine;
        cur ^= 1;
        __syncthreads();
    }
    if (!live) return;
    const bool last_here = t == VOX_TILE_ROWS - 1 || i + 1 >= n;
    const bool tail = last_here || s_voxel[t + 1] != v;
    if (!tail) return;
    rec = s_rec[cur][t];
    const int count = (int)(rec >> 48);
    const bool began_before = t - count + 1 == 0 && i0 > 0 && rank[i0 - 1] - 1 == v;
    const bool goes_on = last_here && i + 1 < n && rank[i + 1] - 1 == v;
    unsigned long long* a = acc + 4 * (int64_t)v;
    const unsigned long long c = (unsigned long long)count, r = (rec >> 32) & 0xFFFF, g = (rec >> 16) & 0xFFFF, b = rec & 0xFFFF;
    if (!began_before && !goes_on) {
        a[0] = c; a[1] = r; a[2] = g; a[3] = b;
    } else {
        atomicAdd(a, c);
        if (colours) { atomicAdd(a + 1, r); atomicAdd(a + 2, g); atomicAdd(a + 3, b); }
    }
}

// counts, and merge = 'mean': floor((2 sum + count) / (2 count)) per channel, which rounds a half up
__global__ void __launch_bounds__(VOX_BLOCK) k_vox_finish(const unsigned long long* __restrict__ acc, int64_t m, int mean,
                                                          int32_t* __restrict__ counts, uint8_t* __restrict__ colours_out) {
    const int64_t v = (int64_t)blockIdx.x * VOX_BLOCK + threadIdx.x;
    if (v >= m) return;
    const unsigned long long c = acc[4 * v];
    counts[v] = (int32_t)c;
    if (mean) {
        for (int k = 0; k < 3; ++k) colours_out[3 * v + k] = (uint8_t)((2 * acc[4 * v + 1 + k] + c) / (2 * c));
    }
}

extern "C" int64_t pcgc_voxelize_merge_workspace_bytes(int64_t m) {
    if (m < 1) m = 1;
    return (int64_t)align256((size_t)m * 4 * sizeof(unsigned long long));
}

extern "C" int pcgc_voxelize_merge(const uint64_t* sorted_keys, const int32_t* sorted_rows, const int32_t* rank, int64_t n, int64_t m,
                                   const uint8_t* colours, int merge_first, int32_t* coords, int32_t* counts, int32_t* voxel_of,
                                   uint8_t* colours_out, void* workspace, size_t workspace_bytes, void* stream) {
    PCGC_REQUIRE(n >= 1 && n <= VOX_MAX_ROWS, "1 .. 2^31 - 1 rows");
    PCGC_REQUIRE(m >= 1 && m <= n, "1 .. n voxels");
    PCGC_REQUIRE(sorted_keys && sorted_rows && rank && coords && counts && voxel_of && workspace, "null argument");
    PCGC_REQUIRE((colours == nullptr) == (colours_out == nullptr), "colours and colours_out go together");
    PCGC_REQUIRE(merge_first == 0 || merge_first == 1, "merge_first is 0 (mean) or 1 (first)");
    PCGC_REQUIRE(workspace_bytes >= (size_t)pcgc_voxelize_merge_workspace_bytes(m), "workspace too small");
    unsigned long long* acc = (unsigned long long*)workspace;
    if (hipMemsetAsync(acc, 0, (size_t)m * 4 * sizeof(unsigned long long), S(stream)) != hipSuccess) {
        pcgc_set_error("voxelize_merge: memset failed"); return -1;
    }
    hipLaunchKernelGGL(k_vox_merge, dim3(grid_for(n, VOX_TILE_ROWS)), dim3(VOX_TILE_ROWS), 0, S(stream), sorted_keys, sorted_rows, rank, n, colours,
                       merge_first, coords, voxel_of, colours_out, acc);
    PCGC_CHECK_LAUNCH("voxelize_merge");
    hipLaunchKernelGGL(k_vox_finish, dim3(grid_for(m, VOX_BLOCK)), dim3(VOX_BLOCK), 0, S(stream), (const unsigned long long*)acc, m,
                       (colours != nullptr && !merge_first) ? 1 : 0, counts, colours_out);
    PCGC_CHECK_LAUNCH("voxelize_merge");
    return 0;
}
