// Training clouds from triangle meshes (the reference's generate_dataset.py:7-36, which calls open3d on the CPU): uniform samples on the
// surface, a rotation, normalisation of ALL coordinates by one scalar minimum and one scalar maximum, rounding to a (resolution+1)^3 grid
// and de-duplication.  open3d draws its samples from std::mt19937 through library distributions, which cannot be restated; this unit
// defines its own arithmetic exactly (tests/mesh_reference.py is the numpy restatement, DESIGN.md 8c the text):
//
//   sample i of seed s:  w = Philox4x32-10(counter (i lo, i hi, 0, 0), key (s lo, s hi))
//     u0 = ((w0 << 20) | (w1 >> 12)) * 2^-52 in [0,1);  u = (w2 + 0.5) * 2^-32,  v = (w3 + 0.5) * 2^-32 in (0,1)      (all exact in fp64)
//     t  = min(#{ j : cdf[j] <= u0 * cdf[T-1] }, T-1)                (cdf = inclusive sum of the triangle areas: never a zero-area one)
//     if u + v > 1: u, v = 1 - u, 1 - v;   p = (A + u (B - A)) + v (C - A)
//   q = p . R;  mn = min q, mx = max (q - mn) over all 3 n values;  voxel = rint(((q - mn) / mx) * resolution)   (half-even, two roundings)
//
// A sample is a pure function of (seed, i), so nothing is stored between the passes of pcgc_mesh_voxelize: the min/max pass and the
// occupancy pass each recompute it (about a hundred integer and fp64 operations).  The distinct voxels come out of an occupancy bitmap
// of (resolution+1)^3 bits in bit order = (z, y, x) order: already de-duplicated and sorted, without a hash table or a sort.
// Built like every unit with -ffp-contract=off and no fast-math: the equality tests rest on IEEE fp64 add, multiply and divide.  No
// floating-point atomics anywhere (min / max are order-independent, the area sum has a fixed order), so results are bitwise reproducible.
#include "pcgc_common.h"

namespace {

constexpr int CDF_CHUNK = 16;                    // consecutive triangles summed by one lane
constexpr int CDF_TILE = 64 * CDF_CHUNK;         // triangles per block (one wave)
constexpr int MM_BLOCK = 256, MM_MAX_BLOCKS = 1024;
constexpr int BM_BLOCK = 256, BM_WORDS = 16;     // bitmap words per thread in the count / emit passes
constexpr int BM_TILE = BM_BLOCK * BM_WORDS;

struct Rot { double m[9]; };

struct Philox4 { uint32_t w0, w1, w2, w3; };

__host__ __device__ inline Philox4 philox4x32_10(uint64_t ctr, uint64_t key) {
    uint32_t c0 = (uint32_t)ctr, c1 = (uint32_t)(ctr >> 32), c2 = 0, c3 = 0, k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return {c0, c1, c2, c3};
}

// 0.5 |(B-A) x (C-A)| with every product and sum rounded on its own; a face with an index outside [0, V) counts as area 0 (and in *bad)
__device__ inline double tri_area(const double* __restrict__ verts, int64_t V, const int32_t* __restrict__ f, int& bad) {
    const uint32_t a = (uint32_t)f[0], b = (uint32_t)f[1], c = (uint32_t)f[2];
    if (a >= (uint64_t)V || b >= (uint64_t)V || c >= (uint64_t)V) { ++bad; return 0.0; }
    const double ax = verts[3 * (int64_t)a], ay = verts[3 * (int64_t)a + 1], az = verts[3 * (int64_t)a + 2];
    const double e1x = verts[3 * (int64_t)b] - ax, e1y = verts[3 * (int64_t)b + 1] - ay, e1z = verts[3 * (int64_t)b + 2] - az;
    const double e2x = verts[3 * (int64_t)c] - ax, e2y = verts[3 * (int64_t)c + 1] - ay, e2z = verts[3 * (int64_t)c + 2] - az;
    const double cx = e1y * e2z - e1z * e2y, cy = e1z * e2x - e1x * e2z, cz = e1x * e2y - e1y * e2x;
    return 0.5 * sqrt((cx * cx + cy * cy) + cz * cz);
}

// One wave per tile of CDF_TILE triangles.  Lane l sums its CDF_CHUNK consecutive areas left to right, lane 0 sums the 64 chunk totals
// left to right, and every value becomes (sum of the chunks before) + (running sum inside the chunk).  The last value of a chunk IS the
// next chunk's offset and fp addition is monotone in each operand, so the values never decrease, whatever the rounding — a tree scan
// gives no such guarantee, and sampling needs it (a zero-area triangle must repeat its predecessor's value exactly).
__global__ __launch_bounds__(64) void k_mesh_area_tile(const double* __restrict__ verts, int64_t V, const int32_t* __restrict__ faces,
                                                      int64_t T, double* __restrict__ cdf, double* __restrict__ tile_sum,
                                                      int32_t* __restrict__ bad_faces) {
    __shared__ double chunk[64];
    const int lane = threadIdx.x;
    const int64_t t0 = (int64_t)blockIdx.x * CDF_TILE + (int64_t)lane * CDF_CHUNK;
    double run[CDF_CHUNK];
    double s = 0.0;
    int bad = 0;
#pragma unroll
    for (int k = 0; k < CDF_CHUNK; ++k) {
        if (t0 + k < T) s = s + tri_area(verts, V, faces + 3 * (t0 + k), bad);
        run[k] = s;
    }
    chunk[lane] = s;
    __syncthreads();
    if (lane == 0) {
        double acc = 0.0;
        for (int l = 0; l < 64; ++l) { const double c = chunk[l]; chunk[l] = acc; acc = acc + c; }
        tile_sum[blockIdx.x] = acc;
    }
    __syncthreads();
    const double off = chunk[lane];
#pragma unroll
    for (int k = 0; k < CDF_CHUNK; ++k)
        if (t0 + k < T) cdf[t0 + k] = off + run[k];
    if (bad) atomicAdd(bad_faces, bad);
}

// exclusive sums of the tile totals, left to right (T / 1024 dependent adds: 80 for a mesh of 80 k triangles)
__global__ void k_mesh_tile_offsets(double* __restrict__ tile_sum, int64_t tiles) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double acc = 0.0;
    for (int64_t b = 0; b < tiles; ++b) { const double c = tile_sum[b]; tile_sum[b] = acc; acc = acc + c; }
}

__global__ void k_mesh_add_offsets(double* __restrict__ cdf, int64_t T, const double* __restrict__ tile_off) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < T) cdf[i] = tile_off[i / CDF_TILE] + cdf[i];
}

// #{ j : cdf[j] <= x }, at most T-1
__device__ inline int64_t cdf_pick(const double* __restrict__ cdf, int64_t T, double x) {
    int64_t lo = 0, hi = T;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (cdf[mid] <= x) lo = mid + 1; else hi = mid;
    }
    return lo < T - 1 ? lo : T - 1;
}

// sample i -> triangle and point; false (and NaNs) if the chosen face names a vertex outside [0, V)
__device__ inline bool mesh_sample_one(const double* __restrict__ verts, int64_t V, const int32_t* __restrict__ faces,
                                       const double* __restrict__ cdf, int64_t T, double total, uint64_t seed, uint64_t i, int64_t& t,
                                       double& px, double& py, double& pz) {
    const Philox4 w = philox4x32_10(i, seed);
    const double u0 = (double)(((uint64_t)w.w0 << 20) | (uint64_t)(w.w1 >> 12)) * 0x1p-52;
    double u = ((double)w.w2 + 0.5) * 0x1p-32, v = ((double)w.w3 + 0.5) * 0x1p-32;
    t = cdf_pick(cdf, T, u0 * total);
    if (u + v > 1.0) { u = 1.0 - u; v = 1.0 - v; }
    const uint32_t a = (uint32_t)faces[3 * t], b = (uint32_t)faces[3 * t + 1], c = (uint32_t)faces[3 * t + 2];
    if (a >= (uint64_t)V || b >= (uint64_t)V || c >= (uint64_t)V) { px = py = pz = __builtin_nan(""); return false; }
    const double* A = verts + 3 * (int64_t)a; const double* B = verts + 3 * (int64_t)b; const double* C = verts + 3 * (int64_t)c;
    px = (A[0] + u * (B[0] - A[0])) + v * (C[0] - A[0]);
    py = (A[1] + u * (B[1] - A[1])) + v * (C[1] - A[1]);
    pz = (A[2] + u * (B[2] - A[2])) + v * (C[2] - A[2]);
    return true;
}

__global__ void k_mesh_sample(const double* __restrict__ verts, int64_t V, const int32_t* __restrict__ faces,
                              const double* __restrict__ cdf, int64_t T, uint64_t seed, uint64_t first, int64_t n,
                              int32_t* __restrict__ tri, double* __restrict__ points) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    int64_t t; double x, y, z;
    mesh_sample_one(verts, V, faces, cdf, T, cdf[T - 1], seed, first + (uint64_t)g, t, x, y, z);
    if (tri) tri[g] = (int32_t)t;
    if (points) { points[3 * g] = x; points[3 * g + 1] = y; points[3 * g + 2] = z; }
}

__device__ inline void rotate(const Rot& R, double px, double py, double pz, double q[3]) {
#pragma unroll
    for (int j = 0; j < 3; ++j) q[j] = (px * R.m[j] + py * R.m[3 + j]) + pz * R.m[6 + j];
}

// min / max over a block; the result is valid in thread 0.  NaNs drop out of fmin / fmax; a cloud of NaNs only fails the status check.
__device__ inline void block_minmax(double& lo, double& hi) {
    __shared__ double slo[MM_BLOCK / 64], shi[MM_BLOCK / 64];
    for (int o = 32; o > 0; o >>= 1) { lo = fmin(lo, __shfl_down(lo, o)); hi = fmax(hi, __shfl_down(hi, o)); }
    if ((threadIdx.x & 63) == 0) { slo[threadIdx.x >> 6] = lo; shi[threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < (int)(blockDim.x >> 6); ++w) { lo = fmin(lo, slo[w]); hi = fmax(hi, shi[w]); }
}

// pass 1: min and max of every rotated coordinate, one pair per block
__global__ __launch_bounds__(MM_BLOCK) void k_mesh_minmax(const double* __restrict__ verts, int64_t V, const int32_t* __restrict__ faces,
                                                          const double* __restrict__ cdf, int64_t T, uint64_t seed, int64_t n, Rot R,
                                                          double* __restrict__ partial /*[2 gridDim]*/) {
    const double total = cdf[T - 1];
    double lo = __builtin_inf(), hi = -__builtin_inf();
    for (int64_t g = (int64_t)blockIdx.x * MM_BLOCK + threadIdx.x; g < n; g += (int64_t)gridDim.x * MM_BLOCK) {
        int64_t t; double x, y, z, q[3];
        if (!mesh_sample_one(verts, V, faces, cdf, T, total, seed, (uint64_t)g, t, x, y, z)) continue;
        rotate(R, x, y, z, q);
        lo = fmin(lo, fmin(q[0], fmin(q[1], q[2])));
        hi = fmax(hi, fmax(q[0], fmax(q[1], q[2])));
    }
    block_minmax(lo, hi);
    if (threadIdx.x == 0) { partial[2 * blockIdx.x] = lo; partial[2 * blockIdx.x + 1] = hi; }
}

// norm[0] = mn, norm[1] = mx = fl(max q - mn) (subtraction is monotone, so this is the maximum of q - mn), norm[2] = status as a double:
// 0 ok, 1 = the total area is not a positive finite number, 2 = mx is not (mx == 0: every sample fell on one value)
__global__ __launch_bounds__(MM_BLOCK) void k_mesh_minmax_final(const double* __restrict__ partial, int blocks, const double* __restrict__ cdf,
                                                                int64_t T, double* __restrict__ norm, int32_t* __restrict__ count) {
    double lo = __builtin_inf(), hi = -__builtin_inf();
    for (int b = threadIdx.x; b < blocks; b += MM_BLOCK) { lo = fmin(lo, partial[2 * b]); hi = fmax(hi, partial[2 * b + 1]); }
    block_minmax(lo, hi);
    if (threadIdx.x == 0) {
        const double total = cdf[T - 1], mx = hi - lo;
        int status = 0;
        if (!(total > 0.0) || total == __builtin_inf()) status = 1;
        else if (!(mx > 0.0) || mx == __builtin_inf()) status = 2;
        norm[0] = lo; norm[1] = mx; norm[2] = (double)status;
        if (status) *count = -status;
    }
}

// pass 2: one bit per occupied voxel, bit (z (res+1) + y)(res+1) + x.  Most samples find their bit already set (4e5 samples on ~1e5 voxels
// at resolution 255; ALL but 8 at resolution 1), so the word is read first and the atomic only issued for a bit still missing.
__global__ __launch_bounds__(256) void k_mesh_occupancy(const double* __restrict__ verts, int64_t V, const int32_t* __restrict__ faces,
                                                        const double* __restrict__ cdf, int64_t T, uint64_t seed, int64_t n, Rot R,
                                                        int32_t res, const double* __restrict__ norm, uint32_t* __restrict__ bitmap) {
    if (norm[2] != 0.0) return;
    const double total = cdf[T - 1], mn = norm[0], mx = norm[1], fres = (double)res;
    const int64_t side = (int64_t)res + 1;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (int64_t)gridDim.x * blockDim.x) {
        int64_t t; double x, y, z, q[3];
        if (!mesh_sample_one(verts, V, faces, cdf, T, total, seed, (uint64_t)g, t, x, y, z)) continue;
        rotate(R, x, y, z, q);
        const double vx = rint(((q[0] - mn) / mx) * fres), vy = rint(((q[1] - mn) / mx) * fres), vz = rint(((q[2] - mn) / mx) * fres);
        if (!(vx >= 0.0 && vx <= fres && vy >= 0.0 && vy <= fres && vz >= 0.0 && vz <= fres)) continue;      // (NaN / inf vertices)
        const int64_t bit = ((int64_t)vz * side + (int64_t)vy) * side + (int64_t)vx;
        const uint32_t m = 1u << (bit & 31);
        uint32_t* w = bitmap + (bit >> 5);
        if (!(*w & m)) atomicOr(w, m);                                // (a stale read only costs a redundant atomic)
    }
}

__device__ inline int load_words(const uint32_t* __restrict__ bitmap, int64_t words, int64_t w0, uint32_t v[BM_WORDS]) {
    int c = 0;
    if (w0 + BM_WORDS <= words) {                                     // (the bitmap is 64-byte aligned and w0 a multiple of 16)
        const uint4* p = (const uint4*)(bitmap + w0);
#pragma unroll
        for (int k = 0; k < BM_WORDS / 4; ++k) { const uint4 a = p[k]; v[4 * k] = a.x; v[4 * k + 1] = a.y; v[4 * k + 2] = a.z; v[4 * k + 3] = a.w; }
    } else {
#pragma unroll
        for (int k = 0; k < BM_WORDS; ++k) v[k] = w0 + k < words ? bitmap[w0 + k] : 0u;
    }
#pragma unroll
    for (int k = 0; k < BM_WORDS; ++k) c += __popc(v[k]);
    return c;
}

// exclusive sum of `c` over the block's threads in thread order; *block_total = the sum
__device__ inline int block_exclusive(int c, int* block_total) {
    __shared__ int wsum[BM_BLOCK / 64 + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = c;
    for (int o = 1; o < 64; o <<= 1) { const int up = __shfl_up(inc, o); if (lane >= o) inc += up; }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    if (threadIdx.x == 0) {
        int acc = 0;
        for (int w = 0; w < BM_BLOCK / 64; ++w) { const int s = wsum[w]; wsum[w] = acc; acc += s; }
        wsum[BM_BLOCK / 64] = acc;
    }
    __syncthreads();
    *block_total = wsum[BM_BLOCK / 64];
    return wsum[wave] + inc - c;
}

// pass 3a: set bits per tile of BM_TILE words
__global__ __launch_bounds__(BM_BLOCK) void k_mesh_tile_count(const uint32_t* __restrict__ bitmap, int64_t words, int32_t* __restrict__ tile_count) {
    uint32_t v[BM_WORDS];
    const int c = load_words(bitmap, words, ((int64_t)blockIdx.x * BM_BLOCK + threadIdx.x) * BM_WORDS, v);
    int total;
    block_exclusive(c, &total);
    if (threadIdx.x == 0) tile_count[blockIdx.x] = total;
}

// pass 3b: exclusive sums of the tile counts in place (one block walks them BM_BLOCK at a time) and the number of voxels
__global__ __launch_bounds__(BM_BLOCK) void k_mesh_tile_scan(int32_t* __restrict__ tile_count, int64_t tiles, const double* __restrict__ norm,
                                                             int32_t* __restrict__ count) {
    if (norm[2] != 0.0) return;                                       // (count already holds the error)
    int carry = 0;
    for (int64_t b0 = 0; b0 < tiles; b0 += BM_BLOCK) {
        const int64_t b = b0 + threadIdx.x;
        const int c = b < tiles ? tile_count[b] : 0;
        int total;
        const int ex = block_exclusive(c, &total);
        if (b < tiles) tile_count[b] = carry + ex;
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) *count = carry;
}

// pass 4: rows (0, x, y, z) of the set bits in bit order
__global__ __launch_bounds__(BM_BLOCK) void k_mesh_emit(const uint32_t* __restrict__ bitmap, int64_t words, const int32_t* __restrict__ tile_off,
                                                        const double* __restrict__ norm, int32_t res, int4* __restrict__ out, int64_t cap) {
    if (norm[2] != 0.0) return;
    uint32_t v[BM_WORDS];
    const int64_t w0 = ((int64_t)blockIdx.x * BM_BLOCK + threadIdx.x) * BM_WORDS;
    const int c = load_words(bitmap, words, w0, v);
    int total;
    int64_t row = (int64_t)tile_off[blockIdx.x] + block_exclusive(c, &total);
    if (c == 0) return;
    const int64_t side = (int64_t)res + 1;
#pragma unroll
    for (int k = 0; k < BM_WORDS; ++k) {
        uint32_t m = v[k];
        while (m) {
            const int64_t bit = ((w0 + k) << 5) + (__ffs((int)m) - 1);
            m &= m - 1;
            const int64_t zy = bit / side;
            if (row < cap) out[row] = make_int4(0, (int)(bit - zy * side), (int)(zy % side), (int)(zy / side));
            ++row;
        }
    }
}

inline int64_t cdf_tiles(int64_t T) { return (T + CDF_TILE - 1) / CDF_TILE; }
inline int64_t bitmap_words(int32_t res) { const int64_t s = (int64_t)res + 1; return (s * s * s + 31) / 32; }
inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
inline int minmax_blocks(int64_t n) { const int64_t b = (n + MM_BLOCK - 1) / MM_BLOCK; return (int)(b < MM_MAX_BLOCKS ? b : MM_MAX_BLOCKS); }

struct VoxWs { size_t norm, partial, bitmap, tiles, total; int64_t words, ntiles; };
inline VoxWs vox_layout(int32_t res) {
    VoxWs w;
    w.words = bitmap_words(res); w.ntiles = (w.words + BM_TILE - 1) / BM_TILE;
    w.norm = 0;
    w.partial = align256(4 * sizeof(double));
    w.bitmap = w.partial + align256((size_t)2 * MM_MAX_BLOCKS * sizeof(double));
    w.tiles = w.bitmap + align256((size_t)w.words * 4);
    w.total = w.tiles + align256((size_t)w.ntiles * 4);
    return w;
}

}  // namespace

extern "C" size_t pcgc_mesh_cdf_workspace_bytes(int64_t T) { return T > 0 ? align256((size_t)cdf_tiles(T) * sizeof(double)) : 0; }

extern "C" int pcgc_mesh_area_cdf(const double* verts, int64_t V, const int32_t* faces, int64_t T, double* cdf, int32_t* bad_faces,
                                  void* ws, size_t ws_bytes, void* stream) {
    PCGC_REQUIRE(verts && faces && cdf && bad_faces && ws, "null pointer");
    PCGC_REQUIRE(V > 0 && V <= 0x7FFFFFFFll, "the vertex count must be in 1 .. 2^31-1");
    PCGC_REQUIRE(T > 0 && T <= 0x7FFFFFFFll, "the triangle count must be in 1 .. 2^31-1");
    PCGC_REQUIRE(ws_bytes >= pcgc_mesh_cdf_workspace_bytes(T), "workspace too small");
    const int64_t tiles = cdf_tiles(T);
    if (hipMemsetAsync(bad_faces, 0, sizeof(int32_t), S(stream)) != hipSuccess) { pcgc_set_error("mesh_area_cdf: memset failed"); return -1; }
    k_mesh_area_tile<<<(unsigned)tiles, 64, 0, S(stream)>>>(verts, V, faces, T, cdf, (double*)ws, bad_faces);
    PCGC_CHECK_LAUNCH("mesh_area_tile");
    if (tiles > 1) {
        k_mesh_tile_offsets<<<1, 64, 0, S(stream)>>>((double*)ws, tiles);
        PCGC_CHECK_LAUNCH("mesh_tile_offsets");
        k_mesh_add_offsets<<<grid_for(T, 256), 256, 0, S(stream)>>>(cdf, T, (const double*)ws);
        PCGC_CHECK_LAUNCH("mesh_add_offsets");
    }
    return 0;
}

extern "C" int pcgc_mesh_sample(const double* verts, int64_t V, const int32_t* faces, const double* cdf, int64_t T, uint64_t seed,
                                uint64_t first, int64_t n, int32_t* tri, double* points, void* stream) {
    PCGC_REQUIRE(verts && faces && cdf, "null pointer");
    PCGC_REQUIRE(V > 0 && V <= 0x7FFFFFFFll && T > 0 && T <= 0x7FFFFFFFll, "vertex and triangle counts must be in 1 .. 2^31-1");
    PCGC_REQUIRE(n > 0 && n <= 0x7FFFFFFFll, "the number of samples must be in 1 .. 2^31-1");
    PCGC_REQUIRE(tri || points, "neither tri nor points requested");
    k_mesh_sample<<<grid_for(n, 256), 256, 0, S(stream)>>>(verts, V, faces, cdf, T, seed, first, n, tri, points);
    PCGC_CHECK_LAUNCH("mesh_sample");
    return 0;
}

extern "C" size_t pcgc_mesh_voxelize_workspace_bytes(int32_t resolution) {
    return resolution >= 1 && resolution <= 1023 ? vox_layout(resolution).total : 0;
}

extern "C" int pcgc_mesh_voxelize(const double* verts, int64_t V, const int32_t* faces, const double* cdf, int64_t T, uint64_t seed, int64_t n,
                                  const double* R, int32_t resolution, int32_t* out, int64_t cap, int32_t* count, void* ws, size_t ws_bytes,
                                  void* stream) {
    PCGC_REQUIRE(verts && faces && cdf && R && out && count && ws, "null pointer");
    PCGC_REQUIRE(V > 0 && V <= 0x7FFFFFFFll && T > 0 && T <= 0x7FFFFFFFll, "vertex and triangle counts must be in 1 .. 2^31-1");
    PCGC_REQUIRE(n > 0 && n <= 0x7FFFFFFFll, "the number of samples must be in 1 .. 2^31-1");
    PCGC_REQUIRE(resolution >= 1 && resolution <= 1023, "resolution must be in 1 .. 1023 (the occupancy bitmap holds (resolution+1)^3 bits)");
    PCGC_REQUIRE(cap >= 0, "negative capacity");
    const VoxWs w = vox_layout(resolution);
    PCGC_REQUIRE(ws_bytes >= w.total, "workspace too small");
    PCGC_REQUIRE(((uintptr_t)ws & 63) == 0, "workspace must be 64-byte aligned");
    char* base = (char*)ws;
    double* norm = (double*)(base + w.norm); double* partial = (double*)(base + w.partial);
    uint32_t* bitmap = (uint32_t*)(base + w.bitmap); int32_t* tiles = (int32_t*)(base + w.tiles);
    Rot rot;
    for (int k = 0; k < 9; ++k) rot.m[k] = R[k];
    hipStream_t s = S(stream);
    if (hipMemsetAsync(bitmap, 0, (size_t)w.words * 4, s) != hipSuccess || hipMemsetAsync(count, 0, sizeof(int32_t), s) != hipSuccess) {
        pcgc_set_error("mesh_voxelize: memset failed"); return -1;
    }
    const int mmb = minmax_blocks(n);
    k_mesh_minmax<<<mmb, MM_BLOCK, 0, s>>>(verts, V, faces, cdf, T, seed, n, rot, partial);
    PCGC_CHECK_LAUNCH("mesh_minmax");
    k_mesh_minmax_final<<<1, MM_BLOCK, 0, s>>>(partial, mmb, cdf, T, norm, count);
    PCGC_CHECK_LAUNCH("mesh_minmax_final");
    k_mesh_occupancy<<<grid_for(n, 256), 256, 0, s>>>(verts, V, faces, cdf, T, seed, n, rot, resolution, norm, bitmap);
    PCGC_CHECK_LAUNCH("mesh_occupancy");
    k_mesh_tile_count<<<(unsigned)w.ntiles, BM_BLOCK, 0, s>>>(bitmap, w.words, tiles);
    PCGC_CHECK_LAUNCH("mesh_tile_count");
    k_mesh_tile_scan<<<1, BM_BLOCK, 0, s>>>(tiles, w.ntiles, norm, count);
    PCGC_CHECK_LAUNCH("mesh_tile_scan");
    k_mesh_emit<<<(unsigned)w.ntiles, BM_BLOCK, 0, s>>>(bitmap, w.words, tiles, norm, resolution, (int4*)out, cap);
    PCGC_CHECK_LAUNCH("mesh_emit");
    return 0;
}
