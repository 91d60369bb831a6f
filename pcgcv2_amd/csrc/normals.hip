// Surface normals of a voxelised cloud, estimated on device from fixed-radius neighbourhoods ("Estimated normals").  The reference
// has no estimator: its D2 figures (test.py:74-75) assume clouds whose normals were estimated offline in another tool.
//
// Definition.  For a row at voxel p, the neighbourhood is every DISTINCT voxel q of the same batch with |q - p|^2 <= r2 (p included,
// duplicated rows count once).  With d = q - p the ten moments k, sum d, sum d d^T are exact integers; S = k sum(d d^T) - (sum d)(sum d)^T
// is k^2 times the covariance, exact too.  valid = (k >= 3 and rank S >= 2), the rank read off the integers; the normal is the unit
// eigenvector of the smallest eigenvalue of S (fp64 cyclic Jacobi), oriented by the caller's rule; invalid rows get (0, 0, 0).
//
// Bounds (r2 <= 64): a neighbourhood holds at most K = 2109 lattice points (those with |d|^2 <= 64) and sum |d|^2 <= 64 K, so every
// entry of S is below K * 64 K < 2.9e8 < 2^29, a 2 x 2 minor (a difference of two products of entries) below 2^58 and the sum of the three
// principal minors below 2^60: all of it fits int64, and every entry of S is exact in fp64.
//
// Pass A (moments) reads the searched cloud through the D2 index (metric.hip): one wave per occupied 4 x 4 x 4 cell, lane = voxel position
// in the cell (the bit numbering of the occupancy masks).  The wave probes the (2 C + 1)^3 surrounding cells once (C = ceil(floor(sqrt r2) / 4):
// 27 cells for r2 < 25, 125 up to 64), each lane ANDs a present cell's occupancy with its "ball" mask for (cell offset, lane), and the
// moments come from popcounts against constant bit-plane masks (x = x0 + 2 x1, x^2 = x0 + 4 x1 + 4 x0 x1, x y = sum of bit-plane products):
// no loop over neighbours.  The ball table ((2 C + 1)^3 x 64 masks: 13.5 KiB or 62.5 KiB) stays in global memory: every wave reads the
// same few KiB, which the caches hold, while staging 62.5 KiB into the 160 KiB LDS of a CU would leave room for two workgroups only.
// Pass B (one thread per ORIGINAL row) turns the moments into eigenvalues, validity and the oriented normal with all lanes busy.
// Everything is a function of the voxel set: integer moments, a fixed-order solve per row, integer atomics only (the per-batch centroid sums).
#include <cmath>
#include "pcgc_common.h"

#define NRM_MAX_R2 64
#define NRM_ORIENT_NONE 0
#define NRM_ORIENT_CENTROID 1
#define NRM_ORIENT_VIEWPOINT 2

// cells a neighbourhood reaches along one axis: a voxel at local position 0 .. 3 and an offset of up to floor(sqrt r2) voxels
static inline int nrm_isqrt(int r2) { int r = 0; while ((r + 1) * (r + 1) <= r2) ++r; return r; }
static inline int nrm_reach_cells(int r2) { return (nrm_isqrt(r2) + 3) / 4; }

extern "C" int64_t pcgc_normals_ball_masks(int32_t r2, uint64_t* table) {
    if (r2 < 1 || r2 > NRM_MAX_R2) { pcgc_set_error("pcgc_normals_ball_masks: r2 = %d outside 1 .. %d", (int)r2, NRM_MAX_R2); return -2; }
    const int C = nrm_reach_cells(r2), side = 2 * C + 1;
    const int64_t n = (int64_t)side * side * side * 64;
    if (!table) return n;
    for (int t = 0; t < side * side * side; ++t) {
        const int ox = 4 * (t % side - C), oy = 4 * ((t / side) % side - C), oz = 4 * (t / (side * side) - C);
        for (int lane = 0; lane < 64; ++lane) {
            uint64_t m = 0;
            for (int bit = 0; bit < 64; ++bit) {
                const int dx = ox + (bit & 3) - (lane & 3), dy = oy + ((bit >> 2) & 3) - ((lane >> 2) & 3), dz = oz + (bit >> 4) - (lane >> 4);
                if (dx * dx + dy * dy + dz * dz <= r2) m |= 1ull << bit;
            }
            table[(int64_t)t * 64 + lane] = m;
        }
    }
    return n;
}

struct NrmIndex {                      // the D2 index of the cloud (sorted rows), as metric.hip reads it
    const int4* qs; const int32_t* perm; const int32_t* runlen;
    const uint64_t* ckeys; const int32_t* cvals; uint64_t cmask; const unsigned long long* masks;
    const uint64_t* vkeys; const int32_t* vvals; uint64_t vmask;
};

// bit planes of the voxel position inside a cell (bit = x | y << 2 | z << 4)
#define NRM_X0 0xAAAAAAAAAAAAAAAAull
#define NRM_X1 0xCCCCCCCCCCCCCCCCull
#define NRM_Y0 0xF0F0F0F0F0F0F0F0ull
#define NRM_Y1 0xFF00FF00FF00FF00ull
#define NRM_Z0 0xFFFF0000FFFF0000ull
#define NRM_Z1 0xFFFFFFFF00000000ull

// moments of u = (voxel position relative to the origin of the query's own cell); int32 holds them: |u| <= 11 and k <= 2109
struct NrmSums { int k, x, y, z, xx, yy, zz, xy, xz, yz; };

__host__ __device__ static inline int pc(unsigned long long m) { return __builtin_popcountll(m); }

// adds the voxels `nb` of the cell whose origin is (ux, uy, uz) voxels from the query's cell origin
__host__ __device__ static inline void nrm_add_cell(NrmSums& s, unsigned long long nb, int ux, int uy, int uz) {
    const int k = pc(nb);
    const unsigned long long x0 = nb & NRM_X0, x1 = nb & NRM_X1, y0 = nb & NRM_Y0, y1 = nb & NRM_Y1, z0 = nb & NRM_Z0, z1 = nb & NRM_Z1;
    const int bx = pc(x0) + 2 * pc(x1), by = pc(y0) + 2 * pc(y1), bz = pc(z0) + 2 * pc(z1);
    const int bxx = pc(x0) + 4 * pc(x1) + 4 * pc(x0 & x1), byy = pc(y0) + 4 * pc(y1) + 4 * pc(y0 & y1), bzz = pc(z0) + 4 * pc(z1) + 4 * pc(z0 & z1);
    const int bxy = pc(x0 & y0) + 2 * pc(x0 & y1) + 2 * pc(x1 & y0) + 4 * pc(x1 & y1);
    const int bxz = pc(x0 & z0) + 2 * pc(x0 & z1) + 2 * pc(x1 & z0) + 4 * pc(x1 & z1);
    const int byz = pc(y0 & z0) + 2 * pc(y0 & z1) + 2 * pc(y1 & z0) + 4 * pc(y1 & z1);
    s.k += k;
    s.x += k * ux + bx; s.y += k * uy + by; s.z += k * uz + bz;
    s.xx += k * ux * ux + 2 * ux * bx + bxx; s.yy += k * uy * uy + 2 * uy * by + byy; s.zz += k * uz * uz + 2 * uz * bz + bzz;
    s.xy += k * ux * uy + ux * by + uy * bx + bxy;
    s.xz += k * ux * uz + ux * bz + uz * bx + bxz;
    s.yz += k * uy * uz + uy * bz + uz * by + byz;
}

// the sums about the cell origin, moved to d = u - l ...
__host__ __device__ static inline void nrm_shift(const NrmSums& s, int lx, int ly, int lz, int64_t* m) {
    m[0] = s.k;
    m[1] = s.x - s.k * lx; m[2] = s.y - s.k * ly; m[3] = s.z - s.k * lz;
    m[4] = s.xx - 2 * lx * s.x + s.k * lx * lx; m[5] = s.yy - 2 * ly * s.y + s.k * ly * ly; m[6] = s.zz - 2 * lz * s.z + s.k * lz * lz;
    m[7] = s.xy - lx * s.y - ly * s.x + s.k * lx * ly;
    m[8] = s.xz - lx * s.z - lz * s.x + s.k * lx * lz;
    m[9] = s.yz - ly * s.z - lz * s.y + s.k * ly * lz;
}
// ... and written to the rows of the voxel's run (every duplicate row receives its voxel's moments)
__device__ static inline void nrm_store(const NrmSums& s, int lx, int ly, int lz, const NrmIndex& q, int32_t run_start,
                                        int64_t* __restrict__ moments) {
    int64_t m[10];
    nrm_shift(s, lx, ly, lz, m);
    const int r = q.runlen[run_start];
    for (int j = 0; j < r; ++j) {
        int64_t* out = moments + (int64_t)q.perm[run_start + j] * 10;
#pragma unroll
        for (int t = 0; t < 10; ++t) out[t] = m[t];
    }
}

// the sorted rows that own a cell's mask (pcgc_d1_cell_masks leaves every other slot of `masks` zero), in any order
__global__ void __launch_bounds__(256) k_nrm_cell_list(const unsigned long long* __restrict__ masks, int64_t n, int32_t* __restrict__ cells,
                                                       int32_t* __restrict__ n_cells) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool own = i < n && masks[i] != 0;
    const unsigned long long b = __ballot(own);
    if (b == 0) return;
    const int lane = threadIdx.x & 63;
    int base = 0;
    if (lane == 0) base = atomicAdd(n_cells, pc(b));
    base = __shfl(base, 0);
    if (own) cells[base + pc(b & ((1ull << lane) - 1))] = (int32_t)i;
}

// pass A: one wave per occupied cell (a fixed grid of waves strides over the cell list, whose length stays on the device)
__global__ void __launch_bounds__(256) k_nrm_moments_cells(NrmIndex q, const int32_t* __restrict__ cells, const int32_t* __restrict__ n_cells,
                                                           const unsigned long long* __restrict__ ball, int C, int64_t* __restrict__ moments) {
    const int lane = threadIdx.x & 63;
    const int side = 2 * C + 1, n_off = side * side * side;           // 27 or 125: two probes per lane at the most
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6, nc = *n_cells;
    for (int64_t w = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; w < nc; w += n_waves) {      // (wave-uniform)
        const int32_t s0 = cells[w];
        const int4 c = q.qs[s0];
        const int X = c.y & ~3, Y = c.z & ~3, Z = c.w & ~3;
        const unsigned long long own = q.masks[s0];
        unsigned long long found[2] = {0, 0};
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int t = 64 * h + lane;
            if (t < n_off) {
                // (a cell at a negative or too large coordinate is out of the key's range: hash_lookup misses, nothing wraps)
                const int32_t row = hash_lookup(q.ckeys, q.cvals, q.cmask, c.x, X + 4 * (t % side - C), Y + 4 * ((t / side) % side - C),
                                                Z + 4 * (t / (side * side) - C));
                if (row >= 0) found[h] = q.masks[row];
            }
        }
        NrmSums s = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            unsigned long long present = __ballot(found[h] != 0);
            while (present) {                                         // (wave-uniform walk over the present cells)
                const int src = __ffsll((long long)present) - 1;
                present &= present - 1;
                const int t = 64 * h + src;
                const unsigned long long m = __shfl(found[h], src);
                const unsigned long long nb = m & ball[(int64_t)t * 64 + lane];
                nrm_add_cell(s, nb, 4 * (t % side - C), 4 * ((t / side) % side - C), 4 * (t / (side * side) - C));
            }
        }
        if (!((own >> lane) & 1)) continue;
        const int lx = lane & 3, ly = (lane >> 2) & 3, lz = lane >> 4;
        // (the cell masks and the voxel hash are built from the same rows: the voxel is always found)
        const int32_t run = hash_lookup(q.vkeys, q.vvals, q.vmask, c.x, X + lx, Y + ly, Z + lz);
        if (run >= 0) nrm_store(s, lx, ly, lz, q, run, moments);
    }
}

// pass A, the other mapping (pcgc_set_normals_mapping(1); DESIGN.md has both timings): one thread per distinct voxel, which probes the
// surrounding cells itself.  The same masks and sums, so the same moments.
__global__ void __launch_bounds__(256) k_nrm_moments_voxels(NrmIndex q, int64_t n, const unsigned long long* __restrict__ ball, int C,
                                                            int64_t* __restrict__ moments) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || q.runlen[i] == 0) return;
    const int4 c = q.qs[i];
    const int X = c.y & ~3, Y = c.z & ~3, Z = c.w & ~3;
    const int lx = c.y & 3, ly = c.z & 3, lz = c.w & 3, pos = lx | (ly << 2) | (lz << 4);
    NrmSums s = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    int t = 0;
    for (int oz = -C; oz <= C; ++oz)
        for (int oy = -C; oy <= C; ++oy)
            for (int ox = -C; ox <= C; ++ox, ++t) {
                const int32_t row = hash_lookup(q.ckeys, q.cvals, q.cmask, c.x, X + 4 * ox, Y + 4 * oy, Z + 4 * oz);
                if (row < 0) continue;
                const unsigned long long nb = q.masks[row] & ball[(int64_t)t * 64 + pos];
                if (nb) nrm_add_cell(s, nb, 4 * ox, 4 * oy, 4 * oz);
            }
    nrm_store(s, lx, ly, lz, q, (int32_t)i, moments);
}

// pass B: moments -> eigenvalues, validity, oriented normal; one thread per original row.
// One Jacobi rotation of the symmetric 3 x 3 matrix in the (p, q) plane; r is the third index, (vp, vq) the eigenvector columns.
__host__ __device__ static inline void nrm_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double* vp, double* vq) {
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));       // (theta^2 = inf gives t = 0)
    const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
    app -= t * apq; aqq += t * apq; apq = 0.0;
    const double rp = arp, rq = arq;
    arp = cs * rp - sn * rq; arq = sn * rp + cs * rq;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double a = vp[i], b = vq[i];
        vp[i] = cs * a - sn * b; vq[i] = sn * a + cs * b;
    }
}

#define NRM_SWEEPS 16      // cyclic Jacobi converges quadratically: a 3 x 3 matrix is diagonal to the last bit after 5 .. 7 sweeps

__host__ __device__ static inline void nrm_swap_cols(double& la, double& lb, double* va, double* vb) {
    if (lb < la) {
        const double t = la; la = lb; lb = t;
        for (int i = 0; i < 3; ++i) { const double u = va[i]; va[i] = vb[i]; vb[i] = u; }
    }
}

// one row: moments m [10], the row's coordinates c and the sums of its batch bs = (N_b, sum x, sum y, sum z) -> lam [3], normal [3], valid
__host__ __device__ static inline bool nrm_solve_row(const int64_t* m, int4 c, int orient, double vx, double vy, double vz, const long long* bs,
                                                     double* lam, double* nrm) {
    const int64_t k = m[0];
    // S = k sum(d d^T) - (sum d)(sum d)^T, exact (bounds at the head of this file)
    const int64_t sxx = k * m[4] - m[1] * m[1], syy = k * m[5] - m[2] * m[2], szz = k * m[6] - m[3] * m[3];
    const int64_t sxy = k * m[7] - m[1] * m[2], sxz = k * m[8] - m[1] * m[3], syz = k * m[9] - m[2] * m[3];
    // rank >= 2 <=> the second elementary symmetric function of the eigenvalues, the sum of the principal 2 x 2 minors, is non-zero
    const int64_t minors = (sxx * syy - sxy * sxy) + (sxx * szz - sxz * sxz) + (syy * szz - syz * syz);
    const bool ok = k >= 3 && minors != 0;
    double a00 = (double)sxx, a11 = (double)syy, a22 = (double)szz, a01 = (double)sxy, a02 = (double)sxz, a12 = (double)syz;
    double v0[3] = {1.0, 0.0, 0.0}, v1[3] = {0.0, 1.0, 0.0}, v2[3] = {0.0, 0.0, 1.0};      // columns
    for (int sweep = 0; sweep < NRM_SWEEPS; ++sweep) {
        if (a01 == 0.0 && a02 == 0.0 && a12 == 0.0) break;
        nrm_rotate(a00, a11, a01, a02, a12, v0, v1);                  // (p, q) = (0, 1), r = 2
        nrm_rotate(a00, a22, a02, a01, a12, v0, v2);                  // (0, 2), r = 1
        nrm_rotate(a11, a22, a12, a01, a02, v1, v2);                  // (1, 2), r = 0
    }
    nrm_swap_cols(a00, a11, v0, v1); nrm_swap_cols(a11, a22, v1, v2); nrm_swap_cols(a00, a11, v0, v1);     // ascending
    lam[0] = a00; lam[1] = a11; lam[2] = a22;
    double nx = 0.0, ny = 0.0, nz = 0.0;
    if (ok) {
        const double len = sqrt(v0[0] * v0[0] + v0[1] * v0[1] + v0[2] * v0[2]);
        nx = v0[0] / len; ny = v0[1] / len; nz = v0[2] / len;
        double dot = 0.0;
        if (orient == NRM_ORIENT_CENTROID)                            // away from the centroid: n . (N_b p - sum q), the vector exact
            dot = nx * (double)(bs[0] * c.y - bs[1]) + ny * (double)(bs[0] * c.z - bs[2]) + nz * (double)(bs[0] * c.w - bs[3]);
        else if (orient == NRM_ORIENT_VIEWPOINT)                      // towards the viewpoint
            dot = nx * (vx - (double)c.y) + ny * (vy - (double)c.z) + nz * (vz - (double)c.w);
        bool flip = dot < 0.0;
        if (dot == 0.0) {                                             // no rule, or an exact zero: the largest component is positive
            const double ax = fabs(nx), ay = fabs(ny), az = fabs(nz);
            const double big = (ax >= ay && ax >= az) ? nx : (ay >= az ? ny : nz);
            flip = big < 0.0;
        }
        if (flip) { nx = 0.0 - nx; ny = 0.0 - ny; nz = 0.0 - nz; }     // (0.0 - x: no negative zeros)
    }
    nrm[0] = nx; nrm[1] = ny; nrm[2] = nz;
    return ok;
}

__global__ void __launch_bounds__(256) k_nrm_solve(const int4* __restrict__ coords, int64_t n, const int64_t* __restrict__ moments,
                                                   int orient, double vx, double vy, double vz, const long long* __restrict__ batch_sums,
                                                   double* __restrict__ normals, double* __restrict__ lam, int32_t* __restrict__ count,
                                                   uint8_t* __restrict__ valid) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int64_t m[10];
#pragma unroll
    for (int t = 0; t < 10; ++t) m[t] = moments[i * 10 + t];
    const int4 c = coords[i];
    double l[3], v[3];
    const bool ok = nrm_solve_row(m, c, orient, vx, vy, vz, batch_sums + 4 * (c.x & 15), l, v);
#pragma unroll
    for (int t = 0; t < 3; ++t) { lam[i * 3 + t] = l[t]; normals[i * 3 + t] = v[t]; }
    count[i] = (int32_t)m[0];
    valid[i] = ok ? 1 : 0;
}

// per batch: (distinct voxels, sum x, sum y, sum z) as int64; integer atomics, so the order of arrival does not matter
__global__ void __launch_bounds__(256) k_nrm_batch_sums(const int4* __restrict__ qs, const int32_t* __restrict__ runlen, int64_t n,
                                                        unsigned long long* __restrict__ sums) {
    __shared__ unsigned long long acc[64];
    if (threadIdx.x < 64) acc[threadIdx.x] = 0;
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && runlen[i] > 0) {
        const int4 c = qs[i];
        if ((uint32_t)c.x < 16u) {
            atomicAdd(&acc[4 * c.x + 0], 1ull); atomicAdd(&acc[4 * c.x + 1], (unsigned long long)c.y);
            atomicAdd(&acc[4 * c.x + 2], (unsigned long long)c.z); atomicAdd(&acc[4 * c.x + 3], (unsigned long long)c.w);
        }
    }
    __syncthreads();
    if (threadIdx.x < 64 && acc[threadIdx.x]) atomicAdd(&sums[threadIdx.x], acc[threadIdx.x]);
}

// Pass A's mapping, a process-wide A/B knob like pcgc_set_oct_tiled: 0 = one wave per occupied cell (default), 1 = one thread per voxel.
static int g_nrm_mapping = 0;
extern "C" int pcgc_set_normals_mapping(int mode) {
    const int old = g_nrm_mapping;
    if (mode == 0 || mode == 1) g_nrm_mapping = mode;
    return old;
}
#define NRM_CELL_BLOCKS 4096       // 256 CUs x 8 workgroups x 2: the waves stride over the cell list

// workspace: int64 [64] batch sums | int32 n_cells (+ padding) | int32 [n] cell list
#define NRM_WS_HEAD (64 * 8 + 16)
extern "C" size_t pcgc_normals_workspace_bytes(int64_t n) { return NRM_WS_HEAD + (size_t)(n < 1 ? 1 : n) * 4; }

extern "C" int pcgc_normals_estimate(const int32_t* coords, int64_t n, const int32_t* qs, const int32_t* perm, const uint64_t* cell_keys,
                                     const int32_t* cell_vals, int64_t cell_cap, const uint64_t* masks, const uint64_t* keys, const int32_t* vals,
                                     int64_t cap, const int32_t* runlen, const uint64_t* ball, int32_t r2, int orient, const double* viewpoint,
                                     int64_t* moments, double* normals, double* lam, int32_t* count, uint8_t* valid, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    PCGC_REQUIRE(r2 >= 1 && r2 <= NRM_MAX_R2, "r2 outside 1 .. 64");
    PCGC_REQUIRE(orient == NRM_ORIENT_NONE || orient == NRM_ORIENT_CENTROID || orient == NRM_ORIENT_VIEWPOINT, "bad orientation mode");
    PCGC_REQUIRE(orient != NRM_ORIENT_VIEWPOINT || viewpoint, "orientation towards a viewpoint needs one");
    PCGC_REQUIRE(n >= 0 && n <= 0x7FFFFFFF, "row count");
    PCGC_REQUIRE(cell_cap > 0 && (cell_cap & (cell_cap - 1)) == 0 && cap > 0 && (cap & (cap - 1)) == 0, "bad hash capacity");
    PCGC_REQUIRE(workspace_bytes >= pcgc_normals_workspace_bytes(n), "workspace too small");
    PCGC_REQUIRE(coords && qs && perm && masks && runlen && ball && moments && normals && lam && count && valid && workspace, "null argument");
    if (n == 0) return 0;
    unsigned long long* sums = (unsigned long long*)workspace;
    int32_t* n_cells = (int32_t*)((char*)workspace + 64 * 8);
    int32_t* cells = (int32_t*)((char*)workspace + NRM_WS_HEAD);
    hipError_t e = hipMemsetAsync(workspace, 0, NRM_WS_HEAD, S(stream));
    if (e != hipSuccess) { pcgc_set_error("normals_estimate: %s", hipGetErrorString(e)); return -1; }
    NrmIndex q;
    q.qs = (const int4*)qs; q.perm = perm; q.runlen = runlen;
    q.ckeys = cell_keys; q.cvals = cell_vals; q.cmask = (uint64_t)(cell_cap - 1); q.masks = (const unsigned long long*)masks;
    q.vkeys = keys; q.vvals = vals; q.vmask = (uint64_t)(cap - 1);
    const int C = nrm_reach_cells(r2);
    if (g_nrm_mapping == 0) {
        hipLaunchKernelGGL(k_nrm_cell_list, dim3(grid_for(n, 256)), dim3(256), 0, S(stream), q.masks, n, cells, n_cells);
        PCGC_CHECK_LAUNCH("normals_cell_list");
        const int64_t blocks = (n + 3) / 4 < NRM_CELL_BLOCKS ? (n + 3) / 4 : NRM_CELL_BLOCKS;        // (at most one cell per row)
        hipLaunchKernelGGL(k_nrm_moments_cells, dim3((unsigned)blocks), dim3(256), 0, S(stream), q, cells, n_cells,
                           (const unsigned long long*)ball, C, moments);
    } else {
        hipLaunchKernelGGL(k_nrm_moments_voxels, dim3(grid_for(n, 256)), dim3(256), 0, S(stream), q, n, (const unsigned long long*)ball, C,
                           moments);
    }
    PCGC_CHECK_LAUNCH("normals_moments");
    if (orient == NRM_ORIENT_CENTROID) {
        hipLaunchKernelGGL(k_nrm_batch_sums, dim3(grid_for(n, 256)), dim3(256), 0, S(stream), q.qs, runlen, n, sums);
        PCGC_CHECK_LAUNCH("normals_batch_sums");
    }
    const double vx = viewpoint ? viewpoint[0] : 0.0, vy = viewpoint ? viewpoint[1] : 0.0, vz = viewpoint ? viewpoint[2] : 0.0;
    hipLaunchKernelGGL(k_nrm_solve, dim3(grid_for(n, 256)), dim3(256), 0, S(stream), (const int4*)coords, n, moments, orient, vx, vy, vz,
                       (const long long*)sums, normals, lam, count, valid);
    PCGC_CHECK_LAUNCH("normals_solve");
    return 0;
}
