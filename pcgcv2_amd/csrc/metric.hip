// D2 (point-to-plane) geometry distortion on device: mpeg-pcc-dmetric 0.13.4 with `-n infile1` (pc_error.py:27-74; the reference's
// test.py:74-75 asks for it with normal=True), the semantics of pc_error.d2_psnr and oracle/pcgc_oracle.py:d2_metrics.
//
// A searched cloud Q is held as (a) its rows sorted by (batch, z, y, x) — stable, so the duplicates of a voxel form one run in ascending
// original row — with the run length at each run start, (b) the coordinate hash of the sorted rows (voxel -> run start), and (c) the
// stride-4 cells of coords.hip's D1 search (cell hash + 64-bit occupancy mask per cell).  A query walks the cell offsets in ascending
// lower bound and stops only when the bound EXCEEDS the best distance, so every voxel at the nearest distance is seen (its tie set).
//
// Passes per direction P -> Q: count (best d2, tie rows, unresolved flag) -> scan -> fill (tie rows into each point's segment) -> per-segment
// selection of the lowest rows (at most 30 kept).  Points whose ties cannot be proven complete within the offset table are appended to a
// list and searched again with a larger table, and finally against every row of Q of their batch.  Then the normals of B (rows of B receive
// the normals of the A-points that tie to them, summed in ascending A row in fp64), c2p per point, and reductions in a fixed order: no
// floating-point atomics anywhere, so every result is bitwise reproducible.
#include <cstring>
#include "pcgc_common.h"
#include <rocprim/rocprim.hpp>

#define D2_NONE 0x7FFFFFFFFFFFFFFFll

__device__ static inline int64_t d2_point(const int32_t* __restrict__ sel, int64_t t) { return sel ? (int64_t)sel[t] : t; }
__device__ static inline bool same_voxel(int4 a, int4 b) { return a.x == b.x && a.y == b.y && a.z == b.z && a.w == b.w; }

// run length at each run start of the sorted rows, 0 elsewhere
__global__ void k_d2_runs(const int4* __restrict__ qs, int64_t nq, int32_t* __restrict__ runlen) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    const int4 c = qs[i];
    if (i > 0 && same_voxel(qs[i - 1], c)) { runlen[i] = 0; return; }
    int64_t j = i + 1;
    while (j < nq && same_voxel(qs[j], c)) ++j;
    runlen[i] = (int32_t)(j - i);
}

struct D2Index {                       // the searched cloud (sorted rows)
    const uint64_t* ckeys; const int32_t* cvals; uint64_t cmask; const unsigned long long* masks;
    const uint64_t* vkeys; const int32_t* vvals; uint64_t vmask; const int32_t* runlen; const int32_t* perm;
};

// Walks the cell table for query c.  mode 0: best squared distance and the number of rows at it.  mode 1 (best known): writes the original
// rows of every voxel at distance `best` to rows[w ..] (bounded by `end`).
template <int MODE>
__device__ static inline void d2_walk(const D2Index& q, int4 c, const int4* __restrict__ offsets, int n_off, int& best, int& cnt,
                                      int32_t* __restrict__ rows, int64_t w, int64_t end) {
    const int lx = c.y & 3, ly = c.z & 3, lz = c.w & 3;
    const int X = c.y & ~3, Y = c.z & ~3, Z = c.w & ~3;
    for (int t = 0; t < n_off; ++t) {
        const int4 o = offsets[t];                                   // (cell offset x, y, z; lower bound of the squared distance)
        if (o.w > best) break;                                       // (equal bounds may still hold ties)
        const int32_t row = hash_lookup(q.ckeys, q.cvals, q.cmask, c.x, X + 4 * o.x, Y + 4 * o.y, Z + 4 * o.z);
        if (row < 0) continue;
        unsigned long long m = q.masks[row];
        const int bx = 4 * o.x - lx, by = 4 * o.y - ly, bz = 4 * o.z - lz;
        while (m) {
            const int bit = __ffsll((long long)m) - 1;
            m &= m - 1;
            const int dx = bx + (bit & 3), dy = by + ((bit >> 2) & 3), dz = bz + (bit >> 4);
            const int d2 = dx * dx + dy * dy + dz * dz;
            if (MODE == 0 ? d2 > best : d2 != best) continue;
            // (the cell masks and the voxel hash are built from the same rows: the voxel is always found)
            const int32_t s = hash_lookup(q.vkeys, q.vvals, q.vmask, c.x, X + 4 * o.x + (bit & 3), Y + 4 * o.y + ((bit >> 2) & 3),
                                          Z + 4 * o.z + (bit >> 4));
            if (s < 0) continue;
            const int r = q.runlen[s];
            if (MODE == 0) {
                if (d2 < best) { best = d2; cnt = r; } else cnt += r;
            } else {
                for (int k = 0; k < r && w < end; ++k) rows[w++] = q.perm[s + k];
            }
        }
    }
}

__global__ void __launch_bounds__(256) k_d2_count(const int4* __restrict__ p, int64_t n, const int32_t* __restrict__ sel, D2Index q,
                                                  const int4* __restrict__ offsets, int n_off, int32_t reach2, int64_t* __restrict__ best_out,
                                                  int32_t* __restrict__ cnt_out, int32_t* __restrict__ unres, int32_t* __restrict__ n_unres) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const int64_t i = d2_point(sel, t);
    int best = 0x7FFFFFFF, cnt = 0;
    d2_walk<0>(q, p[i], offsets, n_off, best, cnt, nullptr, 0, 0);
    if (best < reach2) { best_out[i] = best; cnt_out[i] = cnt; return; }
    best_out[i] = D2_NONE; cnt_out[i] = 0;                           // a nearer voxel could lie outside the table: search again
    unres[atomicAdd(n_unres, 1)] = (int32_t)i;
}

__global__ void __launch_bounds__(256) k_d2_fill(const int4* __restrict__ p, int64_t n, const int32_t* __restrict__ sel, D2Index q,
                                                 const int4* __restrict__ offsets, int n_off, int32_t reach2, const int64_t* __restrict__ best_in,
                                                 const int64_t* __restrict__ seg, int32_t* __restrict__ rows) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const int64_t i = d2_point(sel, t);
    const int64_t b = best_in[i];
    if (b >= reach2) return;                                         // (settled by a larger table or the exhaustive pass)
    int best = (int)b, cnt = 0;
    d2_walk<1>(q, p[i], offsets, n_off, best, cnt, rows, seg[i], seg[i + 1]);
}

// The exhaustive finish: every row of Q with the query's batch (a contiguous range of the batch-major sorted rows).
__device__ static inline int64_t batch_lower_bound(const int4* __restrict__ qs, int64_t nq, int32_t b) {
    int64_t lo = 0, hi = nq;
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (qs[mid].x < b) lo = mid + 1; else hi = mid; }
    return lo;
}
__global__ void __launch_bounds__(256) k_d2_exhaustive(const int4* __restrict__ p, int64_t n, const int32_t* __restrict__ sel,
                                                       const int4* __restrict__ qs, int64_t nq, const int32_t* __restrict__ perm, int fill,
                                                       int64_t* __restrict__ best_io, int32_t* __restrict__ cnt_out, const int64_t* __restrict__ seg,
                                                       int32_t* __restrict__ rows, int32_t* __restrict__ n_empty) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const int64_t i = d2_point(sel, t);
    const int4 c = p[i];
    const int64_t lo = batch_lower_bound(qs, nq, c.x), hi = batch_lower_bound(qs, nq, c.x + 1);
    if (lo == hi) { if (!fill) { best_io[i] = D2_NONE; cnt_out[i] = 0; atomicAdd(n_empty, 1); } return; }
    int64_t best = fill ? best_io[i] : D2_NONE;
    int32_t cnt = 0;
    int64_t w = fill ? seg[i] : 0;
    const int64_t end = fill ? seg[i + 1] : 0;
    for (int64_t j = lo; j < hi; ++j) {
        const int4 o = qs[j];
        const int64_t dx = c.y - o.y, dy = c.z - o.z, dz = c.w - o.w;
        const int64_t d2 = dx * dx + dy * dy + dz * dz;
        if (fill) { if (d2 == best && w < end) rows[w++] = perm[j]; }
        else if (d2 < best) { best = d2; cnt = 1; }
        else if (d2 == best) ++cnt;
    }
    if (!fill) { best_io[i] = best; cnt_out[i] = cnt; }
}

// Per segment: the `cap` lowest rows in ascending order at its head (selection; segments are a few rows, more than 30 only on rare
// lattice configurations or duplicated rows).  kept (optional) = min(size, cap).
__global__ void __launch_bounds__(256) k_d2_segment_lowest(const int64_t* __restrict__ seg, int64_t n, int32_t* __restrict__ rows, int32_t cap,
                                                           int32_t* __restrict__ kept) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t s = seg[i], m = seg[i + 1] - s;
    const int64_t k_end = m < cap ? m : cap;
    for (int64_t k = 0; k < k_end; ++k) {
        int64_t arg = s + k;
        int32_t v = rows[arg];
        for (int64_t j = s + k + 1; j < s + m; ++j) { const int32_t u = rows[j]; if (u < v) { v = u; arg = j; } }
        rows[arg] = rows[s + k]; rows[s + k] = v;
    }
    if (kept) kept[i] = (int32_t)k_end;
}

// The reverse relation B <- A: count of A-points whose kept tie set holds b, then the A rows into b's segment (ordered afterwards).
__global__ void __launch_bounds__(256) k_d2_recv_count(const int64_t* __restrict__ seg, const int32_t* __restrict__ kept, int64_t na,
                                                       const int32_t* __restrict__ rows, int64_t nb, int32_t* __restrict__ rcnt) {
    const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= na) return;
    const int64_t s = seg[a];
    for (int k = 0; k < kept[a]; ++k) {
        const int32_t b = rows[s + k];
        if ((uint32_t)b < (uint64_t)nb) atomicAdd(&rcnt[b], 1);
    }
}
__global__ void __launch_bounds__(256) k_d2_recv_fill(const int64_t* __restrict__ seg, const int32_t* __restrict__ kept, int64_t na,
                                                      const int32_t* __restrict__ rows, int64_t nb, const int64_t* __restrict__ rseg,
                                                      int32_t* __restrict__ cursor, int32_t* __restrict__ recv) {
    const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= na) return;
    const int64_t s = seg[a];
    for (int k = 0; k < kept[a]; ++k) {
        const int32_t b = rows[s + k];
        if ((uint32_t)b >= (uint64_t)nb) continue;
        const int32_t pos = atomicAdd(&cursor[b], 1);
        if (rseg[b] + pos < rseg[b + 1]) recv[rseg[b] + pos] = (int32_t)a;
    }
}

// Normals of B: the mean of the received normals, summed in ascending A row (np.add.at's order), or — nothing received — the mean normal
// of b's own kept B -> A tie set.
__global__ void __launch_bounds__(256) k_d2_normals(const int64_t* __restrict__ rseg, const int32_t* __restrict__ recv, int64_t nb,
                                                    const double* __restrict__ na, const int64_t* __restrict__ seg_ba, const int32_t* __restrict__ kept_ba,
                                                    const int32_t* __restrict__ rows_ba, double* __restrict__ nb_out) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nb) return;
    const int64_t r0 = rseg[j], r1 = rseg[j + 1];
    const bool got = r1 > r0;
    const int32_t* src = got ? recv + r0 : rows_ba + seg_ba[j];
    const int64_t m = got ? r1 - r0 : (int64_t)kept_ba[j];
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int64_t k = 0; k < m; ++k) {
        const int64_t a = src[k];
        sx += na[3 * a]; sy += na[3 * a + 1]; sz += na[3 * a + 2];
    }
    const double d = (double)m;
    nb_out[3 * j] = sx / d; nb_out[3 * j + 1] = sy / d; nb_out[3 * j + 2] = sz / d;
}

// c2p(p) = mean over p's kept tie set of ((p - q) . n_q)^2, the dot product summed x, y, z in that order (no contraction: -ffp-contract=off)
__global__ void __launch_bounds__(256) k_d2_c2p(const int4* __restrict__ p, int64_t n, const int4* __restrict__ q, const double* __restrict__ nq,
                                                const int64_t* __restrict__ seg, const int32_t* __restrict__ kept, const int32_t* __restrict__ rows,
                                                double* __restrict__ c2p) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int4 c = p[i];
    const int64_t s = seg[i];
    const int m = kept[i];
    double acc = 0.0;
    for (int k = 0; k < m; ++k) {
        const int64_t r = rows[s + k];
        const int4 o = q[r];
        const double ex = (double)(c.y - o.y), ey = (double)(c.z - o.z), ez = (double)(c.w - o.w);
        double dot = ex * nq[3 * r] + ey * nq[3 * r + 1];
        dot = dot + ez * nq[3 * r + 2];
        acc += dot * dot;
    }
    c2p[i] = m > 0 ? acc / (double)m : 0.0;
}

// Sum and max of c2c, sum of c2p: a fixed grid with a strided loop per thread and a fixed tree per block, then one block over the partials.
#define D2_RED_BLOCKS 1024
__device__ static inline void block_tree(double* sd, long long* ss, long long* sm) {
    for (int h = 128; h > 0; h >>= 1) {
        __syncthreads();
        if ((int)threadIdx.x < h) {
            sd[threadIdx.x] += sd[threadIdx.x + h];
            ss[threadIdx.x] += ss[threadIdx.x + h];
            sm[threadIdx.x] = sm[threadIdx.x] > sm[threadIdx.x + h] ? sm[threadIdx.x] : sm[threadIdx.x + h];
        }
    }
    __syncthreads();
}
__global__ void __launch_bounds__(256) k_d2_reduce(const int64_t* __restrict__ c2c, const double* __restrict__ c2p, int64_t n, int stride_blocks,
                                                   double* __restrict__ pd, long long* __restrict__ ps, long long* __restrict__ pm) {
    __shared__ double sd[256];
    __shared__ long long ss[256], sm[256];
    double d = 0.0; long long s = 0, m = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)stride_blocks * 256) {
        d += c2p[i]; s += c2c[i]; m = c2c[i] > m ? c2c[i] : m;
    }
    sd[threadIdx.x] = d; ss[threadIdx.x] = s; sm[threadIdx.x] = m;
    block_tree(sd, ss, sm);
    if (threadIdx.x == 0) { pd[blockIdx.x] = sd[0]; ps[blockIdx.x] = ss[0]; pm[blockIdx.x] = sm[0]; }
}
__global__ void __launch_bounds__(256) k_d2_reduce_final(const double* __restrict__ pd, const long long* __restrict__ ps, const long long* __restrict__ pm,
                                                         int blocks, double* __restrict__ c2p_sum, long long* __restrict__ c2c_sum_max) {
    __shared__ double sd[256];
    __shared__ long long ss[256], sm[256];
    double d = 0.0; long long s = 0, m = 0;
    for (int i = threadIdx.x; i < blocks; i += 256) { d += pd[i]; s += ps[i]; m = pm[i] > m ? pm[i] : m; }
    sd[threadIdx.x] = d; ss[threadIdx.x] = s; sm[threadIdx.x] = m;
    block_tree(sd, ss, sm);
    if (threadIdx.x == 0) { c2p_sum[0] = sd[0]; c2c_sum_max[0] = ss[0]; c2c_sum_max[1] = sm[0]; }
}

extern "C" int pcgc_d2_runs(const int32_t* qs, int64_t nq, int32_t* runlen, void* stream) {
    if (nq == 0) return 0;
    hipLaunchKernelGGL(k_d2_runs, dim3(grid_for(nq, 256)), dim3(256), 0, S(stream), (const int4*)qs, nq, runlen);
    PCGC_CHECK_LAUNCH("d2_runs");
    return 0;
}

static D2Index make_index(const uint64_t* cell_keys, const int32_t* cell_vals, int64_t cell_cap, const uint64_t* masks, const uint64_t* keys,
                          const int32_t* vals, int64_t cap, const int32_t* runlen, const int32_t* perm) {
    D2Index q;
    q.ckeys = cell_keys; q.cvals = cell_vals; q.cmask = (uint64_t)(cell_cap - 1); q.masks = (const unsigned long long*)masks;
    q.vkeys = keys; q.vvals = vals; q.vmask = (uint64_t)(cap - 1); q.runlen = runlen; q.perm = perm;
    return q;
}

extern "C" int pcgc_d2_count(const int32_t* p, int64_t n, const int32_t* sel, const uint64_t* cell_keys, const int32_t* cell_vals, int64_t cell_cap,
                             const uint64_t* masks, const uint64_t* keys, const int32_t* vals, int64_t cap, const int32_t* runlen,
                             const int32_t* offsets, int n_offsets, int32_t reach2, int64_t* best, int32_t* cnt, int32_t* unresolved,
                             int32_t* n_unresolved, void* stream) {
    PCGC_REQUIRE(cell_cap > 0 && (cell_cap & (cell_cap - 1)) == 0 && cap > 0 && (cap & (cap - 1)) == 0, "bad hash capacity");
    hipError_t e = hipMemsetAsync(n_unresolved, 0, 4, S(stream));
    if (e != hipSuccess) { pcgc_set_error("d2_count: %s", hipGetErrorString(e)); return -1; }
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_d2_count, dim3(grid_for(n, 256)), dim3(256), 0, S(stream), (const int4*)p, n, sel,
                       make_index(cell_keys, cell_vals, cell_cap, masks, keys, vals, cap, runlen, nullptr), (const int4*)offsets, n_offsets, reach2,
                       best, cnt, unresolved, n_unresolved);
    PCGC_CHECK_LAUNCH("d2_count");
    return 0;
}

extern "C" int pcgc_d2_fill(const int32_t* p, int64_t n, const int32_t* sel, const uint64_t* cell_keys, const int32_t* cell_vals, int64_t cell_cap,
                            const uint64_t* masks, const uint64_t* keys, const int32_t* vals, int64_t cap, const int32_t* runlen, const int32_t* perm,
                            const int32_t* offsets, int n_offsets, int32_t reach2, const int64_t* best, const int64_t* seg, int32_t* rows, void* stream) {
    PCGC_REQUIRE(cell_cap > 0 && (cell_cap & (cell_cap - 1)) == 0 && cap > 0 && (cap & (cap - 1)) == 0, "bad hash capacity");
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_d2_fill, dim3(grid_for(n, 256)), dim3(256), 0, S(stream), (const int4*)p, n, sel,
                       make_index(cell_keys, cell_vals, cell_cap, masks, keys, vals, cap, runlen, perm), (const int4*)offsets, n_offsets, reach2,
                       best, seg, rows);
    PCGC_CHECK_LAUNCH("d2_fill");
    return 0;
}

extern "C" int pcgc_d2_exhaustive(const int32_t* p, int64_t n, const int32_t* sel, const int32_t* qs, int64_t nq, const int32_t* perm, int fill,
                                  int64_t* best, int32_t* cnt, const int64_t* seg, int32_t* rows, int32_t* n_empty, void* stream) {
    PCGC_REQUIRE(fill ? (seg && rows && perm) : (cnt && n_empty), "null argument");
    if (!fill) {
        hipError_t e = hipMemsetAsync(n_empty, 0, 4, S(stream));
        if (e != hipSuccess) { pcgc_set_error("d2_exhaustive: %s", hipGetErrorString(e)); return -1; }
    }
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_d2_exhaustive, dim3(grid_for(n, 256)), dim3(256), 0, S(stream), (const int4*)p, n, sel, (const int4*)qs, nq, perm, fill,
                       best, cnt, seg, rows, n_empty);
    PCGC_CHECK_LAUNCH("d2_exhaustive");
    return 0;
}

static size_t scan_temp_bytes(int64_t n) {
    size_t tmp = 0;
    (void)rocprim::inclusive_scan((void*)nullptr, tmp, (const int32_t*)nullptr, (int64_t*)nullptr, (size_t)(n < 1 ? 1 : n),
                                  rocprim::plus<int64_t>(), (hipStream_t)0);
    return tmp;
}
extern "C" size_t pcgc_d2_scan_workspace_bytes(int64_t n) { return scan_temp_bytes(n) + 256; }
extern "C" int pcgc_d2_scan(const int32_t* cnt, int64_t n, int64_t* seg, void* workspace, size_t workspace_bytes, void* stream) {
    PCGC_REQUIRE(workspace_bytes >= pcgc_d2_scan_workspace_bytes(n), "workspace too small");
    hipError_t e = hipMemsetAsync(seg, 0, 8, S(stream));
    if (e == hipSuccess && n > 0) {
        size_t tmp = scan_temp_bytes(n);
        e = rocprim::inclusive_scan(workspace, tmp, cnt, seg + 1, (size_t)n, rocprim::plus<int64_t>(), S(stream));
    }
    if (e != hipSuccess) { pcgc_set_error("d2_scan: %s", hipGetErrorString(e)); return -1; }
    PCGC_CHECK_LAUNCH("d2_scan");
    return 0;
}

extern "C" int pcgc_d2_segment_lowest(const int64_t* seg, int64_t n, int32_t* rows, int32_t cap, int32_t* kept, void* stream) {
    PCGC_REQUIRE(cap > 0, "bad cap");
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_d2_segment_lowest, dim3(grid_for(n, 256)), dim3(256), 0, S(stream), seg, n, rows, cap, kept);
    PCGC_CHECK_LAUNCH("d2_segment_lowest");
    return 0;
}

extern "C" int pcgc_d2_recv_count(const int64_t* seg, const int32_t* kept, int64_t na, const int32_t* rows, int64_t nb, int32_t* rcnt, void* stream) {
    hipError_t e = hipMemsetAsync(rcnt, 0, (size_t)nb * 4, S(stream));
    if (e != hipSuccess) { pcgc_set_error("d2_recv_count: %s", hipGetErrorString(e)); return -1; }
    if (na == 0) return 0;
    hipLaunchKernelGGL(k_d2_recv_count, dim3(grid_for(na, 256)), dim3(256), 0, S(stream), seg, kept, na, rows, nb, rcnt);
    PCGC_CHECK_LAUNCH("d2_recv_count");
    return 0;
}

extern "C" int pcgc_d2_recv_fill(const int64_t* seg, const int32_t* kept, int64_t na, const int32_t* rows, int64_t nb, const int64_t* rseg,
                                 int32_t* cursor, int32_t* recv, void* stream) {
    hipError_t e = hipMemsetAsync(cursor, 0, (size_t)nb * 4, S(stream));
    if (e != hipSuccess) { pcgc_set_error("d2_recv_fill: %s", hipGetErrorString(e)); return -1; }
    if (na == 0) return 0;
    hipLaunchKernelGGL(k_d2_recv_fill, dim3(grid_for(na, 256)), dim3(256), 0, S(stream), seg, kept, na, rows, nb, rseg, cursor, recv);
    PCGC_CHECK_LAUNCH("d2_recv_fill");
    return 0;
}

extern "C" int pcgc_d2_normals(const int64_t* rseg, const int32_t* recv, int64_t nb, const double* na, const int64_t* seg_ba, const int32_t* kept_ba,
                               const int32_t* rows_ba, double* nb_out, void* stream) {
    if (nb == 0) return 0;
    hipLaunchKernelGGL(k_d2_normals, dim3(grid_for(nb, 256)), dim3(256), 0, S(stream), rseg, recv, nb, na, seg_ba, kept_ba, rows_ba, nb_out);
    PCGC_CHECK_LAUNCH("d2_normals");
    return 0;
}

extern "C" int pcgc_d2_c2p(const int32_t* p, int64_t n, const int32_t* q, const double* nq, const int64_t* seg, const int32_t* kept,
                           const int32_t* rows, double* c2p, void* stream) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_d2_c2p, dim3(grid_for(n, 256)), dim3(256), 0, S(stream), (const int4*)p, n, (const int4*)q, nq, seg, kept, rows, c2p);
    PCGC_CHECK_LAUNCH("d2_c2p");
    return 0;
}

extern "C" size_t pcgc_d2_reduce_workspace_bytes(void) { return (size_t)D2_RED_BLOCKS * 3 * 8; }
extern "C" int pcgc_d2_reduce(const int64_t* c2c, const double* c2p, int64_t n, int64_t* c2c_sum_max, double* c2p_sum, void* workspace,
                              size_t workspace_bytes, void* stream) {
    PCGC_REQUIRE(workspace_bytes >= pcgc_d2_reduce_workspace_bytes(), "workspace too small");
    int blocks = (int)grid_for(n < 1 ? 1 : n, 256);
    blocks = blocks < D2_RED_BLOCKS ? blocks : D2_RED_BLOCKS;          // (a function of n only: the summation order is fixed)
    double* pd = (double*)workspace;
    long long* ps = (long long*)(pd + D2_RED_BLOCKS);
    long long* pm = ps + D2_RED_BLOCKS;
    hipLaunchKernelGGL(k_d2_reduce, dim3(blocks), dim3(256), 0, S(stream), c2c, c2p, n, blocks, pd, ps, pm);
    PCGC_CHECK_LAUNCH("d2_reduce");
    // second stage: the block partials as the input of one block (c2c sums in the same buffer layout; max of maxima)
    hipLaunchKernelGGL(k_d2_reduce_final, dim3(1), dim3(256), 0, S(stream), pd, ps, pm, blocks, c2p_sum, (long long*)c2c_sum_max);
    PCGC_CHECK_LAUNCH("d2_reduce");
    return 0;
}
