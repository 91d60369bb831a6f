/*
 * pcgc_hip.h — C-ABI of libpcgc_hip.so: the MI355X (gfx950) native operators under PCGCv2's encode/decode path.
 *
 * The reference (NJUVISION/PCGCv2) has no FFI layer of its own: its native code is reached through
 * `import MinkowskiEngine` and `import torchac`.  Each entry point below replaces one of those Python->native call
 * sites (cited as reference file:line); INTEGRATION.md shows the ctypes binding a maintainer would add.
 *
 * Conventions
 *   - plain pointers and sizes only; no torch / C++ types cross this boundary.
 *   - every pointer marked [dev] is a device buffer owned by the caller (PyTorch-ROCm's allocator in our host code);
 *     [host] is host memory.  The library never allocates a result the caller must free.
 *   - variable-size results are two-phase: a count comes back through a [dev] int32, the caller sizes the output.
 *   - `stream` is a hipStream_t passed as void*; every device call is asynchronous on that stream.
 *   - return value: 0 = OK, <0 = error (message via pcgc_last_error()).
 *   - coordinates: int32 [N,4] rows (batch, x, y, z), 0 <= x,y,z < 2^20, 0 <= batch < 16  (ME.SparseTensor.C layout).
 *   - features: fp32 row-major, leading dimension given explicitly (`*_ld`, in floats) so concat / slices are views.
 *   - kernel maps: int32 [K][N_out], entry = input row feeding output row o through kernel offset k, or -1.
 *     offset order: k3 -> (k%3-1, (k/3)%3-1, k/9-1)*stride ; k2 -> (k&1, (k>>1)&1, k>>2)*stride  (x fastest, ME ‡).
 *   - canonical arithmetic: out = ( fp32 fmaf chain over k ascending, ci ascending, from +0 ) + bias ; then
 *     + residual ; then ReLU.   Bit-identical to oracle/pcgc_oracle.c.
 */
#ifndef PCGC_HIP_H
#define PCGC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

const char* pcgc_last_error(void);
int pcgc_version(void);

/* ---- coordinate hash map: replaces ME's CoordinateManager / coordinate map (ME.SparseTensor ctor at
 *      data_utils.py:96,108,116 and coder.py:102).  Open addressing, 64-slot spatial blocks (4x4x4 voxels). ---- */
int64_t pcgc_hash_capacity(int64_t n);                                   /* slots needed for n coordinates (pow2) */
int pcgc_hash_clear(uint64_t* keys /*[dev cap]*/, int32_t* vals /*[dev cap]*/, int64_t cap, void* stream);
/* `stride` = tensor stride of the level the table indexes.  Kept in the signatures for the callers' bookkeeping: the slot of a
 * key is a mix of the whole coordinate key and does not depend on it (the round-1 spatially blocked layout did). */
int pcgc_hash_insert(const int32_t* coords /*[dev n,4]*/, int64_t n, int32_t stride, uint64_t* keys, int32_t* vals,
                     int64_t cap, void* stream);                         /* vals[slot] = smallest row with that key */
/* dedup policy as an argument: keep_last = 0 is pcgc_hash_insert; 1 keeps the LARGEST row per key (ME's dedup policy for equal
 * coordinates is a ‡ convention; hash_first_mask then marks the kept rows either way: keep[i] = (vals[slot] == i)). */
int pcgc_hash_insert_policy(const int32_t* coords, int64_t n, int32_t stride, uint64_t* keys, int32_t* vals, int64_t cap,
                            int keep_last, void* stream);
int pcgc_hash_first_mask(const int32_t* coords, int64_t n, int32_t stride, const uint64_t* keys, const int32_t* vals,
                         int64_t cap, uint8_t* keep /*[dev n]*/, int32_t* first_row /*[dev n] or NULL*/, void* stream);
                         /* keep[i] = row i is the first occurrence of its coordinate; first_row[i] = that first row */

/* Validation of caller-supplied coordinates (ME accepts any int32 coordinate; this library keys levels by 4+20+20+20 bits, so the host layer
 * — SparseTensor ctor, scale_sparse_tensor — raises instead of silently dropping rows) + how ordered the rows are: out2[0] = rows out of range
 * (negative, >= 2^20, batch >= 16), out2[1] = descents of the (batch, z, y, x) key along the
 * rows (0: the rows are in sort_spare_tensor's order, data_utils.py:91-101).  The reference takes rows in any order (ME hashes them); here
 * the canonical row order of every level follows the input order, so an unordered PLY would drive every encoder gather through a random
 * row order — Coder.encode sorts such a cloud once at ingest (no output byte depends on it: the latent is sorted before coding). */
int pcgc_coords_check_order(const int32_t* coords /*[dev n,4]*/, int64_t n, int32_t* out2 /*[dev 2]*/, void* stream);

/* ---- coordinate transforms ---- */
/* output coords of MinkowskiConvolution(kernel_size=2, stride=2): floor(c / stride_out) * stride_out per row
 * (autoencoder.py:78-84,97-103,116-122); dedup with the hash calls above. */
int pcgc_coords_quantize(const int32_t* coords, int64_t n, int32_t stride_out, int32_t* out /*[dev n,4]*/, void* stream);
/* output coords of MinkowskiGenerativeConvolutionTranspose(k=2,s=2): row 8*i+k = c_i + (k&1,(k>>1)&1,k>>2)*stride_in/2
 * (autoencoder.py:155-161,182-188,209-215). */
int pcgc_coords_children(const int32_t* coords, int64_t n, int32_t stride_in, int32_t* out /*[dev 8n,4]*/, void* stream);
/* scale_sparse_tensor: round_half_even(float32(c) * float32(factor)) (data_utils.py:112-118); batch column kept. */
int pcgc_coords_scale(const int32_t* coords, int64_t n, float factor, int32_t* out /*[dev n,4]*/, void* stream);

/* ---- stream compaction (MinkowskiPruning, autoencoder.py:237,247; also dedup) ---- */
size_t pcgc_scan_workspace_bytes(int64_t n);
/* prefix[i] = number of set mask bytes before i; *total = number set. */
int pcgc_mask_scan(const uint8_t* mask /*[dev n]*/, int64_t n, int32_t* prefix /*[dev n]*/, int32_t* total /*[dev 1]*/,
                   void* workspace /*[dev]*/, size_t workspace_bytes, void* stream);
/* the same for a workspace (and *total, if n may be 0) the caller has already zeroed: several scans behind one memset */
int pcgc_mask_scan_zeroed(const uint8_t* mask, int64_t n, int32_t* prefix, int32_t* total, void* workspace, size_t workspace_bytes,
                          void* stream);
int pcgc_compact_coords(const int32_t* coords, const uint8_t* mask, const int32_t* prefix, int64_t n,
                        int32_t* out /*[dev total,4]*/, void* stream);
/* any C, in_ld >= C and any 4-byte aligned `in` / `out` (a column slice of a wider buffer): 16-byte accesses are used only when C and
 * in_ld are multiples of 4 AND both bases are 16-byte aligned, a scalar kernel otherwise. */
int pcgc_compact_feats(const float* in, int C, int in_ld, const uint8_t* mask, const int32_t* prefix, int64_t n,
                       float* out /*[dev total,C]*/, void* stream);

/* ---- kernel maps (ME kernel maps, built once per coordinate level and reused by every conv on it) ---- */
int pcgc_kmap_k3(const int32_t* coords, int64_t n, int32_t stride, const uint64_t* keys, const int32_t* vals,
                 int64_t cap, int32_t* nbr /*[dev 27,n]*/, void* stream);

/* Hierarchical kernel maps: a level's 27-neighbourhood is a gather through its PARENT level's map (octree relation), so
 * only the coarsest level of a pyramid probes the hash.  (ME rebuilds a hash-probed map per level ‡.) */
/* children of a generative transpose (all 8 children exist, rows 8*i+j):  [27, 8*n_parent] from [27, n_parent] */
int pcgc_kmap_k3_children(const int32_t* parent_nbr, int64_t n_parent, int32_t* nbr /*[dev 27,8n]*/, void* stream);
/* pruned level: surviving rows orig[r] of a candidate level, neighbours renumbered through mask/prefix */
int pcgc_kmap_k3_prune(const int32_t* cand_nbr /*[27,n_cand]*/, int64_t n_cand, const uint8_t* mask, const int32_t* prefix,
                       const int32_t* orig /*[n_out]*/, int64_t n_out, int32_t* nbr /*[dev 27,n_out]*/, void* stream);
/* the same pruned-level map derived straight from the PARENT level's map when the candidate level is a children level
 * (mask / prefix / orig index candidate rows 8 i + j): the candidates' own [27][8 n_parent] map is never materialised. */
int pcgc_kmap_k3_prune_parent(const int32_t* parent_nbr /*[dev 27,n_parent]*/, int64_t n_parent, const uint8_t* mask,
                              const int32_t* prefix, const int32_t* orig, int64_t n_out, int32_t* nbr /*[dev 27,n_out]*/, void* stream);
/* strided pyramid (encoder): fine level from the coarse level's map + the down map + each fine row's parent row */
int pcgc_kmap_k3_from_coarse(const int32_t* fine /*[n_fine,4]*/, int64_t n_fine, int32_t stride_fine,
                             const int32_t* parent_of /*[n_fine]*/, const int32_t* coarse_nbr /*[27,n_coarse]*/,
                             const int32_t* down /*[8,n_coarse]*/, int64_t n_coarse, int32_t* nbr /*[dev 27,n_fine]*/,
                             void* stream);
/* parent_of[c] = prefix[first_row[c]]; down[slot(c)][parent_of[c]] = c — the k2s2 kernel map without hash probes */
int pcgc_down_maps(const int32_t* fine, const int32_t* first_row, const int32_t* prefix, int64_t n_fine, int32_t stride_fine,
                   int64_t n_coarse, int32_t* parent_of /*[dev n_fine]*/, int32_t* down /*[dev 8,n_coarse]*/, void* stream);
/* One strided pyramid level = pcgc_coords_quantize + hash clear/insert/first_mask + pcgc_mask_scan (prepare), then — after
 * the host has read *total = n_coarse — pcgc_compact_coords + pcgc_down_maps (finish).  Same kernels, two calls. */
int pcgc_down_prepare(const int32_t* fine /*[dev n,4]*/, int64_t n, int32_t stride_fine, int32_t* q /*[dev n,4] quantised*/,
                      uint64_t* keys, int32_t* vals, int64_t cap, uint8_t* keep /*[dev n]*/, int32_t* first_row /*[dev n]*/,
                      int32_t* prefix /*[dev n]*/, int32_t* total /*[dev 1]*/, void* scan_ws, size_t scan_ws_bytes, void* stream);
int pcgc_down_finish(const int32_t* fine, const int32_t* q, const uint8_t* keep, const int32_t* first_row, const int32_t* prefix,
                     int64_t n, int32_t stride_fine, int64_t n_coarse, int32_t* coarse /*[dev n_coarse,4]*/,
                     int32_t* parent_of /*[dev n]*/, int32_t* down /*[dev 8,n_coarse]*/, void* stream);
/* prepare + read-back of n_coarse (synchronises `stream`) + finish in one call.  coarse / down are caller buffers of upper-bound
 * size ([n,4] and 8*n int32: a coarse level has at most n rows); down is written as [8][n_coarse] at the front of its buffer. */
int pcgc_down_level(const int32_t* fine /*[dev n,4]*/, int64_t n, int32_t stride_fine, int32_t* q, uint64_t* keys, int32_t* vals,
                    int64_t cap, uint8_t* keep, int32_t* first_row, int32_t* prefix, int32_t* total, void* scan_ws,
                    size_t scan_ws_bytes, int32_t* coarse /*[dev n,4] capacity*/, int32_t* parent_of /*[dev n]*/,
                    int32_t* down /*[dev 8*n] capacity*/, int64_t* n_coarse_out /*host*/, void* stream);
/* `levels` (1..4) successive levels at once, every one deduplicated straight from the input rows (the canonical order of a level —
 * first occurrence in the level below — equals first occurrence in the input), so that the sizes of all levels come back in ONE
 * synchronising copy.  Level l (0-based) has stride `stride << (l + 1)`; coarse[l] / down[l] are caller buffers of upper-bound size
 * ([n,4] and 8*n int32), parent_of[l] has one entry per row of the level below it ([n] for l = 0, counts[l-1] after); counts[l] (host)
 * = rows of level l.  scratch: pcgc_pyramid_scratch_bytes(n, levels) device bytes, 16-byte aligned. */
size_t pcgc_pyramid_scratch_bytes(int64_t n, int levels);
int pcgc_pyramid(const int32_t* fine /*[dev n,4]*/, int64_t n, int32_t stride, int levels, void* scratch, size_t scratch_bytes,
                 int32_t* const* coarse, int32_t* const* parent_of, int32_t* const* down, int64_t* counts /*host*/, void* stream);
/* orig[prefix[i]] = i for set mask bytes (row indices that survive a compaction) */
int pcgc_compact_index(const uint8_t* mask, const int32_t* prefix, int64_t n, int32_t* orig /*[dev total]*/, void* stream);

/* ---- sparse convolution family ---- */
/* Gather convolution: MinkowskiConvolution k=3,s=1 (K=27), k=2,s=2 (K=8), k=1 (K=1, nbr may be NULL = identity)
 * (autoencoder.py:13-48,71-134,162-234).  W = ME `kernel` [K,Cin,Cout]; bias [Cout] or NULL;
 * residual (same row, columns res_coff..) or NULL (SparseTensor.__add__, autoencoder.py:55); relu = MinkowskiReLU. */
int pcgc_conv_gather(const int32_t* nbr, int K, int64_t n_out, const float* in, int64_t n_in /*rows of `in`*/, int Cin,
                     int in_ld, int in_coff, const float* W, const float* bias, const float* residual, int res_ld,
                     int res_coff, int relu, float* out, int Cout, int out_ld, int out_coff, void* stream);
/* Which kernel family the calling thread's last pcgc_conv_gather launched (0 v0 VALU | 1 v1 LDS-DMA + VALU | 2 v2 MFMA | 3 v2b MFMA with
 * LDS-shared weights, 2 M tiles | 4 v2b, 4 M tiles | 5 v1 burst | 6 row-split | 7 v2c MFMA, both operands in LDS; -1 none yet).  The policy
 * is written down once, in pcgcv2_amd/dispatch.py; the parity tests read this back for every entry of that table.  HOST. */
int pcgc_last_conv_impl(void);
/* kernel selection for the gather conv: -1 auto (default), 0 = v0 direct-load kernel, 1 = v1 LDS-DMA kernel, 2 / 3 = the fp32-MFMA
 * kernels, 5 / 6 = the 16-row "burst" and row-split forms that small levels get (each where eligible).  All produce bit-identical results; the
 * switch exists for A/B measurements and tests. */
/* The codec's first layer (Encoder.conv0, autoencoder.py:71-77) on its actual input, the all-ones single-channel occupancy indicator
 * (data_utils.py:104,114): out = relu?(sum over PRESENT offsets k, ascending, of W[k][0][:] + bias).  fmaf(1, w, acc) = acc + w exactly,
 * so this IS pcgc_conv_gather's chain on that input, without the 27 feature gathers per row.  W: [K, 1, Cout]. */
int pcgc_conv_gather_unit(const int32_t* nbr /*[dev K,n_out]*/, int K, int64_t n_out, const float* W, const float* bias, int relu,
                          float* out, int Cout, int out_ld, void* stream);
/* the same layer on a level whose own kernel map has not been built (a level of the encoder's strided pyramid): presence of every offset
 * is derived on the fly from the PARENT level's map + the level pair's down map + parent_of — what pcgc_kmap_k3_from_coarse would write —
 * so the finest level's [27][n] map, which only this layer reads, is never materialised. */
int pcgc_conv_unit_from_coarse(const int32_t* fine /*[n_fine,4]*/, int64_t n_fine, int32_t stride_fine, const int32_t* parent_of,
                               const int32_t* coarse_nbr /*[27,n_coarse]*/, const int32_t* down /*[8,n_coarse]*/, int64_t n_coarse,
                               const float* W /*[27,1,Cout]*/, const float* bias, int relu, float* out, int Cout, int out_ld, void* stream);
/* force a family of pcgc_conv_gather: -1 auto (default) | 0 VALU | 2 MFMA | 6 row-split (A/B tests; bit-identical) */
int pcgc_set_conv_impl(int impl);
/* generative transpose 64->32 / 32->16: 2 fp32-MFMA kernel with the weight fragments resident in LDS (default), 1 fragments read from L2, 0 VALU kernel.  Bit-identical. */
int pcgc_set_up2_impl(int mfma);
/* Fused InceptionResNet block (autoencoder.py:7-57):  out = cat(conv0_1(relu(conv0_0 x)), conv1_2(relu(conv1_1(relu(conv1_0 x))))) + x
 * in two gather passes.  params[10] = {conv0_0.kernel, .bias, conv0_1.kernel, .bias, conv1_0.kernel, .bias, conv1_1.kernel,
 * .bias, conv1_2.kernel, .bias} (ME layouts).  t_scratch: [n, C/2] fp32 workspace.  Bit-identical to the five
 * pcgc_conv_gather calls it replaces. */
int pcgc_irn_block(const int32_t* nbr /*[27,n]*/, int64_t n, const float* x /*[n,C], ld x_ld*/, int C, int x_ld,
                   const float* const* params, float* t_scratch, float* out, int out_ld, void* stream);
/* the two gather passes of pcgc_irn_block separately (pass 1 = A: x -> t_scratch, pass 2 = B: t_scratch, x -> out);
 * same arguments; used to time the passes individually. */
int pcgc_irn_pass(const int32_t* nbr, int64_t n, const float* x, int C, int x_ld, const float* const* params,
                  float* t_scratch, float* out, int out_ld, int pass, void* stream);
/* MinkowskiGenerativeConvolutionTranspose(k=2,s=2): out[8i+k] = in[i] @ W[k] + bias (+ReLU). */
int pcgc_conv_up2(int64_t n_in, const float* in, int Cin, int in_ld, const float* W /*[8,Cin,Cout]*/, const float* bias,
                  int relu, float* out /*[dev 8n,Cout]*/, int Cout, void* stream);
/* the same on a pruned level read in place (autoencoder.py:247 followed by :155-161 / :182-188 of the next stage): input row p = row rows[p]
 * of `in`, rows = the survivors' candidate rows (pcgc_topk_select's orig), so MinkowskiPruning's compacted feature tensor is never written.
 * Returns -3 (nothing launched, no error text) for shapes other than 64 -> 32 / 32 -> 16: gather the rows, then pcgc_conv_up2. */
int pcgc_conv_up2_gather(int64_t n_in, const float* in, int Cin, int in_ld, const int32_t* rows, const float* W /*[8,Cin,Cout]*/,
                         const float* bias, int relu, float* out /*[dev 8n,Cout]*/, int Cout, void* stream);

/* ---- k3 convolution on a CHILDREN level (the output level of a generative transpose: row 8p+j = child j of parent p) through
 *      the PARENT level's kernel map: each neighbour row is gathered once per 16-parent tile and feeds every child that
 *      reaches it (csrc/child.hip).  Replaces MinkowskiConvolution(k=3) at the decoder call sites autoencoder.py:162-168,
 *      189-195,216-222 (conv0/1/2 after up0/1/2).  `table` = the layer's `kernel` re-laid-out as MFMA B fragments
 *      [k][Cout/16][Cin/16][lane 64][4] (pcgcv2_amd/ops.py:child_conv_table).  Same canonical arithmetic. ---- */
int pcgc_conv_child(const int32_t* parent_nbr /*[dev 27,n_parent]*/, int64_t n_parent, const float* in /*[dev 8 n_parent rows]*/,
                    int Cin, int in_ld, const float* table /*[dev]*/, int64_t table_bytes,
                    const float* bias, const float* residual, int res_ld, int relu, float* out, int Cout, int out_ld, void* stream);
/* Cout == 1 (the classification heads conv0/1/2_cls, autoencoder.py:169-175,196-202,223-229) is served by the same entry with a
 * 64-fragment table (ops.child_cls_table): the 8 children are the 8 used columns of one accumulator tile. */
/* Fused InceptionResNet (autoencoder.py:52-57) on a children level, C = 16 or 32, as two parent-map passes:
 *   pass 1 (A): in = x [8 n_parent, C]      -> out = t [8 n_parent, C/2] = [relu(conv0_0 x + b0) | relu(conv1_0 x + b1)]
 *   pass 2 (B): in = t [8 n_parent, C/2]    -> out [.., C] = [conv0_1(t[:, :Q]) + b0 | conv1_2(relu(conv1_1(t[:, Q:]) + b1)) + b2] + x
 * The narrow layers pack (child, output channel) pairs into the MFMA N dimension; tables: ops.child_irn_tables. */
int pcgc_irn_child_pass(const int32_t* parent_nbr, int64_t n_parent, int C, int pass, const float* in, int in_ld,
                        const float* table, int64_t table_bytes, const float* b0, const float* b1, const float* b2,
                        const float* x, int x_ld, float* out, int out_ld, void* stream);
/* The same block at C = 16 with pass 1 (A) in QUAD-BLOCK form (round 5, csrc/child_q4.h): `v_mfma_f32_4x4x1_16b_f32`, one 4 x 4 block per
 * (4 parents, cell, child) — only the (cell, child) pairs that exist are issued, where the packed-N tiles of pcgc_irn_child_pass multiply
 * 44 % structural zero columns.  Replaces autoencoder.py:52-57 (InceptionResNet) on the level of autoencoder.py:209-237, bit for bit the
 * same chains.  pass 1: table = ops.child_q4_tables: [27][4 co][16 ci] = conv0_0.kernel, then [4 co][16 ci] = conv1_0.kernel (7168
 * bytes); it writes t in the T2 layout (per parent 256 bytes = [z half][conv0_0 | conv1_0][child & 3][4 channels]: a quad of lanes stores
 * 64 contiguous bytes).  pass 2: the packed-N pass B of pcgc_irn_child_pass gathering through the T2 layout (table =
 * ops.child_irn_tables()[1]).  The two passes of one block must come from the same entry point.  Arguments as pcgc_irn_child_pass. */
int pcgc_irn_child_q4(const int32_t* parent_nbr, int64_t n_parent, int C, int pass, const float* in, int in_ld,
                      const float* table, int64_t table_bytes, const float* b0, const float* b1, const float* b2,
                      const float* x, int x_ld, float* out, int out_ld, void* stream);
/* Classification head k3 16 -> 1 on a children level (autoencoder.py:228-234 conv2_cls) in quad-block form (csrc/child_q4.h): a 4 x 4
 * block = 4 parents x the four children of one z half; out [8 n_parent, 1] dense, a lane stores its parent's eight logits (32 bytes).
 * table = ops.child_q4_cls_table (96 fragments [4 children][16 ci], zero where a child does not reach the cell).  Same chain as
 * pcgc_conv_child with Cout = 1. */
int pcgc_cls_child_q4(const int32_t* parent_nbr, int64_t n_parent, const float* in, int Cin, int in_ld, const float* table,
                      int64_t table_bytes, const float* bias, float* out, void* stream);
/* The same two passes at C = 64 on a PLAIN level (the encoder's stride-4 level, autoencoder.py:104-110) through the level's own
 * k3 map nbr [27][n]: LDS-resident fragment table, one wave per 16-row tile walking the 27 offsets (csrc/rows_irn.hip); tables as
 * for the children-level C = 64 passes (ops.child_irn_tables). */
int pcgc_irn_rows_pass(const int32_t* nbr, int64_t n, int C, int pass, const float* in, int in_ld, const float* table,
                       int64_t table_bytes, const float* b0, const float* b1, const float* b2, const float* x, int x_ld, float* out,
                       int out_ld, void* stream);
/* The two passes at C = 32 on a plain level (the encoder's block0 / block2, autoencoder.py:85-89,123-127) in QUAD-BLOCK form
 * (csrc/q4x.h, csrc/rows_q4.hip: v_mfma_f32_4x4x1_16b_f32, lane = row, no zero column).  pass 1 (A): in = x [n, >= 32] -> out = t [n, 16]
 * dense; pass 2 (B): in = t -> out [n, >= 32] with the residual x.  tables = ops.rows_q4_tables(params): pass A 112 fragments [co 4][ci 16]
 * ordered [k (27 = conv1_0)][channel half][output group], pass B 83 ([k][conv0_1 outputs 0-7, 8-15, conv1_1 0-7], then conv1_2's two).
 * Same chain as pcgc_irn_rows_pass / pcgc_irn_block: bit-identical. */
int pcgc_irn_rows_q4_pass(const int32_t* nbr, int64_t n, int C, int pass, const float* in, int in_ld, const float* table,
                          int64_t table_bytes, const float* b0, const float* b1, const float* b2, const float* x, int x_ld, float* out,
                          int out_ld, void* stream);
/* A/B knob of that entry (tools/rows32_ab.py): 0 = the default instantiation (3); 1 = 8 waves x 2 M tiles x ring 2; 2 = 8 x 1 x 4 with paired
 * half-row gathers; 3 = pass A 16 x 1 x 2, pass B 12 x 1 x 2.  Results do not depend on it.  Replaces nothing in the reference. */
int pcgc_set_rows_q4_variant(int v);
/* Plain k3 conv 32 -> 32 on a plain level (the encoder's conv1, autoencoder.py:90-96) by the same kernel family: table =
 * ops.child_conv_table(kernel) (108 KB, LDS-resident); epilogue as pcgc_conv_gather. */
int pcgc_conv_rows(const int32_t* nbr, int64_t n, const float* in, int Cin, int in_ld, const float* table, int64_t table_bytes,
                   const float* bias, const float* residual, int res_ld, int relu, float* out, int Cout, int out_ld, void* stream);
/* k2 s2 down conv (the encoder's down0 / down1 / down2, autoencoder.py:78-84,97-103,116-122: 16 -> 32, 32 -> 64, 64 -> 32) by the same
 * kernel family: tile = 16 coarse rows, the 8 child offsets through the level pair's `down` map [8][n_coarse] (fine rows, -1 = absent);
 * table = ops.child_conv_table(kernel). */
int pcgc_conv_down_rows(const int32_t* down, int64_t n_coarse, const float* in, int64_t n_in, int Cin, int in_ld, const float* table,
                        int64_t table_bytes, const float* bias, int relu, float* out, int Cout, int out_ld, void* stream);

/* k3 conv 64 -> 64 (the encoder's conv2, autoencoder.py:109-115, and the decoder's conv0, :162-168 — the two layers whose 442 KB of weights
 * fit no LDS-resident table) with PRESENT-ROW PACKING: per 128-row workgroup tile and kernel offset only the rows that have the neighbour
 * are gathered and multiplied (packed 16 at a time; accumulators in LDS), instead of zero rows for absent neighbours.  nbr [27][n] of the
 * level itself (-1 = absent); table = ops.child_conv_table(kernel) (442 368 bytes); out = (acc + bias) (relu).  Same fmaf chain per
 * output element as pcgc_conv_gather: bit-identical results. */
int pcgc_conv_packed64(const int32_t* nbr, int64_t n, const float* in, int in_ld, const float* table, int64_t table_bytes,
                       const float* bias, int relu, float* out, int out_ld, void* stream);
/* A/B switch of pcgc_conv_packed64: rows per workgroup tile (an even value in 40 .. 128 — the sizes the per-launch choice can take, each of
 * them tested; 0 = chosen per launch from the level size); `waves` must be 0 or 4 (the eight-wave form was removed in round 5).  Anything
 * else returns -1 and changes nothing.  Results do not depend on it. */
int pcgc_set_packed_tuning(int rows, int waves);

/* Tile schedules (csrc/tile_sched.h) under test.  pcgc_set_sched_cus: the compute-unit count every launcher sizes its grid by — 0 = the
 * current device's own (the default), a positive value = that many (1: a persistent grid of 8 workgroups, so a few thousand rows reach a second
 * round; 1 << 20: one tile per wave); negative: -1, nothing changes.  Process-wide; results never depend on it.
 * pcgc_last_sched: out = (work units, workgroups, waves per workgroup) of this thread's most recent launch of a persistent tiled kernel
 * (the children-level and rows kernels, the LDS-table form of pcgc_conv_up2), recorded where the grid is computed; after
 * pcgc_conv_packed64: (tiles, workgroups, rows per workgroup R). */
int pcgc_set_sched_cus(int cus);
int pcgc_last_sched(int64_t out[3]);

/* ‡ conventions the reference's results depend on but its sources do not pin (un-vendored MinkowskiEngine / torch.topk on ME's row
 * order): what = 0: top-k tie rule, value 0 = the lower row wins (default), 1 = the higher row wins.  The dedup policy is an argument of
 * pcgc_hash_insert_policy; the kernel-offset order is a weight permutation done by the host (pcgcv2_amd/conventions.py). */
int pcgc_set_convention(int what, int value);

/* ---- top-k pruning mask: istopk (data_utils.py:77-89).  mask[i]=1 for the k largest logits;
 *      ties -> lower row index; -0.0 == +0.0. ---- */
size_t pcgc_topk_workspace_bytes(int64_t n);
int pcgc_topk_mask(const float* logits /*[dev n], stride ld*/, int ld, int64_t n, int64_t k, uint8_t* mask /*[dev n]*/,
                   void* workspace, size_t workspace_bytes, void* stream);
/* ---- batches (ME.utils.sparse_collate, data_utils.py:107: batch index in column 0; istopk loops over the items, :80-87).  Every
 *      level of a collated batch is the concatenation of its items' levels, so the per-item operators work on contiguous row
 *      segments: seg_rows[b] rows for item b (HOST arrays; workspace as for the largest segment). ---- */
int pcgc_topk_mask_segments(const float* logits, int ld, int nseg, const int64_t* seg_rows, const int64_t* seg_k, uint8_t* mask,
                            void* workspace, size_t workspace_bytes, void* stream);
/* ---- prune_voxel in one sweep (round 4): istopk (data_utils.py:77-89) + MinkowskiPruning (autoencoder.py:237,247) of a candidate level.
 *      After the radix passes one single-pass scan keeps, per segment b, the seg_k[b] largest logits of its seg_rows[b] rows (same tie rule
 *      and ‡ convention switch as pcgc_topk_mask) and writes the pruned level directly: out_coords [K,4] and orig [K] (the candidate row of
 *      every surviving row, ascending), K = sum of the clamped seg_k, plus a RANK BITMAP of the candidate level for the kernel-map
 *      derivation: bits = one bit per candidate row (row m = bit m & 7 of byte m >> 3; ((n + 63) / 64) * 8 bytes, 8-byte aligned),
 *      wprefix [(n + 63) / 64] = survivors before row 64 w.  The candidates' coordinates are either given (`coords` [n,4]) or — a children
 *      level, rows 8 i + j of a generative transpose that never materialised its coordinates — derived from `parent_coords` [n / 8, 4] at
 *      tensor stride `parent_stride` (exactly one of the two is non-NULL).  seg_rows / seg_k: HOST arrays. ---- */
size_t pcgc_topk_select_workspace_bytes(int64_t n);
int pcgc_topk_select(const float* logits /*[dev n], stride ld*/, int ld, int nseg, const int64_t* seg_rows, const int64_t* seg_k,
                     const int32_t* coords, const int32_t* parent_coords, int32_t parent_stride,
                     uint8_t* bits, int32_t* wprefix, int32_t* orig, int32_t* out_coords, void* workspace, size_t workspace_bytes, void* stream);
/* pcgc_kmap_k3_prune / _prune_parent through that rank bitmap instead of a byte mask + int32 prefix per candidate row */
int pcgc_kmap_k3_prune_sel(const int32_t* cand_nbr /*[27,n_cand]*/, int64_t n_cand, const uint8_t* bits, const int32_t* wprefix,
                           const int32_t* orig /*[n_out]*/, int64_t n_out, int32_t* nbr /*[dev 27,n_out]*/, void* stream);
int pcgc_kmap_k3_prune_parent_sel(const int32_t* parent_nbr /*[dev 27,n_parent]*/, int64_t n_parent, const uint8_t* bits, const int32_t* wprefix,
                                  const int32_t* orig, int64_t n_out, int32_t* nbr /*[dev 27,n_out]*/, void* stream);
/* out[r] = in[orig[r]]: rows of C floats (C % 4 == 0, leading dimension in_ld) — the surviving feature rows of a pruned level */
int pcgc_gather_rows_f32_ld(const float* in, int C, int in_ld, const int32_t* orig, int64_t n_out, float* out /*[n_out,C]*/, void* stream);
/* rows per batch item: counts[16] (device) <- histogram of coords[:, 0]. */
int pcgc_batch_counts(const int32_t* coords /*[dev n,4]*/, int64_t n, int32_t* counts /*[dev 16]*/, void* stream);

/* ---- canonical ordering: sort_spare_tensor / array2vector (data_utils.py:55-61,91-101; coder.py:97-99):
 *      perm = argsort of (z, y, x, batch) most-significant first. ---- */
size_t pcgc_sort_workspace_bytes(int64_t n);
int pcgc_sort_zyx(const int32_t* coords, int64_t n, int32_t* perm /*[dev n]*/, void* workspace, size_t workspace_bytes,
                  void* stream);
/* the same with the batch index MOST significant: the items of a batch stay contiguous, each in the (z, y, x) order it has when
 * coded alone */
int pcgc_sort_bzyx(const int32_t* coords, int64_t n, int32_t* perm /*[dev n]*/, void* workspace, size_t workspace_bytes, void* stream);
int pcgc_gather_rows_i32x4(const int32_t* in, const int32_t* perm, int64_t n, int32_t* out, void* stream);
int pcgc_gather_rows_f32(const float* in, int C, const int32_t* perm, int64_t n, float* out, void* stream);

/* ---- pointwise operators of the unfused ME-style graph: ME.MinkowskiReLU (autoencoder.py:50) and SparseTensor.__add__ (:55) on
 *      contiguous feature buffers (in place allowed: out == in / out == a).  The fused forward passes do not call them. ---- */
int pcgc_relu(const float* in, int64_t count, float* out, void* stream);
int pcgc_add(const float* a, const float* b, int64_t count, float* out, void* stream);

/* ---- factorized entropy bottleneck (entropy_model.py:82-196) ---- */
/* values = round_half_even(feats); minmax[0]=min, minmax[1]=max (fp32, -0 canonicalised to +0). */
int pcgc_round_minmax(const float* feats, int64_t count, float* minmax /*[dev 2]*/, void* stream);
/* sym = int16(round(feats) - min_v)  (entropy_model.py:161-163). */
int pcgc_symbolize(const float* feats, int64_t count, float min_v, int16_t* sym /*[dev count]*/, void* stream);
/* feats = float(sym) + min_v  (entropy_model.py:193-194). */
int pcgc_desymbolize(const int16_t* sym, int64_t count, float min_v, float* feats, void* stream);
/* the two calls above with the symbol range kept on the device: minmax[2] <- (min, max), sym <- int16(round(feats) - min).
 * The host fetches both with one copy and evaluates the CDF table itself (reference arithmetic, see
 * pcgcv2_amd/entropy_model.py:reference_table).
 * The symbols are only meaningful for a finite range of fewer than 32768 values (max - min + 1 < 32768: the int16 limit the reference
 * shares, entropy_model.py:151-176).  The kernels do not check it: a NaN / infinite latent shows as a non-finite min or max (NaN orders
 * beyond the infinity of its sign), and the CALLER must test the returned range before it uses the symbols (ops.quantize_symbols does). */
int pcgc_quantize_symbols(const float* feats, int64_t count, float* minmax /*[dev 2]*/, int16_t* sym /*[dev count]*/, void* stream);
/* per batch item (its own header range, coder.py:51-55): minmax [dev nseg,2], seg_rows [host nseg] rows of C channels each. */
int pcgc_quantize_symbols_segments(const float* feats, int C, int nseg, const int64_t* seg_rows, float* minmax, int16_t* sym, void* stream);
/* fused CDF table: _likelihood -> clamp(1e-9) -> cumsum -> clamp(1) -> torchac 16-bit normalisation
 * (entropy_model.py:112-149,165-170 + torchac ‡).  params: 352 fp32 packed matrices|biases|factors.
 * cdf_u16 [C, L+1], L = max_v-min_v+1.  cdf_f32 (optional, may be NULL) receives the fp32 cdf [C, L+1]. */
int pcgc_cdf_table(const float* params /*[dev 352]*/, int C, float min_v, float max_v, uint16_t* cdf_u16 /*[dev]*/,
                   float* cdf_f32 /*[dev] or NULL*/, void* stream);


/* ---- forward losses of the training graph (loss.py:8-40; csrc/loss.hip).  None of this is on the encode/decode path.  Sums are reduced in
 *      a fixed order without floating-point atomics (per-block fp64 partials in `workspace`, added by one block): bitwise reproducible.
 *      workspace: pcgc_loss_workspace_bytes(elements) bytes, 8-byte aligned; elements = n * C (likelihood, bits) or n (BCE). ---- */
size_t pcgc_loss_workspace_bytes(int64_t elements);
/* data_utils.isin (data_utils.py:63-75): mask[i] = 1 iff row i of coords (batch, x, y, z) is a key of the table pcgc_hash_insert filled
 * (cap = 0: the empty table), OR-ed with or_mask[i] when or_mask is given ("top-k | truth" of autoencoder.py:241-244 in one launch).
 * Not pcgc_hash_first_mask, which marks the first occurrence of a row within its OWN table. */
int pcgc_hash_contains(const int32_t* coords /*[dev n,4]*/, int64_t n, const uint64_t* keys, const int32_t* vals, int64_t cap,
                       const uint8_t* or_mask /*[dev n] or NULL*/, uint8_t* mask /*[dev n]*/, void* stream);
/* EntropyBottleneck._likelihood + Low_bound (entropy_model.py:112-140) at any real feats [n, C] (row stride ld): logits at v -+ 0.5, the
 * sign trick, |sigmoid - sigmoid| evaluated in fp64 exactly as pcgc_cdf_table evaluates a table entry, rounded once to fp32, then
 * max(., bound) (bound = 1e-9f in forward(); 0 = none).  likelihood [dev n,C] (may be NULL when only the bits are wanted);
 * bits [dev 1] (may be NULL) = -sum log2(likelihood) over the stored fp32 values, in fp64 (loss.get_bits). */
int pcgc_eb_likelihood(const float* feats, int ld, int64_t n, int C, const float* params /*[dev 44 C]*/, float bound, float* likelihood,
                       double* bits, void* workspace, size_t workspace_bytes, void* stream);
/* loss.get_bits of a likelihood tensor x [n, C] (row stride ld): -sum log2(x) in fp64; the same double pcgc_eb_likelihood returns for it */
int pcgc_neg_log2_sum(const float* x, int ld, int64_t n, int C, double* bits /*[dev 1]*/, void* workspace, size_t workspace_bytes, void* stream);
/* loss.get_bce + the counts of loss.get_cls_metrics in one pass: bce [dev 1] = sum_i (max(x,0) - x y + log1p(exp(-|x|))) / ln 2 over
 * logits x [n] (row stride ld; NULL: counts only, bce = 0) and the truth mask y; counts [dev 4] = TP, FN, FP, TN of (pred, truth)
 * (pred = NULL counts as all zero). */
int pcgc_bce_logits(const float* logits, int64_t ld, int64_t n, const uint8_t* truth /*[dev n]*/, const uint8_t* pred /*[dev n] or NULL*/,
                    double* bce, int64_t* counts, void* workspace, size_t workspace_bytes, void* stream);

/* ---- lossless mode (lossless.py; csrc/occupancy.hip): what the host coder of the occupancy stream `_O.bin` reads, from a level's logits.
 *      packed[i] = ctx << 1 | bit with ctx = clamp(rint(16 z_i), -176, 176) + 176 (ties to even, +-inf clamp, NaN -> 176) and bit = truth[i] != 0;
 *      sums [dev 2] = occupied rows, sum of COST[ctx][bit] in units of 2^-16 bit (integers; per-block partials in `workspace`, added by one
 *      block; the grid is a function of n alone).  truth = sums = NULL (the decoder's side): contexts only, bit 0, no workspace.
 *      logits [dev n] with row stride ld; workspace: pcgc_occ_workspace_bytes(n) bytes, 8-byte aligned. ---- */
size_t pcgc_occ_workspace_bytes(int64_t n);
int pcgc_occ_symbols(const float* logits, int64_t ld, int64_t n, const uint8_t* truth /*[dev n] or NULL*/, uint16_t* packed /*[dev n]*/,
                     int64_t* sums /*[dev 2] or NULL*/, void* workspace, size_t workspace_bytes, void* stream);
/* the same pass over the nseg (1 .. 16) contiguous frames of a batch's level: frame f is the next seg_rows[f] rows (seg_rows [host nseg]; a
 * frame may be empty).  packed is what pcgc_occ_symbols writes for the whole level; sums [dev nseg][2] = every frame's pair, each equal to
 * pcgc_occ_symbols of that frame alone (integer adds: exact in any order; no workspace).  truth = sums = NULL: contexts only. */
int pcgc_occ_symbols_segments(const float* logits, int64_t ld, int nseg, const int64_t* seg_rows /*[host nseg]*/, const uint8_t* truth /*[dev n] or NULL*/,
                              uint16_t* packed /*[dev n]*/, int64_t* sums /*[dev nseg,2] or NULL*/, void* stream);
/* the library's copy of the format tables: P1 uint16 [353], COST int32 [353][2] (either may be NULL) -> number of contexts.  HOST. */
int pcgc_occ_tables(uint16_t* p1, int32_t* cost);

/* ---- lossless mode, `_O.bin` version 2 (csrc/occupancy_rans.hip): the same bits coded ON THE DEVICE by interleaved rANS.  One wave per
 *      chunk of 64 S rows; 64 independent states, one per lane, share one stream of 32-bit words.  A level's payload, little endian:
 *          u32 S             steps per chunk, 1 .. 2^24
 *          u32 K             chunks = ceil(rows / (64 S))  (rows = 0: K = 0)
 *          K x 64 x u64      the decoder's initial state of every lane, chunk by chunk, lane 0 .. 63
 *          K x u32           W_k: 32-bit words of chunk k
 *          u32 words         chunk 0's W_0 words, then chunk 1's, ...
 *      Chunk k covers rows [64 S k, min(rows, 64 S (k + 1))); lane j codes rows base + 64 t + j, t = 0 .. S - 1.  64-bit state, L = 2^31,
 *      probabilities straight from P1: bit b under ctx has f = b ? P1 : 65536 - P1, c = b ? 65536 - P1 : 0.
 *      Encoder, per chunk: every lane starts at x = L; steps t = S - 1 .. 0, lanes j = 63 .. 0 within a step, rows past the end skipped; at a
 *      row: if x >= f << 47, emit x & 0xffffffff and x >>= 32; then x = ((x / f) << 16) + x % f + c.  The stream is the emitted words in
 *      reverse order; the final x of each lane is its stored state (a lane without rows stores L).
 *      Decoder, per chunk: steps t = 0 .. S - 1, lanes j = 0 .. 63; at a row: s = x & 0xffff, b = s >= 65536 - P1, x = f (x >> 16) + s - c;
 *      if x < L, x = x << 32 | next word (within a step, words go to the renormalising lanes in ascending lane order).  A chunk is sound
 *      iff every stored state is in [2^31, 2^63), exactly W_k words were consumed and every lane ends at x == L; a word index at or past
 *      W_k reads as 0 and marks the chunk unsound.  The decoder reads nothing outside a chunk's words, whatever the bytes say.
 *      rows < 2^31.  workspace: pcgc_occ_rans_workspace_bytes(n, steps) = pcgc_occ_rans_batch_workspace_bytes(n, K) device bytes, 8-byte
 *      aligned (no allocation inside): the single entries are the batch of one on the batch's slot layout.  The decoder uses its first
 *      384 + 8 ceil(K / 2) bytes only and accepts as little (it accepted 32 + 8 ceil(K / 2) while the single entries had a slot layout of
 *      their own).  The coder's shared parts are csrc/rans_core.h. ---- */
size_t pcgc_occ_rans_workspace_bytes(int64_t n, int steps);
/* packed [dev n] as pcgc_occ_symbols writes it -> payload [dev, 8-byte aligned, capacity >= 8 + 516 K + 4 n bytes] in the layout above;
 * host3 [host 3] = the payload's length in bytes and, when sums (pcgc_occ_symbols' [dev 2]) is given, sums[0] and sums[1]: ONE small
 * synchronising copy.  The caller then copies the finished payload. */
int pcgc_occ_rans_encode(const uint16_t* packed /*[dev n]*/, int64_t n, int steps, const int64_t* sums /*[dev 2] or NULL*/, uint8_t* payload,
                         size_t payload_capacity, int64_t* host3, void* workspace, size_t workspace_bytes, void* stream);
/* packed [dev n]: the contexts (bit 0 is ignored: pcgc_occ_symbols with truth = NULL); payload [dev, 8-byte aligned] of payload_bytes bytes
 * whose head the caller has read: steps = its S, and its K, the table sizes and the sum of W_k agree with n and payload_bytes
 * (ops.occ_rans_decode checks them on the host; here K follows from n and steps, and no access leaves the payload in any case)
 * -> mask [dev n] (0 empty, 1 occupied); host2 [host 2] = occupied rows, unsound chunks (0: the payload is sound), in one small copy. */
int pcgc_occ_rans_decode(const uint16_t* packed /*[dev n]*/, int64_t n, const uint8_t* payload, int64_t payload_bytes, int steps,
                         uint8_t* mask /*[dev n]*/, int64_t* host2, void* workspace, size_t workspace_bytes, void* stream);
/* A batch of 1 .. 16 frames (the items of a collated batch at one decoder level) in ONE launch sequence.  Frame f is rows
 * row[f] .. row[f + 1] of packed and of mask (row [host frames + 1], ascending from 0, below 2^31; any row counts, a frame may be empty) and
 * is cut into K_f = ceil(rows_f / (64 steps[f])) chunks from its own first row: chunks never straddle frames, the launch has sum K_f
 * single-wave workgroups.  Its payload is exactly the layout above — what pcgc_occ_rans_encode writes for that frame alone at steps[f] — at
 * byte pay[f] (a multiple of 8) of the payload buffer; a frame without rows has the 8-byte head S | 0.  The single entries run the same
 * kernels and host bodies at frames = 1.  workspace: pcgc_occ_rans_batch_workspace_bytes(n, sum K_f) device bytes, 8-byte aligned; the
 * decoder uses its first 384 + 8 ceil(K / 2) bytes only and accepts as little.  Every entry refuses (-2) before anything is launched. */
int64_t pcgc_occ_rans_batch_workspace_bytes(int64_t n, int64_t chunks);
/* steps [host frames] in 1 .. 2^24; pay [host frames + 1]: frame f's room pay[f + 1] - pay[f] >= 8 + 516 K_f + 4 rows_f; sums: NULL or
 * pcgc_occ_symbols_segments' [dev frames,2].  host [host 3 frames] = every frame's payload bytes, then every frame's sums[0], then every
 * frame's sums[1] (0 without sums): ONE small synchronising copy.  The finished payloads stay on the device for the caller to fetch. */
int pcgc_occ_rans_encode_batch(const uint16_t* packed /*[dev n]*/, int frames, const int64_t* row, const int32_t* steps, const int64_t* sums,
                               uint8_t* payload, const int64_t* pay, int64_t* host, void* workspace, size_t workspace_bytes, void* stream);
/* steps [host frames]: the S of the frame's head, or 0 for a frame that is not decoded here (its slice of mask is left alone and pay /
 * pay_bytes of it are not read); pay_bytes [host frames]: the frame's payload bytes, whose head and lengths the caller has checked as for
 * pcgc_occ_rans_decode.  No access leaves a frame's own payload, whatever its bytes say.  host [host 2 frames] = every frame's occupied
 * rows, then every frame's unsound chunks (0: sound), in one small copy. */
int pcgc_occ_rans_decode_batch(const uint16_t* packed /*[dev n]*/, int frames, const int64_t* row, const int32_t* steps, const uint8_t* payload,
                               const int64_t* pay, const int64_t* pay_bytes, uint8_t* mask /*[dev n]*/, int64_t* host, void* workspace,
                               size_t workspace_bytes, void* stream);

/* ---- backward pass of the training graph (trainer.py:127-134 `sum_loss.backward()`; csrc/grad.hip).  None of this is on the encode/decode
 *      path.  No floating-point atomics: every reduction has a fixed order (per-workgroup partials in `workspace`, added in ascending
 *      workgroup order by a second stage) and every grid is a function of the shapes alone, so gradients are bitwise reproducible.
 *      The INPUT gradient of a convolution is a forward gather convolution (pcgc_conv_gather, Cout -> Cin) through a transposed map:
 *      k3 on one level: the same map with W'[k] = W[26 - k]^T (the map is its own transpose under k <-> 26 - k, in both offset orders);
 *      k2 s2 down / generative up: pcgc_kmap_invert of the forward map (up on an unpruned level: inv[j][p] = 8 p + j) with W[k]^T. ---- */
/* Weight gradient of MinkowskiConvolution (k3 / k1 / k2 s2) through its forward map nbr [K, n_out] (NULL: identity, K = 1):
 *   gW[k][a][b] = sum over present pairs o of x[nbr[k][o]][a] * gy[o][b]   [K, Cin, Cout];   gb[b] = sum_o gy[o][b] (NULL: not wanted).
 * x [n_in rows, ld x_ld], gy [n_out rows, ld gy_ld] (column slices allowed), 1 <= Cin, Cout <= 64.  fp32 MFMA (v_mfma_f32_16x16x4_f32) with
 * the gathered, transposed x rows as the A operand; channel counts below 16 run in a zero-padded tile.  workspace: 4-byte aligned,
 * pcgc_conv_wgrad_workspace_bytes(K, n_out, Cin, Cout) bytes; a workgroup covers pcgc_conv_wgrad_rows_per_group(..) consecutive rows. */
size_t pcgc_conv_wgrad_workspace_bytes(int K, int64_t n_rows, int Cin, int Cout);
int64_t pcgc_conv_wgrad_rows_per_group(int K, int64_t n_rows, int Cin, int Cout);
int pcgc_conv_wgrad(const int32_t* nbr, int K, int64_t n_out, const float* x, int64_t n_in, int Cin, int x_ld, const float* gy, int Cout,
                    int gy_ld, float* gW, float* gb, void* workspace, size_t workspace_bytes, void* stream);
/* The same for MinkowskiGenerativeConvolutionTranspose(k=2,s=2): gW[j][a][b] = sum_p x[p][a] * gy[8 p + j][b], gb[b] = sum over all 8 n_in rows
 * of gy.  rows (or NULL): input row p is row rows[p] of x (a pruned level read in place, as pcgc_conv_up2_gather reads it); x has x_rows rows.
 * workspace: pcgc_conv_wgrad_workspace_bytes(8, n_in, Cin, Cout). */
int pcgc_conv_up2_wgrad(int64_t n_in, const float* x, int64_t x_rows, int Cin, int x_ld, const int32_t* rows, const float* gy, int Cout,
                        int gy_ld, float* gW, float* gb, void* workspace, size_t workspace_bytes, void* stream);
/* inv [K, n_in]: inv[k][nbr[k][o]] = o for every present pair of nbr [K, n_out], -1 elsewhere.  For a fixed k the map o -> nbr[k][o] must be
 * injective (true for k3, k2 s2 down and generative-up maps). */
int pcgc_kmap_invert(const int32_t* nbr, int K, int64_t n_out, int64_t n_in, int32_t* inv /*[dev K,n_in]*/, void* stream);
/* adjoint of MinkowskiReLU: out = g where y > 0 (y = the ReLU's output or input), else 0; [n, C] views with leading dimensions */
int pcgc_relu_bwd(const float* g, int g_ld, const float* y, int y_ld, int64_t n, int C, float* out, int out_ld, void* stream);
/* adjoint of a row gather (pcgc_gather_rows_f32_ld / pcgc_compact_feats): gx [n_out, C] (ld gx_ld) = 0, then gx[orig[r]] = gy[r], r < n_rows;
 * orig holds distinct rows */
int pcgc_scatter_rows(const float* gy, int C, int gy_ld, const int32_t* orig, int64_t n_rows, float* gx, int64_t n_out, int gx_ld, void* stream);
/* gradient of pcgc_bce_logits' bce with respect to the logits: g[i] = scale * (sigmoid(z_i) - t_i) / ln 2 (fp64, rounded once); g [n] dense */
int pcgc_bce_logits_bwd(const float* logits, int64_t ld, int64_t n, const uint8_t* truth, double scale, float* g /*[dev n]*/, void* stream);
/* gradient of pcgc_eb_likelihood's bits (= -sum log2 max(likelihood, bound)), times `scale`: gy [n, C] dense = d bits / d feats and gparams
 * [44 C] in the packing of `params` (through softplus of the matrices and tanh of the factors; the sign of entropy_model.py:124 is a
 * constant; an element whose likelihood is below the bound contributes zero: Low_bound.backward, entropy_model.py:27-39).  fp64 throughout,
 * parameter sums reduced in fp64 in a fixed order, one rounding.  workspace: 8-byte aligned, pcgc_eb_bwd_workspace_bytes(n, C). */
size_t pcgc_eb_bwd_workspace_bytes(int64_t n, int C);
int pcgc_eb_likelihood_bwd(const float* feats, int ld, int64_t n, int C, const float* params /*[dev 44 C]*/, float bound, double scale,
                           float* gy, float* gparams, void* workspace, size_t workspace_bytes, void* stream);

/* ---- range coder, bit-compatible with torchac 0.9.3 ‡ encode_float_cdf / decode_float_cdf
 *      (entropy_model.py:174,192).  HOST functions; symbols row-major [point, channel], one CDF row per channel. ---- */
int64_t pcgc_rc_encode(const uint16_t* cdf /*[host C,Lp]*/, int C, int Lp, const int16_t* sym /*[host n]*/, int64_t n,
                       uint8_t* out /*[host cap]*/, int64_t cap);          /* returns bytes, or -needed if cap too small */
int pcgc_rc_decode(const uint16_t* cdf, int C, int Lp, const uint8_t* in, int64_t nbytes, int16_t* sym, int64_t n);
/* The same stream plus a decoding index.  A range-coded stream is sequential, but only because the decoder state at a later symbol is
 * unknown: pcgc_rc_encode_indexed also returns that state — (first symbol, bit position, low, span - 1, value - low), PCGC_RC_CKPT_WORDS
 * uint32 each — at n_ckpt evenly spread row boundaries, and pcgc_rc_decode_indexed decodes the segments in between on several threads
 * (pcgc_set_rc_threads; 0 = min(8, hardware threads)).  `_F.bin` is bit-identical with or without the index and decodes without it
 * (pcgc_rc_decode, torchac); the host side stores the index in a sidecar file next to it (`_F.idx`, coder.py). */
#define PCGC_RC_CKPT_WORDS 6
int64_t pcgc_rc_encode_indexed(const uint16_t* cdf, int C, int Lp, const int16_t* sym, int64_t n, uint8_t* out, int64_t cap, int n_ckpt,
                               uint32_t* ckpt /*[host n_ckpt][PCGC_RC_CKPT_WORDS]; unused entries have first symbol 0xFFFFFFFF*/);
int pcgc_rc_decode_indexed(const uint16_t* cdf, int C, int Lp, const uint8_t* in, int64_t nbytes, int16_t* sym, int64_t n, int n_ckpt,
                           const uint32_t* ckpt);
/* The same coder with the CDF row chosen per symbol: row ctx[i] of cdf [host R, Lp] instead of row i % C (the occupancy stream of the
 * lossless mode).  With ctx[i] = i % R the bytes are pcgc_rc_encode's.  encode: bytes, -needed if cap is too small, INT64_MIN for a
 * symbol or context outside the table.  decode: 0; -2 bad arguments; -3 when `in` is not exactly the stream the encoder writes for the
 * symbols it decodes to — a cut, extended or damaged stream (the decoded symbols are coded again and compared).  Never reads past nbytes. */
int64_t pcgc_rc_encode_ctx(const uint16_t* cdf /*[host R,Lp]*/, int R, int Lp, const uint16_t* ctx /*[host n]*/, const int16_t* sym /*[host n]*/,
                           int64_t n, uint8_t* out /*[host cap]*/, int64_t cap);
int pcgc_rc_decode_ctx(const uint16_t* cdf, int R, int Lp, const uint16_t* ctx /*[host n]*/, const uint8_t* in, int64_t nbytes,
                       int16_t* sym /*[host n]*/, int64_t n);
int pcgc_set_rc_threads(int threads);
/* The lane-parallel form of the indexed decoder: eight segments per 512-bit register on the calling thread (AVX-512 F/BW/DQ/CD/VL) instead
 * of one or two segments per pool thread.  -1 (default): when the thread budget (pcgc_set_rc_threads) is one or two; 0 never; 1 always.
 * Same symbols either way.  HOST. */
int pcgc_set_rc_lanes(int mode);
/* decoder selection for A/B tests: 0 automatic (AVX-512 boundary count when the host CPU has it and Lp <= 64, else the
 * portable scalar search), 1 portable scalar.  Both are bit-identical. */
int pcgc_set_rc_impl(int impl);

/* ---- native lossless coordinate codec for _C.bin when the external tmc3 binary (gpcc.py:6-41) is absent.
 *      Occupancy-octree + adaptive range coder.  NOT interoperable with G-PCC; flagged by its magic "PCGO". HOST. ---- */
int64_t pcgc_oct_encode(const int32_t* xyz /*[host n,3]*/, int64_t n, uint8_t* out, int64_t cap);   /* bytes or -needed */
int64_t pcgc_oct_decode_count(const uint8_t* in, int64_t nbytes);                                   /* points or <0 */
int pcgc_oct_decode(const uint8_t* in, int64_t nbytes, int32_t* xyz /*[host n,3]*/, int64_t n);
/* clouds of >= 8192 points are coded as up to 8 independent groups of subtrees (stream version 3), encoded and decoded side by side on
 * the threads of pcgc_set_rc_threads; 0 = always the single-stream form (version 2); n > 1 = that many groups (A/B tests).  The
 * decoder reads both versions. */
int pcgc_set_oct_tiled(int on);
/* Context model the ENCODER uses (the decoder reads every version): 1 (default, round 5) = stream versions 4 / 5 — every stream starts from
 * contexts trained on a mix of integer-defined shapes (sphere, ellipsoid, tilted plane, ragged noisy shell: none of them a bench cloud) and
 * a context adapts fast on its first visits; 0 = the round-3 versions 2 / 3 (p = 1/2 / sphere-trained prior), kept so that files written
 * by earlier builds stay covered by the format tests.  Replaces nothing in the reference (gpcc.py:6-41 hands `_C.bin` to tmc3). */
int pcgc_set_oct_model(int model);
/* Builds the octree coder's trained priors now rather than inside the first encode / decode call of the process (a cold decoder's first
 * frame would pay tens of milliseconds).  Idempotent and thread-safe; pcgcv2_amd.Coder calls it at construction.  (pcgc_set_oct_model /
 * pcgc_set_oct_tiled are process-wide A/B and test knobs, not per-call options.)  Replaces nothing in the reference (gpcc.py:6-41). */
int pcgc_oct_warm(void);

/* ---- D1 point-to-point distortion (pc_error.py:27-74 -> mpeg-pcc-dmetric ‡): sum and max over A of the squared distance to
 *      the nearest point of B, B given by its coordinate hash (stride 1).  offsets: int32 [n,4] = (dx,dy,dz,d2) sorted by d2. ---- */
int pcgc_d1_nn(const int32_t* a /*[dev na,4]*/, int64_t na, const uint64_t* b_keys, const int32_t* b_vals, int64_t b_cap,
               const int32_t* offsets /*[dev n_offsets,4]*/, int n_offsets, double* sum /*[dev 1]*/, uint64_t* max_d2 /*[dev 1]*/,
               int32_t* unresolved /*[dev 1]*/, void* stream);
/* The same sums through 4 x 4 x 4 cells of cloud B: cell_keys / cell_vals = coordinate hash of B's stride-4 level (vals = row), masks [n_cells] =
 * 64-bit voxel occupancy per cell (pcgc_d1_cell_masks fills it: bit x & 3 | (y & 3) << 2 | (z & 3) << 4); offsets [n,4] = cell offsets (x, y, z) +
 * the lower bound of the squared distance to any voxel of that cell, ascending; reach2 = squared distance from which a voxel outside the offset
 * table could be nearer (such points count as unresolved).  A few dozen probes per point whatever the distance. */
int pcgc_d1_cell_masks(const int32_t* b /*[dev nb,4]*/, int64_t nb, const uint64_t* cell_keys, const int32_t* cell_vals, int64_t cell_cap,
                       uint64_t* masks /*[dev n_cells]*/, int64_t n_cells, void* stream);
int pcgc_d1_nn_cells(const int32_t* a /*[dev na,4]*/, int64_t na, const uint64_t* cell_keys, const int32_t* cell_vals, int64_t cell_cap,
                     const uint64_t* masks, const int32_t* offsets /*[dev n,4]*/, int n_offsets, int32_t reach2, double* sum, uint64_t* max_d2,
                     int32_t* unresolved, void* stream);

/* ---- D2 point-to-plane distortion (pc_error.py:27-74 with normal=True, as the reference's test.py:74-75 asks for it -> mpeg-pcc-dmetric ‡
 *      with `-n infile1`; semantics of pc_error.d2_psnr, restated by oracle/pcgc_oracle.py:d2_metrics).  csrc/metric.hip.
 *      A searched cloud Q is given by its rows sorted with pcgc_sort_bzyx (qs [nq,4], perm = original row of each sorted row), runlen
 *      (pcgc_d2_runs), the coordinate hash of qs (keys / vals, stride 1: vals = first sorted row of a voxel) and the stride-4 cells of qs
 *      (cell_keys / cell_vals / masks exactly as for pcgc_d1_nn_cells).  Tie sets are ORIGINAL rows of Q; all buffers caller-owned, on `stream`. */
/* run length of the equal rows starting at each sorted row (0 where a run does not start) */
int pcgc_d2_runs(const int32_t* qs /*[dev nq,4]*/, int64_t nq, int32_t* runlen /*[dev nq]*/, void* stream);
/* per query point p[sel[t]] (sel = NULL: every point, n = rows of p): best = nearest squared distance, cnt = rows of Q at it (duplicates
 * included).  The walk stops only at a bound ABOVE the best distance; a point whose best is not below reach2 (a nearer or tied row could lie
 * outside the offset table) gets best = INT64_MAX, cnt = 0 and is appended to unresolved (n_unresolved is zeroed first). */
int pcgc_d2_count(const int32_t* p /*[dev np,4]*/, int64_t n, const int32_t* sel, const uint64_t* cell_keys, const int32_t* cell_vals,
                  int64_t cell_cap, const uint64_t* masks, const uint64_t* keys, const int32_t* vals, int64_t cap, const int32_t* runlen,
                  const int32_t* offsets /*[dev n_offsets,4]*/, int n_offsets, int32_t reach2, int64_t* best /*[dev np]*/, int32_t* cnt /*[dev np]*/,
                  int32_t* unresolved /*[dev n]*/, int32_t* n_unresolved /*[dev 1]*/, void* stream);
/* the tie rows of every listed point whose best is below reach2 into rows[seg[i] .. seg[i+1]) (other points are left to another table) */
int pcgc_d2_fill(const int32_t* p, int64_t n, const int32_t* sel, const uint64_t* cell_keys, const int32_t* cell_vals, int64_t cell_cap,
                 const uint64_t* masks, const uint64_t* keys, const int32_t* vals, int64_t cap, const int32_t* runlen, const int32_t* perm,
                 const int32_t* offsets, int n_offsets, int32_t reach2, const int64_t* best, const int64_t* seg /*[dev np+1]*/, int32_t* rows, void* stream);
/* the exhaustive finish of listed points: every row of qs with the point's batch.  fill = 0: best / cnt (n_empty counts points whose batch
 * has no row in Q); fill = 1: the tie rows into their segments. */
int pcgc_d2_exhaustive(const int32_t* p, int64_t n, const int32_t* sel, const int32_t* qs, int64_t nq, const int32_t* perm, int fill,
                       int64_t* best, int32_t* cnt, const int64_t* seg, int32_t* rows, int32_t* n_empty /*[dev 1]*/, void* stream);
/* seg[0] = 0, seg[i+1] = cnt[0] + ... + cnt[i] (int64) */
size_t pcgc_d2_scan_workspace_bytes(int64_t n);
int pcgc_d2_scan(const int32_t* cnt /*[dev n]*/, int64_t n, int64_t* seg /*[dev n+1]*/, void* workspace, size_t workspace_bytes, void* stream);
/* per segment: its `cap` lowest values in ascending order at its head; kept (optional) [n] = min(size, cap) */
int pcgc_d2_segment_lowest(const int64_t* seg, int64_t n, int32_t* rows, int32_t cap, int32_t* kept, void* stream);
/* the reverse relation of the kept A -> B tie sets: rcnt [nb] = A-points holding b (zeroed first); after pcgc_d2_scan(rcnt) -> rseg, recv holds
 * the A rows of each b (cursor [nb] is scratch; order them with pcgc_d2_segment_lowest) */
int pcgc_d2_recv_count(const int64_t* seg, const int32_t* kept, int64_t na, const int32_t* rows, int64_t nb, int32_t* rcnt, void* stream);
int pcgc_d2_recv_fill(const int64_t* seg, const int32_t* kept, int64_t na, const int32_t* rows, int64_t nb, const int64_t* rseg, int32_t* cursor,
                      int32_t* recv, void* stream);
/* normals of B (scaleNormals): mean of the received normals of A summed in ascending A row in fp64, or, none received, the mean normal of
 * b's kept B -> A tie set.  na, nb_out: double [n,3]. */
int pcgc_d2_normals(const int64_t* rseg, const int32_t* recv, int64_t nb, const double* na, const int64_t* seg_ba, const int32_t* kept_ba,
                    const int32_t* rows_ba, double* nb_out, void* stream);
/* c2p [np] (double) = mean over p's kept tie set of ((p - q) . n_q)^2, q the original rows of Q [nq,4], nq normals double [nq,3] */
int pcgc_d2_c2p(const int32_t* p, int64_t n, const int32_t* q, const double* nq, const int64_t* seg, const int32_t* kept, const int32_t* rows,
                double* c2p, void* stream);
/* c2c_sum_max [2] = (sum, max) of c2c [n] (int64), c2p_sum [1] = sum of c2p [n]: fixed summation order (a function of n only) */
size_t pcgc_d2_reduce_workspace_bytes(void);
int pcgc_d2_reduce(const int64_t* c2c, const double* c2p, int64_t n, int64_t* c2c_sum_max, double* c2p_sum, void* workspace, size_t workspace_bytes,
                   void* stream);

/* ---- Per-point attributes (colours) between two clouds (csrc/colour.hip).  Tie sets are the kept ones of pcgc_d2_fill +
 *      pcgc_d2_segment_lowest: seg [n+1], kept [n], rows.  Integer arithmetic throughout: exact, bitwise reproducible, independent of the
 *      order of atomics and of the row order of the source (as long as no tie set exceeds its cap). */
/* attr_t [nt,C] (uint8, C = 1 .. 4) from attr_s [ns,C]: (st) = tie sets of S in T, (ts) = tie sets of T in S.  R(t) = the sources whose tie
 * set holds t; attr(t) = (2 sum + |R|) / (2 |R|) per channel over R(t) (the mean rounded half up), over t's own tie set when R(t) is empty.
 * Accumulators are 32-bit fields: ns above 16 843 009 (255 ns >= 2^32) is refused with -2, never wrapped; C outside 1 .. 4 is -2. */
size_t pcgc_attr_transfer_workspace_bytes(int64_t ns, int64_t nt, int channels);
int pcgc_attr_transfer(const int64_t* seg_st, const int32_t* kept_st, const int32_t* rows_st, int64_t ns, const int64_t* seg_ts,
                       const int32_t* kept_ts, const int32_t* rows_ts, int64_t nt, const uint8_t* attr_s, int channels, uint8_t* attr_t,
                       void* workspace, size_t workspace_bytes, void* stream);
/* per point i of P (colours cp uint8 [n,3]) against the rounded mean colour of its kept tie set in Q (cq uint8 [nq,3]), d = own - mean:
 * yuv2 [n,3] (int64) = (2126 dr + 7152 dg + 722 db)^2, (-1146 dr - 3854 dg + 5000 db)^2, (5000 dr - 4542 dg - 458 db)^2 — the squared BT.709
 * differences times (255 * 10^4)^2; rgb2 [n,3] (int32) = dr^2, dg^2, db^2 */
int pcgc_colour_dist(const uint8_t* cp, int64_t n, const uint8_t* cq, int64_t nq, const int64_t* seg, const int32_t* kept, const int32_t* rows,
                     int64_t* yuv2, int32_t* rgb2, void* stream);
/* out [9] (int64): sums over i of the low 32 bits of yuv2[i][k] (k = 0..2), of the high 32 bits (3..5): total_k = out[3+k] * 2^32 + out[k],
 * exact for n < 2^31; maxima of rgb2[i][k] (6..8).  The grid is a function of n only. */
size_t pcgc_colour_reduce_workspace_bytes(void);
int pcgc_colour_reduce(const int64_t* yuv2, const int32_t* rgb2, int64_t n, int64_t* out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- Colour transform of the attribute stream `_A.bin` (csrc/raht.hip; the definition is tests/raht_reference.py): integer
 *      lifting RAHT on YCoCg-R over the binary radix tree of the Morton keys.  n = 1 .. 2^24 rows of ONE frame, distinct voxels.  Integer
 *      arithmetic throughout: every output is exact and the same on every run.  A gap i (0 .. n-2) lies between sorted leaves i and i + 1
 *      and is one merge of the tree.  Buffers are the caller's; everything runs on `stream`. */
/* leaves per workgroup of the tile form (form 1) of pcgc_raht_forward / pcgc_raht_inverse */
int64_t pcgc_raht_tile_leaves(void);
/* keys [n] (uint64): Morton keys (bit 3 i + 0 / 1 / 2 = bit i of x / y / z; columns 1 .. 3 of coords [n,4]) in ascending order;
 * perm [n]: sorted leaf i is row perm[i]; status [2] (dev): the number of adjacent equal keys (duplicate voxels), and bit 0 = a coordinate
 * outside [0, 2^20), bit 1 = a non-zero batch column.  The caller refuses the cloud when either is non-zero.  n > 2^24 is -2 before
 * anything is touched. */
size_t pcgc_raht_keys_workspace_bytes(int64_t n);
int pcgc_raht_keys(const int32_t* coords, int64_t n, uint64_t* keys, int32_t* perm, int32_t* status, void* workspace, size_t workspace_bytes,
                   void* stream);
/* per gap: d (uint8) = msb(key_i ^ key_{i+1}); [lo, hi] = the leaves of the merged node (w1 = i - lo + 1, w2 = hi - i); left / right = its
 * children, a gap index, or ~leaf for a leaf.  order [n-1]: the gaps in coding order (d descending, gap ascending); cross_order [n-1]:
 * first the gaps whose range crosses a multiple of pcgc_raht_tile_leaves(), in coding order, then the others.  offsets [130] (dev):
 * bucket [65] then cross [65]; the gaps of split bit d are order[bucket[63 - d] .. bucket[64 - d]), likewise cross_order and cross. */
size_t pcgc_raht_tree_workspace_bytes(int64_t n);
int pcgc_raht_tree(const uint64_t* keys, int64_t n, uint8_t* d, int32_t* lo, int32_t* hi, int32_t* left, int32_t* right, int32_t* order,
                   int32_t* cross_order, int32_t* offsets, void* workspace, size_t workspace_bytes, void* stream);
/* rgb [n,3] (uint8, the caller's row order) -> H [n-1,3] (int32, per gap: Y, Co, Cg) and val [n,3] (int32) whose row 0 is the DC.
 * H = a2 - a1, L = a1 + floor(w2 H / (w1 + w2)).  bucket_off [65] on the HOST, cross_off [65] on the device (the two halves of
 * pcgc_raht_tree's offsets).  form 0: one launch per populated split bit; form 1: tiles in LDS, then the crossing gaps by one workgroup.
 * Same integers either way. */
int pcgc_raht_forward(const uint8_t* rgb, const int32_t* perm, int64_t n, const uint8_t* d, const int32_t* lo, const int32_t* hi,
                      const int32_t* order, const int32_t* bucket_off, const int32_t* cross_order, const int32_t* cross_off, int form,
                      int32_t* val, int32_t* H, void* stream);
/* H^ [n-1,3] and the DC -> rgb [n,3] (uint8) in the caller's row order (through perm), clamped to 0 .. 255.  val [n,3]: scratch. */
int pcgc_raht_inverse(const int32_t* Hhat, int32_t dc_y, int32_t dc_co, int32_t dc_cg, const int32_t* perm, int64_t n, const uint8_t* d,
                      const int32_t* lo, const int32_t* hi, const int32_t* order, const int32_t* bucket_off, const int32_t* cross_order,
                      const int32_t* cross_off, int form, int32_t* val, uint8_t* rgb, void* stream);
/* in coding order, Y, Co, Cg within a gap: tokens [3(n-1)] (int16, 0 .. 63), ctx [3(n-1)] (uint16) = 16 channel + min(d / 3, 15),
 * escapes (uint16, room for 3(n-1)) = z - 63 of the tokens that are 63, n_escapes [1] (dev), hist [48,64] (int32, dev).
 * step in sixteenths D16 = 16 (Q = 0) or max(16, isqrt(256 Q^2 (w1 + w2) / (w1 w2))); k = sign(H) (32 |H| + D16) / (2 D16);
 * z = 2 k (k >= 0) or -2 k - 1. */
size_t pcgc_raht_quantize_workspace_bytes(int64_t n);
int pcgc_raht_quantize(const int32_t* H, int64_t n, const uint8_t* d, const int32_t* lo, const int32_t* hi, const int32_t* order, int q_luma,
                       int q_chroma, int16_t* tokens, uint16_t* ctx, uint16_t* escapes, int32_t* n_escapes, int32_t* hist, void* workspace,
                       size_t workspace_bytes, void* stream);
/* tokens and escapes -> H^ [n-1,3] per gap = sign(k) (|k| D16 + 8) / 16.  n_escape_tokens [1] (dev) = the tokens that are 63: the caller
 * refuses a stream whose escape list has another length (escapes past n_escapes read as 0, never past the list). */
size_t pcgc_raht_dequantize_workspace_bytes(int64_t n);
int pcgc_raht_dequantize(const int16_t* tokens, const uint16_t* escapes, int64_t n_escapes, int64_t n, const int32_t* lo, const int32_t* hi,
                         const int32_t* order, int q_luma, int q_chroma, int32_t* Hhat, int32_t* n_escape_tokens, void* workspace,
                         size_t workspace_bytes, void* stream);

/* ---- The colour transform of a BATCH of 1 .. 16 frames in one pass.  coords [n,4] rows (b, x, y, z) in any order, n = 1 ..
 *      2^24 rows in all.  The frame index is bits 60 .. 63 of the key (compared unsigned), so after one sort frame b is the run of leaves
 *      [start_b, start_b + n_b); a gap with d < 60 lies inside one frame and has there the lo, hi and children it has in that frame alone,
 *      shifted by start_b.  The B - 1 gaps with d >= 60 are frame boundaries: no merge, no token, lo = hi = -1.  Every output of frame b is
 *      what the single-frame entries above give for its rows alone: a single frame is the batch of one, and the entries above run the
 *      kernels and host bodies of the entries below at frames = 1 (likewise pcgc_attr_rans_encode / _decode and their _batch entries). ---- */
/* status [34] (dev): [0 .. 15] adjacent equal keys per frame (the same voxel in two frames is no duplicate), [16 .. 31] rows per frame,
 * [32] bit 0 = a coordinate outside [0, 2^20), bit 1 = a frame index outside 0 .. frames - 1. */
int64_t pcgc_raht_keys_batch_workspace_bytes(int64_t n);
int pcgc_raht_keys_batch(const int32_t* coords, int64_t n, int frames, uint64_t* keys, int32_t* perm, int32_t* status, void* workspace,
                         size_t workspace_bytes, void* stream);
/* as pcgc_raht_tree.  order [n-1]: the n - frames merges in coding order (frame, then d descending, then gap ascending), then the frame
 * boundaries; cross_order [n-1]: the merges whose range crosses a multiple of pcgc_raht_tile_leaves() by d descending, then the other
 * merges by d descending, then the boundaries.  offsets [(frames + 1) x 65] (dev): bucket [65] of every frame, counted from the frame's own
 * first position of the order, then cross [65] of the batch. */
int64_t pcgc_raht_tree_batch_workspace_bytes(int64_t n);
int pcgc_raht_tree_batch(const uint64_t* keys, int64_t n, int frames, uint8_t* d, int32_t* lo, int32_t* hi, int32_t* left, int32_t* right,
                         int32_t* order, int32_t* cross_order, int32_t* offsets, void* workspace, size_t workspace_bytes, void* stream);
/* as pcgc_raht_forward; row start_b of val is frame b's DC.  bit_off [130] on the HOST: the 65 offsets into cross_order of the crossing
 * merges (= cross), then those of the others (they start at cross[64]); form 0 launches both runs of a split bit.  cross_off [65] (dev):
 * the last row of pcgc_raht_tree_batch's offsets. */
int pcgc_raht_forward_batch(const uint8_t* rgb, const int32_t* perm, int64_t n, const uint8_t* d, const int32_t* lo, const int32_t* hi,
                            const int32_t* cross_order, const int32_t* bit_off, const int32_t* cross_off, int form, int32_t* val, int32_t* H,
                            void* stream);
/* as pcgc_raht_inverse; dc [frames,3] and starts [frames] (= start_b) on the device. */
int pcgc_raht_inverse_batch(const int32_t* Hhat, const int32_t* dc, const int32_t* starts, int frames, const int32_t* perm, int64_t n,
                            const uint8_t* d, const int32_t* lo, const int32_t* hi, const int32_t* cross_order, const int32_t* bit_off,
                            const int32_t* cross_off, int form, int32_t* val, uint8_t* rgb, void* stream);
/* as pcgc_raht_quantize over the 3 (n - frames) tokens of the batch's coding order: frame b's tokens, contexts and escapes are consecutive,
 * frame by frame.  q_luma, q_chroma [frames] on the HOST.  hist [frames,48,64] (dev); n_escapes [1] (dev) counts all frames, frame b's
 * share is the sum of hist[b][.][63]. */
int64_t pcgc_raht_quantize_batch_workspace_bytes(int64_t n, int frames);
int pcgc_raht_quantize_batch(const int32_t* H, int64_t n, int frames, const uint64_t* keys, const uint8_t* d, const int32_t* lo, const int32_t* hi,
                             const int32_t* order, const int32_t* q_luma, const int32_t* q_chroma, int16_t* tokens, uint16_t* ctx,
                             uint16_t* escapes, int32_t* n_escapes, int32_t* hist, void* workspace, size_t workspace_bytes, void* stream);
/* as pcgc_raht_dequantize; escapes: the frames' lists one after the other, n_escapes in all.  n_escape_tokens [17] (dev): the tokens that
 * are 63 per frame [0 .. 15], then of the batch; the caller refuses a frame whose escape list has another length. */
int64_t pcgc_raht_dequantize_batch_workspace_bytes(int64_t n, int frames);
int pcgc_raht_dequantize_batch(const int16_t* tokens, const uint16_t* escapes, int64_t n_escapes, int64_t n, int frames, const uint64_t* keys,
                               const int32_t* lo, const int32_t* hi, const int32_t* order, const int32_t* q_luma, const int32_t* q_chroma,
                               int32_t* Hhat, int32_t* n_escape_tokens, void* workspace, size_t workspace_bytes, void* stream);

/* ---- Colour codec, `_A.bin` version 2 (csrc/attribute_rans.hip; the definition is tests/attr_rans_reference.py): the tokens
 *      of pcgc_raht_quantize coded ON THE DEVICE by interleaved rANS, the coder of `_O.bin` version 2 above with a 64-ary token in place of
 *      a bit.  One wave per chunk of 64 S tokens; 64 independent states, one per lane, share one stream of 32-bit words.  The payload,
 *      little endian:
 *          u32 S             steps per chunk, 1 .. 2^24
 *          u32 K             chunks = ceil(tokens / (64 S))
 *          K x 64 x u64      the decoder's initial state of every lane, chunk by chunk, lane 0 .. 63
 *          K x u32           W_k: 32-bit words of chunk k
 *          u32 words         chunk 0's W_0 words, then chunk 1's, ...
 *      (no token: the payload is empty and nothing is launched; the entries below take n >= 1).
 *      Chunk k covers tokens [64 S k, min(tokens, 64 S (k + 1))) in coding order; lane j codes tokens base + 64 t + j, t = 0 .. S - 1.
 *      64-bit state, L = 2^31.  table [48][65] (uint16, dev) in rc_encode_ctx's convention: cdf[ctx][0] = 0 and cdf[ctx][64] = 65536
 *      whatever entries 0 and 64 say; token a under ctx has c = cdf[ctx][a], f = cdf[ctx][a + 1] - c.
 *      Encoder, per chunk: every lane starts at x = L; steps t = S - 1 .. 0, lanes j = 63 .. 0 within a step, tokens past the end skipped;
 *      at a token: if x >= f << 47, emit x & 0xffffffff and x >>= 32; then x = ((x / f) << 16) + x % f + c.  The stream is the emitted
 *      words in reverse order; the final x of each lane is its stored state (a lane without tokens stores L).  f = 65536 (a token that owns
 *      its row) is legal: it never emits and leaves x as it is.  f = 1 costs sixteen bits.
 *      Decoder, per chunk: steps t = 0 .. S - 1, lanes j = 0 .. 63; at a token: s = x & 0xffff, a = the token with cdf[a] <= s < cdf[a + 1]
 *      (the number of entries 1 .. 63 that are <= s), x = f (x >> 16) + s - c; if x < L, x = x << 32 | next word (within a step, words go
 *      to the renormalising lanes in ascending lane order).  A chunk is sound iff every stored state is in [2^31, 2^63), exactly W_k words
 *      were consumed and every lane ends at x == L; a word index at or past W_k reads as 0 and marks the chunk unsound.  The decoder reads
 *      nothing outside a chunk's words and the table, and writes tokens in 0 .. 63 only, whatever the bytes say.
 *      tokens < 2^31.  workspace: pcgc_attr_rans_workspace_bytes(n, steps) device bytes, 8-byte aligned (no allocation inside); an entry
 *      given less refuses with -2 before anything is launched. ---- */
int64_t pcgc_attr_rans_workspace_bytes(int64_t n, int steps);
/* ctx and tokens [dev n] as pcgc_raht_quantize writes them -> payload [dev, 8-byte aligned, capacity >= 8 + 516 K + 4 n bytes] in the layout
 * above; host2 [host 2] = the payload's length in bytes, and the number of tokens that could not be coded (a token outside 0 .. 63, a context
 * outside 0 .. 47, f <= 0: they are skipped, nothing is divided by 0, and the payload is not a stream): ONE small synchronising copy.  The
 * caller then copies the finished payload. */
int pcgc_attr_rans_encode(const uint16_t* table /*[dev 48,65]*/, const uint16_t* ctx /*[dev n]*/, const int16_t* tokens /*[dev n]*/, int64_t n,
                          int steps, uint8_t* payload, size_t payload_capacity, int64_t* host2, void* workspace, size_t workspace_bytes,
                          void* stream);
/* bucket [dev 65]: the first half of pcgc_raht_tree's offsets; token 3 p + channel of the coding order has ctx = 16 channel + min(d / 3, 15)
 * with d = 63 - (the last b with bucket[b] <= p), computed here on the device.  payload [dev, 8-byte aligned] of payload_bytes bytes whose
 * head the caller has read: steps = its S, and its K, the table sizes and the sum of W_k agree with n and payload_bytes
 * (ops.attr_rans_layout checks them on the host; here K follows from n and steps, and no access leaves the payload in any case).  The rows of
 * `table` that occur are monotone (attributes.read_stream refuses a file whose rows are not)
 * -> tokens [dev n] (int16, 0 .. 63); host2 [host 2] = tokens that are 63, unsound chunks (0: the payload is sound), in one small copy. */
int pcgc_attr_rans_decode(const uint16_t* table /*[dev 48,65]*/, const int32_t* bucket /*[dev 65]*/, int64_t n, const uint8_t* payload,
                          int64_t payload_bytes, int steps, int16_t* tokens /*[dev n]*/, int64_t* host2, void* workspace,
                          size_t workspace_bytes, void* stream);
/* A batch of 1 .. 16 frames in ONE launch sequence.  Chunks never straddle frames: frame f holds tokens [tok[f], tok[f+1])
 * of the batch's coding order (tok [frames + 1] on the HOST, ascending multiples of 3 from 0, tok[frames] = n) in K_f = ceil(n_f / (64
 * steps[f])) chunks (steps [frames] on the HOST), and its payload, in the layout above with its own S | K | states | W_k | words, stands at
 * byte pay[f] (a multiple of 8, HOST) of `payload`.  A frame without tokens has no chunk and an empty payload.  tables [dev frames,48,65];
 * a workgroup serves chunks of one frame and loads that frame's table.  workspace: pcgc_attr_rans_batch_workspace_bytes(n, K) device
 * bytes, K = the chunks of all frames; an entry given less refuses with -2 before anything is launched, as does a batch without tokens. */
int64_t pcgc_attr_rans_batch_workspace_bytes(int64_t n, int64_t chunks);
/* pay [frames + 1]: frame f has room for 8 + 516 K_f + 4 n_f bytes between pay[f] and pay[f + 1].  host [2 frames] = every frame's payload
 * length in bytes, then every frame's tokens that could not be coded: ONE small synchronising copy for the batch. */
int pcgc_attr_rans_encode_batch(const uint16_t* tables, const uint16_t* ctx, const int16_t* tokens, int frames, const int64_t* tok,
                                const int32_t* steps, uint8_t* payload, const int64_t* pay, int64_t* host, void* workspace,
                                size_t workspace_bytes, void* stream);
/* bucket [dev frames,65]: the first `frames` rows of pcgc_raht_tree_batch's offsets.  steps[f] = 0: frame f is not decoded here (its file
 * is version 1, or it has no token) and its slice of `tokens` is left alone.  pay_bytes [frames] (HOST): the length of each payload, whose
 * head the caller has checked as for pcgc_attr_rans_decode.  host [2 frames] = every frame's tokens that are 63, then every frame's
 * unsound chunks: ONE small synchronising copy for the batch. */
int pcgc_attr_rans_decode_batch(const uint16_t* tables, const int32_t* bucket, int frames, const int64_t* tok, const int32_t* steps,
                                const uint8_t* payload, const int64_t* pay, const int64_t* pay_bytes, int16_t* tokens, int64_t* host,
                                void* workspace, size_t workspace_bytes, void* stream);

/* ---- Estimated surface normals of a voxelised cloud (csrc/normals.hip; nothing in the reference: its D2 figures assume clouds whose normals
 *      another tool estimated).  Per row at voxel p: the neighbourhood is every DISTINCT voxel q of the row's batch with |q - p|^2 <= r2 (p
 *      included); moments [n,10] = k, sum dx dy dz, sum dx^2 dy^2 dz^2 dxdy dxdz dydz over d = q - p (exact); S = k sum(d d^T) - (sum d)(sum d)^T;
 *      lam [n,3] = eigenvalues of S ascending (fp64); valid = k >= 3 and rank S >= 2 (on the integers); normals [n,3] = unit eigenvector of
 *      lam[0], (0, 0, 0) where not valid; count = k.  Every duplicate row receives its voxel's result.  orient 0: the component of largest
 *      magnitude is positive; 1: away from the centroid of the batch's distinct voxels; 2: towards viewpoint [host 3]; an exactly zero dot
 *      product falls back to rule 0.  The cloud is given by its original rows (coords) and by its D2 index exactly as for pcgc_d2_count
 *      (qs, perm, cell hash, masks, voxel hash, runlen); ball = pcgc_normals_ball_masks(r2) uploaded by the caller.  r2 outside 1 .. 64 is an
 *      error (-2), never clamped; coordinates must have passed pcgc_coords_check_order.  Bitwise reproducible, independent of the row order. */
/* ball [(2 C + 1)^3][64], C = ceil(floor(sqrt r2) / 4): bit b of ball[t][l] = voxel b of the cell at offset t (x fastest, from -C) lies within
 * r2 of voxel l of the centre cell.  HOST.  -> number of masks (table = NULL: only that), < 0: error */
int64_t pcgc_normals_ball_masks(int32_t r2, uint64_t* table /*[host] or NULL*/);
size_t pcgc_normals_workspace_bytes(int64_t n);
int pcgc_normals_estimate(const int32_t* coords /*[dev n,4]*/, int64_t n, const int32_t* qs /*[dev n,4]*/, const int32_t* perm,
                          const uint64_t* cell_keys, const int32_t* cell_vals, int64_t cell_cap, const uint64_t* masks, const uint64_t* keys,
                          const int32_t* vals, int64_t cap, const int32_t* runlen, const uint64_t* ball /*[dev]*/, int32_t r2, int orient,
                          const double* viewpoint /*[host 3] or NULL*/, int64_t* moments /*[dev n,10]*/, double* normals /*[dev n,3]*/,
                          double* lam /*[dev n,3]*/, int32_t* count /*[dev n]*/, uint8_t* valid /*[dev n]*/, void* workspace,
                          size_t workspace_bytes, void* stream);
/* process-wide A/B knob of the moments pass: 0 = one wave per occupied 4 x 4 x 4 cell (default), 1 = one thread per voxel.  Same results.
 * -> the previous mode */
int pcgc_set_normals_mapping(int mode);

/* ---- ASCII PLY geometry I/O (data_utils.py:19-48: read_ply_ascii_geo / write_ply_ascii_geo), HOST.
 *      read: returns the number of data rows (call with xyz = NULL to size the buffer); same acceptance rule as the
 *      reference (a line is data iff all its ' '-separated tokens parse as floats); columns 0:3 truncated to int. ---- */
int64_t pcgc_ply_read_ascii_geo(const char* path, int32_t* xyz /*[host cap,3] or NULL*/, int64_t cap);
int pcgc_ply_write_ascii_geo(const char* path, const int32_t* xyz /*[host n,3]*/, int64_t n);
/* the same with `property uchar red / green / blue` after the coordinates, integer text */
int pcgc_ply_write_ascii_geo_rgb(const char* path, const int32_t* xyz /*[host n,3]*/, const uint8_t* rgb /*[host n,3]*/, int64_t n);

/* ---- the bitstream files of several items at once (HOST; native threads): the host half of Coder.encode / Coder.decode
 *      (coder.py:49-55,85-87,93-100) for the items of a collated batch or for one cloud.  stems[i] = "<prefix><postfix>" of item i;
 *      sym: int16 symbols [sum rows, C] (items contiguous), ranges [n,2] = (min_v, max_v) per item, counts [n,3] = (N4, N2, N1),
 *      xyz = stride-8 coordinates / 8, [sum rows, 3].  table_fn = pcgc_reference_table of libpcgc_reftable.so (include/pcgc_reftable.h)
 *      or any function of that signature; eb_params as it expects them.  index_segments = coder.INDEX_SEGMENTS (0: no sidecar).
 *      write_coords = 0: `_C.bin` is left to the caller (tmc3).  threads <= 0: the CPUs this process may use. ---- */
typedef int (*pcgc_table_fn)(const float* params, int C, float min_v, float max_v, uint16_t* table_u16, float* cdf_f32);
int pcgc_items_encode(int n_items, const char* const* stems, const int16_t* sym, const int32_t* xyz, const int64_t* rows, const float* ranges,
                      int C, const int32_t* counts, const float* eb_params, pcgc_table_fn table_fn, int index_segments, int write_coords,
                      int threads);
/* sizes first: rows[i], channels[0], ranges, counts, native_coords[i] (1: `_C.bin` is a native octree stream of rows[i] points) ... */
int pcgc_items_probe(int n_items, const char* const* stems, int64_t* rows, int32_t* channels, float* ranges, int32_t* counts,
                     int32_t* native_coords);
/* ... then the streams: sym [sum rows, C] and the coordinates of the items with native_coords — coord_layout 0: xyz [sum rows, 3], voxel
 * indices in stream order; coord_layout 1: xyz [sum rows, 4] = the coordinate level Coder.decode starts from (coder.py:97-102), rows
 * (item index, coord_scale x, coord_scale y, coord_scale z), every item in (z, y, x) order (sort_spare_tensor, data_utils.py:91-101).
 * -5: a sidecar names another CDF table than this host derives (the stream would decode to noise). */
int pcgc_items_decode(int n_items, const char* const* stems, const int64_t* rows, int C, const float* ranges, const int32_t* native_coords,
                      const float* eb_params, pcgc_table_fn table_fn, int use_sidecar, int16_t* sym, int32_t* xyz, int coord_layout,
                      int coord_scale, int threads);

/* The coordinate-only part of the first decoder stage on a freshly decoded level in one call: hash (cap = pcgc_hash_capacity(n)), k3 map
 * nbr [27][n], children level [8 n][4] (MinkowskiGenerativeConvolutionTranspose's coordinates, autoencoder.py:155-161) and its k3 map
 * [27][8 n] — pcgc_hash_clear + _insert + pcgc_kmap_k3 + pcgc_coords_children + pcgc_kmap_k3_children without the host in between. */
int pcgc_level_prepare_children(const int32_t* coords, int64_t n, int32_t stride, uint64_t* keys, int32_t* vals, int64_t cap, int32_t* nbr,
                                int32_t* children, int32_t* nbr_children, void* stream);

/* One cloud in one call — Coder.decode's host half (coder.py:93-104): probe + both streams, into buffers the caller keeps (pinned memory:
 * both uploads are then asynchronous copies).  sym [cap_rows, C], level [cap_rows, 4] (coord_layout 1 above, coord_scale = the level's
 * tensor stride).  info[6] = rows, channels, N4, N2, N1, native_coords; range[2] = min_v, max_v.  -> 0; 1: cap_rows too small (info[0]
 * rows needed, nothing decoded); < 0: error (-5 as above).  `_C.bin` not a native stream (tmc3): info[5] = 0, `level` untouched. */
int pcgc_frame_decode(const char* stem, int C, const float* eb_params, pcgc_table_fn table_fn, int use_sidecar, int coord_scale,
                      int64_t cap_rows, int16_t* sym, int32_t* level, int64_t* info, float* range, int threads);
/* The same call in two halves: `_begin` returns as soon as the coordinate level is in `level` (info / range filled; 1 = buffers too small,
 * nothing pending) while the feature stream keeps decoding on the library's threads; the caller uploads the level and enqueues the decoder's
 * coordinate-only kernels (pcgc_level_prepare_children), then `_end` waits for `sym` and returns pcgc_frame_decode's code.  Every
 * successful `_begin` must be followed by `_end` on the same thread.  With fewer than three CPUs, or while another thread's frame is
 * pending, `_begin` does everything synchronously and `_end` nothing. */
int pcgc_frame_decode_begin(const char* stem, int C, const float* eb_params, pcgc_table_fn table_fn, int use_sidecar, int coord_scale,
                            int64_t cap_rows, int16_t* sym, int32_t* level, int64_t* info, float* range, int threads);
int pcgc_frame_decode_end(void);
/* Test hook of the two-halves form: the library's frame worker takes every job `delay_us` late (0 = off; negative = leave unchanged)
 * -> how many feature-stream jobs `_end` has run on the calling thread because the worker had not taken them yet. */
int pcgc_frame_worker_test(int delay_us);

/* The CDF-table cache behind pcgc_items_encode / pcgc_items_decode / pcgc_frame_decode (a table is a pure function of the entropy
 * parameters and the symbol range; the reference evaluates it in every compress() and decompress(), entropy_model.py:165-171,185-190).
 * mode 0: drop every cached table; 1: cache (default); -1: never cache.  -> tables dropped.  HOST. */
int pcgc_table_cache(int mode);

/* zlib's crc32(crc, buf, len) (the CRC-32 of the `_F.idx` sidecar's stream and table guards; coder.py of this package uses
 * zlib.crc32 for the same fields), folded with carry-less multiplies on long buffers.  HOST. */
uint32_t pcgc_crc32(uint32_t crc, const uint8_t* buf, int64_t len);

/* ---- training clouds from triangle meshes (the reference's generate_dataset.py:7-36, open3d on the CPU there).  The sampling
 *      arithmetic is this project's own, exact in fp64 and counter-based (Philox4x32-10): sample i is a pure function of (seed, i).
 *      csrc/mesh.hip states it; tests/mesh_reference.py restates it in numpy; DESIGN.md 8c explains it. ---- */
/* ASCII OFF (header on one line, on two, or glued "OFF8 6 0") and OBJ (v; f with a, a/b, a/b/c, a//c tokens, 1-based or negative
 * indices; other records skipped); polygons are fanned (v0, vi, vi+1).  counts[0] = vertices, counts[1] = triangles; verts = faces =
 * NULL: sizes only.  0 ok; -1 the file cannot be read; -3 malformed or truncated; -4 a face names a missing vertex; -5 buffers too
 * small.  HOST. */
int pcgc_mesh_read(const char* path, double* verts /*[host vcap,3]*/, int64_t vcap, int32_t* faces /*[host fcap,3]*/, int64_t fcap,
                   int64_t* counts /*[host 2]*/);
/* cdf[t] = sum of the areas 0.5 |(B-A) x (C-A)| of triangles 0..t, in an order that depends on T alone (bitwise reproducible, no
 * floating-point atomics) and never decreasing.  A face with an index outside [0, V) has area 0 and is counted in *bad_faces. */
size_t pcgc_mesh_cdf_workspace_bytes(int64_t T);
int pcgc_mesh_area_cdf(const double* verts /*[dev V,3]*/, int64_t V, const int32_t* faces /*[dev T,3]*/, int64_t T,
                       double* cdf /*[dev T]*/, int32_t* bad_faces /*[dev 1]*/, void* workspace, size_t workspace_bytes, void* stream);
/* samples first .. first+n-1: the triangle each falls on and / or its point */
int pcgc_mesh_sample(const double* verts, int64_t V, const int32_t* faces, const double* cdf, int64_t T, uint64_t seed, uint64_t first,
                     int64_t n, int32_t* tri /*[dev n] or NULL*/, double* points /*[dev n,3] or NULL*/, void* stream);
/* mesh2pc after the file read: samples 0..n-1, q = p . R, d = q - min q, rint((d / max d) * resolution), distinct rows (0, x, y, z) in
 * (z, y, x) order.  1 <= resolution <= 1023.  *count = rows found (the first `cap` of them are written; min(n, (resolution+1)^3)
 * always suffices); -1: the total area is not positive and finite; -2: max d is not (every sample fell on one value). */
size_t pcgc_mesh_voxelize_workspace_bytes(int32_t resolution);
int pcgc_mesh_voxelize(const double* verts, int64_t V, const int32_t* faces, const double* cdf, int64_t T, uint64_t seed, int64_t n,
                       const double* R /*[host 9] row-major*/, int32_t resolution, int32_t* out /*[dev cap,4]*/, int64_t cap,
                       int32_t* count /*[dev 1]*/, void* workspace /*[dev] 64-byte aligned*/, size_t workspace_bytes, void* stream);

/* ---- batches out of the data loader's device-resident arena (pcgcv2_amd/data_loader.py, csrc/collate.hip) ---- */
#define PCGC_COLLATE_MAX_ITEMS 16
/* One cloud of a batch: `rows` rows of three values, `width` bytes each (1: uint8, 2: uint16, 4: int32), packed from byte `offset` of
 * the arena (a multiple of 16) in file order.  symmetry = perm + 6 * flips, one of the 48 symmetries of the cube: a row v becomes w with
 * w[a] = (flips >> a & 1) ? extent - v[a] : v[a], then out = w[perm], perm counted through (0,1,2) (0,2,1) (1,0,2) (1,2,0) (2,0,1)
 * (2,1,0); 0 leaves the row as it is.  first_row = the sum of the rows of the items before it. */
typedef struct pcgc_collate_item {
    int64_t offset;
    int32_t first_row, rows, width, symmetry, extent, reserved;
} pcgc_collate_item;
/* coords_out[first_row + r] = (item, x, y, z), feats_out[first_row + r] = 1.0f for every row of every item, N = the sum of the rows; one
 * launch, the items by value in the kernel arguments.  n_items == 0 and N == 0 launch nothing.  The caller vouches that every item lies
 * inside the arena (ops.collate_rows checks it). */
int pcgc_collate_rows(const uint8_t* arena /*[dev] 16-byte aligned*/, const pcgc_collate_item* items /*[host n_items]*/, int n_items,
                      int32_t* coords_out /*[dev N,4] 16-byte aligned*/, float* feats_out /*[dev N,1]*/, void* stream);

/* ---- Voxelising a raw cloud (csrc/voxelize.hip; the definition is tests/voxelize_reference.py): points [n,3], float32
 *      (is_f64 = 0) or float64 (1) rows in the caller's units, packed, n = 1 .. 2^31 - 1 (anything else is -2 before anything is touched)
 *      -> the distinct voxels of a `bits`-bit lattice (1 .. 20) in (z, y, x) order, the rows merged into each, one colour per voxel.
 *      float32 values are widened exactly and take the float64 path from there.  Minima, maxima and integer sums only: every output is
 *      exact and the same on every run.  Four entries, called in this order; the host decides the frame between the first two and sizes
 *      the outputs between the last two.  Buffers are the caller's; everything runs on `stream`. ---- */
/* sorted rows per workgroup of pcgc_voxelize_merge */
int64_t pcgc_voxelize_tile_rows(void);
/* bounds [6] (dev, double): the minimum of x, y, z and then the maximum of x, y, z over the rows that hold neither a NaN nor an infinity
 * (a zero is written as +0; +inf / -inf when there is no such row); bad_rows [1] (dev): the rows that do. */
int64_t pcgc_voxelize_bounds_workspace_bytes(int64_t n);
int pcgc_voxelize_bounds(const void* points, int is_f64, int64_t n, double* bounds, int64_t* bad_rows, void* workspace,
                         size_t workspace_bytes, void* stream);
/* q[a] = rint((double(p[a]) - origin[a]) * scale): the difference and the product each rounded once to fp64, ties to even.
 * keys [n] (uint64) = qz << 40 | qy << 20 | qx; rows [n] = 0 .. n - 1; outside [1] (dev): the rows with a q outside [0, 2^bits - 1] or
 * not a number (their key is 0; the caller refuses the cloud when the count is not 0). */
int pcgc_voxelize_quantize(const void* points, int is_f64, int64_t n, int bits, double origin_x, double origin_y, double origin_z,
                           double scale, uint64_t* keys, int32_t* rows, int64_t* outside, void* stream);
/* (keys, rows) sorted by key, stably: inside a voxel the rows ascend -> sorted_keys [n], sorted_rows [n]; rank [n]: 1 + the output row
 * of the voxel of sorted row i, so rank[n - 1] is the number of voxels m.  The inputs are left as they are. */
int64_t pcgc_voxelize_heads_workspace_bytes(int64_t n);
int pcgc_voxelize_heads(const uint64_t* keys, const int32_t* rows, int64_t n, int bits, uint64_t* sorted_keys, int32_t* sorted_rows,
                        int32_t* rank, void* workspace, size_t workspace_bytes, void* stream);
/* coords [m,4] (16-byte aligned): rows (0, x, y, z) ascending in (z, y, x); counts [m]: the input rows of each voxel; voxel_of [n]: the
 * output row of every input row.  colours [n,3] (uint8) or NULL, colours_out [m,3] or NULL with it: merge_first = 0 the mean per channel,
 * floor((2 sum + count) / (2 count)) over 64-bit sums; 1 the colour of the voxel's lowest input row.  A run of equal keys is reduced
 * inside its workgroup; only a run that crosses a multiple of pcgc_voxelize_tile_rows() is added up with (integer) atomics. */
int64_t pcgc_voxelize_merge_workspace_bytes(int64_t m);
int pcgc_voxelize_merge(const uint64_t* sorted_keys, const int32_t* sorted_rows, const int32_t* rank, int64_t n, int64_t m,
                        const uint8_t* colours, int merge_first, int32_t* coords, int32_t* counts, int32_t* voxel_of, uint8_t* colours_out,
                        void* workspace, size_t workspace_bytes, void* stream);

/* ---- Cleaning a voxelised cloud (csrc/clean.hip; the definition is tests/clean_reference.py): rows are DISTINCT voxels
 *      (batch, x, y, z) that have passed pcgc_coords_check_order, n = 0 .. 2^24 (anything else, a null pointer or an undersized workspace is
 *      -2 before anything is touched).  Integers only; every output is a function of the voxel set and the row order.  Buffers are the
 *      caller's; everything runs on `stream`. ---- */
/* Stage 1: neighbours [n] (ORIGINAL rows) = the other voxels of the row's batch with |q - p|^2 <= r2 (1 .. 64, never clamped); keep [n] =
 * neighbours >= min_neighbours; repeated [1] (dev) = the rows that repeat an earlier voxel (the caller refuses the cloud when it is not 0).
 * The cloud is given by its D2 index as for pcgc_normals_estimate (qs, perm, cell hash, masks, runlen); ball = pcgc_normals_ball_masks(r2). */
int pcgc_clean_neighbours(const int32_t* qs /*[dev n,4]*/, const int32_t* perm, int64_t n, const uint64_t* cell_keys, const int32_t* cell_vals,
                          int64_t cell_cap, const uint64_t* masks, const int32_t* runlen, const uint64_t* ball /*[dev]*/, int32_t r2,
                          int32_t min_neighbours, int32_t* neighbours /*[dev n]*/, uint8_t* keep /*[dev n]*/, int32_t* repeated /*[dev 1]*/,
                          void* stream);
/* Stage 2: connected components of the rows of a k3 map nbr [27][n] (pcgc_kmap_k3 at stride 1; -1 = absent; 26-connectivity).  labels [n] =
 * the smallest row of the row's component, sizes [n] = its row count; *n_components and *rounds (the launches of the labelling round, the
 * one that changed nothing included) are HOST values.  Entries of the map that are no row of it are never followed.
 * Rounds are launched by the host, which reads a device counter every few rounds; at most n + 1 of them (the argument is in clean.hip), -3
 * when that cap is reached.  The call synchronises with `stream`. */
int64_t pcgc_components_workspace_bytes(int64_t n);
int pcgc_components(const int32_t* nbr /*[dev 27,n]*/, int64_t n, int32_t* labels /*[dev n]*/, int32_t* sizes /*[dev n]*/,
                    int64_t* n_components /*host*/, int32_t* rounds /*host*/, void* workspace, size_t workspace_bytes, void* stream);
/* labels_c / sizes_c [n_c] of the compacted survivors (keep1, prefix of pcgc_mask_scan, orig of pcgc_compact_index) -> labels [n] = INPUT
 * row of the component's smallest row (-1 for a row keep1 drops), sizes [n] (0 for such a row) */
int pcgc_clean_expand(const uint8_t* keep1, const int32_t* prefix, const int32_t* orig, const int32_t* labels_c, const int32_t* sizes_c,
                      int64_t n, int64_t n_c, int32_t* labels, int32_t* sizes, void* stream);
/* keep [n] = labels >= 0 and sizes >= min_component (>= 1) and, with keep_largest > 0, the row's component is one of the keep_largest
 * largest of its batch item (ties to the smaller label; a 64-bit key per root, sorted).  coords [n,4] 16-byte aligned. */
int64_t pcgc_clean_select_workspace_bytes(int64_t n);
int pcgc_clean_select(const int32_t* coords, const int32_t* labels, const int32_t* sizes, int64_t n, int32_t min_component,
                      int64_t keep_largest, uint8_t* keep /*[dev n]*/, void* workspace, size_t workspace_bytes, void* stream);
/* out[prefix[i]] = colours[i] (three bytes a row) where mask[i] is set: pcgc_compact_coords for colours */
int pcgc_clean_compact_colours(const uint8_t* colours /*[dev n,3]*/, const uint8_t* mask, const int32_t* prefix, int64_t n,
                               uint8_t* out /*[dev total,3]*/, void* stream);

/* ---- Rendering a cloud into views (csrc/render.hip; the definition is tests/render_reference.py): a z-buffer splat.  Integers
 *      only; every output is a function of the rows, their order and the matrices.  Buffers are the caller's; everything runs on `stream`. ---- */
/* coords [n,4] (batch, x, y, z), 16-byte aligned, n = 0 .. 2^31 - 1, rows in any order; colours [n,3] or null (the depth shade); B items and V
 * views, B V <= 64; H, W in 1 .. 4096; r in 0 .. 4 (a point covers (2 r + 1)^2 pixels); matrices [dev V,12] int64, Q16, row-major 3x4, which
 * the caller has range-checked (|3x3| <= 2^20, |translation| <= 2^60, d inside int32 for coordinates below 2^21); planes [dev V,2] int32 = near,
 * far of the depth shade; background = R | G << 8 | B << 16.  Outputs [B,V,H,W]: index (the winning row or -1), depth (d, 0 on background), mask
 * (0 / 1), image [.,3].  bad [dev 1] = rows whose batch item is not below B or whose coordinates are not in [0, 2^21): they touch nothing and
 * the caller refuses the cloud.  The workspace (one 64-bit word per item, view and pixel) is cleared on every call.  issued: null, or [dev 1]
 * = the atomics the splat sent (a measurement; it depends on the order the threads ran in).  phases: 7; a sum of 1 clear, 2 splat, 4 resolve
 * runs only those, on whatever the workspace holds (tools/render_time.py); bad and issued are zeroed by every call. */
int64_t pcgc_render_splat_rows(void);
int64_t pcgc_render_workspace_bytes(int B, int V, int H, int W);
int pcgc_render(const int32_t* coords, const uint8_t* colours, int64_t n, int B, int V, int H, int W, int r, const int64_t* matrices,
                const int32_t* planes, uint32_t background, int32_t* index, int32_t* depth, uint8_t* mask, uint8_t* image, int32_t* bad,
                uint64_t* issued, int phases, void* workspace, size_t workspace_bytes, void* stream);
/* two renderings of the same views, slices = B V of `pixels` pixels each -> sums [dev slices,8] uint64: pixels of the union U and of the
 * intersection I of the masks, the SSE of R, G, B and of Y = (13933 R + 46871 G + 4732 B + 32768) >> 16 over U, the SSE of depth_a - depth_b
 * over the pixels of I where it is below 2^19 in magnitude, and the number of pixels of I where it is not (the caller refuses those). */
int pcgc_render_metric(const uint8_t* mask_a, const uint8_t* mask_b, const uint8_t* image_a, const uint8_t* image_b, const int32_t* depth_a,
                       const int32_t* depth_b, int slices, int64_t pixels, uint64_t* sums, void* stream);

/* ---- Partition of a cloud into kd-tree blocks of at most max_num rows (csrc/partition.hip; the definition is
 *      tests/partition_reference.py).  Integers only; every output equals the definition's.  Buffers are the caller's; everything runs on
 *      `stream`, with which the call synchronises once per round.  A wrong argument, a null pointer or an undersized workspace is -2 before
 *      anything is touched. ---- */
#define PARTITION_MAX_BLOCKS 1024
enum { PARTITION_INFO_ROUNDS, PARTITION_INFO_BLOCKS, PARTITION_INFO_OVERSIZE, PARTITION_INFO_BAD_RANGE, PARTITION_INFO_BAD_BATCH,
       PARTITION_INFO_WOULD_BE, PARTITION_INFO_WORDS = 8 };
enum { PARTITION_PHASE_BOUNDS, PARTITION_PHASE_COARSE, PARTITION_PHASE_CUT, PARTITION_PHASE_FINE, PARTITION_PHASE_ASSIGN, PARTITION_PHASE_ORDER,
       PARTITION_PHASE_COPIES, PARTITION_PHASE_WORDS = 8 };
/* coords [dev n,cols] int32, cols = 3 (x, y, z) or 4 (batch, x, y, z; batch 0), n = 0 .. 2^27, rows in any order and not necessarily distinct;
 * max_num >= 1; align a power of two in 8 .. 1024.  -> block_of [dev n], perm [dev n] (the rows in block-major order, stable), table [dev
 * 1024,8] of which the first `blocks` rows are written: (first_row, rows, lo_x, lo_y, lo_z, hi_x, hi_y, hi_z), the inclusive box of the block's
 * voxels.  info [host 8]: rounds, blocks, oversize (blocks of more than max_num rows in one cell), then the counts behind a refusal.
 * phase_seconds: null, or [host 8] to which the seconds of each phase are ADDED (a measurement hook: the call then waits for the stream after
 * every phase).  Returns 0; -3 when rows have a coordinate outside [0, 2^20) or a batch index other than 0 (info names how many); -4 when block
 * 1 025 would be created (info names the count the round would have left).  With -3 and -4 no output has been written. */
int64_t pcgc_partition_workspace_bytes(int64_t n);
int pcgc_partition(const int32_t* coords, int64_t n, int32_t cols, int64_t max_num, int32_t align, int32_t* block_of, int32_t* perm,
                   int32_t* table, int64_t* info /*host*/, double* phase_seconds /*host or null*/, void* workspace, size_t workspace_bytes,
                   void* stream);
/* out [dev rows,4] (16-byte aligned) = (block_of - first_block, x, y, z) of the rows perm[first_row .. first_row + rows): the collated
 * coordinates of a run of blocks, batch column = block - the run's first block */
int pcgc_partition_gather(const int32_t* coords, int64_t n, int32_t cols, const int32_t* perm, const int32_t* block_of, int64_t first_row,
                          int64_t rows, int32_t first_block, int32_t* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PCGC_HIP_H */
