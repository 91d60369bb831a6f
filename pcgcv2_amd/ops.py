"""Thin functional layer over the C-ABI (include/pcgc_hip.h): torch tensors in, torch tensors out.

PyTorch is used for device memory and streams only; all arithmetic happens in libpcgc_hip.so.  Every function
requires ROCm device tensors and raises otherwise — there is no CPU path in the product.  What a sparse-conv launch is charged in the
roofline report is written down in roofline.py; `PROFILE`, its one instance, brackets the launches here.
"""
import ctypes
import os as _os
from collections import namedtuple

import numpy as np
import torch

from . import roofline
from ._lib import lib, check, PcgcError, CONSTANTS
from .roofline import MFMA_F32_PEAK_TFLOPS, child_pairs, _halo_cells          # noqa: F401  (read as ops.<name> by bench.py, tools/ and tests)


def _stream(t=None):
    """HIP stream the call is enqueued on: the current stream of the OPERAND's device (not of the current device — they differ
    in a single-process multi-GPU program that never calls set_device)."""
    if t is None:
        return torch.cuda.current_stream().cuda_stream
    return torch.cuda.current_stream(t.device).cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _dev(t, dtype, what):
    if not t.is_cuda:
        raise PcgcError(f'{what}: expected a ROCm device tensor, got {t.device} (no CPU fallback exists)')
    if t.dtype != dtype:
        raise PcgcError(f'{what}: expected {dtype}, got {t.dtype}')
    if not t.is_contiguous():
        raise PcgcError(f'{what}: tensor must be contiguous')
    return t


def _i32(t, what='coords'):
    return _dev(t, torch.int32, what)


def _f32(t, what='feats'):
    if t.dtype != torch.float32 or not t.is_cuda:
        raise PcgcError(f'{what}: expected float32 device tensor, got {t.dtype} on {t.device}')
    return t


def _ld(t):
    """leading dimension (row stride in floats) of a 2-D row-major view whose rows are contiguous."""
    if t.dim() != 2 or t.stride(1) != 1:
        raise PcgcError('feature views must be 2-D with unit column stride')
    return t.stride(0)


# ------------------------------------------------------------------------------------------------ profiling hook (pcgcv2_amd/roofline.py)
PROFILE = roofline._Profile()


# ------------------------------------------------------------------------------------------------ dispatch policy (pcgcv2_amd/pathconfig.py)
from .pathconfig import PathConfig, FIELDS as _PATH_FIELDS

PATH = PathConfig.from_env()          # the process-wide default record: frozen; replaced as a whole, never mutated


def configure(cfg=None, **changes):
    """replace the default PathConfig: configure(FIELD=value, ...) or configure(a_record) -> the PREVIOUS record (hand it back to restore)"""
    global PATH
    prev = PATH
    PATH = (PATH if cfg is None else cfg).replace(**changes)
    return prev


class path:
    """with ops.path(ROWS_Q4=False): ...  — the default record replaced inside the block, the previous one restored on exit"""

    def __init__(self, **changes):
        self.changes = changes

    def __enter__(self):
        self.prev = configure(**self.changes)
        return PATH

    def __exit__(self, *exc):
        configure(self.prev)
        return False


class _OpsModule(type(_os)):
    """`ops.FIELD` reads the current record; `ops.FIELD = v` replaces the record (the spelling of the A/B tools and tests of rounds 1-5)"""

    def __getattr__(self, name):
        if name in _PATH_FIELDS:
            return getattr(self.__dict__['PATH'], name)
        raise AttributeError(f"module 'pcgcv2_amd.ops' has no attribute '{name}'")

    def __setattr__(self, name, value):
        if name in _PATH_FIELDS:
            self.__dict__['PATH'] = self.__dict__['PATH'].replace(**{name: value})
        else:
            super().__setattr__(name, value)


import sys as _sys
_sys.modules[__name__].__class__ = _OpsModule


# ------------------------------------------------------------------------------------------------ hash / coords
class HashTable:
    """Coordinate hash of one level (keys/vals device buffers + the stride its spatial blocking was built with).  Defined: WHICH slots are
    occupied, WHICH keys are stored and what every lookup returns.  Not defined: which of two keys of one probe chain holds the earlier slot
    (the order their compare-and-swaps arrive in) — the raw keys / vals arrays of two builds of one level may differ there."""

    def __init__(self, coords, stride, keep_last=False):
        n = coords.shape[0]
        self.cap = int(lib().pcgc_hash_capacity(n))
        self.stride = int(stride)
        self.keys = torch.empty(self.cap, dtype=torch.int64, device=coords.device)
        self.vals = torch.empty(self.cap, dtype=torch.int32, device=coords.device)
        check(lib().pcgc_hash_clear(_p(self.keys), _p(self.vals), self.cap, _stream(self.keys)), 'hash_clear')
        check(lib().pcgc_hash_insert_policy(_p(_i32(coords)), n, self.stride, _p(self.keys), _p(self.vals), self.cap, int(keep_last),
                                            _stream(coords)), 'hash_insert')


def level_prepare_children(coords, stride):
    """hash table, k3 map, children level and the children level's k3 map of a level, in one library call
    -> (HashTable, nbr [27, n], children [8 n, 4], nbr_children [27, 8 n])"""
    n, dev = coords.shape[0], coords.device
    table = HashTable.__new__(HashTable)
    table.cap, table.stride = int(lib().pcgc_hash_capacity(n)), int(stride)
    table.keys = torch.empty(table.cap, dtype=torch.int64, device=dev)
    table.vals = torch.empty(table.cap, dtype=torch.int32, device=dev)
    ints = torch.empty(27 * n + 32 * n + 27 * 8 * n, dtype=torch.int32, device=dev)      # one allocation: nbr | children | nbr_children
    nbr, children, nbr_c = ints[:27 * n].view(27, n), ints[27 * n:59 * n].view(8 * n, 4), ints[59 * n:].view(27, 8 * n)
    check(lib().pcgc_level_prepare_children(_p(_i32(coords)), n, int(stride), _p(table.keys), _p(table.vals), table.cap, _p(nbr), _p(children),
                                            _p(nbr_c), _stream(coords)), 'level_prepare_children')
    return table, nbr, children, nbr_c


def check_coords(coords, what='coordinates'):
    """Raise PcgcError if any row is outside the range the coordinate key can hold (the hash kernels would skip it).
    -> descents of the (batch, z, y, x) key along the rows: 0 = sorted like sort_spare_tensor's output, ~n/2 = no order at all."""
    out2 = torch.empty(2, dtype=torch.int32, device=coords.device)
    check(lib().pcgc_coords_check_order(_p(_i32(coords)), coords.shape[0], _p(out2), _stream(coords)), 'coords_check_order')
    n_bad, descents = out2.tolist()
    if n_bad:
        raise PcgcError(f'{what}: {n_bad} of {coords.shape[0]} rows are outside the supported range '
                        '(0 <= x, y, z < 2^20, 0 <= batch < 16)')
    return int(descents)


def first_occurrence_mask(coords, table, want_rows=False):
    """-> keep uint8 [n] (and, if want_rows, first_row int32 [n]: the first row holding each row's coordinate)."""
    n = coords.shape[0]
    keep = torch.empty(n, dtype=torch.uint8, device=coords.device)
    first = torch.empty(n, dtype=torch.int32, device=coords.device) if want_rows else None
    check(lib().pcgc_hash_first_mask(_p(_i32(coords)), n, table.stride, _p(table.keys), _p(table.vals), table.cap, _p(keep),
                                     _p(first), _stream(coords)), 'hash_first_mask')
    return (keep, first) if want_rows else keep


def down_maps(fine, first_row, prefix, stride_fine, n_coarse):
    """-> (parent_of int32 [n_fine], down int32 [8, n_coarse]) of the k2s2 down-sampling, no hash probes."""
    n = fine.shape[0]
    parent_of = torch.empty(n, dtype=torch.int32, device=fine.device)
    down = torch.empty((8, n_coarse), dtype=torch.int32, device=fine.device)
    check(lib().pcgc_down_maps(_p(_i32(fine)), _p(first_row), _p(prefix), n, int(stride_fine), n_coarse, _p(parent_of), _p(down),
                               _stream(fine)), 'down_maps')
    return parent_of, down


def down_level(fine, stride_fine):
    """One strided pyramid level (MinkowskiConvolution k=2 s=2, coordinate side) in one library call, which reads the coarse
    count back in the middle (the one host synchronisation of a level) and finishes into upper-bound buffers
    -> (coarse int32 [n_coarse,4], parent_of int32 [n], down int32 [8,n_coarse]); coarse and down are views of buffers
    sized for n rows.  Canonical order: coarse rows in first-occurrence order of the quantised fine rows."""
    fine = _i32(fine)
    n, dev = fine.shape[0], fine.device
    cap = int(lib().pcgc_hash_capacity(n))
    ws_bytes = int(lib().pcgc_scan_workspace_bytes(n))
    # two allocations per level (scratch, outputs) instead of eleven: this runs between two device synchronisations, where every
    # microsecond of interpreter time is GPU idle time
    a8 = lambda v: (v + 7) & ~7
    off, sizes = 0, []
    for nbytes in (16 * n, 8 * cap, 4 * cap, 4 * n, 4 * n, 8, n, ws_bytes):        # q | keys | vals | first_row | prefix | total | keep | scan ws
        sizes.append((off, nbytes)); off += a8(nbytes)
    scratch = torch.empty(off, dtype=torch.uint8, device=dev)
    part = lambda i, dt: scratch[sizes[i][0]:sizes[i][0] + sizes[i][1]].view(dt)
    q, keys, vals, first_row, prefix, total, keep, ws = (part(0, torch.int32), part(1, torch.int64), part(2, torch.int32), part(3, torch.int32),
                                                       part(4, torch.int32), part(5, torch.int32), part(6, torch.uint8), part(7, torch.uint8))
    outbuf = torch.empty(13 * n, dtype=torch.int32, device=dev)                     # coarse [n,4] | parent_of [n] | down [8n]
    coarse_ub, parent_of, down_ub = outbuf[:4 * n].view(n, 4), outbuf[4 * n:5 * n], outbuf[5 * n:]
    n_coarse = ctypes.c_int64(0)
    check(lib().pcgc_down_level(_p(fine), n, int(stride_fine), _p(q), _p(keys), _p(vals), cap, _p(keep), _p(first_row), _p(prefix),
                                _p(total), _p(ws), ws_bytes, _p(coarse_ub), _p(parent_of), _p(down_ub), ctypes.byref(n_coarse),
                                _stream(fine)), 'down_level')
    nc = int(n_coarse.value)
    return coarse_ub[:nc], parent_of, down_ub[:8 * nc].view(8, nc)


def pyramid(fine, stride_fine, levels):
    """`levels` strided levels below `fine` in one library call with ONE host synchronisation (pcgc_pyramid): every level is
    deduplicated straight from the input rows.  -> [(coarse, parent_of, down)] per level, the same tensors `levels` nested
    down_level() calls return (views of upper-bound buffers)."""
    fine = _i32(fine)
    n, dev = fine.shape[0], fine.device
    nbytes = int(lib().pcgc_pyramid_scratch_bytes(n, levels))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    outbuf = torch.empty(levels * 13 * n, dtype=torch.int32, device=dev)            # per level: coarse [n,4] | parent_of [n] | down [8n]
    parts = [(outbuf[13 * n * l:13 * n * l + 4 * n].view(n, 4), outbuf[13 * n * l + 4 * n:13 * n * l + 5 * n], outbuf[13 * n * l + 5 * n:13 * n * (l + 1)])
             for l in range(levels)]
    ptrs = lambda k: (ctypes.c_void_p * levels)(*[p[k].data_ptr() for p in parts])
    counts = (ctypes.c_int64 * levels)()
    check(lib().pcgc_pyramid(_p(fine), n, int(stride_fine), int(levels), _p(scratch), nbytes, ptrs(0), ptrs(1), ptrs(2), counts, _stream(fine)),
          'pyramid')
    out, below = [], n
    for l, (coarse_ub, parent_ub, down_ub) in enumerate(parts):
        nc = int(counts[l])
        out.append((coarse_ub[:nc], parent_ub[:below], down_ub[:8 * nc].view(8, nc)))
        below = nc
    return out


def compact_index(mask, prefix, n_out):
    orig = torch.empty(n_out, dtype=torch.int32, device=mask.device)
    check(lib().pcgc_compact_index(_p(mask), _p(prefix), mask.shape[0], _p(orig), _stream(mask)), 'compact_index')
    return orig


def kmap_k3_children(parent_nbr):
    n_parent = parent_nbr.shape[1]
    nbr = torch.empty((27, 8 * n_parent), dtype=torch.int32, device=parent_nbr.device)
    check(lib().pcgc_kmap_k3_children(_p(parent_nbr), n_parent, _p(nbr), _stream(parent_nbr)), 'kmap_k3_children')
    return nbr


def kmap_k3_prune(cand_nbr, mask, prefix, orig):
    n_out = orig.shape[0]
    nbr = torch.empty((27, n_out), dtype=torch.int32, device=cand_nbr.device)
    check(lib().pcgc_kmap_k3_prune(_p(cand_nbr), cand_nbr.shape[1], _p(mask), _p(prefix), _p(orig), n_out, _p(nbr), _stream(cand_nbr)),
          'kmap_k3_prune')
    return nbr


def kmap_k3_prune_parent(parent_nbr, mask, prefix, orig):
    """k3 map of a pruned children level from the PARENT level's map (no [27][8 n_parent] candidate map)."""
    n_out = orig.shape[0]
    nbr = torch.empty((27, n_out), dtype=torch.int32, device=parent_nbr.device)
    check(lib().pcgc_kmap_k3_prune_parent(_p(parent_nbr), parent_nbr.shape[1], _p(mask), _p(prefix), _p(orig), n_out, _p(nbr),
                                          _stream(parent_nbr)), 'kmap_k3_prune_parent')
    return nbr


def kmap_k3_from_coarse(fine, stride_fine, parent_of, coarse_nbr, down):
    n = fine.shape[0]
    nbr = torch.empty((27, n), dtype=torch.int32, device=fine.device)
    check(lib().pcgc_kmap_k3_from_coarse(_p(_i32(fine)), n, int(stride_fine), _p(parent_of), _p(coarse_nbr), _p(down),
                                         coarse_nbr.shape[1], _p(nbr), _stream(fine)), 'kmap_k3_from_coarse')
    return nbr


def mask_scan(mask):
    """-> (prefix int32 [n], total int32 [1] on device)."""
    n = mask.shape[0]
    prefix = torch.empty(n, dtype=torch.int32, device=mask.device)
    total = torch.empty(1, dtype=torch.int32, device=mask.device)
    ws_bytes = int(lib().pcgc_scan_workspace_bytes(n))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=mask.device)
    check(lib().pcgc_mask_scan(_p(_dev(mask, torch.uint8, 'mask')), n, _p(prefix), _p(total), _p(ws), ws_bytes, _stream(mask)),
          'mask_scan')
    return prefix, total


def compact_coords(coords, mask, prefix, n_out):
    out = torch.empty((n_out, 4), dtype=torch.int32, device=coords.device)
    check(lib().pcgc_compact_coords(_p(_i32(coords)), _p(mask), _p(prefix), coords.shape[0], _p(out), _stream(coords)),
          'compact_coords')
    return out


def compact_feats(feats, mask, prefix, n_out):
    _f32(feats)
    C = feats.shape[1]
    out = torch.empty((n_out, C), dtype=torch.float32, device=feats.device)
    check(lib().pcgc_compact_feats(_p(feats), C, _ld(feats), _p(mask), _p(prefix), feats.shape[0], _p(out), _stream(feats)),
          'compact_feats')
    return out


def coords_quantize(coords, stride_out):
    out = torch.empty_like(coords)
    check(lib().pcgc_coords_quantize(_p(_i32(coords)), coords.shape[0], int(stride_out), _p(out), _stream(coords)), 'coords_quantize')
    return out


def coords_children(coords, stride_in):
    out = torch.empty((8 * coords.shape[0], 4), dtype=torch.int32, device=coords.device)
    check(lib().pcgc_coords_children(_p(_i32(coords)), coords.shape[0], int(stride_in), _p(out), _stream(coords)), 'coords_children')
    return out


def coords_scale(coords, factor):
    out = torch.empty_like(coords)
    check(lib().pcgc_coords_scale(_p(_i32(coords)), coords.shape[0], float(np.float32(factor)), _p(out), _stream(coords)),
          'coords_scale')
    return out


def kmap_k3(coords, stride, table):
    n = coords.shape[0]
    nbr = torch.empty((27, n), dtype=torch.int32, device=coords.device)
    check(lib().pcgc_kmap_k3(_p(_i32(coords)), n, int(stride), _p(table.keys), _p(table.vals), table.cap, _p(nbr), _stream(coords)),
          'kmap_k3')
    return nbr


# ------------------------------------------------------------------------------------------------ conv family
def set_conv_impl(impl):
    """family of pcgc_conv_gather: -1 auto, 0 = direct-load VALU kernel, 2 = LDS-DMA + MFMA, 6 = row-split (bit-identical results)."""
    check(lib().pcgc_set_conv_impl(int(impl)), 'set_conv_impl')


def conv_gather(nbr, x, W, bias, out=None, residual=None, relu=False, n_out=None):
    """out (view, may be a column slice) = relu?( fmaf-chain(nbr, x, W) + bias (+ residual) )."""
    _f32(x, 'x'); _f32(W, 'W')
    if W.dim() == 2:
        K, (Cin, Cout) = 1, W.shape
    else:
        K, Cin, Cout = W.shape
    if x.shape[1] != Cin:
        raise PcgcError(f'conv_gather: input has {x.shape[1]} channels, kernel expects {Cin}')
    if nbr is None:
        n_out = x.shape[0]
    else:
        n_out = nbr.shape[1]
        if nbr.shape[0] != K:
            raise PcgcError('conv_gather: kernel map / kernel volume mismatch')
    if out is None:
        out = torch.empty((n_out, Cout), dtype=torch.float32, device=x.device)
    res_p, res_ld = (None, 0) if residual is None else (_p(_f32(residual)), _ld(residual))
    key = ('conv', Cin, Cout, n_out)
    wanted = K == 27 and PROFILE.want(key) and (key, roofline.k3_conv(
        f'k3 gather conv Cin={Cin} Cout={Cout} (k_conv_gather_mfma*/dma, per-row gather)', Cin, Cout, n_out, n_in=x.shape[0],
        issued=roofline.dense_issued(27, n_out, Cin, Cout) if Cin in (16, 32, 64) and Cout in (16, 32, 64) and n_out >= 8192 else None))
    check(PROFILE.launch(wanted, nbr if K == 27 else None, None, lib().pcgc_conv_gather, _p(nbr), K, n_out, _p(x), x.shape[0], Cin, _ld(x), 0, _p(W),
                         _p(bias), res_p, res_ld, 0, int(relu), _p(out), Cout, _ld(out), 0, _stream(nbr)), 'conv_gather')
    return out


def conv_gather_unit(nbr, W, bias, relu=False):
    """conv_gather for the all-ones single-channel input (the occupancy indicator every coded cloud starts from):
    out = relu?(sum of W[k][0][:] over the present offsets k, ascending, + bias)."""
    _f32(W, 'W')
    K, Cin, Cout = W.shape
    if Cin != 1 or nbr.shape[0] != K:
        raise PcgcError('conv_gather_unit: kernel [K, 1, Cout] and a [K, n] map expected')
    n_out = nbr.shape[1]
    out = torch.empty((n_out, Cout), dtype=torch.float32, device=W.device)
    key = ('conv', 1, Cout, n_out)
    wanted = K == 27 and PROFILE.want(key) and (key, roofline.unit_conv(
        f'k3 conv 1->{Cout} on the unit input (k_conv_unit: kernel map only, no feature gather)', Cout, n_out))
    check(PROFILE.launch(wanted, nbr if K == 27 else None, None, lib().pcgc_conv_gather_unit, _p(nbr), K, n_out, _p(W), _p(bias), int(relu), _p(out),
                         Cout, Cout, _stream(nbr)), 'conv_gather_unit')
    return out


def conv_unit_from_coarse(fine, stride_fine, parent_of, coarse_nbr, down, W, bias, relu=False):
    """conv_gather_unit on a pyramid level whose own k3 map was never built: presence from the parent level's map + the down map
    (pcgc_conv_unit_from_coarse); same sums, same order."""
    _f32(W, 'W')
    K, Cin, Cout = W.shape
    if Cin != 1 or K != 27:
        raise PcgcError('conv_unit_from_coarse: kernel [27, 1, Cout] expected')
    n = fine.shape[0]
    out = torch.empty((n, Cout), dtype=torch.float32, device=W.device)
    key = ('conv', 1, Cout, n)
    wanted = PROFILE.want(key) and (key, roofline.unit_conv(
        f'k3 conv 1->{Cout} on the unit input (k_conv_unit_coarse: presence from the parent level\'s map, no map of its own)', Cout, n, mapless=True))
    check(PROFILE.launch(wanted, None, None, lib().pcgc_conv_unit_from_coarse, _p(_i32(fine)), n, int(stride_fine), _p(parent_of), _p(coarse_nbr),
                         _p(down), coarse_nbr.shape[1], _p(W), _p(bias), int(relu), _p(out), Cout, Cout, _stream(fine)), 'conv_unit_from_coarse')
    return out


def set_sched_cus(cus):
    """the CU count every launcher sizes its grid by: 0 = the device's own; 1 = persistent grids of 8 workgroups (a few thousand rows reach a
    second round); 1 << 20 = one tile per wave.  Results never depend on it (tests of the tile schedules, csrc/tile_sched.h)."""
    check(lib().pcgc_set_sched_cus(int(cus)), 'set_sched_cus')


def last_sched():
    """(work units, workgroups, waves per workgroup) of this thread's most recent persistent tiled launch; after conv_packed64:
    (tiles, workgroups, rows per workgroup R)"""
    out = (ctypes.c_int64 * 3)()
    check(lib().pcgc_last_sched(out), 'last_sched')
    return tuple(int(v) for v in out)


def set_packed_rows(R):
    """rows per workgroup of conv_packed64: an even value in 40 .. 128, or 0 = chosen per launch (bit-identical results)"""
    check(lib().pcgc_set_packed_tuning(int(R), 0), 'set_packed_rows')


def set_up2_impl(mfma):
    """generative transpose conv kernel for 64->32 / 32->16: 2 fp32 MFMA with LDS-resident fragments (default), 1 fragments from L2, 0 VALU."""
    check(lib().pcgc_set_up2_impl(int(mfma)), 'set_up2_impl')


def irn_block(nbr, x, params):
    """Fused InceptionResNet block; params = [conv0_0.kernel, .bias, conv0_1.kernel, .bias, conv1_0..., conv1_1..., conv1_2...]."""
    _f32(x, 'x')
    n, C = x.shape
    t = torch.empty((n, C // 2), dtype=torch.float32, device=x.device)
    out = torch.empty((n, C), dtype=torch.float32, device=x.device)
    arr = (ctypes.c_void_p * 10)(*[p.data_ptr() for p in params])
    if PROFILE.counting:
        PROFILE.count(nbr)
    names = (f'k_irn_a<{C}, 16>', f'k_irn_b<{C}, 16>') if C == 64 else (f'k_irn_a_split<{C}>', f'k_irn_b_split<{C}>')
    if not (PROFILE.want((names[0], n)) or PROFILE.want((names[1], n))):
        check(lib().pcgc_irn_block(_p(nbr), n, _p(x), C, _ld(x), arr, _p(t), _p(out), C, _stream(nbr)), 'irn_block')
        return out
    for ps in (1, 2):
        key = (names[ps - 1], n)
        wanted = PROFILE.want(key) and (key, roofline.irn_pass(ps, key[0] + ' (per-row gather, VALU)', n, C, n))
        check(PROFILE.launch(wanted, None, None, lib().pcgc_irn_pass, _p(nbr), n, _p(x), C, _ld(x), arr, _p(t), _p(out), C, ps, _stream(nbr)), 'irn_pass')
    return out


# The MFMA forms of the block share one native signature (include/pcgc_hip.h: pcgc_irn_rows_pass, _rows_q4_pass, _child_pass, _child_q4) and
# differ in data only.  per_tile: MFMA instructions of pass A and pass B (its conv1_2 products included) per tile of `tile_rows` rows of the
# map the kernel walks — the level's own, or (parent_map) its parents' [27][n / 8] map; mfma_flops: flops of one such instruction.
_IrnVariant = namedtuple('_IrnVariant', 'entry label names desc per_tile tile_rows mfma_flops parent_map')
_ROWS, _CHILD = ' (fused InceptionResNet pass on a plain level, ', ' (fused InceptionResNet pass on a children level, packed-N fp32 MFMA)'
_IRN = {
    'rows64': _IrnVariant('pcgc_irn_rows_pass', 'irn_rows_pass', ('k_rows_irn_a64', 'k_rows_irn_b64'),
                          _ROWS + 'LDS-resident table + per-wave row ring, fp32 MFMA)', (27 * 16 + 16, 27 * 12 + 8), 16, 2048, False),
    # (pass A: 8 K-steps per offset; pass B: 2 + 2, + conv1_2)
    'rows32': _IrnVariant('pcgc_irn_rows_pass', 'irn_rows_pass', ('k_rows_irn_a32', 'k_rows_irn_b32'),
                          _ROWS + 'LDS-resident table + per-wave row ring, packed-N fp32 MFMA)', (27 * 8, 27 * 4 + 2), 16, 2048, False),
    # (4x4x1 instructions per 64-row M tile)
    'rows32_q4': _IrnVariant('pcgc_irn_rows_q4_pass', 'irn_rows_q4_pass', ('k_rows_q4_a32', 'k_rows_q4_b32'),
                             _ROWS + 'quad-block 4x4x1 fp32 MFMA, lane = row)', (112 * 16, 81 * 16 + 32), 64, 512, False),
    'child<16>': _IrnVariant('pcgc_irn_child_pass', 'irn_child_pass', ('k_child_irn_a<16>', 'k_child_irn_b<16>'), _CHILD, (416, 248), 16, 2048, True),
    'child<32>': _IrnVariant('pcgc_irn_child_pass', 'irn_child_pass', ('k_child_irn_a<32>', 'k_child_irn_b<32>'), _CHILD, (1216, 736), 16, 2048, True),
    # pass A in quad-block form writes t in its T2 layout; pass B is the packed-N kernel with T2 gather addresses (csrc/child_q4.hip).  Pass A per
    # 16 parents, in units of 2048 flops: 224 groups x 16 4x4x1 instructions (512 flops each) per 64 parents + the 128 transposing ones per 128
    'child_q4': _IrnVariant('pcgc_irn_child_q4', 'irn_child_pass', ('k_child_q4<0, 8, 2>', 'k_child_irn_b<16>'), _CHILD,
                            ((216 + 8) * 16 // 4 // 4 + 128 // 8 // 4, 248), 16, 2048, True),
}


def _irn_passes(v, nbr, x, params, ta, tb, passes=(1, 2), t=None):
    """Pass A (x -> t [n, C/2], table ta) and pass B (t, x -> out [n, C], table tb) of the fused block in the form `v` of _IRN, through
    the map `nbr` -> out; asked for pass A alone -> t."""
    _f32(x, 'x')
    n, C = x.shape
    m = nbr.shape[1]
    if 1 in passes:
        t = torch.empty((n, C // 2), dtype=torch.float32, device=x.device)
    out = torch.empty((n, C), dtype=torch.float32, device=x.device) if 2 in passes else None
    P = [p.data_ptr() for p in params]
    s = _stream(x)
    entry = getattr(lib(), v.entry)
    if PROFILE.counting:
        (PROFILE.count_children if v.parent_map else PROFILE.count)(nbr)
    for ps in passes:
        key = (v.names[ps - 1], n)
        wanted = PROFILE.want(key) and (key, roofline.irn_pass(ps, key[0] + v.desc, n, C, m,
                                                               (m + v.tile_rows - 1) // v.tile_rows * v.per_tile[ps - 1] * v.mfma_flops))
        if ps == 1:
            rc = PROFILE.launch(wanted, None, None, entry, _p(nbr), m, C, 1, _p(x), _ld(x), _p(ta), ta.numel() * 4, P[1], P[5], None, None, 0, _p(t), C // 2, s)
        else:
            rc = PROFILE.launch(wanted, None, None, entry, _p(nbr), m, C, 2, _p(t), C // 2, _p(tb), tb.numel() * 4, P[3], P[7], P[9], _p(x), _ld(x), _p(out), C, s)
        check(rc, v.label)
    return t if out is None else out


def irn_form_pass(form, nbr, x, params, tables, ps, t=None):
    """one pass of the fused block in the form `form` (a key of _IRN: 'rows64', 'rows32', 'rows32_q4', 'child<16>', 'child<32>', 'child_q4') on
    its own (A/B tools, schedule tests): ps = 1 -> t [n, C/2]; ps = 2 (t given) -> out [n, C]"""
    return _irn_passes(_IRN[form], nbr, x, params, *tables, passes=(ps,), t=t)


def irn_block_rows64(nbr, x, params, tables):
    """C = 64 InceptionResNet on a plain level through its own k3 map (k_rows_irn_a64, k_rows_irn_b64; tables = child_irn_tables(params));
    bit-identical to irn_block."""
    return _irn_passes(_IRN['rows64'], nbr, x, params, *tables)


def _rows_irn32_index():
    """Gather indices of the two pass tables of the plain-level C = 32 InceptionResNet (csrc/rows_irn.hip: RowsPassA32 / RowsPassB32)."""
    C, Q = 32, 8
    shapes = [(27, C, Q), (27, Q, 2 * Q), (C, Q), (27, Q, Q), (Q, 2 * Q)]
    off, Ws = 0, []
    for shp in shapes:
        n = int(np.prod(shp))
        Ws.append(np.arange(off, off + n, dtype=np.int64).reshape(shp))
        off += n
    W00, W01, W10, W11, W12 = Ws
    # pass A: one fragment per offset and 16-channel block: columns 0-7 conv0_0, columns 8-15 conv1_0 (centre offset only)
    fa = [_fragment([W00[k][:, co] for co in range(Q)] + [(W10[:, co] if k == 13 else None) for co in range(Q)], 2) for k in range(27)]
    # pass B: t rows are 16 wide: channels 0-7 (K-steps 0, 1) feed conv0_1, channels 8-15 (K-steps 2, 3) conv1_1 (columns 8-15 zero)
    pad = lambda w: np.concatenate([np.full(Q, -1, np.int64), w])
    fb = [_fragment([W01[k][:, co] for co in range(16)], 1, KS=2, k0=0) for k in range(27)]
    fb += [_fragment([pad(W11[k][:, co]) for co in range(Q)] + [None] * Q, 1, KS=2, k0=2) for k in range(27)]
    fb.append(_fragment([W12[:, co] for co in range(16)], 1, KS=2, k0=0))
    return np.concatenate([f.reshape(-1) for f in fa]), np.concatenate([f.reshape(-1) for f in fb])


def rows_irn32_tables(params):
    """(table A 54 KB, table B 27.5 KB) of the plain-level C = 32 InceptionResNet passes; params as in irn_block."""
    W00, b00, W01, b01, W10, b10, W11, b11, W12, b12 = params
    ia, ib = _table_index(('rows_irn32', W00.device), _rows_irn32_index)
    flat = torch.cat([w.detach().reshape(-1) for w in (W00, W01, W10, W11, W12)])
    return _gather_table(ia, flat), _gather_table(ib, flat)


def irn_block_rows32(nbr, x, params, tables):
    """C = 32 InceptionResNet on a plain level through its own k3 map (k_rows_irn_a32 / _b32); bit-identical to irn_block."""
    return _irn_passes(_IRN['rows32'], nbr, x, params, *tables)


def rows32_pass(nbr, x, params, tables, ps, t=None):
    """one pass of irn_block_rows32 on its own (A/B tools): ps = 1 -> t [n, 16]; ps = 2 (t given) -> out [n, 32]"""
    return _irn_passes(_IRN['rows32'], nbr, x, params, *tables, passes=(ps,), t=t)


def rows_q4_tables(params):
    """(table A 28 672 B, table B 21 248 B) of the quad-block C = 32 InceptionResNet passes on plain levels (csrc/rows_q4.hip); params as in
    irn_block.  Every fragment is [co 4][16 floats]: a lane's operands of one group are its output channel's 16 values, contiguous.
      A: [k = 0..26][channel half h][output group g] = W00[k][16 h + j][4 g + co], then [h][g] = W10[16 h + j][4 g + co]
      B: [k][X0, X1, Y]: X_p[co][8 half + j] = W01[k][j][4 (2 p + half) + co], Y[co][8 half + j] = W11[k][j][4 half + co];
         then conv1_2's two: [p][co][8 half + j] = W12[j][4 (2 p + half) + co]."""
    W00, b00, W01, b01, W10, b10, W11, b11, W12, b12 = params
    C = W00.shape[1]
    if C != 32:
        raise PcgcError('rows_q4_tables: C = 32')
    a0 = W00.detach().reshape(27, 2, 16, 2, 4).permute(0, 1, 3, 4, 2).reshape(-1)                 # [k][h][g][co][j]
    a1 = W10.detach().reshape(2, 16, 2, 4).permute(0, 2, 3, 1).reshape(-1)                          # [h][g][co][j]
    x01 = W01.detach().reshape(27, 8, 2, 2, 4).permute(0, 2, 4, 3, 1).reshape(27, 2, 64)            # [k][p][co][half][j]
    y11 = W11.detach().reshape(27, 8, 2, 4).permute(0, 3, 2, 1).reshape(27, 1, 64)                  # [k][co][half][j]
    w12 = W12.detach().reshape(8, 2, 2, 4).permute(1, 3, 2, 0).reshape(-1)                          # [p][co][half][j]
    return torch.cat([a0, a1]).contiguous(), torch.cat([torch.cat([x01, y11], 1).reshape(-1), w12]).contiguous()


def rows_q4_pass(nbr, x, params, tables, ps, t=None):
    """one pass of irn_block_rows32_q4 on its own (A/B tools)"""
    return _irn_passes(_IRN['rows32_q4'], nbr, x, params, *tables, passes=(ps,), t=t)


def irn_block_rows32_q4(nbr, x, params, tables):
    """C = 32 InceptionResNet on a plain level through its own k3 map, quad-block form (k_rows_q4_a32 / _b32); bit-identical to irn_block."""
    return _irn_passes(_IRN['rows32_q4'], nbr, x, params, *tables)


def set_rows_q4_variant(v):
    check(lib().pcgc_set_rows_q4_variant(int(v)), 'set_rows_q4_variant')


# ------------------------------------------------------------------------------------------------ children-level convs
def child_conv_table(W):
    """B-fragment table of pcgc_conv_child for a plain k3 conv `kernel` [27, Cin, Cout]:
    table[k][n][cb][lane][jj] = W[k][16 cb + 4 jj + (lane >> 4)][16 n + (lane & 15)]   (one lane-linear 1 KB fragment per
    (offset, column tile, 16-channel block): a lane's four K-step values are contiguous -> one conflict-free ds_read_b128)."""
    K, Cin, Cout = W.shape                                     # (K = 27; 8 for the k2 s2 down convs of conv_down_rows)
    NB, NT = Cin // 16, Cout // 16
    return W.detach().reshape(K, NB, 4, 4, NT, 16).permute(0, 4, 1, 3, 5, 2).contiguous().reshape(-1)       # [k][n][cb][mq][mi][jj]


def _fragment(col_weights, NB, KS=4, k0=0, half=False):
    """One B fragment per 16-channel block from `col_weights`: a list of 16 (8 if half) columns, each None (zero column) or an
    array [Cin_rows] giving that column's weight per input channel.  Layout [cb][lane = mq*16 + mi (mq*8 + mi if half)][jj]:
    value = column mi at input channel 16 cb + 4 (k0 + jj) + mq.  Entries nothing maps to are -1 (the builders below run on
    INDEX-valued weights: each "weight" is its own position in the flat parameter vector, so the result is a gather index)."""
    ncol = 8 if half else 16
    out = np.full((NB, 4, ncol, KS), -1, np.int64)
    for mi, w in enumerate(col_weights):
        if w is None:
            continue
        for cb in range(NB):
            for jj in range(KS):
                for mq in range(4):
                    ch = 16 * cb + 4 * (k0 + jj) + mq
                    if ch < len(w):
                        out[cb, mq, mi, jj] = w[ch]
    return out.reshape(NB, -1)


_TABLE_INDEX = {}          # (kind, C, device) -> int64 gather index (-1 = zero) into the flat parameter vector


def _table_index(key, make):
    """the weight-independent gather index (or tuple of indices) under `key`, uploaded on first use.  Published complete: the upload is
    a copy from pageable host memory, which returns only when the data is on the device, and the uploading stream is synchronised before
    the entry is stored (once per kind, C and device for the life of the process) — whichever stream or thread finds the entry may read it."""
    hit = _TABLE_INDEX.get(key)
    if hit is None:
        made = make()
        dev = key[-1]
        up = lambda a: None if a is None else torch.from_numpy(a).to(dev)
        hit = tuple(up(a) for a in made) if isinstance(made, tuple) else up(made)
        if torch.device(dev).type == 'cuda':
            torch.cuda.current_stream(dev).synchronize()
        _TABLE_INDEX[key] = hit
    return hit


def _gather_table(index, flat):
    return torch.where(index >= 0, flat[index.clamp(min=0)], torch.zeros((), dtype=flat.dtype, device=flat.device)).contiguous()


def _cls_index(C):
    """gather index of the compact classification-head table (csrc/child_kernels.h: ClsHead): 125 rows k' = 25 (kz + 1) + 5 (ky + 1) + (kx + 1),
    kz, ky, kx in -1 .. 3; a row with all three in 0 .. 2 is kernel[9 kz + 3 ky + kx] as [cb][mq][jj] -> channel 16 cb + 4 jj + mq, every other
    row is zero; rows are (C / 16) * 64 + 16 bytes apart, the table is padded to a multiple of 1 KB."""
    nb = C // 16
    rowf = nb * 16 + 4
    idx = np.full(((125 * rowf * 4 + 1023) // 1024 * 256,), -1, np.int64)
    for kz in range(3):
        for ky in range(3):
            for kx in range(3):
                r = 25 * (kz + 1) + 5 * (ky + 1) + (kx + 1)
                k = 9 * kz + 3 * ky + kx
                for cb in range(nb):
                    for mq in range(4):
                        for jj in range(4):
                            idx[r * rowf + cb * 16 + mq * 4 + jj] = k * C + 16 * cb + 4 * jj + mq
    return idx


def child_cls_table(W):
    """Table of the classification head (k3 conv C -> 1) for pcgc_conv_child: the kernel in a zero-padded 5 x 5 x 5 offset space (one
    ds_read_b128 per lane fetches the weights through which ITS child sees a cell, or zeros).  Built by one device gather through a
    cached index."""
    C = W.shape[1]
    return _gather_table(_table_index(('cls', C, W.device), lambda: _cls_index(C)), W.detach().reshape(-1))


def _q4_cls_index(C):
    """gather index of the quad-block classification head's table: one fragment [s 4][ci C] per (cell, z half h) group in the kernel's
    schedule order (cells ascending; h = 0 if the cell's z plane is reached by the children with z bit 0, then h = 1): column s =
    kernel[k(cell, 4 h + s)][:, 0] where child 4 h + s reaches the cell, zero elsewhere."""
    W = np.arange(27 * C, dtype=np.int64).reshape(27, C)
    frags = []
    for c, (kp, jc, reach) in enumerate(_halo_cells()):
        cz = c >> 4
        kof = dict(reach)
        for h in range(2):
            if not 0 <= cz - h <= 2:
                continue
            f = np.full((4, C), -1, np.int64)
            for sidx in range(4):
                if 4 * h + sidx in kof:
                    f[sidx] = W[kof[4 * h + sidx]]
            frags.append(f.reshape(-1))
    assert len(frags) == 96
    return np.concatenate(frags)


def child_q4_cls_table(W):
    """Table of pcgc_cls_child_q4 (k3 conv 16 -> 1 on a children level, quad-block form)."""
    C = W.shape[1]
    return _gather_table(_table_index(('q4cls', C, W.device), lambda: _q4_cls_index(C)), W.detach().reshape(-1))


def cls_child_q4(parent_nbr, x, table, bias):
    """Classification head k3 16 -> 1 on the children level of `parent_nbr`'s level in quad-block form (csrc/child_q4.h): -> [8 n_parent, 1]."""
    _f32(x, 'x')
    n_p = parent_nbr.shape[1]
    if x.shape[0] != 8 * n_p:
        raise PcgcError('cls_child_q4: feature rows must be 8 x the parent level')
    Cin = x.shape[1]
    n = 8 * n_p
    out = torch.empty((n, 1), dtype=torch.float32, device=x.device)
    key = ('child_conv', Cin, 1, n)
    wanted = PROFILE.want(key) and (key, roofline.child_conv(
        f'k_child_q4<1, 8, 2> (k3 {Cin}->1 on a children level, parent-map halo gather + quad-block 4x4x1 fp32 MFMA)', Cin, 1, n_p,
        issued=((n_p + 63) // 64) * 96 * 16 * 512))
    check(PROFILE.launch(wanted, None, parent_nbr, lib().pcgc_cls_child_q4, _p(parent_nbr), n_p, _p(x), Cin, _ld(x), _p(table), table.numel() * 4,
                         _p(bias), _p(out), _stream(x)), 'cls_child_q4')
    return out


def _irn_index(C):
    """Gather indices (into cat(W00, W01, W10, W11, W12) flattened) of the two pass tables; the fragment order is the one
    csrc/child_kernels.h's PassA / PassB variants index (frag())."""
    Q, NB = C // 4, C // 16
    shapes = [(27, C, Q), (27, Q, 2 * Q), (C, Q), (27, Q, Q), (Q, 2 * Q)]
    off, Ws = 0, []
    for shp in shapes:
        n = int(np.prod(shp))
        Ws.append(np.arange(off, off + n, dtype=np.int64).reshape(shp))
        off += n
    W00, W01, W10, W11, W12 = Ws
    cpt = 16 // Q                                             # children per Q-wide tile: 4 (C=16) or 2 (C=32)

    def packed(Wk3, width, kz, ky, cy, cx):
        """columns (child-in-tile, channel) of a tile whose children differ in x only (ky given) or in (y, x) (ky None):
        -> list of 16 columns for the cell at (cy, cx) seen through z-offset kz"""
        cols = []
        nchild = 16 // width
        for sub in range(nchild):
            if ky is None:                                     # tile = z half: sub = jy*2 + jx
                jy, jx = sub >> 1, sub & 1
                kyy = cy - jy
            else:                                              # tile = (z, y) quarter: sub = jx
                jx, kyy = sub, ky
            kxx = cx - jx
            ok = 0 <= kyy <= 2 and 0 <= kxx <= 2
            for co in range(width):
                cols.append(Wk3[kz * 9 + kyy * 3 + kxx][:, co] if ok else None)
        return cols

    # ---- pass A: conv0_0 (k3 C -> Q) fragments, then conv1_0 (k1) fragments for the cell that is the child itself
    fa = []
    if cpt == 1:                                               # C = 64: one child per tile = the offset's own slice; pass B stays on the per-row kernels
        for k in range(27):
            fa.append(_fragment([W00[k][:, co] for co in range(16)], NB))
        fa.append(_fragment([W10[:, co] for co in range(16)], NB))
        # pass B: conv0_1 (k3 16 -> 32) fragments (k, n), conv1_1 (k3 16 -> 16) fragments k, conv1_2 (k1 16 -> 32) fragments n: one 16-channel block each
        fb = []
        for k in range(27):
            for n2 in range(2):
                fb.append(_fragment([W01[k][:, 16 * n2 + co] for co in range(16)], 1))
        for k in range(27):
            fb.append(_fragment([W11[k][:, co] for co in range(16)], 1))
        for n2 in range(2):
            fb.append(_fragment([W12[:, 16 * n2 + co] for co in range(16)], 1))
        return np.concatenate([f.reshape(-1) for f in fa]), np.concatenate([f.reshape(-1) for f in fb])
    if cpt == 4:
        for kz in range(3):
            for cy in range(4):
                for cx in range(4):
                    fa.append(_fragment(packed(W00, Q, kz, None, cy, cx), NB))
        for vy in range(2):
            for vx in range(2):
                fa.append(_fragment([W10[:, co] if sub == vy * 2 + vx else None for sub in range(4) for co in range(Q)], NB))
    else:
        for kz in range(3):
            for ky in range(3):
                for cx in range(4):
                    fa.append(_fragment(packed(W00, Q, kz, ky, None, cx), NB))
        for vx in range(2):
            fa.append(_fragment([W10[:, co] if sub == vx else None for sub in range(2) for co in range(Q)], NB))
    table_a = np.concatenate([f.reshape(-1) for f in fa])
    # ---- pass B: input rows are t (2Q wide): conv0_1 reads channels [0, Q) = K-steps [0, KS), conv1_1 channels [Q, 2Q) = [KS, 2KS)
    KS = Q // 4
    H = 2 * Q
    fb = []
    pad = lambda w, lo: np.concatenate([np.full(lo, -1, np.int64), w])          # place a Q-vector at channel offset lo of the 2Q row
    if H == 16:                                                # C = 32: conv0_1 tile = one child, 16 columns
        for k in range(27):
            fb.append(_fragment([W01[k][:, co] for co in range(16)], 1, KS=KS, k0=0))
    else:                                                      # C = 16: conv0_1 tile = (z, y) quarter, (jx, 8 columns)
        for kz in range(3):
            for ky in range(3):
                for cx in range(4):
                    fb.append(_fragment(packed(W01, H, kz, ky, None, cx), 1, KS=KS, k0=0))
    W11p = np.stack([np.stack([pad(W11[k][:, co], Q) for co in range(Q)], 1) for k in range(27)])      # [27][2Q][Q]: rows Q.. hold W11
    if cpt == 2:                                               # C = 32: conv1_1 tile = (z, y) quarter, (jx, 8 columns)
        for kz in range(3):
            for ky in range(3):
                for cx in range(4):
                    fb.append(_fragment(packed(W11p, Q, kz, ky, None, cx), 1, KS=KS, k0=KS))
    else:                                                      # C = 16: conv1_1 tile = z half, (jy jx, 4 columns)
        for kz in range(3):
            for cy in range(4):
                for cx in range(4):
                    fb.append(_fragment(packed(W11p, Q, kz, None, cy, cx), 1, KS=KS, k0=KS))
    fb.append(_fragment([W12[:, co] if co < H else None for co in range(16)], 1, KS=KS, k0=0))     # conv1_2 (k1 Q -> 2Q)
    table_b = np.concatenate([f.reshape(-1) for f in fb])
    return table_a, table_b


def child_irn_tables(params):
    """(table A, table B) of the parent-map InceptionResNet passes (C = 16 or 32); params as in irn_block.  Two device gathers
    through cached indices: cheap enough to redo whenever a checkpoint is loaded (R-D sweeps load one per rate)."""
    W00, b00, W01, b01, W10, b10, W11, b11, W12, b12 = params
    C = W00.shape[1]
    ia, ib = _table_index(('irn', C, W00.device), lambda: _irn_index(C))
    flat = torch.cat([w.detach().reshape(-1) for w in (W00, W01, W10, W11, W12)])
    return _gather_table(ia, flat), (None if ib is None else _gather_table(ib, flat))


def child_q4_tables(params):
    """Table of the quad-block pass A (pcgc_irn_child_q4, C = 16): [27][co 4][ci 16] = conv0_0.kernel[k][ci][co], then [co 4][ci 16] =
    conv1_0.kernel[0][ci][co] — a lane's operands of one (cell, child) pair are its output channel's 16 input channels, contiguous."""
    W00, W10 = params[0], params[4]
    C = W00.shape[1]
    return torch.cat([W00.detach().reshape(27, C, C // 4).permute(0, 2, 1).reshape(-1),
                      W10.detach().reshape(C, C // 4).t().reshape(-1)]).contiguous()


def irn_block_child(parent_nbr, x, params, tables, q4_table=None):
    """Fused InceptionResNet on a children level through the parent map (C = 16, 32); bit-identical to irn_block."""
    _f32(x, 'x')
    n, C = x.shape
    if n != 8 * parent_nbr.shape[1]:
        raise PcgcError('irn_block_child: feature rows must be 8 x the parent level')
    if PATH.CHILD_Q4 and C == 16 and q4_table is not None:
        return _irn_passes(_IRN['child_q4'], parent_nbr, x, params, q4_table, tables[1])
    return _irn_passes(_IRN[f'child<{C}>'], parent_nbr, x, params, *tables)


def conv_child(parent_nbr, x, table, bias, Cout, out=None, residual=None, relu=False):
    """k3 conv on the children level of `parent_nbr`'s level: x has 8 * n_parent rows."""
    _f32(x, 'x')
    n_p = parent_nbr.shape[1]
    if x.shape[0] != 8 * n_p:
        raise PcgcError('conv_child: feature rows must be 8 x the parent level')
    Cin = x.shape[1]
    if out is None:
        out = torch.empty((8 * n_p, Cout), dtype=torch.float32, device=x.device)
    res_p, res_ld = (None, 0) if residual is None else (_p(_f32(residual)), _ld(residual))
    n = 8 * n_p
    key = ('child_conv', Cin, Cout, n)
    # (MFMA instructions per 16-parent tile: 64 per 16-channel block and K-step for the head, 216 per block pair and K-step otherwise)
    wanted = PROFILE.want(key) and (key, roofline.child_conv(
        (f'k_child_cls<{Cin // 16}>' if Cout == 1 else f'k_child_conv<{Cin // 16}, {Cout // 16}>')
        + f' (k3 {Cin}->{Cout} on a children level, parent-map halo gather + fp32 MFMA)', Cin, Cout, n_p, residual is not None,
        (n_p + 15) // 16 * (64 * (Cin // 16) * 4 if Cout == 1 else 216 * (Cin // 16) * (Cout // 16) * 4) * 2048))
    check(PROFILE.launch(wanted, None, parent_nbr, lib().pcgc_conv_child, _p(parent_nbr), n_p, _p(x), Cin, _ld(x), _p(table), table.numel() * 4,
                         _p(bias), res_p, res_ld, int(relu), _p(out), Cout, _ld(out), _stream(x)), 'conv_child')
    return out


def conv_rows(nbr, x, table, bias, Cout, out=None, residual=None, relu=False):
    """k3 conv 32 -> 32 on a plain level through its own map (csrc/rows_irn.hip: k_rows_conv); table = child_conv_table(kernel)."""
    _f32(x, 'x')
    n, Cin = x.shape
    if out is None:
        out = torch.empty((n, Cout), dtype=torch.float32, device=x.device)
    res_p, res_ld = (None, 0) if residual is None else (_p(_f32(residual)), _ld(residual))
    key = ('conv', Cin, Cout, n)
    wanted = PROFILE.want(key) and (key, roofline.k3_conv(
        f'k_rows_conv<{Cin // 16}, {Cout // 16}> (k3 {Cin}->{Cout} on a plain level, LDS-resident table + per-wave row ring, fp32 MFMA)', Cin, Cout, n,
        residual=residual is not None, issued=roofline.dense_issued(27, n, Cin, Cout)))
    check(PROFILE.launch(wanted, nbr, None, lib().pcgc_conv_rows, _p(nbr), n, _p(x), Cin, _ld(x), _p(table), table.numel() * 4, _p(bias), res_p, res_ld,
                         int(relu), _p(out), Cout, _ld(out), _stream(x)), 'conv_rows')
    return out


def conv_packed64(nbr, x, table, bias, relu=False):
    """k3 conv 64 -> 64 on a level with its own map, present rows packed per workgroup tile and offset (pcgc_conv_packed64)."""
    _f32(x, 'x')
    n = x.shape[0]
    out = torch.empty((n, 64), dtype=torch.float32, device=x.device)
    key = ('conv', 64, 64, n)
    # MFMA flops issued: the present pairs in packed 16-row tiles, plus about half a tile of padding per (workgroup tile of ~96 rows, offset)
    wanted = PROFILE.want(key) and (key, roofline.k3_conv(
        'k_conv_packed64 (k3 64->64, present-row packing: accumulators in LDS, B fragments in registers, fp32 MFMA)', 64, 64, n,
        issued=lambda P: 2 * (P + 8 * 27 * ((n + 95) // 96)) * 64 * 64))
    check(PROFILE.launch(wanted, nbr, None, lib().pcgc_conv_packed64, _p(nbr), n, _p(x), _ld(x), _p(table), table.numel() * 4, _p(bias), int(relu),
                         _p(out), 64, _stream(x)), 'conv_packed64')
    return out


def conv_down_rows(down, x, table, bias, Cout, relu=False):
    """k2 s2 down conv through the `down` map [8][n_coarse] (csrc/rows_irn.hip: k_rows_down); table = child_conv_table(kernel)."""
    _f32(x, 'x')
    n_in, Cin = x.shape
    n_c = down.shape[1]
    out = torch.empty((n_c, Cout), dtype=torch.float32, device=x.device)
    key = ('down', Cin, Cout, n_c)
    wanted = PROFILE.want(key) and (key, roofline.down_conv(
        f'k_rows_down<{Cin // 16}, {Cout // 16}> (k2 s2 {Cin}->{Cout} through the down map, LDS-resident table, fp32 MFMA)', Cin, Cout, n_c, n_in))
    check(PROFILE.launch(wanted, None, None, lib().pcgc_conv_down_rows, _p(down), n_c, _p(x), n_in, Cin, _ld(x), _p(table), table.numel() * 4, _p(bias),
                         int(relu), _p(out), Cout, _ld(out), _stream(x)), 'conv_down_rows')
    return out


def conv_up2(x, W, bias, relu=False, rows=None):
    """MinkowskiGenerativeConvolutionTranspose k2 s2.  rows (int32 [n]): the input level is rows `rows` of x, read in place (a pruned
    level whose compacted features were never written); shapes without such a kernel gather the rows first."""
    _f32(x, 'x'); _f32(W, 'W')
    K, Cin, Cout = W.shape
    n_in = x.shape[0] if rows is None else rows.shape[0]
    key = ('up2', Cin, Cout, 8 * n_in)
    wanted = PROFILE.want(key) and (key, _up2_work(Cin, Cout, n_in, rows is not None))
    return PROFILE.launch(wanted, None, None, _conv_up2, x, W, bias, relu, rows)      # (the bracket closes on the early return too)


def _up2_work(Cin, Cout, n_in, rows):
    mfma = (Cin, Cout) in ((64, 32), (32, 16))
    return roofline.up2_conv(f'k_conv_up2<{Cin}, {Cout}> (generative transpose k2 s2, ' + ('eight GEMMs sharing the A fragments, fp32 MFMA)' if mfma else
                             'one thread per (row, 16-byte chunk), VALU)'), Cin, Cout, n_in, rows, mfma)


def _conv_up2(x, W, bias, relu, rows):
    Cin, Cout = W.shape[1:]
    if rows is not None:
        out = torch.empty((8 * rows.shape[0], Cout), dtype=torch.float32, device=x.device)
        rc = lib().pcgc_conv_up2_gather(rows.shape[0], _p(x), Cin, _ld(x), _p(rows), _p(W), _p(bias), int(relu), _p(out), Cout, _stream(x))
        if rc == 0:
            return out
        if rc != -3:
            check(rc, 'conv_up2_gather')
        x = gather_rows(x, rows)
    out = torch.empty((8 * x.shape[0], Cout), dtype=torch.float32, device=x.device)
    check(lib().pcgc_conv_up2(x.shape[0], _p(x), Cin, _ld(x), _p(W), _p(bias), int(relu), _p(out), Cout, _stream(x)), 'conv_up2')
    return out


# ------------------------------------------------------------------------------------------------ select / sort
def topk_mask(logits, k):
    """logits: [n,1] or [n] fp32 view -> uint8 mask [n] of the k largest (ties: lower row)."""
    _f32(logits, 'logits')
    n = logits.shape[0]
    ld = logits.stride(0)
    mask = torch.empty(n, dtype=torch.uint8, device=logits.device)
    ws_bytes = int(lib().pcgc_topk_workspace_bytes(n))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=logits.device)
    check(lib().pcgc_topk_mask(_p(logits), ld, n, int(k), _p(mask), _p(ws), ws_bytes, _stream(logits)), 'topk_mask')
    return mask


def sort_zyx(coords, batch_major=False):
    """argsort by (z, y, x, batch) — array2vector's order — or, batch_major, by (batch, z, y, x): the items of a collated batch stay
    contiguous, each in the order it has when coded alone."""
    n = coords.shape[0]
    perm = torch.empty(n, dtype=torch.int32, device=coords.device)
    ws_bytes = int(lib().pcgc_sort_workspace_bytes(n))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=coords.device)
    fn = lib().pcgc_sort_bzyx if batch_major else lib().pcgc_sort_zyx
    check(fn(_p(_i32(coords)), n, _p(perm), _p(ws), ws_bytes, _stream(coords)), 'sort_zyx')
    return perm


def batch_counts(coords):
    """rows per batch item (column 0), trailing empty items dropped -> list of ints (one device histogram + read-back)."""
    counts = torch.empty(16, dtype=torch.int32, device=coords.device)
    check(lib().pcgc_batch_counts(_p(_i32(coords)), coords.shape[0], _p(counts), _stream(coords)), 'batch_counts')
    c = counts.cpu().tolist()
    while len(c) > 1 and c[-1] == 0:
        c.pop()
    return c


def _i64_array(values):
    return (ctypes.c_int64 * len(values))(*[int(v) for v in values])


def topk_mask_segments(logits, seg_rows, seg_k):
    """istopk per batch item (data_utils.py:77-89): item b = the next seg_rows[b] rows, keeps its seg_k[b] largest logits."""
    _f32(logits, 'logits')
    n = logits.shape[0]
    if sum(seg_rows) != n:
        raise PcgcError(f'topk_mask_segments: segments cover {sum(seg_rows)} of {n} rows')
    mask = torch.empty(n, dtype=torch.uint8, device=logits.device)
    ws_bytes = int(lib().pcgc_topk_workspace_bytes(n))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=logits.device)
    check(lib().pcgc_topk_mask_segments(_p(logits), logits.stride(0), len(seg_rows), _i64_array(seg_rows), _i64_array(seg_k), _p(mask), _p(ws),
                                        ws_bytes, _stream(logits)), 'topk_mask_segments')
    return mask


def topk_select(logits, seg_rows, seg_k, coords=None, parent_coords=None, parent_stride=0):
    """prune_voxel in one sweep (autoencoder.py:239-249): per item b the seg_k[b] largest logits among its seg_rows[b] rows (istopk's tie
    rule) -> (bits uint8, wprefix int32: the rank bitmap of the candidate level; orig int32 [K]: the candidate row of every survivor;
    out_coords int32 [K, 4]).  The candidates' coordinates are `coords`, or derived from `parent_coords` (rows 8 i + j of a children
    level at parent_stride / 2)."""
    _f32(logits, 'logits')
    n = logits.shape[0]
    if sum(seg_rows) != n:
        raise PcgcError(f'topk_select: segments cover {sum(seg_rows)} of {n} rows')
    if len(seg_rows) > 16:
        raise PcgcError('topk_select: at most 16 segments')
    K = sum(int(min(max(k, 0), r)) for r, k in zip(seg_rows, seg_k))
    dev = logits.device
    words = (n + 63) // 64
    bits = torch.empty(words * 8, dtype=torch.uint8, device=dev)
    wprefix = torch.empty(words, dtype=torch.int32, device=dev)
    orig = torch.empty(K, dtype=torch.int32, device=dev)
    out = torch.empty((K, 4), dtype=torch.int32, device=dev)
    ws_bytes = int(lib().pcgc_topk_select_workspace_bytes(n))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    check(lib().pcgc_topk_select(_p(logits), logits.stride(0), len(seg_rows), _i64_array(seg_rows), _i64_array(seg_k),
                                 _p(None if coords is None else _i32(coords)), _p(None if parent_coords is None else _i32(parent_coords)),
                                 int(parent_stride), _p(bits), _p(wprefix), _p(orig), _p(out), _p(ws), ws_bytes, _stream(logits)), 'topk_select')
    return bits, wprefix, orig, out


def kmap_k3_prune_sel(cand_nbr, bits, wprefix, orig):
    n_out = orig.shape[0]
    nbr = torch.empty((27, n_out), dtype=torch.int32, device=cand_nbr.device)
    check(lib().pcgc_kmap_k3_prune_sel(_p(cand_nbr), cand_nbr.shape[1], _p(bits), _p(wprefix), _p(orig), n_out, _p(nbr), _stream(cand_nbr)),
          'kmap_k3_prune_sel')
    return nbr


def kmap_k3_prune_parent_sel(parent_nbr, bits, wprefix, orig):
    """k3 map of a pruned children level from the PARENT level's map and the rank bitmap of ops.topk_select."""
    n_out = orig.shape[0]
    nbr = torch.empty((27, n_out), dtype=torch.int32, device=parent_nbr.device)
    check(lib().pcgc_kmap_k3_prune_parent_sel(_p(parent_nbr), parent_nbr.shape[1], _p(bits), _p(wprefix), _p(orig), n_out, _p(nbr),
                                              _stream(parent_nbr)), 'kmap_k3_prune_parent_sel')
    return nbr


def gather_rows(feats, orig):
    """out[r] = feats[orig[r]] (feats: 2-D row-major view with a leading dimension; channels % 4 == 0)."""
    _f32(feats)
    C = feats.shape[1]
    out = torch.empty((orig.shape[0], C), dtype=torch.float32, device=feats.device)
    check(lib().pcgc_gather_rows_f32_ld(_p(feats), C, _ld(feats), _p(orig), orig.shape[0], _p(out), _stream(feats)), 'gather_rows_f32_ld')
    return out


def gather_coords(coords, perm):
    out = torch.empty_like(coords)
    check(lib().pcgc_gather_rows_i32x4(_p(_i32(coords)), _p(perm), coords.shape[0], _p(out), _stream(coords)), 'gather_rows_i32x4')
    return out


def gather_feats(feats, perm):
    feats = _f32(feats).contiguous()
    out = torch.empty_like(feats)
    check(lib().pcgc_gather_rows_f32(_p(feats), feats.shape[1], _p(perm), feats.shape[0], _p(out), _stream(feats)), 'gather_rows_f32')
    return out


# ------------------------------------------------------------------------------------------------ pointwise (ME-style graphs)
def relu(x, inplace=False):
    x = _f32(x).contiguous()
    out = x if inplace else torch.empty_like(x)
    check(lib().pcgc_relu(_p(x), x.numel(), _p(out), _stream(x)), 'relu')
    return out


def add(a, b):
    a, b = _f32(a).contiguous(), _f32(b).contiguous()
    if a.shape != b.shape:
        raise PcgcError(f'add: shapes {tuple(a.shape)} and {tuple(b.shape)} differ')
    out = torch.empty_like(a)
    check(lib().pcgc_add(_p(a), _p(b), a.numel(), _p(out), _stream(a)), 'add')
    return out


# ------------------------------------------------------------------------------------------------ entropy
def round_minmax(feats):
    feats = _f32(feats).contiguous()
    mm = torch.empty(2, dtype=torch.float32, device=feats.device)
    check(lib().pcgc_round_minmax(_p(feats), feats.numel(), _p(mm), _stream(feats)), 'round_minmax')
    return mm


def symbolize(feats, min_v):
    feats = _f32(feats).contiguous()
    sym = torch.empty(feats.shape, dtype=torch.int16, device=feats.device)
    check(lib().pcgc_symbolize(_p(feats), feats.numel(), float(min_v), _p(sym), _stream(feats)), 'symbolize')
    return sym


def desymbolize(sym, min_v):
    out = torch.empty(sym.shape, dtype=torch.float32, device=sym.device)
    check(lib().pcgc_desymbolize(_p(_dev(sym, torch.int16, 'sym')), sym.numel(), float(min_v), _p(out), _stream(sym)), 'desymbolize')
    return out


def check_symbol_range(min_v, max_v, what='latent'):
    """Raise PcgcError unless [min_v, max_v] is a range int16 symbols can code: both finite and fewer than 32768 values (the reference has the
    same limit, entropy_model.py:151-176, and wraps silently beyond it).  A NaN or infinite latent shows here: the device's min / max order
    NaN beyond the infinity of its sign.  Called with the range that comes back with the symbols anyway: no launch, no copy."""
    lo, hi = float(min_v), float(max_v)
    if not (np.isfinite(lo) and np.isfinite(hi)):
        raise PcgcError(f'{what}: the rounded values range from {lo} to {hi}: a latent that is not finite cannot be coded')
    if hi - lo + 1 >= 32768:
        raise PcgcError(f'{what}: the rounded values range from {lo:.0f} to {hi:.0f}, an alphabet of {hi - lo + 1:.0f} symbols; '
                        'int16 symbols code at most 32767')


def quantize_symbols(feats):
    """-> (min_v, max_v as np.float32, sym int16 ndarray of feats.shape): round + symbol range + symbolise on the device,
    ONE synchronising device->host copy of [min | max | symbols].  Raises PcgcError for a range int16 symbols cannot code."""
    feats = _f32(feats).contiguous()
    n = feats.numel()
    buf = torch.empty(4 + n, dtype=torch.int16, device=feats.device)          # [minmax as 2 fp32 = 4 int16 | sym]
    check(lib().pcgc_quantize_symbols(_p(feats), n, _p(buf), buf.data_ptr() + 8, _stream(feats)), 'quantize_symbols')
    host = buf.cpu().numpy()
    mm = host[:4].view(np.float32)
    check_symbol_range(mm[0], mm[1], 'quantize_symbols')
    return np.float32(mm[0]), np.float32(mm[1]), host[4:].reshape(feats.shape)


def quantize_symbols_segments(feats, seg_rows):
    """quantize_symbols per batch item (contiguous row segments), ONE synchronising copy
    -> ([(min_v, max_v)] per item as np.float32, sym int16 ndarray of feats.shape)."""
    feats = _f32(feats).contiguous()
    n, C = feats.shape
    B = len(seg_rows)
    if sum(seg_rows) != n:
        raise PcgcError(f'quantize_symbols_segments: segments cover {sum(seg_rows)} of {n} rows')
    buf = torch.empty(4 * B + n * C, dtype=torch.int16, device=feats.device)          # [B x (min, max) fp32 | symbols]
    check(lib().pcgc_quantize_symbols_segments(_p(feats), C, B, _i64_array(seg_rows), _p(buf), buf.data_ptr() + 8 * B, _stream(feats)),
          'quantize_symbols_segments')
    host = buf.cpu().numpy()
    mm = host[:4 * B].view(np.float32).reshape(B, 2)
    for b, (lo, hi) in enumerate(mm):
        check_symbol_range(lo, hi, f'quantize_symbols_segments: item {b}')
    return [(np.float32(a), np.float32(b)) for a, b in mm], host[4 * B:].reshape(n, C)


def cdf_table(params, C, min_v, max_v):
    """-> (cdf_u16 as int16-typed tensor [C, L+1] holding the uint16 bit patterns, cdf_f32 [C, L+1])."""
    L = int(max_v - min_v) + 1
    q = torch.empty((C, L + 1), dtype=torch.int16, device=params.device)
    f = torch.empty((C, L + 1), dtype=torch.float32, device=params.device)
    check(lib().pcgc_cdf_table(_p(_f32(params, 'params')), C, float(min_v), float(max_v), _p(q), _p(f), _stream(params)), 'cdf_table')
    return q, f


# ------------------------------------------------------------------------------------------------ forward losses (csrc/loss.hip)
def _loss_ws(elements, device):
    nbytes = int(lib().pcgc_loss_workspace_bytes(int(elements)))
    return torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=device), nbytes


def hash_contains(coords, table, or_mask=None):
    """data_utils.isin on device: uint8 [n], 1 where row i of coords [n, 4] (batch, x, y, z) is a key of `table` (a HashTable, or None for
    the empty set), OR-ed with the uint8 mask `or_mask` when given."""
    n = coords.shape[0]
    mask = torch.empty(n, dtype=torch.uint8, device=coords.device)
    if or_mask is not None and (_dev(or_mask, torch.uint8, 'or_mask').shape[0] != n):
        raise PcgcError('hash_contains: or_mask length differs from the number of rows')
    keys, vals, cap = (None, None, 0) if table is None else (table.keys, table.vals, table.cap)
    check(lib().pcgc_hash_contains(_p(_i32(coords)), n, _p(keys), _p(vals), cap, _p(or_mask), _p(mask), _stream(coords)), 'hash_contains')
    return mask


def eb_likelihood(feats, params, bound=1e-9, want_likelihood=True, want_bits=False):
    """EntropyBottleneck._likelihood (+ the lower bound, 0 = none) at feats [n, C] -> likelihood fp32 [n, C] and / or bits float64 [1]
    = -sum log2(likelihood); (likelihood, bits) with None for what was not asked for."""
    _f32(feats, 'feats')
    n, C, ld = feats.shape[0], feats.shape[1], _ld(feats)
    dev = feats.device
    lik = torch.empty((n, C), dtype=torch.float32, device=dev) if want_likelihood else None
    bits = torch.empty(1, dtype=torch.float64, device=dev) if want_bits else None
    ws, ws_bytes = _loss_ws(n * C, dev) if want_bits else (None, 0)
    check(lib().pcgc_eb_likelihood(_p(feats), ld, n, C, _p(_f32(params, 'params')), float(bound), _p(lik), _p(bits), _p(ws), ws_bytes,
                                   _stream(feats)), 'eb_likelihood')
    return lik, bits


def neg_log2_sum(x):
    """-sum log2(x) of an fp32 [n, C] view, in fp64 and in a fixed order -> float64 [1]"""
    _f32(x, 'likelihood')
    n, C, ld = x.shape[0], x.shape[1], _ld(x)
    bits = torch.empty(1, dtype=torch.float64, device=x.device)
    ws, ws_bytes = _loss_ws(n * C, x.device)
    check(lib().pcgc_neg_log2_sum(_p(x), ld, n, C, _p(bits), _p(ws), ws_bytes, _stream(x)), 'neg_log2_sum')
    return bits


def bce_logits(logits, truth, pred=None):
    """One pass over logits ([n] or [n, 1] fp32 view, or None), the uint8 truth mask and an optional uint8 prediction mask
    -> (bce float64 [1] = sum of the BCE-with-logits terms / ln 2, counts int64 [4] = TP, FN, FP, TN)."""
    n, dev = truth.shape[0], truth.device
    _dev(truth, torch.uint8, 'truth')
    if pred is not None and _dev(pred, torch.uint8, 'pred').shape[0] != n:
        raise PcgcError('bce_logits: masks of different lengths')
    ld = 1
    if logits is not None:
        _f32(logits, 'logits')
        if logits.shape[0] != n or logits.dim() > 2 or (logits.dim() == 2 and logits.shape[1] != 1):
            raise PcgcError(f'bce_logits: logits {tuple(logits.shape)} against a mask of {n} rows')
        ld = max(int(logits.stride(0)), 1)
    bce = torch.empty(1, dtype=torch.float64, device=dev)
    counts = torch.empty(4, dtype=torch.int64, device=dev)
    ws, ws_bytes = _loss_ws((n + 3) // 4, dev)
    check(lib().pcgc_bce_logits(_p(logits), ld, n, _p(truth), _p(pred), _p(bce), _p(counts), _p(ws), ws_bytes, _stream(truth)), 'bce_logits')
    return bce, counts


# ------------------------------------------------------------------------------------------------ lossless mode (csrc/occupancy.hip)
def occ_symbols(logits, truth=None):
    """One pass over a level's logits ([n] or [n, 1] fp32 view) -> packed int16 [n] = ctx << 1 | bit (occupancy_model.py: ctx from the
    logit, bit = truth[i] != 0; the words are < 2^10), and, with the uint8 truth mask, sums int64 [2] = (occupied rows, ideal code
    length in 2^-16 bit).  truth=None (the decoder's side): contexts only, (packed, None).  Both are views of ONE buffer, sums first."""
    _f32(logits, 'logits')
    n, dev = logits.shape[0], logits.device
    if logits.dim() > 2 or (logits.dim() == 2 and logits.shape[1] != 1):
        raise PcgcError(f'occ_symbols: logits {tuple(logits.shape)}, expected [n] or [n, 1]')
    ld = max(int(logits.stride(0)), 1)
    buf = torch.empty(8 + n, dtype=torch.int16, device=dev)                    # [sums as 2 int64 = 8 int16 | packed]
    packed, sums, ws, ws_bytes = buf[8:], None, None, 0
    if truth is not None:
        if _dev(truth, torch.uint8, 'truth').shape[0] != n:
            raise PcgcError(f'occ_symbols: {n} logits against a mask of {truth.shape[0]} rows')
        sums = buf[:8].view(torch.int64)
        ws_bytes = int(lib().pcgc_occ_workspace_bytes(n))
        ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=dev)
    check(lib().pcgc_occ_symbols(_p(logits), ld, n, _p(truth), _p(packed), _p(sums), _p(ws), ws_bytes, _stream(logits)), 'occ_symbols')
    return packed, sums


def occ_words_host(packed, sums=None):
    """what occ_symbols returned, brought to the host in ONE synchronising copy -> (words uint16 ndarray [n] in candidate-row order,
    occupied rows, ideal code length in 2^-16 bit); the two numbers are None without sums."""
    if sums is None:
        return packed.cpu().numpy().view(np.uint16), None, None
    host = packed._base.cpu().numpy()                                          # [sums | packed]: one buffer (occ_symbols)
    both = host[:8].view(np.int64)
    return host[8:].view(np.uint16), int(both[0]), int(both[1])


OCC_MAX_FRAMES = 16                                                               # frames of one pcgc_occ_symbols_segments / pcgc_occ_rans_*_batch call


def _frame_rows(rows_per_frame, what):
    rows = np.asarray(rows_per_frame, dtype=np.int64).reshape(-1)
    if not 1 <= rows.size <= OCC_MAX_FRAMES:
        raise ValueError(f'{what}: {rows.size} frames; a call takes 1 to {OCC_MAX_FRAMES}')
    if (rows < 0).any() or int(rows.sum()) >= 1 << 31:
        raise ValueError(f'{what}: row counts {rows.tolist()} (each >= 0, below 2^31 in all)')
    return rows


def occ_symbols_segments(logits, seg_rows, truth=None):
    """occ_symbols over the contiguous frames of a batch's level: frame f is the next seg_rows[f] rows -> (packed int16 [n], what occ_symbols
    gives for the whole level, sums int64 [B, 2] on the device: every frame's pair, equal to occ_symbols of that frame alone).  truth=None:
    contexts only, (packed, None).  Both are views of ONE buffer, sums first."""
    rows = _frame_rows(seg_rows, 'occ_symbols_segments')
    _f32(logits, 'logits')
    n, dev = logits.shape[0], logits.device
    if logits.dim() > 2 or (logits.dim() == 2 and logits.shape[1] != 1) or int(rows.sum()) != n:
        raise PcgcError(f'occ_symbols_segments: logits {tuple(logits.shape)}, expected [n] or [n, 1] with n = {int(rows.sum())}, the frames\' rows')
    B, ld = rows.size, max(int(logits.stride(0)), 1)
    buf = torch.empty(8 * B + n, dtype=torch.int16, device=dev)                # [sums as 2 B int64 = 8 B int16 | packed]
    packed, sums = buf[8 * B:], None
    if truth is not None:
        if _dev(truth, torch.uint8, 'truth').shape[0] != n:
            raise PcgcError(f'occ_symbols_segments: {n} logits against a mask of {truth.shape[0]} rows')
        sums = buf[:8 * B].view(torch.int64).view(B, 2)
    check(lib().pcgc_occ_symbols_segments(_p(logits), ld, B, rows.ctypes.data, _p(truth), _p(packed), _p(sums), _stream(logits)), 'occ_symbols_segments')
    return packed, sums


def occ_words_host_segments(packed, sums):
    """what occ_symbols_segments returned with a truth mask, brought to the host in ONE synchronising copy -> (words uint16 ndarray [n],
    occupied rows per frame, ideal code length per frame in 2^-16 bit; both int64 ndarrays [B])."""
    B = sums.shape[0]
    host = packed._base.cpu().numpy()                                          # [sums | packed]: one buffer (occ_symbols_segments)
    both = host[:8 * B].view(np.int64).reshape(B, 2)
    return host[8 * B:].view(np.uint16), both[:, 0].copy(), both[:, 1].copy()


def occ_tables():
    """the library's copy of the lossless mode's format tables -> (P1 uint16 [353], COST int32 [353, 2]) (host call)"""
    n = int(lib().pcgc_occ_tables(None, None))
    p1, cost = np.empty(n, np.uint16), np.empty((n, 2), np.int32)
    lib().pcgc_occ_tables(p1.ctypes.data, cost.ctypes.data)
    return p1, cost


# ------------------------------------------------------------------------------------------------ lossless mode, device coder (csrc/occupancy_rans.hip)
RANS_LANES = 64
RANS_MAX_STEPS = 1 << 24


def occ_rans_chunks(n, steps):
    """chunks of 64 x steps rows that n rows make"""
    return -(-int(n) // (RANS_LANES * int(steps)))


# What the two device coders share on this side (csrc/rans_core.h).  kind: 'occ' (units are rows; a frame without rows still
# has its 8-byte head) or 'attr' (units are tokens; a frame without tokens has the empty payload).
_RANS_UNITS = {'occ': 'rows', 'attr': 'tokens'}


def _rans_ws(kind, n, steps, dev):
    nbytes = int(getattr(lib(), f'pcgc_{kind}_rans_workspace_bytes')(n, steps))
    return torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev), nbytes


def _rans_batch_ws(kind, n, chunks, dev):
    nbytes = int(getattr(lib(), f'pcgc_{kind}_rans_batch_workspace_bytes')(n, chunks))
    return torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev), nbytes


def _rans_layout(kind, payload, n):
    """the host's checks of one frame's version-2 payload against its n units and its own size -> (S, K)"""
    who, units, n = f'{kind}_rans', _RANS_UNITS[kind], int(n)
    if n == 0 and kind == 'attr':
        if len(payload):
            raise PcgcError(f'{who}: a payload of {len(payload)} bytes without {units}')
        return 0, 0
    if len(payload) < 8:
        raise PcgcError(f'{who}: {len(payload)} bytes, shorter than the head')
    steps, chunks = (int(v) for v in np.frombuffer(payload, '<u4', 2))
    if not 1 <= steps <= RANS_MAX_STEPS:
        raise PcgcError(f'{who}: {steps} steps per chunk (1 .. 2^24)')
    if chunks != occ_rans_chunks(n, steps):
        raise PcgcError(f'{who}: {chunks} chunks declared; {n} {units} in chunks of 64 x {steps} make {occ_rans_chunks(n, steps)}')
    if len(payload) < 8 + 516 * chunks:
        raise PcgcError(f'{who}: {len(payload)} bytes, cut inside the tables of {chunks} chunks')
    words = int(np.frombuffer(payload, '<u4', chunks, 8 + 512 * chunks).astype(np.int64).sum())
    if 8 + 516 * chunks + 4 * words != len(payload):
        raise PcgcError(f'{who}: {len(payload)} bytes, but the chunks declare {words} words in all')
    return steps, chunks


def _rans_batch_layout(kind, counts, want):
    """counts, want [B] int64 as their caller has checked them: units and steps per chunk asked for per frame (0: the frame is one chunk)
    -> the dictionary of occ_rans_batch_layout / attr_rans_batch_layout; the frames' first units under 'row' or 'tok'"""
    some = (counts > 0) | (kind == 'occ')                                          # the frame has a payload at all
    steps = np.where(some, np.where(want > 0, want, np.maximum(1, -(-counts // RANS_LANES))), 0)
    chunks = -(-counts // (RANS_LANES * np.maximum(steps, 1)))
    room = np.where(some, 8 + 516 * chunks + 4 * counts, 0)
    edge = lambda v: np.concatenate([[0], np.cumsum(v)]).astype(np.int64)
    return {'steps': steps.astype(np.int32), 'chunks': chunks, 'first_chunk': edge(chunks), 'row' if kind == 'occ' else 'tok': edge(counts),
            'room': room, 'pay': edge((room + 7) // 8 * 8)}


def _rans_decode_blob(kind, payloads, counts, names):
    """payloads: per frame bytes, or None for a frame that is not decoded here; every one is checked against its frame's units (a PcgcError
    names the frame) -> (steps int32 [B], chunks, pay, size int64 [B], blob: the payloads one behind the other, each padded to 8 bytes)"""
    B = len(payloads)
    steps, chunks, pay, size, blob = np.zeros(B, np.int32), np.zeros(B, np.int64), np.zeros(B, np.int64), np.zeros(B, np.int64), bytearray()
    for f, payload in enumerate(payloads):
        if payload is None:
            continue
        try:
            steps[f], chunks[f] = _rans_layout(kind, payload, int(counts[f]))
        except PcgcError as e:
            raise PcgcError(f'{names[f]}: {e}') from None
        pay[f], size[f] = len(blob), len(payload)
        blob += bytes(payload) + bytes(-len(payload) % 8)
    return steps, chunks, pay, size, blob


def _rans_unsound(who, bad, of=''):
    return PcgcError(f'{who}: unsound payload ({bad}{of} chunks fail their check: states in [2^31, 2^63), exactly W_k words consumed, '
                     'every lane back at 2^31)')


def occ_rans_encode(packed, steps, sums=None):
    """packed int16 [n] as occ_symbols returns it -> the level's payload of `_O.bin` version 2 (include/pcgc_hip.h) as bytes, coded on the
    device in chunks of 64 x steps rows.  One small synchronising copy (the length) and one copy of the finished payload.  With sums
    (occ_symbols' second result) the small copy brings them along: -> (bytes, occupied rows, ideal code length in 2^-16 bit)."""
    n, dev, steps = _dev(packed, torch.int16, 'packed').shape[0], packed.device, int(steps)
    if packed.dim() != 1 or not 1 <= steps <= RANS_MAX_STEPS:
        raise PcgcError(f'occ_rans_encode: packed {tuple(packed.shape)}, {steps} steps per chunk (1 .. 2^24)')
    if sums is not None and (_dev(sums, torch.int64, 'sums').numel() != 2):
        raise PcgcError('occ_rans_encode: sums is occ_symbols\' int64 [2]')
    cap = 8 + 516 * occ_rans_chunks(n, steps) + 4 * n
    out = torch.empty((cap + 7) // 8, dtype=torch.int64, device=dev)
    ws, ws_bytes = _rans_ws('occ', n, steps, dev)
    host = np.zeros(3, dtype=np.int64)
    check(lib().pcgc_occ_rans_encode(_p(packed), n, steps, _p(sums), _p(out), cap, host.ctypes.data, _p(ws), ws_bytes, _stream(packed)), 'occ_rans_encode')
    payload = out.view(torch.uint8)[:int(host[0])].cpu().numpy().tobytes()
    return payload if sums is None else (payload, int(host[1]), int(host[2]))


def occ_rans_layout(payload, n):
    """the host's checks of one level's payload of `_O.bin` version 2 against its n rows and its own size -> (S, K).  PcgcError when S is
    outside 1 .. 2^24, K is not ceil(n / (64 S)), the tables do not fit or the word counts do not add up to the byte length."""
    return _rans_layout('occ', payload, n)


def occ_rans_decode(packed, payload, n):
    """packed int16 [n]: the contexts (occ_symbols without truth); payload: bytes of one level of `_O.bin` version 2 -> (uint8 mask [n] on
    the device, occupied rows).  The payload goes up in one copy, the two numbers come back in one.  PcgcError on a payload whose S, K or
    lengths disagree with n and its own size (checked here, before any launch) and on an unsound chunk (the kernel's verdict)."""
    n, dev = int(n), packed.device
    if _dev(packed, torch.int16, 'packed').dim() != 1 or packed.shape[0] != n:
        raise PcgcError(f'occ_rans_decode: packed {tuple(packed.shape)} for {n} rows')
    payload = bytes(payload)
    steps, chunks = occ_rans_layout(payload, n)
    up = torch.frombuffer(bytearray(payload) + bytes(-len(payload) % 8), dtype=torch.int64).to(dev)        # (8-byte aligned on the device)
    mask = torch.empty(n, dtype=torch.uint8, device=dev)
    ws, ws_bytes = _rans_batch_ws('occ', 0, chunks, dev)                           # (the slot + K offsets; no scratch on this side)
    host = np.zeros(2, dtype=np.int64)
    check(lib().pcgc_occ_rans_decode(_p(packed), n, _p(up), len(payload), steps, _p(mask), host.ctypes.data, _p(ws), ws_bytes, _stream(packed)),
          'occ_rans_decode')
    if host[1]:
        raise _rans_unsound('occ_rans_decode', int(host[1]), f' of {chunks}')
    return mask, int(host[0])


def occ_rans_batch_layout(rows_per_frame, chunk_steps):
    """How a batch's frames are cut into chunks and where their payloads stand in one device buffer (pure host).  rows_per_frame: 1 to 16 row
    counts; chunk_steps: steps per chunk for every frame (0: each frame is one chunk with its own S_f = max(1, ceil(rows_f / 64))), or one
    value per frame -> {steps [B] int32, chunks [B], first_chunk [B + 1], row [B + 1], room [B] (8 + 516 K_f + 4 rows_f: a frame without rows
    has its 8-byte head), pay [B + 1] (byte offsets, multiples of 8)}, int64 but for steps.  Chunks never straddle frames.  ValueError on
    0 or more than 16 frames, a negative row count or steps outside 0 .. 2^24."""
    rows = _frame_rows(rows_per_frame, 'occ_rans_batch_layout')
    want = np.asarray(chunk_steps, dtype=np.int64)
    if want.ndim > 1 or (want.ndim == 1 and want.size != rows.size) or (want < 0).any() or (want > RANS_MAX_STEPS).any():
        raise ValueError(f'occ_rans_batch_layout: steps per chunk {want.tolist()} for {rows.size} frames (one value or one per frame, 0 .. 2^24)')
    lay = _rans_batch_layout('occ', rows, np.broadcast_to(want, rows.shape))
    if (lay['steps'] > RANS_MAX_STEPS).any():
        raise ValueError(f'occ_rans_batch_layout: one chunk per frame needs {int(lay["steps"].max())} steps (at most 2^24)')
    return lay


def occ_rans_payloads(pending):
    """pending: what occ_rans_encode_batch(.., fetch=False) returned, of one or several calls -> per call the list of its frames' payloads
    (bytes), all brought down in ONE copy."""
    return _rans_fetch(pending)


def _rans_fetch(pending):
    """pending: per call (the payload buffer as uint8 on the device, the frames' byte offsets, their lengths) -> per call its frames' bytes"""
    parts =[raw[int(pay[f]):int(pay[f]) + int(size[f])] for raw, pay, size in pending for f in range(len(size))]
    down = torch.cat(parts).cpu().numpy().tobytes()
    out, at = [], 0
    for _, _, size in pending:
        out.append([])
        for f in range(len(size)):
            out[-1].append(down[at:at + int(size[f])])
            at += int(size[f])
    return out


def occ_rans_encode_batch(packed, rows_per_frame, chunk_steps, sums=None, fetch=True):
    """packed int16 [n] as occ_symbols_segments returns it, frame f the next rows_per_frame[f] rows -> B payloads (bytes), every one what
    occ_rans_encode gives for that frame alone at its own steps per chunk (occ_rans_batch_layout).  ONE launch sequence and one small
    synchronising copy for the batch; fetch=False leaves the finished payloads on the device and returns (buffer, offsets, lengths) for
    occ_rans_payloads to bring down later.  With sums (occ_symbols_segments' int64 [B, 2]) the small copy brings them along:
    -> (payloads, occupied rows per frame, ideal code length per frame in 2^-16 bit)."""
    lay = occ_rans_batch_layout(rows_per_frame, chunk_steps)
    B, n, dev = lay['steps'].size, int(lay['row'][-1]), packed.device
    if _dev(packed, torch.int16, 'occ_rans_encode_batch: packed').dim() != 1 or packed.shape[0] != n:
        raise PcgcError(f'occ_rans_encode_batch: packed {tuple(packed.shape)} for {B} frames of {n} rows in all')
    if sums is not None and tuple(_dev(sums, torch.int64, 'occ_rans_encode_batch: sums').shape) != (B, 2):
        raise PcgcError(f'occ_rans_encode_batch: sums is occ_symbols_segments\' int64 [{B}, 2]')
    pay = lay['pay']
    out = torch.empty(int(pay[-1]) // 8, dtype=torch.int64, device=dev)
    ws, ws_bytes = _rans_batch_ws('occ', n, int(lay['first_chunk'][-1]), dev)
    host = np.zeros(3 * B, dtype=np.int64)
    check(lib().pcgc_occ_rans_encode_batch(_p(packed), B, lay['row'].ctypes.data, lay['steps'].ctypes.data, _p(sums), _p(out), pay.ctypes.data,
                                           host.ctypes.data, _p(ws), ws_bytes, _stream(packed)), 'occ_rans_encode_batch')
    pending = (out.view(torch.uint8), pay, host[:B].copy())
    payloads = occ_rans_payloads([pending])[0] if fetch else pending
    return payloads if sums is None else (payloads, host[B:2 * B].copy(), host[2 * B:].copy())


def occ_rans_decode_batch(packed, rows_per_frame, payloads, mask=None, names=None):
    """packed int16 [n]: the contexts of a batch's level (occ_symbols_segments without truth), frame f the next rows_per_frame[f] rows;
    payloads: per frame the bytes of a version-2 payload, or None for a frame that is not decoded here (its slice of the mask keeps what it
    holds) -> (uint8 mask [n] on the device, occupied rows per frame).  Every payload's S, K and lengths are checked through occ_rans_layout
    before any launch; one upload, ONE launch sequence and one small copy for the batch.  mask: the uint8 [n] device tensor to write into.
    PcgcError naming the frame (names[f], else 'frame f') of a bad head or an unsound chunk."""
    rows = _frame_rows(rows_per_frame, 'occ_rans_decode_batch')
    B, n, dev = rows.size, int(rows.sum()), packed.device
    if len(payloads) != B:
        raise ValueError(f'occ_rans_decode_batch: {len(payloads)} payloads for {B} frames')
    if _dev(packed, torch.int16, 'occ_rans_decode_batch: packed').dim() != 1 or packed.shape[0] != n:
        raise PcgcError(f'occ_rans_decode_batch: packed {tuple(packed.shape)} for {B} frames of {n} rows in all')
    names = [f'frame {f}' for f in range(B)] if names is None else list(names)
    steps, chunks, pay, size, blob = _rans_decode_blob('occ', payloads, rows, names)
    if mask is None:
        mask = torch.empty(n, dtype=torch.uint8, device=dev)
    elif tuple(_dev(mask, torch.uint8, 'occ_rans_decode_batch: mask').shape) != (n,):
        raise PcgcError(f'occ_rans_decode_batch: a mask of {tuple(mask.shape)} for {n} rows')
    occupied = np.zeros(B, np.int64)
    if not steps.any():
        return mask, occupied
    up = torch.frombuffer(blob, dtype=torch.int64).to(dev)                         # (8-byte aligned on the device)
    ws, ws_bytes = _rans_batch_ws('occ', 0, int(chunks.sum()), dev)                # (the slot + K offsets; no scratch on this side)
    row = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    host = np.zeros(2 * B, dtype=np.int64)
    check(lib().pcgc_occ_rans_decode_batch(_p(packed), B, row.ctypes.data, steps.ctypes.data, _p(up), pay.ctypes.data, size.ctypes.data, _p(mask),
                                           host.ctypes.data, _p(ws), ws_bytes, _stream(packed)), 'occ_rans_decode_batch')
    for f in range(B):
        if host[B + f]:
            raise _rans_unsound(f'{names[f]}: occ_rans_decode_batch', int(host[B + f]), f' of {int(chunks[f])}')
    return mask, host[:B].copy()


# ------------------------------------------------------------------------------------------------ backward pass (csrc/grad.hip)
def conv_wgrad_rows_per_group(K, n_rows, Cin, Cout):
    """consecutive rows one workgroup of conv_wgrad reduces (a function of the shapes alone)"""
    return int(lib().pcgc_conv_wgrad_rows_per_group(int(K), int(n_rows), int(Cin), int(Cout)))


def _wgrad_ws(K, n_rows, Cin, Cout, device):
    nbytes = int(lib().pcgc_conv_wgrad_workspace_bytes(K, n_rows, Cin, Cout))
    return torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=device), nbytes


def conv_wgrad(nbr, x, gy, want_bias=True):
    """Weight (and bias) gradient of a gather convolution through its forward map nbr [K, n_out] (None: identity, k1):
    gW [K, Cin, Cout] = sum over present pairs of x[nbr[k][o]]^T gy[o]; gb [1, Cout] = column sums of gy (None unless want_bias).
    x / gy: fp32 2-D views (column slices allowed)."""
    _f32(x, 'x'); _f32(gy, 'gy')
    Cin, Cout = x.shape[1], gy.shape[1]
    if nbr is None:
        K, n_out = 1, gy.shape[0]
        if x.shape[0] != n_out:
            raise PcgcError('conv_wgrad: identity map with different row counts')
    else:
        K, n_out = nbr.shape
        _i32(nbr, 'nbr')
        if gy.shape[0] != n_out:
            raise PcgcError(f'conv_wgrad: gy has {gy.shape[0]} rows, the map {n_out}')
    gW = torch.empty((K, Cin, Cout), dtype=torch.float32, device=x.device)
    gb = torch.empty((1, Cout), dtype=torch.float32, device=x.device) if want_bias else None
    ws, ws_bytes = _wgrad_ws(K, n_out, Cin, Cout, x.device)
    check(lib().pcgc_conv_wgrad(_p(nbr), K, n_out, _p(x), x.shape[0], Cin, _ld(x), _p(gy), Cout, _ld(gy), _p(gW), _p(gb), _p(ws), ws_bytes,
                                _stream(x)), 'conv_wgrad')
    return gW, gb


def conv_up2_wgrad(x, gy, rows=None, want_bias=True):
    """Weight (and bias) gradient of the generative transpose k2 s2: gW [8, Cin, Cout] = sum_p x[p]^T gy[8 p + j]; rows: as in conv_up2."""
    _f32(x, 'x'); _f32(gy, 'gy')
    Cin, Cout = x.shape[1], gy.shape[1]
    n_in = x.shape[0] if rows is None else rows.shape[0]
    if gy.shape[0] != 8 * n_in:
        raise PcgcError(f'conv_up2_wgrad: gy has {gy.shape[0]} rows for {n_in} input rows')
    gW = torch.empty((8, Cin, Cout), dtype=torch.float32, device=x.device)
    gb = torch.empty((1, Cout), dtype=torch.float32, device=x.device) if want_bias else None
    ws, ws_bytes = _wgrad_ws(8, n_in, Cin, Cout, x.device)
    check(lib().pcgc_conv_up2_wgrad(n_in, _p(x), x.shape[0], Cin, _ld(x), _p(None if rows is None else _i32(rows, 'rows')), _p(gy), Cout,
                                    _ld(gy), _p(gW), _p(gb), _p(ws), ws_bytes, _stream(x)), 'conv_up2_wgrad')
    return gW, gb


def kmap_invert(nbr, n_in):
    """inv [K, n_in] with inv[k][nbr[k][o]] = o for the present pairs of nbr [K, n_out], -1 elsewhere"""
    K, n_out = nbr.shape
    inv = torch.empty((K, int(n_in)), dtype=torch.int32, device=nbr.device)
    check(lib().pcgc_kmap_invert(_p(_i32(nbr, 'nbr')), K, n_out, int(n_in), _p(inv), _stream(nbr)), 'kmap_invert')
    return inv


def kmap_up_inverse(n_in, device):
    """the transposed map of a generative transpose on an unpruned children level: inv[j][p] = 8 p + j (no lookup)"""
    return (8 * torch.arange(n_in, dtype=torch.int32, device=device)[None] + torch.arange(8, dtype=torch.int32, device=device)[:, None]).contiguous()


def relu_bwd(g, y, out=None):
    """g where y > 0, else 0 (2-D fp32 views; out may be a column slice)"""
    _f32(g, 'g'); _f32(y, 'y')
    if g.shape != y.shape:
        raise PcgcError(f'relu_bwd: shapes {tuple(g.shape)} and {tuple(y.shape)} differ')
    n, C = g.shape
    if out is None:
        out = torch.empty((n, C), dtype=torch.float32, device=g.device)
    check(lib().pcgc_relu_bwd(_p(g), _ld(g), _p(y), _ld(y), n, C, _p(out), _ld(out), _stream(g)), 'relu_bwd')
    return out


def scatter_rows(gy, orig, n_out):
    """adjoint of gather_rows / compact_feats: zeros [n_out, C] with row orig[r] = gy[r]"""
    _f32(gy, 'gy')
    C = gy.shape[1]
    gx = torch.empty((int(n_out), C), dtype=torch.float32, device=gy.device)
    check(lib().pcgc_scatter_rows(_p(gy), C, _ld(gy), _p(_i32(orig, 'orig')), orig.shape[0], _p(gx), int(n_out), C, _stream(gy)), 'scatter_rows')
    return gx


def bce_logits_bwd(logits, truth, scale=1.0):
    """d(bce_logits' bce) / d logits times scale -> fp32 [n, 1]"""
    _f32(logits, 'logits'); _dev(truth, torch.uint8, 'truth')
    n = truth.shape[0]
    if logits.shape[0] != n or logits.dim() > 2 or (logits.dim() == 2 and logits.shape[1] != 1):
        raise PcgcError(f'bce_logits_bwd: logits {tuple(logits.shape)} against a mask of {n} rows')
    g = torch.empty((n, 1), dtype=torch.float32, device=logits.device)
    check(lib().pcgc_bce_logits_bwd(_p(logits), max(int(logits.stride(0)), 1), n, _p(truth), float(scale), _p(g), _stream(logits)), 'bce_logits_bwd')
    return g


def eb_likelihood_bwd(feats, params, bound=1e-9, scale=1.0):
    """gradient of eb_likelihood's bits times scale -> (d / d feats fp32 [n, C], d / d params fp32 [44 C], the packing of `params`)"""
    _f32(feats, 'feats')
    n, C, ld = feats.shape[0], feats.shape[1], _ld(feats)
    gy = torch.empty((n, C), dtype=torch.float32, device=feats.device)
    gp = torch.empty(44 * C, dtype=torch.float32, device=feats.device)
    nbytes = int(lib().pcgc_eb_bwd_workspace_bytes(n, C))
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=feats.device)
    check(lib().pcgc_eb_likelihood_bwd(_p(feats), ld, n, C, _p(_f32(params, 'params')), float(bound), float(scale), _p(gy), _p(gp), _p(ws), nbytes,
                                       _stream(feats)), 'eb_likelihood_bwd')
    return gy, gp


# ------------------------------------------------------------------------------------------------ D1 metric
_D1_OFFSETS = {}


def _d1_offsets(device, radius=12):
    """(dx,dy,dz,d2) for every lattice offset with max|d| <= radius, sorted by d2 (ties in a fixed order)."""
    key = (str(device), radius)
    if key not in _D1_OFFSETS:
        r = np.arange(-radius, radius + 1)
        g = np.stack(np.meshgrid(r, r, r, indexing='ij'), -1).reshape(-1, 3)
        d2 = (g * g).sum(1)
        order = np.lexsort((g[:, 0], g[:, 1], g[:, 2], d2))
        tab = np.concatenate([g[order], d2[order, None]], 1).astype(np.int32)
        # an offset at Chebyshev distance > radius could be closer than the corner offsets: keep only d2 <= radius^2
        tab = tab[tab[:, 3] <= radius * radius]
        _D1_OFFSETS[key] = torch.from_numpy(np.ascontiguousarray(tab)).to(device)
    return _D1_OFFSETS[key]


_D1_CELL_OFFSETS = {}


def _d1_cell_offsets(device, reach_cells=4):
    """(ox, oy, oz, lower bound of the squared distance) for every CELL offset with max|o| <= reach_cells, ascending in the bound: a voxel of the
    query's own cell and a voxel of the cell at offset o are at least max(0, 4 |o| - 3) apart per axis."""
    key = (str(device), reach_cells)
    if key not in _D1_CELL_OFFSETS:
        r = np.arange(-reach_cells, reach_cells + 1)
        g = np.stack(np.meshgrid(r, r, r, indexing='ij'), -1).reshape(-1, 3)
        gap = np.maximum(0, 4 * np.abs(g) - 3)
        lb = (gap * gap).sum(1)
        order = np.lexsort((g[:, 0], g[:, 1], g[:, 2], lb))
        tab = np.concatenate([g[order], lb[order, None]], 1).astype(np.int32)
        _D1_CELL_OFFSETS[key] = torch.from_numpy(np.ascontiguousarray(tab)).to(device)
    return _D1_CELL_OFFSETS[key]


def d1_nn(a, b, radius=12):
    """a, b: int32 [N,4] device coordinate tensors (stride 1).  -> (sum of squared NN distances a->b, max, unresolved count)."""
    s = torch.empty(1, dtype=torch.float64, device=a.device)
    m = torch.empty(1, dtype=torch.int64, device=a.device)
    u = torch.empty(1, dtype=torch.int32, device=a.device)
    if PATH.D1_CELLS and b.shape[0] > 0:
        # cloud B as stride-4 cells: hash of the cells + a 64-bit occupancy mask per cell; reach: cells up to 4 away, i.e. every voxel nearer
        # than 4 * 5 - 3 = 17 has been seen when the search ends
        reach_cells = max(1, (int(radius) + 3) // 4 + 1)
        # (the hash of the quantised rows maps a cell to the FIRST row that lies in it: that row's slot of `masks` is the cell's mask)
        table = HashTable(coords_quantize(_i32(b), 4), 4)
        masks = torch.empty(b.shape[0], dtype=torch.int64, device=b.device)
        check(lib().pcgc_d1_cell_masks(_p(b), b.shape[0], _p(table.keys), _p(table.vals), table.cap, _p(masks), b.shape[0], _stream(b)),
              'd1_cell_masks')
        off = _d1_cell_offsets(a.device, reach_cells)
        reach = 4 * (reach_cells + 1) - 3
        check(lib().pcgc_d1_nn_cells(_p(_i32(a)), a.shape[0], _p(table.keys), _p(table.vals), table.cap, _p(masks), _p(off), off.shape[0],
                                     reach * reach, _p(s), _p(m), _p(u), _stream(a)), 'd1_nn_cells')
        return s, m, u
    table = HashTable(_i32(b), 1)
    off = _d1_offsets(a.device, radius)
    check(lib().pcgc_d1_nn(_p(_i32(a)), a.shape[0], _p(table.keys), _p(table.vals), table.cap, _p(off), off.shape[0], _p(s), _p(m),
                           _p(u), _stream(a)), 'd1_nn')
    return s, m, u


# ------------------------------------------------------------------------------------------------ D2 metric (csrc/metric.hip)
D2_TIES = 30                       # tie sets hold at most this many rows: the lowest original rows (mpeg-pcc-dmetric's k = 30 search)
D2_REACH_CELLS = (4, 16)           # cell tables searched in turn (reach 17 and 65 voxels); what neither settles is searched exhaustively


class D2Index:
    """A cloud as the D2 search reads it: rows sorted by (batch, z, y, x) (stable: the duplicates of a voxel are one run in ascending
    original row), run lengths, the voxel hash of the sorted rows and their stride-4 cells with occupancy masks."""

    def __init__(self, q):
        q = _i32(q)
        n = q.shape[0]
        self.coords, self.n = q, n
        self.perm = sort_zyx(q, batch_major=True)
        self.qs = torch.empty_like(q)
        check(lib().pcgc_gather_rows_i32x4(_p(q), _p(self.perm), n, _p(self.qs), _stream(q)), 'gather_rows_i32x4')
        self.runlen = torch.empty(n, dtype=torch.int32, device=q.device)
        check(lib().pcgc_d2_runs(_p(self.qs), n, _p(self.runlen), _stream(q)), 'd2_runs')
        self.voxels = HashTable(self.qs, 1)                 # voxel -> first sorted row of its run
        self.cells = HashTable(coords_quantize(self.qs, 4), 4)
        self.masks = torch.empty(n, dtype=torch.int64, device=q.device)
        check(lib().pcgc_d1_cell_masks(_p(self.qs), n, _p(self.cells.keys), _p(self.cells.vals), self.cells.cap, _p(self.masks), n, _stream(q)),
              'd1_cell_masks')

    def tables(self):
        return (_p(self.cells.keys), _p(self.cells.vals), self.cells.cap, _p(self.masks), _p(self.voxels.keys), _p(self.voxels.vals),
                self.voxels.cap, _p(self.runlen))


def _d2_scan(cnt):
    n = cnt.shape[0]
    seg = torch.empty(n + 1, dtype=torch.int64, device=cnt.device)
    ws_bytes = int(lib().pcgc_d2_scan_workspace_bytes(n))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=cnt.device)
    check(lib().pcgc_d2_scan(_p(cnt), n, _p(seg), _p(ws), ws_bytes, _stream(cnt)), 'd2_scan')
    return seg


def d2_nn(p, q):
    """Nearest-distance tie sets of every point of p in q (q: a D2Index or an int32 [N,4] device tensor), exact at any distance.
    -> (c2c int64 [Np] = nearest squared distance, seg int64 [Np+1], kept int32 [Np], rows int32): the tie set of point i is
    rows[seg[i] : seg[i] + kept[i]], ascending ORIGINAL rows of q, at most D2_TIES of them (the lowest rows when more tie)."""
    p = _i32(p, 'p')
    q = q if isinstance(q, D2Index) else D2Index(q)
    n, dev, st = p.shape[0], p.device, _stream(p)
    best = torch.empty(n, dtype=torch.int64, device=dev)
    cnt = torch.empty(n, dtype=torch.int32, device=dev)
    n_out = torch.empty(1, dtype=torch.int32, device=dev)
    stages = []                                             # (offset table, reach2, selection list or None, its length)
    sel, n_sel = None, n
    for reach_cells in D2_REACH_CELLS:
        off = _d1_cell_offsets(dev, reach_cells)
        reach = 4 * (reach_cells + 1) - 3
        out = torch.empty(max(n_sel, 1), dtype=torch.int32, device=dev)
        check(lib().pcgc_d2_count(_p(p), n_sel, _p(sel), *q.tables(), _p(off), off.shape[0], reach * reach, _p(best), _p(cnt), _p(out),
                                  _p(n_out), st), 'd2_count')
        stages.append((off, reach * reach, sel, n_sel))
        sel, n_sel = out, int(n_out.item())
        if n_sel == 0:
            break
    if n_sel:                                               # farther than every table reaches: every row of q with the point's batch
        check(lib().pcgc_d2_exhaustive(_p(p), n_sel, _p(sel), _p(q.qs), q.n, _p(q.perm), 0, _p(best), _p(cnt), None, None, _p(n_out), st),
              'd2_exhaustive')
        if int(n_out.item()):
            raise PcgcError(f'd2_nn: {int(n_out.item())} points have a batch index with no point in the other cloud')
    seg = _d2_scan(cnt)
    rows = torch.empty(max(int(seg[-1].item()), 1), dtype=torch.int32, device=dev)
    for off, reach2, s, ns in stages:
        check(lib().pcgc_d2_fill(_p(p), ns, _p(s), *q.tables(), _p(q.perm), _p(off), off.shape[0], reach2, _p(best), _p(seg),
                                 _p(rows), st), 'd2_fill')
    if n_sel:
        check(lib().pcgc_d2_exhaustive(_p(p), n_sel, _p(sel), _p(q.qs), q.n, _p(q.perm), 1, _p(best), None, _p(seg), _p(rows), None, st),
              'd2_exhaustive')
    kept = torch.empty(n, dtype=torch.int32, device=dev)
    check(lib().pcgc_d2_segment_lowest(_p(seg), n, _p(rows), D2_TIES, _p(kept), st), 'd2_segment_lowest')
    return best, seg, kept, rows


def d2_normals(nb, ab, na, ba):
    """Normals of cloud B (nb rows) from those of A (na: float64 [Na,3] device): ab = d2_nn(A, B), ba = d2_nn(B, A).  -> float64 [nb,3]"""
    _, seg, kept, rows = ab
    _, seg_ba, kept_ba, rows_ba = ba
    na = _dev(na, torch.float64, 'normals')
    dev, st = na.device, _stream(na)
    rcnt = torch.empty(max(nb, 1), dtype=torch.int32, device=dev)
    check(lib().pcgc_d2_recv_count(_p(seg), _p(kept), kept.shape[0], _p(rows), nb, _p(rcnt), st), 'd2_recv_count')
    rseg = _d2_scan(rcnt[:nb])
    recv = torch.empty(max(int(rseg[-1].item()), 1), dtype=torch.int32, device=dev)
    cursor = torch.empty(max(nb, 1), dtype=torch.int32, device=dev)
    check(lib().pcgc_d2_recv_fill(_p(seg), _p(kept), kept.shape[0], _p(rows), nb, _p(rseg), _p(cursor), _p(recv), st), 'd2_recv_fill')
    check(lib().pcgc_d2_segment_lowest(_p(rseg), nb, _p(recv), 0x7FFFFFFF, None, st), 'd2_segment_lowest')     # ascending A row
    out = torch.empty((nb, 3), dtype=torch.float64, device=dev)
    check(lib().pcgc_d2_normals(_p(rseg), _p(recv), nb, _p(na), _p(seg_ba), _p(kept_ba), _p(rows_ba), _p(out), st), 'd2_normals')
    return out


def d2_c2p(p, q, nq, nn):
    """c2p float64 [Np] of p against q (int32 [Nq,4]) with q's normals nq (float64 [Nq,3]) over the tie sets nn = d2_nn(p, q)"""
    _, seg, kept, rows = nn
    out = torch.empty(p.shape[0], dtype=torch.float64, device=p.device)
    check(lib().pcgc_d2_c2p(_p(_i32(p, 'p')), p.shape[0], _p(_i32(q, 'q')), _p(_dev(nq, torch.float64, 'normals')), _p(seg), _p(kept), _p(rows),
                            _p(out), _stream(p)), 'd2_c2p')
    return out


def d2_reduce(c2c, c2p):
    """-> (int64 [2] = sum and max of c2c, float64 [1] = sum of c2p), in a fixed order"""
    n, dev = c2c.shape[0], c2c.device
    sm = torch.empty(2, dtype=torch.int64, device=dev)
    s = torch.empty(1, dtype=torch.float64, device=dev)
    ws_bytes = int(lib().pcgc_d2_reduce_workspace_bytes())
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    check(lib().pcgc_d2_reduce(_p(c2c), _p(c2p), n, _p(sm), _p(s), _p(ws), ws_bytes, _stream(c2c)), 'd2_reduce')
    return sm, s


# ------------------------------------------------------------------------------------------------ colours (csrc/colour.hip)
ATTR_MAX_CHANNELS = 4
ATTR_MAX_SOURCES = 0xFFFFFFFF // 255          # the accumulator fields are 32 bits wide: 255 * ns has to fit (pcgc_attr_transfer)


def _u8(t, what):
    if t.dtype != torch.uint8:
        raise ValueError(f'{what}: expected uint8, got {t.dtype}')
    if not t.is_cuda:
        raise PcgcError(f'{what}: expected a device tensor')
    return t.contiguous()


def attr_transfer(nt, st, attr_s, ts):
    """Attributes of cloud T (nt rows) from those of S (attr_s: uint8 [ns,C] device, C = 1 .. 4): st = d2_nn(S, T), ts = d2_nn(T, S).
    A target takes the mean, rounded half up, over the sources whose tie set holds it, or — none does — over its own tie set in S.
    Exact and bitwise reproducible (integer sums).  -> uint8 [nt,C]"""
    _, seg, kept, rows = st
    _, seg_ts, kept_ts, rows_ts = ts
    attr_s = _u8(attr_s, 'attr_transfer: attributes')
    if attr_s.dim() != 2 or not 1 <= attr_s.shape[1] <= ATTR_MAX_CHANNELS:
        raise ValueError(f'attr_transfer: attributes must be [ns,C] with C in 1 .. {ATTR_MAX_CHANNELS}, got {tuple(attr_s.shape)}')
    ns, C = attr_s.shape
    if kept.shape[0] != ns or kept_ts.shape[0] != nt:
        raise ValueError(f'attr_transfer: {ns} source rows and {nt} target rows, but the tie sets are of {kept.shape[0]} and {kept_ts.shape[0]}')
    if ns == 0 or nt == 0:
        raise ValueError('attr_transfer: empty point cloud')
    dev = attr_s.device
    out = torch.empty((nt, C), dtype=torch.uint8, device=dev)
    ws_bytes = int(lib().pcgc_attr_transfer_workspace_bytes(ns, nt, C))
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=dev)
    check(lib().pcgc_attr_transfer(_p(seg), _p(kept), _p(rows), ns, _p(seg_ts), _p(kept_ts), _p(rows_ts), nt, _p(attr_s), C, _p(out), _p(ws),
                                   ws_bytes, _stream(attr_s)), 'attr_transfer')
    return out


def colour_dist(cp, cq, nn):
    """Per point of P (cp: uint8 [np,3] device) against the rounded mean colour of its tie set nn = d2_nn(P, Q) in Q (cq: uint8 [nq,3]):
    -> (yuv2 int64 [np,3], rgb2 int32 [np,3]), the squared BT.709 differences times (255 * 10^4)^2 and the squared RGB differences."""
    _, seg, kept, rows = nn
    cp, cq = _u8(cp, 'colour_dist: colours'), _u8(cq, 'colour_dist: colours')
    for c in (cp, cq):
        if c.dim() != 2 or c.shape[1] != 3:
            raise ValueError(f'colour_dist: colours must be [n,3], got {tuple(c.shape)}')
    n = cp.shape[0]
    if kept.shape[0] != n:
        raise ValueError(f'colour_dist: {n} colours but tie sets of {kept.shape[0]} points')
    if n == 0 or cq.shape[0] == 0:
        raise ValueError('colour_dist: empty point cloud')
    yuv2 = torch.empty((n, 3), dtype=torch.int64, device=cp.device)
    rgb2 = torch.empty((n, 3), dtype=torch.int32, device=cp.device)
    check(lib().pcgc_colour_dist(_p(cp), n, _p(cq), cq.shape[0], _p(seg), _p(kept), _p(rows), _p(yuv2), _p(rgb2), _stream(cp)), 'colour_dist')
    return yuv2, rgb2


def colour_reduce(yuv2, rgb2):
    """-> int64 [9] device: low-word sums and high-word sums of yuv2's three columns (total_k = out[3+k] * 2**32 + out[k], exact), maxima of
    rgb2's three columns"""
    n, dev = yuv2.shape[0], yuv2.device
    out = torch.empty(9, dtype=torch.int64, device=dev)
    ws_bytes = int(lib().pcgc_colour_reduce_workspace_bytes())
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=dev)
    check(lib().pcgc_colour_reduce(_p(yuv2), _p(rgb2), n, _p(out), _p(ws), ws_bytes, _stream(yuv2)), 'colour_reduce')
    return out


# ------------------------------------------------------------------------------------------------ colour transform (csrc/raht.hip)
RAHT_MAX_POINTS = 1 << 24
RAHT_CONTEXTS = 48
RAHT_ESCAPE = 63
RAHT_FORMS = {'bits': 0, 'tiles': 1}          # one launch per populated split bit | tiles in LDS + the crossing gaps by one workgroup
RAHT_FORM = 'tiles'                           # the form raht_forward / raht_inverse take unless told otherwise


def raht_tile_leaves():
    return int(lib().pcgc_raht_tile_leaves())


class RahtTree:
    """The binary radix tree of a cloud's Morton keys (pcgc_raht_keys + pcgc_raht_tree): geometry only, shared by the three channels and by
    encoder and decoder.  Per gap i (between sorted leaves i and i + 1): d, lo, hi, left, right (a gap, or ~leaf); w1 = i - lo + 1,
    w2 = hi - i.  perm: sorted leaf i is row perm[i] of the caller.  order: the gaps in coding order; bucket: its 65 offsets on the host."""
    __slots__ = ('n', 'keys', 'perm', 'd', 'lo', 'hi', 'left', 'right', 'order', 'cross_order', 'offsets', 'bucket', 'cross', 'device')

    @property
    def w1(self):
        return torch.arange(self.n - 1, dtype=torch.int32, device=self.device) - self.lo + 1

    @property
    def w2(self):
        return self.hi - torch.arange(self.n - 1, dtype=torch.int32, device=self.device)


def tick_phase(times, phase, t0, dev=None):
    """The measurement hook of the colour codec (raht_tree, raht_tree_batch, attributes.AttributeCoder).  times None: nothing happens.
    Else: dev is synchronised (when given) and the seconds since t0 are added to times[phase] (when phase is given) -> now"""
    import time
    if times is None:
        return 0.0
    if dev is not None:
        torch.cuda.synchronize(dev)
    now = time.perf_counter()
    if phase is not None:
        times[phase] = times.get(phase, 0.0) + now - t0
    return now


def _raht_gap_arrays(t, n, dev):
    """the seven per-gap arrays of a tree of n leaves: d uint8 and lo, hi, left, right, order, cross_order int32, each [n - 1]"""
    g = max(n - 1, 1)
    t.d = torch.empty(g, dtype=torch.uint8, device=dev)[:n - 1]
    t.lo, t.hi, t.left, t.right, t.order, t.cross_order = (torch.empty(g, dtype=torch.int32, device=dev)[:n - 1] for _ in range(6))


def raht_tree(coords, times=None):
    """coords int32 [n,4] (batch 0, x, y, z in [0, 2^20)) of ONE frame of distinct voxels -> RahtTree.  ValueError for a batch, coordinates
    out of range, duplicates, an empty cloud or more than 2^24 rows.  times (measurement hook): a dict -> seconds of 'keys + sort' and
    'tree' added to it, with a synchronisation after each."""
    coords = _i32(coords)
    if coords.dim() != 2 or coords.shape[1] != 4:
        raise ValueError(f'raht_tree: coordinates must be [n,4], got {tuple(coords.shape)}')
    n, dev = coords.shape[0], coords.device
    if not 1 <= n <= RAHT_MAX_POINTS:
        raise ValueError(f'raht_tree: {n} rows; the colour transform takes 1 .. 2^24')
    t = RahtTree()
    t.n, t.device = n, dev
    t.keys = torch.empty(n, dtype=torch.int64, device=dev)
    t.perm = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.empty(2, dtype=torch.int32, device=dev)
    ws_bytes = max(int(lib().pcgc_raht_keys_workspace_bytes(n)), int(lib().pcgc_raht_tree_workspace_bytes(n)))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    s = _stream(coords)
    t0 = tick_phase(times, None, 0.0, dev)
    check(lib().pcgc_raht_keys(_p(coords), n, _p(t.keys), _p(t.perm), _p(status), _p(ws), ws_bytes, s), 'raht_keys')
    t0 = tick_phase(times, 'keys + sort', t0, dev)
    _raht_gap_arrays(t, n, dev)
    t.offsets = torch.empty(130, dtype=torch.int32, device=dev)
    check(lib().pcgc_raht_tree(_p(t.keys), n, _p(t.d), _p(t.lo), _p(t.hi), _p(t.left), _p(t.right), _p(t.order), _p(t.cross_order),
                               _p(t.offsets), _p(ws), ws_bytes, s), 'raht_tree')
    dups, flags = status.cpu().tolist()
    if flags & 2:
        raise ValueError('raht_tree: the colour transform codes one frame at a time; got rows with a non-zero batch index')
    if flags & 1:
        raise ValueError('raht_tree: coordinates outside [0, 2^20)')
    if dups:
        raise ValueError(f'raht_tree: {dups} duplicate voxels; the colour transform needs distinct voxels')
    off = t.offsets.cpu().numpy()
    tick_phase(times, 'tree', t0, dev)
    t.bucket, t.cross = np.ascontiguousarray(off[:65]), np.ascontiguousarray(off[65:])
    return t


def _raht_form(form):
    form = RAHT_FORM if form is None else form
    if form not in RAHT_FORMS:
        raise ValueError(f'raht form {form!r}: one of {sorted(RAHT_FORMS)}')
    return RAHT_FORMS[form]


def raht_forward(tree, rgb, form=None):
    """rgb uint8 [n,3] in the row order of the tree's coordinates -> (H int32 [n-1,3] per gap, DC int32 [3]); form: RAHT_FORMS"""
    rgb = _u8(rgb, 'raht_forward: colours')
    if rgb.dim() != 2 or tuple(rgb.shape) != (tree.n, 3):
        raise ValueError(f'raht_forward: colours must be [{tree.n},3], got {tuple(rgb.shape)}')
    val = torch.empty((tree.n, 3), dtype=torch.int32, device=tree.device)
    H = torch.empty((max(tree.n - 1, 1), 3), dtype=torch.int32, device=tree.device)[:tree.n - 1]
    check(lib().pcgc_raht_forward(_p(rgb), _p(tree.perm), tree.n, _p(tree.d), _p(tree.lo), _p(tree.hi), _p(tree.order), tree.bucket.ctypes.data,
                                  _p(tree.cross_order), _p(tree.offsets) + 65 * 4, _raht_form(form), _p(val), _p(H), _stream(rgb)), 'raht_forward')
    return H, val[0].clone()


def raht_quantize(tree, H, q_luma, q_chroma):
    """-> (tokens int16 [3(n-1)], ctx uint16 as int16 storage [3(n-1)], escapes uint16-valued int16 [E], hist int32 [48,64]) on the device,
    in coding order"""
    n, dev = tree.n, tree.device
    t = max(3 * (n - 1), 1)
    tokens = torch.empty(t, dtype=torch.int16, device=dev)[:3 * (n - 1)]
    ctx = torch.empty(t, dtype=torch.int16, device=dev)[:3 * (n - 1)]
    esc = torch.empty(t, dtype=torch.int16, device=dev)
    n_esc = torch.empty(1, dtype=torch.int32, device=dev)
    hist = torch.empty((RAHT_CONTEXTS, 64), dtype=torch.int32, device=dev)
    ws_bytes = int(lib().pcgc_raht_quantize_workspace_bytes(n))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    check(lib().pcgc_raht_quantize(_p(_dev(H, torch.int32, 'raht_quantize: H')), n, _p(tree.d), _p(tree.lo), _p(tree.hi), _p(tree.order),
                                   int(q_luma), int(q_chroma), _p(tokens), _p(ctx), _p(esc), _p(n_esc), _p(hist), _p(ws), ws_bytes, _stream(H)),
          'raht_quantize')
    return tokens, ctx, esc[:int(n_esc.item())], hist


def raht_dequantize(tree, tokens, escapes, q_luma, q_chroma):
    """tokens int16 [3(n-1)] and escapes (int16 storage) on the device -> H^ int32 [n-1,3].  PcgcError when the number of escape tokens is
    not the length of the escape list."""
    n, dev = tree.n, tree.device
    if tokens.shape[0] != 3 * (n - 1):
        raise PcgcError(f'raht_dequantize: {tokens.shape[0]} tokens for {n} points')
    Hhat = torch.empty((max(n - 1, 1), 3), dtype=torch.int32, device=dev)[:n - 1]
    count = torch.empty(1, dtype=torch.int32, device=dev)
    ws_bytes = int(lib().pcgc_raht_dequantize_workspace_bytes(n))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    tokens, escapes = _dev(tokens, torch.int16, 'raht_dequantize: tokens'), _dev(escapes, torch.int16, 'raht_dequantize: escapes')
    check(lib().pcgc_raht_dequantize(_p(tokens), _p(escapes) if escapes.shape[0] else None, escapes.shape[0], n, _p(tree.lo), _p(tree.hi),
                                     _p(tree.order), int(q_luma), int(q_chroma), _p(Hhat), _p(count), _p(ws), ws_bytes, _stream(tokens)),
          'raht_dequantize')
    if int(count.item()) != escapes.shape[0]:
        raise PcgcError(f'raht_dequantize: {int(count.item())} escape tokens but {escapes.shape[0]} escapes')
    return Hhat


def raht_inverse(tree, Hhat, dc, form=None):
    """H^ int32 [n-1,3] and the DC (three ints) -> rgb uint8 [n,3] in the row order of the tree's coordinates"""
    val = torch.empty((tree.n, 3), dtype=torch.int32, device=tree.device)
    rgb = torch.empty((tree.n, 3), dtype=torch.uint8, device=tree.device)
    if tuple(Hhat.shape) != (tree.n - 1, 3):
        raise ValueError(f'raht_inverse: H^ must be [{tree.n - 1},3], got {tuple(Hhat.shape)}')
    dc = [int(v) for v in dc]
    check(lib().pcgc_raht_inverse(_p(_dev(Hhat, torch.int32, 'raht_inverse: H^')), dc[0], dc[1], dc[2], _p(tree.perm), tree.n, _p(tree.d),
                                  _p(tree.lo), _p(tree.hi), _p(tree.order), tree.bucket.ctypes.data, _p(tree.cross_order),
                                  _p(tree.offsets) + 65 * 4, _raht_form(form), _p(val), _p(rgb), _stream(Hhat)), 'raht_inverse')
    return rgb


# ------------------------------------------------------------------------------------------------ colour transform, a batch of frames
RAHT_MAX_FRAMES = 16


class RahtBatchTree(RahtTree):
    """The trees of B frames from one key build, one sort and one tree build (pcgc_raht_keys_batch + pcgc_raht_tree_batch).  Sorted leaves
    [starts[b], starts[b + 1]) are frame b; gap arrays are indexed by the batch's gaps, a frame boundary has lo = hi = -1.  order: the
    n - B merges in coding order, frame by frame (frame b's are positions [starts[b] - b, starts[b + 1] - b - 1)), then the boundaries.
    bucket: int32 [B,65] on the host, row b the offsets of frame b alone; offsets: [(B + 1) x 65] on the device, the last row = cross.
    bit_off: int32 [130] on the host, for the form that launches per split bit (include/pcgc_hip.h)."""
    __slots__ = ('frames', 'starts', 'starts_dev', 'bit_off')

    @property
    def tok(self):
        """int64 [B + 1]: frame b's tokens are [tok[b], tok[b + 1]) of the batch's coding order"""
        return 3 * (self.starts - np.arange(self.frames + 1))


def raht_tree_batch(coords, frames, times=None):
    """coords int32 [n,4] rows (b, x, y, z), b in 0 .. frames - 1 and x, y, z in [0, 2^20), in any order -> RahtBatchTree.  ValueError for
    frames outside 1 .. 16, a frame index outside 0 .. frames - 1 or without rows, coordinates out of range, duplicates within a frame (the
    frame is named), an empty batch or more than 2^24 rows."""
    coords = _i32(coords)
    if coords.dim() != 2 or coords.shape[1] != 4:
        raise ValueError(f'raht_tree_batch: coordinates must be [n,4], got {tuple(coords.shape)}')
    n, dev, B = coords.shape[0], coords.device, int(frames)
    if not 1 <= B <= RAHT_MAX_FRAMES:
        raise ValueError(f'raht_tree_batch: {B} frames; a batch holds 1 .. {RAHT_MAX_FRAMES}')
    if not 1 <= n <= RAHT_MAX_POINTS:
        raise ValueError(f'raht_tree_batch: {n} rows; the colour transform takes 1 .. 2^24 in a batch')
    t = RahtBatchTree()
    t.n, t.device, t.frames = n, dev, B
    t.keys = torch.empty(n, dtype=torch.int64, device=dev)
    t.perm = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.empty(34, dtype=torch.int32, device=dev)
    ws_bytes = max(int(lib().pcgc_raht_keys_batch_workspace_bytes(n)), int(lib().pcgc_raht_tree_batch_workspace_bytes(n)))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    s = _stream(coords)
    t0 = tick_phase(times, None, 0.0, dev)
    check(lib().pcgc_raht_keys_batch(_p(coords), n, B, _p(t.keys), _p(t.perm), _p(status), _p(ws), ws_bytes, s), 'raht_keys_batch')
    t0 = tick_phase(times, 'keys + sort', t0, dev)
    _raht_gap_arrays(t, n, dev)
    t.offsets = torch.empty((B + 1) * 65, dtype=torch.int32, device=dev)
    check(lib().pcgc_raht_tree_batch(_p(t.keys), n, B, _p(t.d), _p(t.lo), _p(t.hi), _p(t.left), _p(t.right), _p(t.order), _p(t.cross_order),
                                     _p(t.offsets), _p(ws), ws_bytes, s), 'raht_tree_batch')
    status = status.cpu().numpy()
    dups, rows, flags = status[:B], status[16:16 + B].astype(np.int64), int(status[32])
    if flags & 2:
        raise ValueError(f'raht_tree_batch: rows with a frame index outside 0 .. {B - 1}')
    if flags & 1:
        raise ValueError('raht_tree_batch: coordinates outside [0, 2^20)')
    if (rows == 0).any():
        raise ValueError(f'raht_tree_batch: frame {int(np.flatnonzero(rows == 0)[0])} has no rows; every frame of a batch needs at least one')
    if dups.any():
        b = int(np.flatnonzero(dups)[0])
        raise ValueError(f'raht_tree_batch: frame {b} has {int(dups[b])} duplicate voxels; the colour transform needs distinct voxels')
    off = t.offsets.cpu().numpy().reshape(B + 1, 65)
    tick_phase(times, 'tree', t0, dev)
    t.bucket, t.cross = np.ascontiguousarray(off[:B]), np.ascontiguousarray(off[B])
    t.starts = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    t.starts_dev = torch.from_numpy(t.starts[:B].astype(np.int32)).to(dev)
    rest = np.diff(t.bucket.astype(np.int64), axis=1).sum(0) - np.diff(t.cross.astype(np.int64))      # merges per bucket that cross no tile
    t.bit_off = np.ascontiguousarray(np.concatenate([t.cross, t.cross[64] + np.concatenate([[0], np.cumsum(rest)])]), dtype=np.int32)
    return t


def _frame_steps(tree, q_luma, q_chroma):
    ql, qc = np.ascontiguousarray(q_luma, dtype=np.int32), np.ascontiguousarray(q_chroma, dtype=np.int32)
    if ql.shape != (tree.frames,) or qc.shape != (tree.frames,):
        raise ValueError(f'quantiser steps per frame: two sequences of {tree.frames}, got {ql.shape} and {qc.shape}')
    return ql, qc


def raht_forward_batch(tree, rgb, form=None):
    """rgb uint8 [n,3] in the row order of the batch's coordinates -> (H int32 [n-1,3] per gap of the batch (a frame boundary's row is not
    written), DC int32 [B,3] on the device); one transform for all frames"""
    rgb = _u8(rgb, 'raht_forward_batch: colours')
    if rgb.dim() != 2 or tuple(rgb.shape) != (tree.n, 3):
        raise ValueError(f'raht_forward_batch: colours must be [{tree.n},3], got {tuple(rgb.shape)}')
    val = torch.empty((tree.n, 3), dtype=torch.int32, device=tree.device)
    H = torch.empty((max(tree.n - 1, 1), 3), dtype=torch.int32, device=tree.device)[:tree.n - 1]
    check(lib().pcgc_raht_forward_batch(_p(rgb), _p(tree.perm), tree.n, _p(tree.d), _p(tree.lo), _p(tree.hi), _p(tree.cross_order),
                                        tree.bit_off.ctypes.data, _p(tree.offsets) + tree.frames * 65 * 4, _raht_form(form), _p(val), _p(H),
                                        _stream(rgb)), 'raht_forward_batch')
    return H, val.index_select(0, tree.starts_dev)


def raht_quantize_batch(tree, H, q_luma, q_chroma):
    """q_luma, q_chroma: B ints each -> (tokens int16 [3(n-B)], ctx [3(n-B)], escapes [E], hist int32 [B,48,64]) on the device in the
    batch's coding order: frame b's tokens are tree.tok[b] .. tree.tok[b + 1], its escapes follow those of the frames before it and are
    hist[b, :, 63].sum() many"""
    n, dev, B = tree.n, tree.device, tree.frames
    ql, qc = _frame_steps(tree, q_luma, q_chroma)
    t = max(3 * (n - B), 1)
    tokens = torch.empty(t, dtype=torch.int16, device=dev)[:3 * (n - B)]
    ctx = torch.empty(t, dtype=torch.int16, device=dev)[:3 * (n - B)]
    esc = torch.empty(t, dtype=torch.int16, device=dev)
    n_esc = torch.empty(1, dtype=torch.int32, device=dev)
    hist = torch.empty((B, RAHT_CONTEXTS, 64), dtype=torch.int32, device=dev)
    ws_bytes = int(lib().pcgc_raht_quantize_batch_workspace_bytes(n, B))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    check(lib().pcgc_raht_quantize_batch(_p(_dev(H, torch.int32, 'raht_quantize_batch: H')), n, B, _p(tree.keys), _p(tree.d), _p(tree.lo),
                                         _p(tree.hi), _p(tree.order), ql.ctypes.data, qc.ctypes.data, _p(tokens), _p(ctx), _p(esc), _p(n_esc),
                                         _p(hist), _p(ws), ws_bytes, _stream(H)), 'raht_quantize_batch')
    return tokens, ctx, esc, hist


def raht_dequantize_batch(tree, tokens, escapes, esc_counts, q_luma, q_chroma):
    """tokens int16 [3(n-B)] and the frames' escape lists one after the other (int16 storage) on the device, esc_counts: the length of
    each list -> H^ int32 [n-1,3].  PcgcError naming the frame whose number of escape tokens is not the length of its list."""
    n, dev, B = tree.n, tree.device, tree.frames
    ql, qc = _frame_steps(tree, q_luma, q_chroma)
    if tokens.shape[0] != 3 * (n - B):
        raise PcgcError(f'raht_dequantize_batch: {tokens.shape[0]} tokens for {n} points in {B} frames')
    Hhat = torch.empty((max(n - 1, 1), 3), dtype=torch.int32, device=dev)[:n - 1]
    count = torch.empty(17, dtype=torch.int32, device=dev)
    ws_bytes = int(lib().pcgc_raht_dequantize_batch_workspace_bytes(n, B))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    tokens, escapes = _dev(tokens, torch.int16, 'raht_dequantize_batch: tokens'), _dev(escapes, torch.int16, 'raht_dequantize_batch: escapes')
    check(lib().pcgc_raht_dequantize_batch(_p(tokens), _p(escapes) if escapes.shape[0] else None, escapes.shape[0], n, B, _p(tree.keys),
                                           _p(tree.lo), _p(tree.hi), _p(tree.order), ql.ctypes.data, qc.ctypes.data, _p(Hhat), _p(count), _p(ws),
                                           ws_bytes, _stream(tokens)), 'raht_dequantize_batch')
    count = count.cpu().tolist()
    for b in range(B):
        if count[b] != int(esc_counts[b]):
            raise PcgcError(f'raht_dequantize_batch: frame {b}: {count[b]} escape tokens but {int(esc_counts[b])} escapes')
    return Hhat


def raht_inverse_batch(tree, Hhat, dc, form=None):
    """H^ int32 [n-1,3] and the frames' DCs ([B,3] ints) -> rgb uint8 [n,3] in the row order of the batch's coordinates"""
    val = torch.empty((tree.n, 3), dtype=torch.int32, device=tree.device)
    rgb = torch.empty((tree.n, 3), dtype=torch.uint8, device=tree.device)
    if tuple(Hhat.shape) != (tree.n - 1, 3):
        raise ValueError(f'raht_inverse_batch: H^ must be [{tree.n - 1},3], got {tuple(Hhat.shape)}')
    dc = np.ascontiguousarray(dc, dtype=np.int32)
    if dc.shape != (tree.frames, 3):
        raise ValueError(f'raht_inverse_batch: the DCs must be [{tree.frames},3], got {dc.shape}')
    dc = torch.from_numpy(dc).to(tree.device)
    check(lib().pcgc_raht_inverse_batch(_p(_dev(Hhat, torch.int32, 'raht_inverse_batch: H^')), _p(dc), _p(tree.starts_dev), tree.frames,
                                        _p(tree.perm), tree.n, _p(tree.d), _p(tree.lo), _p(tree.hi), _p(tree.cross_order),
                                        tree.bit_off.ctypes.data, _p(tree.offsets) + tree.frames * 65 * 4, _raht_form(form), _p(val), _p(rgb),
                                        _stream(Hhat)), 'raht_inverse_batch')
    return rgb


# ------------------------------------------------------------------------------------------------ colour codec, device coder (csrc/attribute_rans.hip)
def attr_rans_chunks(n, steps):
    """chunks of 64 x steps tokens that n tokens make"""
    return -(-int(n) // (RANS_LANES * int(steps)))


def _attr_table(table, dev):
    table = np.ascontiguousarray(table, dtype=np.uint16)
    if table.shape != (RAHT_CONTEXTS, 65):
        raise PcgcError(f'attr_rans: the table is uint16 [{RAHT_CONTEXTS}, 65], got {table.shape}')
    return torch.from_numpy(table.view(np.int16)).to(dev)


def attr_rans_encode(table, ctx, tokens, steps):
    """table uint16 [48, 65] (host; rc_encode_ctx's convention: entry 0 is 0, entry 64 stands for 0x10000), ctx (uint16 in int16 storage)
    and tokens int16 [n] on the device, as raht_quantize returns them -> the payload of `_A.bin` version 2 (include/pcgc_hip.h) as bytes,
    coded on the device in chunks of 64 x steps tokens; b'' for n = 0, without a launch.  One small synchronising copy (the length) and one
    copy of the finished payload.  PcgcError on a token outside 0 .. 63, a context outside 0 .. 47 or a token whose frequency is 0."""
    n, dev, steps = _dev(tokens, torch.int16, 'attr_rans_encode: tokens').shape[0], tokens.device, int(steps)
    if tokens.dim() != 1 or tuple(_dev(ctx, torch.int16, 'attr_rans_encode: ctx').shape) != (n,) or not 1 <= steps <= RANS_MAX_STEPS:
        raise PcgcError(f'attr_rans_encode: tokens {tuple(tokens.shape)}, ctx {tuple(ctx.shape)}, {steps} steps per chunk (1 .. 2^24)')
    table = _attr_table(table, dev)
    if n == 0:
        return b''
    cap = 8 + 516 * attr_rans_chunks(n, steps) + 4 * n
    out = torch.empty((cap + 7) // 8, dtype=torch.int64, device=dev)
    ws, nbytes = _rans_ws('attr', n, steps, dev)
    host = np.zeros(2, dtype=np.int64)
    check(lib().pcgc_attr_rans_encode(_p(table), _p(ctx), _p(tokens), n, steps, _p(out), cap, host.ctypes.data, _p(ws), nbytes, _stream(tokens)),
          'attr_rans_encode')
    if host[1]:
        raise PcgcError(f'attr_rans_encode: {int(host[1])} tokens cannot be coded (outside 0 .. 63, under a context outside 0 .. 47, or of '
                        'frequency 0 in their row)')
    return out.view(torch.uint8)[:int(host[0])].cpu().numpy().tobytes()


def attr_rans_layout(payload, n):
    """the host's checks of the payload of `_A.bin` version 2 against its n tokens and its own size -> (S, K).  PcgcError when S is outside
    1 .. 2^24, K is not ceil(n / (64 S)), the tables do not fit or the word counts do not add up to the byte length; n = 0 takes the empty
    payload alone -> (0, 0)."""
    return _rans_layout('attr', payload, n)


def attr_rans_decode(table, tree, payload, n):
    """table uint16 [48, 65] (host), tree: the RahtTree of the geometry (its `offsets` on the device give every token's context: they are
    computed there, never uploaded), payload: bytes of `_A.bin` version 2, n tokens -> (tokens int16 [n] on the device in coding order,
    the number of tokens that are 63).  The payload goes up in one copy, the two numbers come back in one.  PcgcError on a payload whose S,
    K or lengths disagree with n and its own size (checked here, before any launch) and on an unsound chunk (the kernel's verdict)."""
    n, dev = int(n), tree.offsets.device
    payload = bytes(payload)
    steps, chunks = attr_rans_layout(payload, n)
    if _dev(tree.offsets, torch.int32, 'attr_rans_decode: tree offsets').numel() < 65:
        raise PcgcError('attr_rans_decode: the tree has no bucket offsets')
    table = _attr_table(table, dev)
    if n == 0:
        return torch.empty(0, dtype=torch.int16, device=dev), 0
    up = torch.frombuffer(bytearray(payload) + bytes(-len(payload) % 8), dtype=torch.int64).to(dev)        # (8-byte aligned on the device)
    tokens = torch.empty(n, dtype=torch.int16, device=dev)
    ws, nbytes = _rans_ws('attr', n, steps, dev)
    host = np.zeros(2, dtype=np.int64)
    check(lib().pcgc_attr_rans_decode(_p(table), _p(tree.offsets), n, _p(up), len(payload), steps, _p(tokens), host.ctypes.data, _p(ws), nbytes,
                                      _stream(tokens)), 'attr_rans_decode')
    if host[1]:
        raise _rans_unsound('attr_rans_decode', int(host[1]), f' of {chunks}')
    return tokens, int(host[0])


def attr_rans_batch_layout(tokens_per_frame, chunk_steps):
    """How a batch's frames are cut into chunks and where their payloads stand in one device buffer.  tokens_per_frame: B token counts;
    chunk_steps: steps per chunk for every frame (0: each frame is one chunk with its own S_b = ceil(n_b / 64)), or B values ->
    {steps [B] (0 for a frame without tokens), chunks [B], first_chunk [B + 1], tok [B + 1], room [B] (8 + 516 K_b + 4 n_b, 0 without
    tokens), pay [B + 1] (byte offsets, multiples of 8)}, all int64 except steps (int32).  Chunks never straddle frames."""
    counts = np.asarray(tokens_per_frame, dtype=np.int64).reshape(-1)
    want = np.broadcast_to(np.asarray(chunk_steps, dtype=np.int64), counts.shape)
    if (counts < 0).any() or (want < 0).any() or (want > RANS_MAX_STEPS).any():
        raise ValueError(f'attr_rans_batch_layout: token counts {counts.tolist()}, steps per chunk {want.tolist()} (0 .. 2^24)')
    return _rans_batch_layout('attr', counts, want)


def _attr_tables(tables, frames, dev):
    tables = np.ascontiguousarray(tables, dtype=np.uint16)
    if tables.shape != (frames, RAHT_CONTEXTS, 65):
        raise PcgcError(f'attr_rans: the tables of a batch are uint16 [{frames}, {RAHT_CONTEXTS}, 65], got {tables.shape}')
    return torch.from_numpy(tables.view(np.int16)).to(dev)


def attr_rans_encode_batch(tables, ctx, tokens, tok, chunk_steps):
    """tables uint16 [B,48,65] (host), ctx and tokens [n] on the device as raht_quantize_batch returns them, tok [B + 1]: frame b's tokens
    are tok[b] .. tok[b + 1] -> B payloads (bytes; b'' for a frame without tokens), every one what attr_rans_encode gives for that frame
    alone at its own steps per chunk.  ONE launch sequence, one small synchronising copy and one copy of the payloads for the batch; a batch
    without tokens launches nothing.  PcgcError naming the frame with a token that cannot be coded."""
    tok = np.ascontiguousarray(tok, dtype=np.int64)
    B, n, dev = tok.size - 1, int(tok[-1]), tokens.device
    if _dev(tokens, torch.int16, 'attr_rans_encode_batch: tokens').dim() != 1 or tuple(_dev(ctx, torch.int16, 'attr_rans_encode_batch: ctx').shape) \
            != (n,) or tokens.shape[0] != n or not 1 <= B <= RAHT_MAX_FRAMES:
        raise PcgcError(f'attr_rans_encode_batch: tokens {tuple(tokens.shape)}, ctx {tuple(ctx.shape)}, {B} frames of {n} tokens')
    lay = attr_rans_batch_layout(np.diff(tok), chunk_steps)
    tables = _attr_tables(tables, B, dev)
    if n == 0:
        return [b''] * B
    pay, K = lay['pay'], int(lay['first_chunk'][-1])
    out = torch.empty(int(pay[-1]) // 8, dtype=torch.int64, device=dev)
    ws, nbytes = _rans_batch_ws('attr', n, K, dev)
    host = np.zeros(2 * B, dtype=np.int64)
    check(lib().pcgc_attr_rans_encode_batch(_p(tables), _p(ctx), _p(tokens), B, tok.ctypes.data, lay['steps'].ctypes.data, _p(out), pay.ctypes.data,
                                            host.ctypes.data, _p(ws), nbytes, _stream(tokens)), 'attr_rans_encode_batch')
    for b in range(B):
        if host[B + b]:
            raise PcgcError(f'attr_rans_encode_batch: frame {b}: {int(host[B + b])} tokens cannot be coded (outside 0 .. 63, under a context '
                            'outside 0 .. 47, or of frequency 0 in their row)')
    return _rans_fetch([(out.view(torch.uint8), pay, host[:B])])[0]                # the finished payloads, one copy


def attr_rans_decode_batch(tables, tree, payloads, tokens=None, names=None):
    """tables uint16 [B,48,65] (host), tree: the RahtBatchTree, payloads: per frame the bytes of a version-2 payload, or None for a frame
    that is not decoded here (its slice of the result is left unwritten) -> (tokens int16 [3(n-B)] on the device in the batch's coding
    order, the tokens that are 63 per frame).  Every payload's S, K and lengths are checked here before any launch; one upload, ONE launch
    sequence and one small copy for the batch.  tokens: the int16 [3(n-B)] device tensor to write the decoded frames' slices into (the
    others keep what they hold).  PcgcError naming the frame (names[b], else 'frame b') of a bad head or an unsound chunk."""
    B, dev, tok = tree.frames, tree.offsets.device, np.ascontiguousarray(tree.tok, dtype=np.int64)
    if len(payloads) != B:
        raise PcgcError(f'attr_rans_decode_batch: {len(payloads)} payloads for {B} frames')
    names = [f'frame {b}' for b in range(B)] if names is None else list(names)
    steps, chunks, pay, size, blob = _rans_decode_blob('attr', payloads, np.diff(tok), names)
    tables = _attr_tables(tables, B, dev)
    n = int(tok[-1])
    if tokens is None:
        tokens = torch.empty(max(n, 1), dtype=torch.int16, device=dev)[:n]
    elif tuple(_dev(tokens, torch.int16, 'attr_rans_decode_batch: tokens').shape) != (n,):
        raise PcgcError(f'attr_rans_decode_batch: a token buffer of {tuple(tokens.shape)} for {n} tokens')
    escapes = np.zeros(B, np.int64)
    if not steps.any():
        return tokens, escapes
    up = torch.frombuffer(blob, dtype=torch.int64).to(dev)
    ws, nbytes = _rans_batch_ws('attr', n, int(chunks.sum()), dev)
    host = np.zeros(2 * B, dtype=np.int64)
    check(lib().pcgc_attr_rans_decode_batch(_p(tables), _p(tree.offsets), B, tok.ctypes.data, steps.ctypes.data, _p(up), pay.ctypes.data,
                                            size.ctypes.data, _p(tokens), host.ctypes.data, _p(ws), nbytes, _stream(tokens)),
          'attr_rans_decode_batch')
    for b in range(B):
        if host[B + b]:
            raise _rans_unsound(f'{names[b]}: attr_rans_decode_batch', int(host[B + b]))
    return tokens, host[:B].copy()


# ------------------------------------------------------------------------------------------------ estimated normals (csrc/normals.hip)
NORMALS_MAX_R2 = 64
_NORMALS_BALL = {}


def _normals_ball(device, r2):
    """the ball masks of pcgc_normals_ball_masks(r2) on `device`: built once per (device, r2)"""
    key = (str(device), int(r2))
    if key not in _NORMALS_BALL:
        n = int(lib().pcgc_normals_ball_masks(int(r2), None))
        if n < 0:
            check(n, 'normals_ball_masks')
        tab = np.empty(n, np.uint64)
        if int(lib().pcgc_normals_ball_masks(int(r2), tab.ctypes.data)) != n:
            raise PcgcError('normals_ball_masks: size changed')
        _NORMALS_BALL[key] = torch.from_numpy(tab.view(np.int64)).to(device)
    return _NORMALS_BALL[key]


def estimate_normals(coords, r2=16, orient='centroid', index=None, want_moments=False):
    """Surface normals of a voxelised cloud from fixed-radius neighbourhoods (include/pcgc_hip.h, pcgc_normals_estimate).
    coords: int32 [N,4] (batch, x, y, z) device tensor or a sparse tensor; r2: integer squared radius, 1 .. 64; orient: 'centroid' (away from
    the centroid of the row's batch), a viewpoint (x, y, z) (towards it) or None (largest component positive); index: a D2Index of `coords`
    to reuse.  -> (normals float64 [N,3], lam float64 [N,3] ascending, count int32 [N], valid bool [N]) and, with want_moments, the exact
    moments int64 [N,10].  Rows that are not valid (fewer than 3 neighbours, or all of them on one line) have normal (0, 0, 0)."""
    coords = coords.C if hasattr(coords, 'C') else coords
    coords = _i32(coords, 'coords')
    if coords.dim() != 2 or coords.shape[1] != 4:
        raise PcgcError(f'estimate_normals: coords must be [N,4], got {tuple(coords.shape)}')
    if isinstance(r2, bool) or int(r2) != r2 or not 1 <= int(r2) <= NORMALS_MAX_R2:
        raise ValueError(f'estimate_normals: r2 must be an integer in 1 .. {NORMALS_MAX_R2}, got {r2!r}')
    r2 = int(r2)
    view = None
    if orient is None:
        mode = 0
    elif isinstance(orient, str):
        if orient != 'centroid':
            raise ValueError(f"estimate_normals: orient must be 'centroid', a viewpoint (x, y, z) or None, got {orient!r}")
        mode = 1
    else:
        view = np.ascontiguousarray(np.asarray(orient, np.float64).reshape(-1))
        if view.shape != (3,) or not np.isfinite(view).all():
            raise ValueError(f'estimate_normals: a viewpoint is three finite numbers, got {orient!r}')
        mode = 2
    n, dev = coords.shape[0], coords.device
    if n == 0:
        out = (torch.empty((0, 3), dtype=torch.float64, device=dev), torch.empty((0, 3), dtype=torch.float64, device=dev),
               torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.bool, device=dev))
        return out + (torch.empty((0, 10), dtype=torch.int64, device=dev),) if want_moments else out
    check_coords(coords, 'estimate_normals')
    if index is None:
        index = D2Index(coords)
    elif index.n != n or index.coords.data_ptr() != coords.data_ptr():
        raise PcgcError('estimate_normals: the index was built from another tensor')
    ball = _normals_ball(dev, r2)
    moments = torch.empty((n, 10), dtype=torch.int64, device=dev)
    normals = torch.empty((n, 3), dtype=torch.float64, device=dev)
    lam = torch.empty((n, 3), dtype=torch.float64, device=dev)
    count = torch.empty(n, dtype=torch.int32, device=dev)
    valid = torch.empty(n, dtype=torch.bool, device=dev)
    ws_bytes = int(lib().pcgc_normals_workspace_bytes(n))
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=dev)
    check(lib().pcgc_normals_estimate(_p(coords), n, _p(index.qs), _p(index.perm), *index.tables(), _p(ball), r2, mode,
                                      None if view is None else view.ctypes.data, _p(moments), _p(normals), _p(lam), _p(count), _p(valid),
                                      _p(ws), ws_bytes, _stream(coords)), 'normals_estimate')
    return (normals, lam, count, valid, moments) if want_moments else (normals, lam, count, valid)


# ------------------------------------------------------------------------------------------------ meshes -> training clouds
def _mesh(verts, faces):
    _dev(verts, torch.float64, 'verts')
    _dev(faces, torch.int32, 'faces')
    if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise PcgcError('a mesh is verts [V,3] float64 and faces [T,3] int32')
    return verts.shape[0], faces.shape[0]


def _u64(v, what):
    v = int(v)
    if not 0 <= v < 1 << 64:
        raise ValueError(f'{what} must be an unsigned 64-bit integer, got {v}')
    return v


def mesh_area_cdf(verts, faces):
    """-> float64 [T]: inclusive sums of the triangle areas, never decreasing and bitwise reproducible (fixed summation order).
    Raises PcgcError if a face names a vertex outside [0, V) (reads one int32 back)."""
    V, T = _mesh(verts, faces)
    cdf = torch.empty(T, dtype=torch.float64, device=verts.device)
    bad = torch.empty(1, dtype=torch.int32, device=verts.device)
    ws_bytes = int(lib().pcgc_mesh_cdf_workspace_bytes(T))
    ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=verts.device)
    check(lib().pcgc_mesh_area_cdf(_p(verts), V, _p(faces), T, _p(cdf), _p(bad), _p(ws), ws_bytes, _stream(verts)), 'mesh_area_cdf')
    n_bad = int(bad.item())
    if n_bad:
        raise PcgcError(f'mesh_area_cdf: {n_bad} of {T} faces name a vertex outside [0, {V})')
    return cdf


def mesh_sample(verts, faces, cdf, seed, first, n, want_tri=True, want_points=True):
    """Samples first .. first+n-1 of `seed` -> (tri int32 [n] or None, points float64 [n,3] or None).  Sample i depends on (seed, i) only."""
    V, T = _mesh(verts, faces)
    _dev(cdf, torch.float64, 'cdf')
    if cdf.shape != (T,):
        raise PcgcError(f'cdf: expected shape ({T},), got {tuple(cdf.shape)}')
    n = int(n)
    tri = torch.empty(max(n, 0), dtype=torch.int32, device=verts.device) if want_tri else None
    pts = torch.empty((max(n, 0), 3), dtype=torch.float64, device=verts.device) if want_points else None
    check(lib().pcgc_mesh_sample(_p(verts), V, _p(faces), _p(cdf), T, _u64(seed, 'seed'), _u64(first, 'first'), n, _p(tri), _p(pts),
                                 _stream(verts)), 'mesh_sample')
    return tri, pts


def mesh_voxelize(verts, faces, cdf, seed, n, R, resolution):
    """mesh2pc after the file read: n samples, rotated by R (3x3, points . R), normalised by the scalar min and max of all coordinates,
    rounded half-even onto 0..resolution -> the distinct voxels as int32 [M,4] rows (0, x, y, z) in (z, y, x) order.  Raises PcgcError
    for n < 1, a resolution outside 1..1023, a total area that is not positive, or samples that all fall on one value."""
    V, T = _mesh(verts, faces)
    _dev(cdf, torch.float64, 'cdf')
    if cdf.shape != (T,):
        raise PcgcError(f'cdf: expected shape ({T},), got {tuple(cdf.shape)}')
    R = np.ascontiguousarray(R, dtype=np.float64)
    if R.shape != (3, 3):
        raise PcgcError(f'rotation: expected a 3x3 matrix, got shape {R.shape}')
    n, resolution = int(n), int(resolution)
    dev = verts.device
    ws_bytes = int(lib().pcgc_mesh_voxelize_workspace_bytes(max(min(resolution, 1 << 20), 0)))     # (0 for an unsupported resolution)
    ws = torch.empty(max(ws_bytes, 64), dtype=torch.uint8, device=dev)
    cap = max(min(n, (resolution + 1) ** 3), 0) if ws_bytes else 0
    out = torch.empty((max(cap, 1), 4), dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    check(lib().pcgc_mesh_voxelize(_p(verts), V, _p(faces), _p(cdf), T, _u64(seed, 'seed'), n, R.ctypes.data, resolution, _p(out), cap,
                                   _p(count), _p(ws), ws_bytes, _stream(verts)), 'mesh_voxelize')
    m = int(count.item())
    if m == -1:
        raise PcgcError('mesh_voxelize: the total area of the mesh is not a positive finite number')
    if m < 0:
        raise PcgcError('mesh_voxelize: every sample has the same coordinate value (max - min is not a positive finite number)')
    if m > cap:
        raise PcgcError(f'mesh_voxelize: {m} voxels from {n} samples')           # (cannot happen: one bit per sample at most)
    return out[:m]


# ------------------------------------------------------------------------------------------------ data loader: batches out of the arena
COLLATE_MAX_ITEMS = CONSTANTS['PCGC_COLLATE_MAX_ITEMS']


def collate_rows(arena, items, out=None):
    """One batch out of the data loader's arena in one launch -> (coords int32 [N, 4] rows (item, x, y, z), feats float32 [N, 1] of ones).
    arena: uint8 device tensor; items: up to 16 of (byte offset, rows, width in bytes 1 / 2 / 4, symmetry code 0..47, extent), each cloud
    three packed values per row from its offset (a multiple of 16) in file order.  out = (coords, feats) with at least N rows writes into
    those and returns their first N rows; rows past N are not touched.  No items or no rows: nothing is launched."""
    from ._lib import CollateItem
    _dev(arena, torch.uint8, 'arena')
    items = list(items)
    if len(items) > COLLATE_MAX_ITEMS:
        raise ValueError(f'a batch holds at most {COLLATE_MAX_ITEMS} items, got {len(items)}')
    table = (CollateItem * max(len(items), 1))()
    n = 0
    for k, (offset, rows, width, symmetry, extent) in enumerate(items):
        offset, rows, width = int(offset), int(rows), int(width)
        if width not in (1, 2, 4) or rows < 0 or offset < 0 or offset % 16 or offset + 3 * width * rows > arena.numel():
            raise PcgcError(f'collate_rows: item {k} (offset {offset}, {rows} rows of 3 x {width} bytes) does not lie in the arena of '
                            f'{arena.numel()} bytes on a 16-byte boundary')
        if not 0 <= int(symmetry) < 48:
            raise ValueError(f'collate_rows: symmetry code must be 0..47, got {symmetry}')
        table[k] = CollateItem(offset, n, rows, width, int(symmetry), int(extent), 0)
        n += rows
    if out is None:
        coords = torch.empty((n, 4), dtype=torch.int32, device=arena.device)
        feats = torch.empty((n, 1), dtype=torch.float32, device=arena.device)
    else:
        coords, feats = _i32(out[0], 'out coords'), _dev(out[1], torch.float32, 'out feats')
        if coords.dim() != 2 or coords.shape[1] != 4 or coords.shape[0] < n or feats.numel() < n or feats.device != coords.device \
                or coords.device != arena.device:
            raise PcgcError(f'collate_rows: out must be int32 [>= {n}, 4] and float32 [>= {n}, 1] on the arena\'s device')
    check(lib().pcgc_collate_rows(_p(arena), table, len(items), _p(coords), _p(feats), _stream(arena)), 'collate_rows')
    return coords[:n], feats[:n]


# ------------------------------------------------------------------------------------------------ voxelising a raw cloud
VOXELIZE_MERGES = {'mean': 0, 'first': 1}
VOXELIZE_MAX_ROWS = (1 << 31) - 1
Voxels = namedtuple('Voxels', 'coords counts voxel_of colours origin scale bits')


def voxelize_tile_rows():
    return int(lib().pcgc_voxelize_tile_rows())


def voxelize_frame(lo, hi, bits, origin=None, scale=None):
    """the frame of tests/voxelize_reference.py from the per-axis minima and maxima (fp64) -> (origin (x, y, z), scale), Python floats.
    ValueError for an origin that is not finite and a scale that is not finite and positive."""
    lo, hi = [float(v) for v in lo], [float(v) for v in hi]
    origin = lo if origin is None else [float(v) for v in origin]
    if len(origin) != 3:
        raise ValueError(f'voxelize: origin {origin}: three values')
    if scale is None:
        e = max(h - l for h, l in zip(hi, lo))
        with np.errstate(over='ignore'):
            scale = float(np.float64((1 << bits) - 1) / np.float64(e)) if e != 0 else 1.0
    scale = float(scale)
    if not all(np.isfinite(v) for v in origin):
        raise ValueError(f'voxelize: origin {origin} is not finite')
    if not (np.isfinite(scale) and scale > 0):
        raise ValueError(f'voxelize: scale {scale} is not finite and positive')
    return tuple(origin), scale


def voxelize(points, colours=None, bits=10, origin=None, scale=None, merge='mean', times=None):
    """points float32 or float64 [N,3] (device) in any units, colours uint8 [N,3] or None -> Voxels: coords int32 [M,4] rows (0, x, y, z)
    of the distinct voxels in (z, y, x) order, counts int32 [M], voxel_of int32 [N], colours uint8 [M,3] or None, and the frame: origin
    (x, y, z), scale, bits.  q = rint((float64(p) - origin) * scale); origin and scale default to the minimum and (2^bits - 1) / the largest
    extent.  merge: 'mean' (rounds a half up) or 'first' (the voxel's lowest input row).  Every output equals tests/voxelize_reference.py.
    Strided tensors are packed first.  ValueError naming the count for rows with a NaN or an infinity, and for rows the frame given puts
    outside [0, 2^bits - 1].  N = 0 returns empty outputs without a launch.  times (measurement hook): a dict -> seconds of 'bounds',
    'quantise', 'sort', 'merge' and 'copies' added to it, with a synchronisation after each."""
    if not torch.is_tensor(points) or not points.is_cuda:
        raise PcgcError('voxelize: points must be a ROCm device tensor (no CPU fallback exists)')
    if points.dtype not in (torch.float32, torch.float64):
        raise ValueError(f'voxelize: points must be float32 or float64, got {points.dtype}')
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f'voxelize: points must be [N,3], got {tuple(points.shape)}')
    if isinstance(bits, bool) or not isinstance(bits, (int, np.integer)) or not 1 <= bits <= 20:
        raise ValueError(f'voxelize: bits {bits!r}: an integer in 1 .. 20')
    if merge not in VOXELIZE_MERGES:
        raise ValueError(f'voxelize: merge {merge!r}: one of {sorted(VOXELIZE_MERGES)}')
    n, dev, bits = points.shape[0], points.device, int(bits)
    if n > VOXELIZE_MAX_ROWS:
        raise ValueError(f'voxelize: {n} rows; at most 2^31 - 1')
    if colours is not None:
        if not torch.is_tensor(colours) or colours.device != dev or colours.dtype != torch.uint8 or tuple(colours.shape) != (n, 3):
            raise ValueError(f'voxelize: colours must be uint8 [{n},3] on the device of the points')
        colours = colours.contiguous()
    points = points.contiguous()
    if n == 0:
        o = (0.0, 0.0, 0.0) if origin is None else tuple(float(v) for v in origin)
        return Voxels(torch.empty((0, 4), dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int32, device=dev),
                      torch.empty(0, dtype=torch.int32, device=dev),
                      None if colours is None else torch.empty((0, 3), dtype=torch.uint8, device=dev), o, 1.0 if scale is None else float(scale), bits)
    is_f64 = int(points.dtype == torch.float64)
    L, s = lib(), _stream(points)
    with torch.cuda.device(dev):
        t0 = tick_phase(times, None, 0.0, dev)
        bounds = torch.empty(6, dtype=torch.float64, device=dev)
        status = torch.empty(2, dtype=torch.int64, device=dev)              # rows with a NaN or an infinity | rows outside the lattice
        ws_bytes = max(int(L.pcgc_voxelize_bounds_workspace_bytes(n)), int(L.pcgc_voxelize_heads_workspace_bytes(n)))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        check(L.pcgc_voxelize_bounds(_p(points), is_f64, n, _p(bounds), _p(status), _p(ws), ws_bytes, s), 'voxelize_bounds')
        t0 = tick_phase(times, 'bounds', t0, dev)
        bad = int(status[0].item())
        if bad:
            raise ValueError(f'voxelize: {bad} of {n} rows hold a NaN or an infinity')
        b = bounds.cpu().tolist()
        t0 = tick_phase(times, 'copies', t0, dev)
        origin, scale = voxelize_frame(b[:3], b[3:], bits, origin, scale)
        keys = torch.empty(n, dtype=torch.int64, device=dev)
        rows = torch.empty(n, dtype=torch.int32, device=dev)
        check(L.pcgc_voxelize_quantize(_p(points), is_f64, n, bits, origin[0], origin[1], origin[2], scale, _p(keys), _p(rows),
                                       status[1:].data_ptr(), s), 'voxelize_quantize')
        t0 = tick_phase(times, 'quantise', t0, dev)
        sorted_keys, sorted_rows, rank = torch.empty_like(keys), torch.empty_like(rows), torch.empty_like(rows)
        check(L.pcgc_voxelize_heads(_p(keys), _p(rows), n, bits, _p(sorted_keys), _p(sorted_rows), _p(rank), _p(ws), ws_bytes, s), 'voxelize_heads')
        t0 = tick_phase(times, 'sort', t0, dev)
        outside, m = torch.stack([status[1], rank[n - 1].to(torch.int64)]).cpu().tolist()
        t0 = tick_phase(times, 'copies', t0, dev)
        if outside:
            raise ValueError(f'voxelize: {outside} of {n} rows fall outside [0, 2^{bits} - 1] in the frame given '
                             f'(origin {list(origin)}, scale {scale})')
        del keys, rows
        coords = torch.empty((m, 4), dtype=torch.int32, device=dev)
        counts = torch.empty(m, dtype=torch.int32, device=dev)
        voxel_of = torch.empty(n, dtype=torch.int32, device=dev)
        out = None if colours is None else torch.empty((m, 3), dtype=torch.uint8, device=dev)
        ws_bytes = int(L.pcgc_voxelize_merge_workspace_bytes(m))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        check(L.pcgc_voxelize_merge(_p(sorted_keys), _p(sorted_rows), _p(rank), n, m, _p(colours), VOXELIZE_MERGES[merge], _p(coords), _p(counts),
                                    _p(voxel_of), _p(out), _p(ws), ws_bytes, s), 'voxelize_merge')
        tick_phase(times, 'merge', t0, dev)
    return Voxels(coords, counts, voxel_of, out, origin, scale, bits)


# ------------------------------------------------------------------------------------------------ cleaning a voxelised cloud
CLEAN_MAX_ROWS = 1 << 24
Cleaned = namedtuple('Cleaned', 'keep neighbours labels sizes coords colours removed_density removed_component n_components rounds')


def _clean_int(name, v, lo, hi=None):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo or (hi is not None and v > hi):
        raise ValueError(f'clean: {name} {v!r}: an integer {"of at least " + str(lo) if hi is None else f"in {lo} .. {hi}"}')
    return int(v)


def _clean_coords(coords, who):
    coords = coords.C if hasattr(coords, 'C') else coords
    if not torch.is_tensor(coords) or not coords.is_cuda:
        raise PcgcError(f'{who}: coords must be a ROCm device tensor (no CPU fallback exists)')
    if coords.dtype != torch.int32 or coords.dim() != 2 or coords.shape[1] != 4:
        raise ValueError(f'{who}: coords must be int32 [N,4], got {coords.dtype} {tuple(coords.shape)}')
    if coords.shape[0] > CLEAN_MAX_ROWS:
        raise ValueError(f'{who}: {coords.shape[0]} rows; at most 2^24')
    coords = coords.contiguous()
    if coords.shape[0]:
        try:
            check_coords(coords, who)
        except PcgcError as e:
            raise ValueError(str(e)) from None
    return coords


def _repeated(who, repeated, n):
    if repeated:
        raise ValueError(f'{who}: {repeated} of {n} rows repeat an earlier voxel; the rows must be distinct voxels')


def clean_neighbours(coords, r2=16, min_neighbours=0, index=None):
    """stage 1 of clean on rows that passed check_coords -> (neighbours int32 [N], keep1 uint8 [N], rows that repeat an earlier voxel)"""
    n, dev = coords.shape[0], coords.device
    index = D2Index(coords) if index is None else index
    ball = _normals_ball(dev, r2)
    neighbours = torch.empty(n, dtype=torch.int32, device=dev)
    keep1 = torch.empty(n, dtype=torch.uint8, device=dev)
    repeated = torch.empty(1, dtype=torch.int32, device=dev)
    check(lib().pcgc_clean_neighbours(_p(index.qs), _p(index.perm), n, _p(index.cells.keys), _p(index.cells.vals), index.cells.cap,
                                      _p(index.masks), _p(index.runlen), _p(ball), r2, min_neighbours, _p(neighbours), _p(keep1), _p(repeated),
                                      _stream(coords)), 'clean_neighbours')
    return neighbours, keep1, repeated


def components(nbr):
    """connected components of the rows of a k3 map nbr int32 [27, n] (-1 = absent): -> (labels int32 [n] = the smallest row of the row's
    component, sizes int32 [n], number of components, rounds the labelling took)"""
    _i32(nbr, 'nbr')
    if nbr.dim() != 2 or nbr.shape[0] != 27:
        raise PcgcError(f'components: the map must be [27, n], got {tuple(nbr.shape)}')
    n, dev = nbr.shape[1], nbr.device
    labels = torch.empty(n, dtype=torch.int32, device=dev)
    sizes = torch.empty(n, dtype=torch.int32, device=dev)
    ws_bytes = int(lib().pcgc_components_workspace_bytes(n))
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=dev)
    n_components, rounds = ctypes.c_int64(0), ctypes.c_int32(0)
    check(lib().pcgc_components(_p(nbr), n, _p(labels), _p(sizes), ctypes.byref(n_components), ctypes.byref(rounds), _p(ws), ws_bytes,
                                _stream(nbr)), 'components')
    return labels, sizes, int(n_components.value), int(rounds.value)


def _components_of(coords, who, times=None, t0=0.0, distinct=False):
    """hash + k3 map at stride 1 + components of distinct voxels (checked here unless the caller has) -> (labels, sizes, n_components, rounds)"""
    n, dev = coords.shape[0], coords.device
    if n == 0:
        return torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int32, device=dev), 0, 0
    table = HashTable(coords, 1)
    if not distinct:
        _repeated(who, n - int(mask_scan(first_occurrence_mask(coords, table))[1].item()), n)
    nbr = kmap_k3(coords, 1, table)
    t0 = tick_phase(times, 'map', t0, dev)
    out = components(nbr)
    tick_phase(times, 'components', t0, dev)
    return out


def connected_components(coords):
    """stage 2 of clean on all rows: coords int32 [N,4] (batch, x, y, z), distinct voxels -> (labels int32 [N] = the smallest row of the row's
    26-connected component, sizes int32 [N], number of components); clean(coords).rounds has the rounds the labelling took"""
    coords = _clean_coords(coords, 'connected_components')
    return _components_of(coords, 'connected_components')[:3]


def clean(coords, colours=None, r2=16, min_neighbours=0, min_component=1, keep_largest=0, times=None):
    """Outlier and fragment removal of a voxelised cloud (every output equals tests/clean_reference.py).  coords int32 [N,4]
    (batch, x, y, z) device tensor of DISTINCT voxels, colours uint8 [N,3] or None.  Stage 1: neighbours = the other rows of the batch within
    squared distance r2 (1 .. 64), keep1 = neighbours >= min_neighbours.  Stage 2: the 26-connected components of the survivors; labels = the
    smallest input row of the row's component (-1 where stage 1 dropped the row), sizes = its rows (0 there); a row stays when its component
    has min_component rows and, with keep_largest = n > 0, is one of the n largest of its batch item (ties to the smaller label).
    -> Cleaned(keep bool [N], neighbours, labels, sizes int32 [N], coords [M,4], colours [M,3] or None (input order), removed_density,
    removed_component, n_components, rounds).  ValueError naming the count for rows out of range and rows that repeat a voxel.  times
    (measurement hook): a dict -> seconds of 'index', 'counts', 'map', 'components', 'select', 'compaction' and 'copies' added to it."""
    r2 = _clean_int('r2', r2, 1, NORMALS_MAX_R2)
    min_neighbours, min_component, keep_largest = _clean_int('min_neighbours', min_neighbours, 0, (1 << 31) - 1), \
        _clean_int('min_component', min_component, 1, (1 << 31) - 1), _clean_int('keep_largest', keep_largest, 0, (1 << 31) - 1)
    coords = _clean_coords(coords, 'clean')
    n, dev = coords.shape[0], coords.device
    if colours is not None:
        if not torch.is_tensor(colours) or colours.device != dev or colours.dtype != torch.uint8 or tuple(colours.shape) != (n, 3):
            raise ValueError(f'clean: colours must be uint8 [{n},3] on the device of the coordinates')
        colours = colours.contiguous()
    if n == 0:
        e = lambda dt: torch.empty(0, dtype=dt, device=dev)
        return Cleaned(e(torch.bool), e(torch.int32), e(torch.int32), e(torch.int32), coords, colours, 0, 0, 0, 0)
    L, s = lib(), _stream(coords)
    with torch.cuda.device(dev):
        t0 = tick_phase(times, None, 0.0, dev)
        index = D2Index(coords)
        t0 = tick_phase(times, 'index', t0, dev)
        neighbours, keep1, repeated = clean_neighbours(coords, r2, min_neighbours, index)
        prefix, total = mask_scan(keep1)
        t0 = tick_phase(times, 'counts', t0, dev)
        repeated, n1 = torch.stack([repeated[0], total[0]]).cpu().tolist()
        t0 = tick_phase(times, 'copies', t0, dev)
        _repeated('clean', repeated, n)
        del index
        survivors, orig = compact_coords(coords, keep1, prefix, n1), compact_index(keep1, prefix, n1)
        t0 = tick_phase(times, 'compaction', t0, dev)
        labels_c, sizes_c, n_components, rounds = _components_of(survivors, 'clean', times, t0, distinct=True)
        t0 = tick_phase(times, None, 0.0, dev)
        labels = torch.empty(n, dtype=torch.int32, device=dev)
        sizes = torch.empty(n, dtype=torch.int32, device=dev)
        check(L.pcgc_clean_expand(_p(keep1), _p(prefix), _p(orig), _p(labels_c), _p(sizes_c), n, n1, _p(labels), _p(sizes), s), 'clean_expand')
        keep = torch.empty(n, dtype=torch.uint8, device=dev)
        ws_bytes = int(L.pcgc_clean_select_workspace_bytes(n))
        ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=dev)
        check(L.pcgc_clean_select(_p(coords), _p(labels), _p(sizes), n, min_component, keep_largest, _p(keep), _p(ws), ws_bytes, s), 'clean_select')
        prefix, total = mask_scan(keep)
        t0 = tick_phase(times, 'select', t0, dev)
        m = int(total.item())
        t0 = tick_phase(times, 'copies', t0, dev)
        out = compact_coords(coords, keep, prefix, m)
        out_colours = None
        if colours is not None:
            out_colours = torch.empty((m, 3), dtype=torch.uint8, device=dev)
        if colours is not None and m:
            check(L.pcgc_clean_compact_colours(_p(colours), _p(keep), _p(prefix), n, _p(out_colours), s), 'clean_compact_colours')
        tick_phase(times, 'compaction', t0, dev)
    return Cleaned(keep.view(torch.bool), neighbours, labels, sizes, out, out_colours, n - n1, n1 - m, n_components, rounds)


# ------------------------------------------------------------------------------------------------ kd-tree blocks of a large cloud
PARTITION_MAX_BLOCKS = CONSTANTS['PARTITION_MAX_BLOCKS']
PARTITION_MAX_ROWS = 1 << 27
PARTITION_ALIGNS = (8, 16, 32, 64, 128, 256, 512, 1024)
PARTITION_PHASES = ('bounds', 'coarse', 'cut', 'fine', 'assign', 'order', 'copies')          # the header's PARTITION_PHASE_* enum, in its order
if [CONSTANTS['PARTITION_PHASE_' + phase.upper()] for phase in PARTITION_PHASES] != list(range(CONSTANTS['PARTITION_PHASE_COPIES'] + 1)):
    raise PcgcError('ops.PARTITION_PHASES does not follow the PARTITION_PHASE_* enum of include/pcgc_hip.h')
Partition = namedtuple('Partition', 'block_of perm table rounds oversize')


def _partition_rows(coords, who):
    """the rows of partition and partition_gather: a device tensor int32 [N,3] or [N,4], made contiguous"""
    coords = coords.C if hasattr(coords, 'C') else coords
    if not torch.is_tensor(coords) or not coords.is_cuda:
        raise PcgcError(f'{who}: coords must be a ROCm device tensor (no CPU fallback exists)')
    if coords.dtype != torch.int32 or coords.dim() != 2 or coords.shape[1] not in (3, 4):
        raise ValueError(f'{who}: coords must be int32 [N,3] or [N,4], got {coords.dtype} {tuple(coords.shape)}')
    if coords.shape[0] > PARTITION_MAX_ROWS:
        raise ValueError(f'{who}: {coords.shape[0]} rows; at most 2^27')
    return coords.contiguous()


def partition(coords, max_num, align=8, times=None):
    """kd-tree blocks of at most max_num rows (every output equals tests/partition_reference.py).  coords: device tensor int32
    [N,3] (x, y, z) or [N,4] (batch 0, x, y, z), rows in any order, not necessarily distinct; align: a power of two in 8 .. 1024, no cell of
    that size is shared by two blocks.  -> Partition(block_of int32 [N], perm int32 [N] (rows in block-major order, stable), table int32 [B,8]
    = (first_row, rows, lo_x, lo_y, lo_z, hi_x, hi_y, hi_z), rounds, oversize).  ValueError naming the count for rows outside [0, 2^20), rows
    of another batch item, more than 2^27 rows and more than 1 024 blocks.  times (measurement hook): a dict -> seconds of 'bounds', 'coarse',
    'cut', 'fine', 'assign', 'order' and 'copies' added to it (the call then waits for the device after every phase)."""
    if isinstance(max_num, bool) or not isinstance(max_num, (int, np.integer)) or max_num < 1:
        raise ValueError(f'partition: max_num {max_num!r}: an integer of at least 1')
    if isinstance(align, bool) or not isinstance(align, (int, np.integer)) or align not in PARTITION_ALIGNS:
        raise ValueError(f'partition: align {align!r}: a power of two in 8 .. 1024')
    coords = _partition_rows(coords, 'partition')
    n, cols, dev = coords.shape[0], coords.shape[1], coords.device
    max_num = min(int(max_num), (1 << 63) - 1)
    if n == 0:                                                           # (no rows, no blocks: an empty tensor has no address to hand on)
        e = torch.empty(0, dtype=torch.int32, device=dev)
        return Partition(e, torch.empty(0, dtype=torch.int32, device=dev), torch.empty((0, 8), dtype=torch.int32, device=dev), 0, 0)
    L = lib()
    with torch.cuda.device(dev):
        block_of = torch.empty(n, dtype=torch.int32, device=dev)
        perm = torch.empty(n, dtype=torch.int32, device=dev)
        table = torch.empty((PARTITION_MAX_BLOCKS, 8), dtype=torch.int32, device=dev)
        ws_bytes = int(L.pcgc_partition_workspace_bytes(n))
        ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=dev)
        info = (ctypes.c_int64 * CONSTANTS['PARTITION_INFO_WORDS'])()
        seconds = None if times is None else (ctypes.c_double * CONSTANTS['PARTITION_PHASE_WORDS'])()
        code = L.pcgc_partition(_p(coords), n, cols, max_num, int(align), _p(block_of), _p(perm), _p(table), info, seconds, _p(ws), ws_bytes,
                                _stream(coords))
    rounds, blocks, oversize, bad_range, bad_batch, would_be = (int(info[CONSTANTS['PARTITION_INFO_' + word]]) for word in (
        'ROUNDS', 'BLOCKS', 'OVERSIZE', 'BAD_RANGE', 'BAD_BATCH', 'WOULD_BE'))
    if code == -3:
        if bad_batch:
            raise ValueError(f'partition: {bad_batch} of {n} rows have a batch index other than 0')
        raise ValueError(f'partition: {bad_range} of {n} rows are outside 0 .. 2^20 - 1')
    if code == -4:
        raise ValueError(f'partition: {would_be} blocks; at most {PARTITION_MAX_BLOCKS} (a larger max_num gives fewer)')
    check(code, 'partition')
    if times is not None:
        for j, phase in enumerate(PARTITION_PHASES):
            times[phase] = times.get(phase, 0.0) + seconds[j]
    return Partition(block_of, perm, table[:blocks], rounds, oversize)


def partition_gather(coords, part, first_block, blocks, table=None):
    """the collated rows int32 [rows,4] of blocks first_block .. first_block + blocks - 1 of a Partition: (block - first_block, x, y, z), the
    blocks contiguous and each in the input order of its rows.  table: the partition's table on the host (saves the copy)"""
    coords = _partition_rows(coords, 'partition_gather')
    n, dev = coords.shape[0], coords.device
    table = part.table.cpu().numpy() if table is None else table
    if blocks < 1 or first_block < 0 or first_block + blocks > len(table):
        raise ValueError(f'partition_gather: blocks {first_block} .. {first_block + blocks - 1} of {len(table)}')
    if len(part.perm) != n or len(part.block_of) != n:
        raise ValueError(f'partition_gather: the partition is of {len(part.perm)} rows, the cloud has {n}')
    first_row = int(table[first_block, 0])
    rows = int(table[first_block:first_block + blocks, 1].sum())
    out = torch.empty((rows, 4), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(lib().pcgc_partition_gather(_p(coords), n, coords.shape[1], _p(part.perm), _p(part.block_of), first_row, rows, first_block, _p(out),
                                          _stream(coords)), 'partition_gather')
    return out


# ------------------------------------------------------------------------------------------------ rendering a cloud into views
RENDER_MAX_SLICES = 64                   # batch items x views
RENDER_MAX_SIDE = 4096
RENDER_MAX_R = 4
RENDER_COORD_BITS = 21                   # coordinates lie in [0, 2^21)
RENDER_METRIC_SUMS = ('union', 'intersection', 'sse_r', 'sse_g', 'sse_b', 'sse_y', 'sse_depth', 'depth_out_of_range')
Rendered = namedtuple('Rendered', 'image depth index mask matrices')


def render_splat_rows():
    """rows per workgroup of the splat kernel"""
    return int(lib().pcgc_render_splat_rows())


def _render_int(name, v, lo, hi):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
        raise ValueError(f'render: {name} {v!r}: an integer in {lo} .. {hi}')
    return int(v)


def render(coords, colours, matrices, planes, B, H, W, r=0, background=(255, 255, 255), times=None):
    """The z-buffer splat of csrc/render.hip (every output equals tests/render_reference.py).  coords int32 [N,4] (batch, x, y,
    z) device tensor, batch below B, coordinates in [0, 2^21), rows in any order; colours uint8 [N,3] on the same device or None (the depth
    shade); matrices int64 [V,3,4] in Q16 and planes int32 [V,2] (near, far of the depth shade), host arrays that pcgcv2_amd.render has built
    and range-checked; B V <= 64; H, W in 1 .. 4096; r in 0 .. 4.  (u, v, d) = (M[:, :3] . p + M[:, 3]) >> 16; a row covers [u - r, u + r] x
    [v - r, v + r]; a pixel keeps the smallest d, among equal d the smallest row.  -> Rendered(image uint8 [B,V,H,W,3], depth int32
    [B,V,H,W], index int32 (the winning row or -1), mask bool, matrices int64 [V,3,4] on the device).  ValueError naming the count for rows
    out of range.  times (measurement hook): a dict -> seconds of 'render' and 'copies' added to it."""
    if not torch.is_tensor(coords) or not coords.is_cuda:
        raise PcgcError('render: coords must be a ROCm device tensor (no CPU fallback exists)')
    if coords.dtype != torch.int32 or coords.dim() != 2 or coords.shape[1] != 4:
        raise ValueError(f'render: coords must be int32 [N,4], got {coords.dtype} {tuple(coords.shape)}')
    n, dev = coords.shape[0], coords.device
    if n >= 1 << 31:
        raise ValueError(f'render: {n} rows; fewer than 2^31')
    matrices = np.ascontiguousarray(matrices, dtype=np.int64)
    if matrices.ndim != 3 or matrices.shape[1:] != (3, 4) or matrices.shape[0] < 1:
        raise ValueError(f'render: matrices must be int64 [V,3,4], got {matrices.shape}')
    V = matrices.shape[0]
    planes = np.ascontiguousarray(planes, dtype=np.int32)
    if planes.shape != (V, 2):
        raise ValueError(f'render: planes must be int32 [{V},2], got {planes.shape}')
    B = _render_int('B', B, 1, RENDER_MAX_SLICES)
    if B * V > RENDER_MAX_SLICES:
        raise ValueError(f'render: {B} items x {V} views = {B * V}; at most {RENDER_MAX_SLICES}')
    H, W, r = _render_int('H', H, 1, RENDER_MAX_SIDE), _render_int('W', W, 1, RENDER_MAX_SIDE), _render_int('r', r, 0, RENDER_MAX_R)
    bg = tuple(background) if isinstance(background, (tuple, list)) else ()
    if len(bg) != 3:
        raise ValueError(f'render: background {background!r}: three integers in 0 .. 255')
    bg = [_render_int('background', v, 0, 255) for v in bg]
    if colours is not None:
        if not torch.is_tensor(colours) or colours.device != dev or colours.dtype != torch.uint8 or tuple(colours.shape) != (n, 3):
            raise ValueError(f'render: colours must be uint8 [{n},3] on the device of the coordinates')
        colours = colours.contiguous()
    coords = coords.contiguous()
    L, s = lib(), _stream(coords)
    with torch.cuda.device(dev):
        t0 = tick_phase(times, None, 0.0, dev)
        m_dev = torch.from_numpy(matrices).to(dev)
        p_dev = torch.from_numpy(planes).to(dev)
        t0 = tick_phase(times, 'copies', t0, dev)
        image = torch.empty((B, V, H, W, 3), dtype=torch.uint8, device=dev)
        depth = torch.empty((B, V, H, W), dtype=torch.int32, device=dev)
        index = torch.empty((B, V, H, W), dtype=torch.int32, device=dev)
        mask = torch.empty((B, V, H, W), dtype=torch.uint8, device=dev)
        bad = torch.empty(1, dtype=torch.int32, device=dev)
        ws_bytes = int(L.pcgc_render_workspace_bytes(B, V, H, W))
        ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=dev)
        check(L.pcgc_render(_p(coords) if n else None, _p(colours) if n else None, n, B, V, H, W, r, _p(m_dev), _p(p_dev),
                            bg[0] | bg[1] << 8 | bg[2] << 16, _p(index), _p(depth), _p(mask), _p(image), _p(bad), None, 7, _p(ws), ws_bytes, s),
              'render')
        t0 = tick_phase(times, 'render', t0, dev)
        bad = int(bad.item())
        tick_phase(times, 'copies', t0, dev)
    if bad:
        raise ValueError(f'render: {bad} of {n} rows are outside the cube [0, 2^{RENDER_COORD_BITS}) or the {B} batch items')
    return Rendered(image, depth, index, mask.view(torch.bool), m_dev)


def render_metric(a, b):
    """two Rendered of the same shape -> int64 [B,V,8] device tensor of the sums RENDER_METRIC_SUMS (include/pcgc_hip.h pcgc_render_metric)"""
    for t, u, dt in ((a.image, b.image, torch.uint8), (a.depth, b.depth, torch.int32), (a.mask, b.mask, torch.bool)):
        if not (torch.is_tensor(t) and t.is_cuda and torch.is_tensor(u) and u.device == t.device):
            raise PcgcError('render_metric: both renderings must be on one ROCm device (no CPU fallback exists)')
        if t.dtype != dt or u.dtype != dt or t.shape != u.shape or not t.is_contiguous() or not u.is_contiguous():
            raise ValueError(f'render_metric: the renderings differ in shape or type ({tuple(t.shape)} {t.dtype}, {tuple(u.shape)} {u.dtype})')
    Bn, V, H, W = a.depth.shape
    if a.image.shape != (Bn, V, H, W, 3) or a.mask.shape != a.depth.shape or not 1 <= Bn * V <= RENDER_MAX_SLICES:
        raise ValueError(f'render_metric: not a rendering: image {tuple(a.image.shape)}, depth {tuple(a.depth.shape)}, mask {tuple(a.mask.shape)}')
    with torch.cuda.device(a.depth.device):
        sums = torch.empty((Bn, V, len(RENDER_METRIC_SUMS)), dtype=torch.int64, device=a.depth.device)
        check(lib().pcgc_render_metric(_p(a.mask), _p(b.mask), _p(a.image), _p(b.image), _p(a.depth), _p(b.depth), Bn * V, H * W, _p(sums),
                                       _stream(a.depth)), 'render_metric')
    return sums


# ------------------------------------------------------------------------------------------------ host codecs (numpy)
def _np(a, dt):
    return np.ascontiguousarray(a, dtype=dt)


def set_rc_impl(impl):
    """0 automatic, 1 portable scalar range decoder (bit-identical; for A/B tests)."""
    check(lib().pcgc_set_rc_impl(int(impl)), 'set_rc_impl')


RC_CKPT_WORDS = CONSTANTS['PCGC_RC_CKPT_WORDS']


def set_rc_threads(threads):
    """Threads of the indexed range decoder (0 = min(8, hardware threads))."""
    check(lib().pcgc_set_rc_threads(int(threads)), 'set_rc_threads')


def set_rc_lanes(mode):
    """Lane-parallel indexed range decoder (eight segments per 512-bit register on the calling thread): -1 automatic (thread budget of one
    or two), 0 never, 1 always.  Same symbols either way."""
    check(lib().pcgc_set_rc_lanes(int(mode)), 'set_rc_lanes')


def crc32(data, crc=0):
    """zlib.crc32(data, crc), by the library's carry-less-multiply fold (the value the native item files carry in their sidecars)"""
    src = np.frombuffer(data, np.uint8)
    return int(lib().pcgc_crc32(int(crc) & 0xFFFFFFFF, src.ctypes.data if src.size else None, src.size))


def rc_encode(cdf_u16, sym, checkpoints=0):
    """-> stream bytes, or (stream bytes, index uint32 [checkpoints, RC_CKPT_WORDS]) when checkpoints > 0: the decoder state at
    evenly spread row boundaries, for rc_decode(index=...).  The stream is the same either way."""
    cdf = _np(cdf_u16, np.uint16)
    sym = _np(sym, np.int16).ravel()
    C, Lp = cdf.shape
    cap = sym.size * 2 + 64
    index = np.zeros((int(checkpoints), RC_CKPT_WORDS), np.uint32) if checkpoints > 0 else None
    while True:
        buf = np.empty(cap, np.uint8)
        if index is None:
            n = int(lib().pcgc_rc_encode(cdf.ctypes.data, C, Lp, sym.ctypes.data, sym.size, buf.ctypes.data, cap))
        else:
            n = int(lib().pcgc_rc_encode_indexed(cdf.ctypes.data, C, Lp, sym.ctypes.data, sym.size, buf.ctypes.data, cap,
                                                 index.shape[0], index.ctypes.data))
        if n >= 0:
            return buf[:n].tobytes() if index is None else (buf[:n].tobytes(), index)
        if n == -(2 ** 63):
            raise PcgcError('rc_encode: symbol outside the CDF table')
        cap = -n


def rc_decode(cdf_u16, data, n, index=None):
    """`index` (optional): the checkpoints rc_encode(..., checkpoints=k) returned for this stream -> segments decoded in parallel."""
    cdf = _np(cdf_u16, np.uint16)
    C, Lp = cdf.shape
    src = np.frombuffer(data, np.uint8)
    out = np.empty(n, np.int16)
    if index is None:
        check(lib().pcgc_rc_decode(cdf.ctypes.data, C, Lp, src.ctypes.data, src.size, out.ctypes.data, n), 'rc_decode')
    else:
        idx = np.ascontiguousarray(index, dtype=np.uint32).reshape(-1, RC_CKPT_WORDS)
        check(lib().pcgc_rc_decode_indexed(cdf.ctypes.data, C, Lp, src.ctypes.data, src.size, out.ctypes.data, n, idx.shape[0],
                                           idx.ctypes.data), 'rc_decode_indexed')
    return out


def rc_encode_ctx(cdf_u16, ctx, sym):
    """range-coded bytes of sym [n] with symbol i coded under row ctx[i] of cdf_u16 [R, Lp] (rc_encode's coder, the row chosen per symbol)"""
    cdf = _np(cdf_u16, np.uint16)
    ctx, sym = _np(ctx, np.uint16).ravel(), _np(sym, np.int16).ravel()
    if ctx.size != sym.size:
        raise PcgcError(f'rc_encode_ctx: {sym.size} symbols but {ctx.size} contexts')
    R, Lp = cdf.shape
    cap = sym.size // 4 + 64
    while True:
        buf = np.empty(cap, np.uint8)
        n = int(lib().pcgc_rc_encode_ctx(cdf.ctypes.data, R, Lp, ctx.ctypes.data, sym.ctypes.data, sym.size, buf.ctypes.data, cap))
        if n >= 0:
            return buf[:n].tobytes()
        if n == -(2 ** 63):
            raise PcgcError('rc_encode_ctx: symbol or context outside the CDF table')
        cap = -n


def rc_decode_ctx(cdf_u16, ctx, data):
    """-> int16 [n], n = len(ctx).  Raises PcgcError unless `data` is exactly the stream rc_encode_ctx writes for the symbols it decodes
    to: a cut, extended or damaged stream is refused, never returned as symbols."""
    cdf = _np(cdf_u16, np.uint16)
    ctx = _np(ctx, np.uint16).ravel()
    R, Lp = cdf.shape
    src = np.frombuffer(data, np.uint8)
    out = np.empty(ctx.size, np.int16)
    check(lib().pcgc_rc_decode_ctx(cdf.ctypes.data, R, Lp, ctx.ctypes.data, src.ctypes.data if src.size else None, src.size,
                                   out.ctypes.data, ctx.size), 'rc_decode_ctx')
    return out


def _stems(stems):
    """file stems as a C array of byte strings (+ the Python objects that own the bytes)"""
    enc = [_os.fsencode(s) for s in stems]
    return (ctypes.c_char_p * len(enc))(*enc), enc


def _table_fn():
    """address of pcgc_reference_table (libpcgc_reftable.so): the CDF table in the reference's arithmetic, callable from native threads"""
    from ._lib import reftable_lib
    return ctypes.cast(reftable_lib().pcgc_reference_table, ctypes.c_void_p)


_WARM_SCRATCH = np.zeros((64, 16), np.uint16)


def table_warm(eb_params, C):
    """Run the reference-arithmetic CDF-table evaluation (libpcgc_reftable.so) once on a small dummy range and throw the result away.
    The real evaluation sits on the critical path of every encode, right after the sync that hands over the symbol range, and its ~60
    ATen operators run 2-2.5x slower from cold instruction / data caches (0.36 ms against 0.15 ms hot on the bench host) than from warm
    ones.  Called while the host would otherwise wait for the GPU, it changes no result and memoises nothing — the table the encoder
    codes with is still evaluated for its own range, after the range is known."""
    from ._lib import reftable_lib
    P = _np(eb_params, np.float32)
    if P.size != 44 * C or C > _WARM_SCRATCH.shape[0]:
        return
    reftable_lib().pcgc_reference_table(P.ctypes.data, int(C), -7.0, 7.0, _WARM_SCRATCH.ctypes.data, None)


def items_encode(stems, sym_h, xyz8, rows, ranges, counts, eb_params, index_segments, write_coords=True, threads=0):
    """Write the bitstream files of every item (native threads): sym_h int16 [sum rows, C], xyz8 int32 [sum rows, 3] (stride-8
    coordinates / 8), rows / ranges [(min_v, max_v)] / counts [(N4, N2, N1)] per item, eb_params = the 44*C packed entropy parameters."""
    sym = _np(sym_h, np.int16)
    C = sym.shape[1]
    xyz = _np(xyz8, np.int32)
    arr, keep = _stems(stems)
    r = np.asarray(rows, np.int64)
    rg = _np(ranges, np.float32).reshape(-1, 2)
    ct = _np(counts, np.int32).reshape(-1, 3)
    P = _np(eb_params, np.float32)
    if P.size != 44 * C:
        raise PcgcError(f'items_encode: {P.size} entropy parameters for {C} channels (44 per channel)')
    check(lib().pcgc_items_encode(len(stems), arr, sym.ctypes.data, xyz.ctypes.data, r.ctypes.data, rg.ctypes.data, C, ct.ctypes.data, P.ctypes.data,
                                  _table_fn(), int(index_segments), int(write_coords), int(threads)), 'items_encode')


def items_probe(stems):
    """-> (rows int64 [n], C, ranges float32 [n, 2], counts int32 [n, 3], native_coords int32 [n]) from the files of every item."""
    n = len(stems)
    arr, keep = _stems(stems)
    rows, ranges, counts, native = np.zeros(n, np.int64), np.zeros((n, 2), np.float32), np.zeros((n, 3), np.int32), np.zeros(n, np.int32)
    C = ctypes.c_int32(0)
    check(lib().pcgc_items_probe(n, arr, rows.ctypes.data, ctypes.addressof(C), ranges.ctypes.data, counts.ctypes.data, native.ctypes.data), 'items_probe')
    return rows, int(C.value), ranges, counts, native


def items_decode(stems, rows, C, ranges, native, eb_params, use_sidecar=True, threads=0, level_scale=0, level_out=None):
    """-> (sym int16 [sum rows, C], coordinates) decoded from the files of every item (native threads).  Coordinates: xyz8 int32
    [sum rows, 3] in stream order, or with level_scale = s > 0 the sorted coordinate level int32 [sum rows, 4] = (item, s x, s y, s z),
    every item in (z, y, x) order — written into `level_out` (e.g. a pinned buffer's numpy view, at least [sum rows, 4]) if given."""
    arr, keep = _stems(stems)
    total = int(np.sum(rows))
    sym = np.empty((total, C), np.int16)
    if level_scale:
        if level_out is None:
            level_out = np.empty((total, 4), np.int32)
        if level_out.dtype != np.int32 or level_out.ndim != 2 or level_out.shape[1] != 4 or level_out.shape[0] < total or not level_out.flags.c_contiguous:
            raise PcgcError('items_decode: level_out must be a C-contiguous int32 [>= rows, 4] array')
        xyz = level_out
    else:
        xyz = np.empty((total, 3), np.int32)
    P = _np(eb_params, np.float32)
    if P.size != 44 * C:
        # (the library reads 44 * C floats: a channel count taken from a damaged `_H.bin` must never reach it)
        raise PcgcError(f'items_decode: {P.size} entropy parameters for {C} channels (44 per channel)')
    rc = lib().pcgc_items_decode(len(stems), arr, rows.ctypes.data, C, ranges.ctypes.data, native.ctypes.data, P.ctypes.data, _table_fn(), int(use_sidecar),
                                 sym.ctypes.data, xyz.ctypes.data, 1 if level_scale else 0, int(level_scale) if level_scale else 1, int(threads))
    check(rc, 'items_decode')
    return sym, xyz[:total]


def frame_decode(stem, C, eb_params, sym_buf, level_buf, use_sidecar=True, level_scale=8, threads=2):
    """One cloud's files -> symbols and sorted coordinate level, in ONE library call, into the caller's (pinned) numpy buffers sym_buf
    int16 [cap, C] and level_buf int32 [cap, 4].  -> (rows, (min_v, max_v), (N4, N2, N1), native_coords), or (rows_needed, None, None,
    None) when the buffers are too small (nothing decoded: grow them and call again)."""
    cap = min(sym_buf.shape[0], level_buf.shape[0])
    if sym_buf.dtype != np.int16 or level_buf.dtype != np.int32 or sym_buf.shape[1:] != (C,) or level_buf.shape[1:] != (4,) \
            or not sym_buf.flags.c_contiguous or not level_buf.flags.c_contiguous:
        raise PcgcError('frame_decode: buffers must be C-contiguous int16 [cap, C] and int32 [cap, 4]')
    info = (ctypes.c_int64 * 6)()
    rng = (ctypes.c_float * 2)()
    P = _np(eb_params, np.float32)
    if P.size != 44 * int(C):
        raise PcgcError(f'frame_decode: {P.size} entropy parameters for {C} channels (44 per channel)')
    rc = lib().pcgc_frame_decode(_os.fsencode(stem), int(C), P.ctypes.data, _table_fn(), int(bool(use_sidecar)), int(level_scale), cap,
                                 sym_buf.ctypes.data, level_buf.ctypes.data, info, rng, int(threads))
    if rc == 1:
        return int(info[0]), None, None, None
    check(rc, 'frame_decode')
    return int(info[0]), (np.float32(rng[0]), np.float32(rng[1])), (int(info[2]), int(info[3]), int(info[4])), bool(info[5])


def frame_decode_begin(stem, C, eb_params, sym_buf, level_buf, use_sidecar=True, level_scale=8, threads=2):
    """frame_decode in two halves: returns as soon as the coordinate level is in level_buf (the feature stream keeps decoding on the
    library's threads) -> the same tuple as frame_decode; the symbols in sym_buf are valid only after frame_decode_end().  When the
    buffers are too small (rows_needed, None, None, None) nothing is pending."""
    cap = min(sym_buf.shape[0], level_buf.shape[0])
    if sym_buf.dtype != np.int16 or level_buf.dtype != np.int32 or sym_buf.shape[1:] != (C,) or level_buf.shape[1:] != (4,) \
            or not sym_buf.flags.c_contiguous or not level_buf.flags.c_contiguous:
        raise PcgcError('frame_decode: buffers must be C-contiguous int16 [cap, C] and int32 [cap, 4]')
    info = (ctypes.c_int64 * 6)()
    rng = (ctypes.c_float * 2)()
    P = _np(eb_params, np.float32)
    if P.size != 44 * int(C):
        raise PcgcError(f'frame_decode: {P.size} entropy parameters for {C} channels (44 per channel)')
    rc = lib().pcgc_frame_decode_begin(_os.fsencode(stem), int(C), P.ctypes.data, _table_fn(), int(bool(use_sidecar)), int(level_scale), cap,
                                       sym_buf.ctypes.data, level_buf.ctypes.data, info, rng, int(threads))
    if rc == 1:
        return int(info[0]), None, None, None
    check(rc, 'frame_decode')
    return int(info[0]), (np.float32(rng[0]), np.float32(rng[1])), (int(info[2]), int(info[3]), int(info[4])), bool(info[5])


def frame_decode_end():
    """wait for the feature stream of the frame frame_decode_begin started on this thread (raises what frame_decode would have raised)"""
    check(lib().pcgc_frame_decode_end(), 'frame_decode')


def set_oct_tiled(on):
    """Coordinate codec: groups of subtrees coded independently (1, the default for clouds of >= 8192 points; n > 1: that many
    groups) or always one stream (0).  A/B tests."""
    check(lib().pcgc_set_oct_tiled(int(on)), 'set_oct_tiled')


def set_oct_model(model):
    """context model of the octree ENCODER: 1 = stream versions 4 / 5 (mixed-shape prior, fast start; default), 0 = versions 2 / 3"""
    check(lib().pcgc_set_oct_model(int(model)), 'set_oct_model')


def oct_encode(xyz):
    xyz = _np(xyz, np.int32)
    if xyz.ndim != 2 or xyz.shape[1] != 3:
        raise PcgcError('oct_encode: expected [n,3] coordinates')
    cap = 64 + 4 * len(xyz)
    while True:
        buf = np.empty(cap, np.uint8)
        n = int(lib().pcgc_oct_encode(xyz.ctypes.data, len(xyz), buf.ctypes.data, cap))
        if n >= 0:
            return buf[:n].tobytes()
        if n == -(2 ** 63):
            raise PcgcError('oct_encode: coordinates must be in [0, 2^21)')
        cap = -n


def oct_decode(data):
    src = np.frombuffer(data, np.uint8)
    n = int(lib().pcgc_oct_decode_count(src.ctypes.data, src.size))
    if n < 0:
        raise PcgcError('oct_decode: not a PCGO stream')
    out = np.empty((n, 3), np.int32)
    check(lib().pcgc_oct_decode(src.ctypes.data, src.size, out.ctypes.data, n), 'oct_decode')
    return out
