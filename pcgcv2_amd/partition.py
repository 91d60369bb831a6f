"""Coding a large cloud in kd-tree blocks (csrc/partition.hip; the definition is tests/partition_reference.py): the cloud is cut
on the GPU into blocks of at most max_num voxels, no stride-`align` cell shared by two blocks, and the blocks are coded as the items of
collated batches (Coder.encode_batch / LosslessCoder.encode_batch, unchanged).  `_P.bin` records which block covers what, so a decoder can
put the cloud together again or decode only the blocks that meet a region.  The reference codes a cloud whole; later versions of the upstream
project split large clouds with a kd-tree under a `max_num` option.

`<prefix><postfix>_P.bin`, little endian:
    "PCGP" | u32 version = 1 | u32 align | u64 max_num | u32 mode (0 lossy, 1 lossless) | u32 blocks
    | blocks x (u32 rows, 3 x u32 lo, 3 x u32 hi)          the inclusive box of the block's voxels
    | u32 CRC-32 of everything before
Block i's files carry the postfix `<postfix>_b{i:04d}`.

    python -m pcgcv2_amd.partition --filedir cloud.ply --max_num M [--align 8]
    python -m pcgcv2_amd.partition --filedir cloud.ply --max_num M --ckptdir model.pth [--lossless] [--roi x0,y0,z0,x1,y1,z1] [--outdir out]
"""
import os
import struct
import zlib
from collections import namedtuple

import numpy as np
import torch

from . import ops
from .ops import Partition, PcgcError                              # noqa: F401  (the record partition returns)

SUFFIX = '_P.bin'
MAGIC = b'PCGP'
VERSION = 1
MAX_BLOCKS = ops.PARTITION_MAX_BLOCKS
COORD_LIMIT = 1 << 20
MODES = {'lossy': 0, 'lossless': 1}
_HEAD = struct.Struct('<4sIIQII')                                  # magic, version, align, max_num, mode, blocks
_BLOCK = struct.Struct('<7I')                                      # rows, lo x y z, hi x y z
_CRC = struct.Struct('<I')
Blocks = namedtuple('Blocks', 'align max_num mode rows lo hi')     # rows int64 [B], lo / hi int64 [B,3]


def partition(coords, max_num, align=8, times=None):
    """ops.partition: device tensor int32 [N,3] or [N,4] (batch 0) -> Partition(block_of, perm int32 [N], table int32 [B,8] = (first_row, rows,
    lo_x, lo_y, lo_z, hi_x, hi_y, hi_z), rounds, oversize)"""
    return ops.partition(coords, max_num, align=align, times=times)


def block_postfix(postfix, i):
    return f'{postfix}_b{i:04d}'


# ------------------------------------------------------------------------------------------------ _P.bin
def pack_blocks(table, align, max_num, mode):
    """table: integers [B,8] (a Partition's, on the host) or [B,7] = (rows, lo, hi) -> the bytes of `_P.bin`"""
    t = np.asarray(table, dtype=np.int64)
    t = t.reshape(len(t), -1) if len(t) else np.zeros((0, 7), np.int64)
    t = t[:, 1:] if t.shape[1] == 8 else t
    if t.shape[1] != 7 or len(t) > MAX_BLOCKS or (len(t) and (t.min() < 0 or t[:, 1:].max() >= COORD_LIMIT or t[:, 0].max() >= 1 << 32)):
        raise ValueError(f'pack_blocks: {len(t)} blocks of {t.shape[1]} columns: at most {MAX_BLOCKS} of (rows, lo, hi) inside 0 .. 2^20 - 1')
    if mode not in (0, 1) or align not in ops.PARTITION_ALIGNS or not 1 <= max_num < 1 << 64:
        raise ValueError(f'pack_blocks: mode {mode}, align {align}, max_num {max_num}')
    body = _HEAD.pack(MAGIC, VERSION, int(align), int(max_num), int(mode), len(t)) + b''.join(_BLOCK.pack(*(int(v) for v in row)) for row in t)
    return body + _CRC.pack(zlib.crc32(body))


def unpack_blocks(blob, name='_P.bin'):
    """the bytes of `_P.bin` -> Blocks; PcgcError naming what is wrong: length, magic, version, CRC, a field out of range"""
    if len(blob) < _HEAD.size + _CRC.size:
        raise PcgcError(f'{name}: {len(blob)} bytes, shorter than its header')
    magic, version, align, max_num, mode, blocks = _HEAD.unpack(blob[:_HEAD.size])
    if magic != MAGIC:
        raise PcgcError(f'{name}: magic {magic!r}, not {MAGIC!r}')
    if version != VERSION:
        raise PcgcError(f'{name}: version {version}; this reader knows version {VERSION}')
    if blocks > MAX_BLOCKS:
        raise PcgcError(f'{name}: {blocks} blocks; at most {MAX_BLOCKS}')
    want = _HEAD.size + blocks * _BLOCK.size + _CRC.size
    if len(blob) != want:
        raise PcgcError(f'{name}: {len(blob)} bytes; {blocks} blocks take {want}')
    if _CRC.unpack(blob[-_CRC.size:])[0] != zlib.crc32(blob[:-_CRC.size]):
        raise PcgcError(f'{name}: CRC-32 mismatch')
    if align not in ops.PARTITION_ALIGNS or max_num < 1 or mode not in (0, 1):
        raise PcgcError(f'{name}: align {align}, max_num {max_num}, mode {mode}: align is a power of two in 8 .. 1024, max_num at least 1, mode 0 or 1')
    t = np.frombuffer(blob, dtype='<u4', count=blocks * 7, offset=_HEAD.size).reshape(blocks, 7).astype(np.int64)
    rows, lo, hi = t[:, 0], t[:, 1:4], t[:, 4:7]
    if blocks:
        if max(lo.max(), hi.max()) >= COORD_LIMIT:
            raise PcgcError(f'{name}: {int(((lo >= COORD_LIMIT) | (hi >= COORD_LIMIT)).any(1).sum())} blocks have a coordinate of 2^20 or more')
        if (lo > hi).any():
            raise PcgcError(f'{name}: {int((lo > hi).any(1).sum())} blocks have lo above hi')
        if (rows < 1).any() or (rows > (hi - lo + 1).prod(1)).any():
            raise PcgcError(f'{name}: {int(((rows < 1) | (rows > (hi - lo + 1).prod(1))).sum())} blocks name no row or more rows than their box has voxels')
    return Blocks(align, max_num, mode, rows, lo, hi)


def read_blocks(prefix, postfix=''):
    path = prefix + postfix + SUFFIX
    with open(path, 'rb') as fh:
        return unpack_blocks(fh.read(), path)


def blocks_meeting(blocks, roi):
    """the indices of the blocks whose voxel box meets the region roi = (x0, y0, z0, x1, y1, z1), inclusive"""
    r = check_roi(roi)
    meets = (blocks.lo <= np.array(r[3:])).all(1) & (blocks.hi >= np.array(r[:3])).all(1)
    return [int(i) for i in np.flatnonzero(meets)]


def check_roi(roi):
    try:
        r = tuple(int(v) for v in roi)
        if len(r) != 6 or any(int(v) != v for v in roi):
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError(f'roi {roi!r}: six integers x0, y0, z0, x1, y1, z1') from None
    if any(a > b for a, b in zip(r[:3], r[3:])):
        raise ValueError(f'roi {r}: (x0, y0, z0) must not be above (x1, y1, z1)')
    return r


def block_bits(prefix, postfix=''):
    """bits of a cloud coded in blocks: the blocks' stream_bits summed (with `_O.bin` in lossless mode), plus `_P.bin`"""
    return int(block_stream_bits(prefix, postfix).sum())


def block_stream_bits(prefix, postfix=''):
    """-> int64 [5] or [6]: bits of `_C.bin`, `_F.bin`, `_H.bin`, `_num_points.bin` summed over the blocks, (`_O.bin` likewise,) `_P.bin`"""
    from .coder import stream_bits
    from .lossless import occupancy_bits
    blocks = read_blocks(prefix, postfix)
    per = np.zeros(4, np.int64)
    occ = 0
    for i in range(len(blocks.rows)):
        per += stream_bits(prefix, block_postfix(postfix, i))
        if blocks.mode == MODES['lossless']:
            occ += occupancy_bits(prefix, block_postfix(postfix, i))
    own = os.path.getsize(prefix + postfix + SUFFIX) * 8
    return np.array(list(per) + ([occ] if blocks.mode == MODES['lossless'] else []) + [own], np.int64)


# ------------------------------------------------------------------------------------------------ the coder
class BlockCoder():
    """A cloud coded in kd-tree blocks of at most max_num voxels.  The blocks go through Coder.encode_batch / decode_batch (lossless=True:
    LosslessCoder's) in runs of at most batch_items, each block's files being what coding it alone writes.

    Budgets: a block's last top-k budget is int(rho * rows_i), as decode_batch does it for any item; their sum may differ from int(rho * N)
    of the whole cloud by up to one voxel a block."""

    def __init__(self, model, filename, max_num, batch_items=16, lossless=False, occupancy_coder='host', align=8):
        from .coder import Coder, MAX_BATCH_ITEMS
        if isinstance(max_num, bool) or not isinstance(max_num, (int, np.integer)) or max_num < 1:
            raise ValueError(f'BlockCoder: max_num {max_num!r}: an integer of at least 1')
        if isinstance(batch_items, bool) or not isinstance(batch_items, (int, np.integer)) or not 1 <= batch_items <= MAX_BATCH_ITEMS:
            raise ValueError(f'BlockCoder: batch_items {batch_items!r}: 1 .. {MAX_BATCH_ITEMS}')
        if align not in ops.PARTITION_ALIGNS:
            raise ValueError(f'BlockCoder: align {align!r}: a power of two in 8 .. 1024')
        self.model, self.filename = model, filename
        self.max_num, self.batch_items, self.align, self.lossless = int(max_num), int(batch_items), int(align), bool(lossless)
        if self.lossless:
            from .lossless import LosslessCoder
            self.coder = LosslessCoder(model, filename, occupancy_coder=occupancy_coder)
        else:
            self.coder = Coder(model, filename)

    @property
    def mode(self):
        return MODES['lossless' if self.lossless else 'lossy']

    @torch.no_grad()
    def encode(self, x, postfix='', times=None):
        """x: a stride-1 sparse tensor of one cloud (batch 0).  Partitions it on the device, codes the blocks in runs of at most batch_items
        and writes `_P.bin` -> the Partition.  The files of block i carry block_postfix(postfix, i)."""
        from .sparse import SparseTensor
        if not isinstance(x, SparseTensor):
            raise TypeError('BlockCoder codes a SparseTensor')
        if len(x) == 0:
            raise ValueError('BlockCoder: an empty cloud')
        coords = x.C
        part = ops.partition(coords, self.max_num, align=self.align, times=times)
        table = part.table.cpu().numpy()
        for first in range(0, len(table), self.batch_items):
            n_items = min(self.batch_items, len(table) - first)
            c = ops.partition_gather(coords, part, first, n_items, table)
            # (x is a sparse tensor: its rows are distinct voxels already, and so are any selection of them)
            xb = SparseTensor(torch.ones((c.shape[0], 1), dtype=torch.float32, device=c.device), coordinates=c, tensor_stride=1, assume_unique=True)
            self.coder.encode_batch(xb, [block_postfix(postfix, i) for i in range(first, first + n_items)])
        with open(self.filename + postfix + SUFFIX, 'wb') as fh:
            fh.write(pack_blocks(table, self.align, self.max_num, self.mode))
        return part

    @torch.no_grad()
    def decode(self, rho=1, postfix='', roi=None):
        """reads `_P.bin` and decodes the blocks in runs of at most batch_items -> one stride-1 sparse tensor: the blocks' decoded rows in block
        order, batch column 0.  roi = (x0, y0, z0, x1, y1, z1), inclusive: only the blocks whose voxel box meets the region are decoded,
        whole, not clipped; no file of any other block is opened.  A region that meets no block gives an empty tensor."""
        from .coder import _coords_only
        from .sparse import require_gpu
        blocks = read_blocks(self.filename, postfix)
        if blocks.mode != self.mode:
            raise PcgcError(f'{self.filename + postfix + SUFFIX}: mode {blocks.mode}, this coder is in mode {self.mode} (0 lossy, 1 lossless)')
        if self.lossless and rho != 1:
            raise ValueError('BlockCoder: the lossless mode decodes every voxel; rho must be 1')
        dev = require_gpu(next(self.model.decoder.parameters()).device)
        chosen = list(range(len(blocks.rows))) if roi is None else blocks_meeting(blocks, roi)
        outs = []
        for first in range(0, len(chosen), self.batch_items):
            posts = [block_postfix(postfix, i) for i in chosen[first:first + self.batch_items]]
            outs += self.coder.decode_batch(posts) if self.lossless else self.coder.decode_batch(posts, rho=rho)
        with torch.cuda.device(dev):
            merged = torch.cat([o.C for o in outs], 0) if outs else torch.empty((0, 4), dtype=torch.int32, device=dev)
        return _coords_only(merged.contiguous(), 1)

    def block_bits(self, postfix=''):
        return block_bits(self.filename, postfix)


# ------------------------------------------------------------------------------------------------ CLI
def describe(part, table=None):
    """the line of counts the tools print: rows, blocks, rounds, oversize, largest and smallest block"""
    t = part.table.cpu().numpy() if table is None else table
    rows = t[:, 1] if len(t) else np.zeros(1, np.int64)
    return (f'Blocks:\t {int(t[:, 1].sum()) if len(t) else 0} rows, {len(t)} blocks, {part.rounds} rounds, {part.oversize} oversize, '
            f'largest {int(rows.max())}, smallest {int(rows.min())}')


def parse_roi(text):
    import argparse
    try:
        return check_roi([int(t) for t in text.split(',')])
    except ValueError:
        raise argparse.ArgumentTypeError(f'--roi is x0,y0,z0,x1,y1,z1 (integers, inclusive, the first corner not above the second), got {text!r}') from None


def add_arguments(p):
    """--max_num M [--block_batch B] [--roi x0,y0,z0,x1,y1,z1] of coder.py"""
    p.add_argument("--max_num", type=int, default=None,
                   help="code the cloud in kd-tree blocks of at most M voxels (partition.py): _P.bin and the files of every block, postfix "
                        "_b0000 ..., are written and the decoded cloud is the blocks' merged")
    p.add_argument("--block_batch", type=int, default=None, help="with --max_num: blocks coded in one network pass, 1 .. 16 (default: 16)")
    p.add_argument("--roi", metavar='x0,y0,z0,x1,y1,z1', type=parse_roi, default=None,
                   help="with --max_num: decode only the blocks whose voxel box meets the region (inclusive corners)")


def check_arguments(p, args):
    given, args.block_batch = args.block_batch is not None, 16 if args.block_batch is None else args.block_batch
    if args.max_num is None:
        if args.roi is not None or given:
            p.error('--block_batch and --roi need --max_num')
        return
    if args.max_num < 1:
        p.error(f'--max_num {args.max_num}: at least 1')
    if not 1 <= args.block_batch <= 16:
        p.error(f'--block_batch {args.block_batch}: 1 .. 16')
    if getattr(args, 'lossless', False):
        p.error('--max_num with --lossless: use `python -m pcgcv2_amd.partition --lossless`, which codes the blocks losslessly and checks the round trip')


def parser():
    import argparse
    p = argparse.ArgumentParser(description='cut a voxelised PLY into kd-tree blocks on the GPU; with --ckptdir, code it in those blocks',
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('--filedir', required=True, help='input PLY: integer coordinates (a voxelised cloud)')
    p.add_argument('--max_num', type=int, required=True, help='most voxels of a block')
    p.add_argument('--align', type=int, default=8, help='no cell of this size is shared by two blocks: a power of two in 8 .. 1024')
    p.add_argument('--ckptdir', default=None, help='a checkpoint: code the blocks, decode them and check the round trip')
    p.add_argument('--lossless', action='store_true', help='with --ckptdir: the lossless mode (lossless.py); the decoded voxel set must be the input\'s')
    p.add_argument('--occupancy_coder', choices=('host', 'device'), default='host', help='with --lossless: who codes _O.bin')
    p.add_argument('--block_batch', type=int, default=16, help='with --ckptdir: blocks coded in one network pass, 1 .. 16')
    p.add_argument('--rho', type=float, default=1.0, help='with --ckptdir: output points over input points')
    p.add_argument('--roi', metavar='x0,y0,z0,x1,y1,z1', type=parse_roi, default=None, help='with --ckptdir: also decode only the blocks that meet the region')
    p.add_argument('--outdir', default='./output')
    return p


def parse_args(argv=None):
    p = parser()
    args = p.parse_args(argv)
    if args.max_num < 1:
        p.error(f'--max_num {args.max_num}: at least 1')
    if args.align not in ops.PARTITION_ALIGNS:
        p.error(f'--align {args.align}: a power of two in 8 .. 1024')
    if not 1 <= args.block_batch <= 16:
        p.error(f'--block_batch {args.block_batch}: 1 .. 16')
    if args.ckptdir is None and (args.lossless or args.roi is not None):
        p.error('--lossless and --roi need --ckptdir')
    if args.lossless and args.rho != 1:
        p.error('--lossless decodes every voxel: --rho must be 1')
    return args


def _repeated_rows(coords):
    """rows of a [n,4] coordinate tensor that repeat an earlier row"""
    if coords.shape[0] == 0:
        return 0
    keep = ops.first_occurrence_mask(coords, ops.HashTable(coords, 1))
    return coords.shape[0] - int(ops.mask_scan(keep)[1].item())


def main(argv=None):
    args = parse_args(argv)
    from .coder import device
    from .data_utils import load_sparse_tensor, write_ply_ascii_geo
    from .lossless import same_voxels
    from .sparse import require_gpu
    require_gpu(device)
    x = load_sparse_tensor(args.filedir, device)
    if args.ckptdir is None:
        part = ops.partition(x.C, args.max_num, align=args.align)
        table = part.table.cpu().numpy()
        print('block\t first_row\t rows\t lo\t hi')
        for i, row in enumerate(table):
            print(f'{i}\t {row[0]}\t {row[1]}\t {tuple(int(v) for v in row[2:5])}\t {tuple(int(v) for v in row[5:8])}')
        print(describe(part, table))
        return 0
    from .pcc_model import PCCModel
    if not os.path.exists(args.ckptdir):
        raise FileNotFoundError(args.ckptdir)
    model = PCCModel().to(device)
    model.load_state_dict(torch.load(args.ckptdir, map_location=device)['model'])
    os.makedirs(args.outdir, exist_ok=True)
    prefix = os.path.join(args.outdir, os.path.split(args.filedir)[-1].split('.')[0])
    coder = BlockCoder(model, prefix, args.max_num, batch_items=args.block_batch, lossless=args.lossless, occupancy_coder=args.occupancy_coder,
                       align=args.align)
    part = coder.encode(x)
    print(describe(part))
    out = coder.decode(rho=args.rho)
    bits = block_stream_bits(prefix)
    print('bits:\t', bits, '\nbpp:\t', round(float(bits.sum()) / len(x), 3))
    repeated = _repeated_rows(out.C)
    if repeated:
        raise PcgcError(f'round trip: {repeated} of {len(out)} decoded rows repeat a voxel of another block')
    if args.lossless and not same_voxels(out.C, x.C):
        raise PcgcError(f'round trip: the decoded voxel set ({len(out)} rows) is not the input\'s ({len(x)} rows)')
    print(f'round trip OK:\t {len(out)} rows decoded from {len(part.table)} blocks, no voxel twice' + (', the voxel set is the input\'s' if args.lossless else ''))
    if args.roi is not None:
        blocks = read_blocks(prefix)
        chosen = blocks_meeting(blocks, args.roi)
        region = coder.decode(rho=args.rho, roi=args.roi)
        whole_rows = _rows_of_blocks(coder, args.rho, chosen)
        if not torch.equal(region.C, whole_rows):
            raise PcgcError(f'--roi: the blocks {chosen} decoded for the region differ from the same blocks decoded one by one')
        print(f'roi {args.roi}:\t blocks {chosen}, {len(region)} rows')
        out = region
    write_ply_ascii_geo(prefix + '_dec.ply', out.C.cpu().numpy()[:, 1:])
    return 0


def _rows_of_blocks(coder, rho, chosen):
    """the decoded rows of the blocks `chosen`, each decoded as a batch of one"""
    dev = next(coder.model.decoder.parameters()).device
    outs = []
    for i in chosen:
        post = [block_postfix('', i)]
        outs += coder.coder.decode_batch(post) if coder.lossless else coder.coder.decode_batch(post, rho=rho)
    return torch.cat([o.C for o in outs], 0) if outs else torch.empty((0, 4), dtype=torch.int32, device=dev)


if __name__ == '__main__':
    raise SystemExit(main())
