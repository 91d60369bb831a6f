"""Voxelising a raw point cloud on the GPU (csrc/voxelize.hip; the definition is tests/voxelize_reference.py): points in
metres (or any unit), float32 or float64, several to a voxel -> the vox-B cloud every entry point of the codec takes: integer coordinates
in [0, 2^B), one row and one colour per voxel, in the codec's (z, y, x) order.  The reference has no such stage: it assumes clouds that
were voxelised elsewhere.  The practice is MPEG's (G-PCC's encoder follows it too): quantise to a bit depth, average the attributes of the
points that merge.

    q = rint((float64(p) - origin) * scale)          origin: the per-axis minimum; scale: (2^B - 1) / the largest extent (1 when it is 0)

`_V.bin`, the frame that takes the voxels back to the input's units (48 bytes, little endian):
    4s magic "PCGV" | u32 version = 1 | u32 bits | 3 x f64 origin | f64 scale | u32 CRC-32 of all that precedes (ops.crc32)

    python -m pcgcv2_amd.voxelize --filedir raw.ply --bits 10 [--merge mean|first] [--out vox.ply] [--origin x,y,z --scale s]
                                  [--clean K,M [--clean_r2 R] [--keep_largest n]]     (then cleaned into <out>_clean.ply, clean.py)
"""
import math
import os
import struct

import numpy as np
import torch

from . import ops
from ._lib import PcgcError
from .ops import Voxels                                         # noqa: F401  (the record voxelize returns)

SUFFIX = '_V.bin'
MAGIC, VERSION = b'PCGV', 1
MERGES = tuple(ops.VOXELIZE_MERGES)
_FRAME = struct.Struct('<4sII4d')
FRAME_BYTES = _FRAME.size + 4


def voxelize(points, colours=None, bits=10, origin=None, scale=None, merge='mean', times=None):
    """ops.voxelize: device tensors points float32 / float64 [N,3] and colours uint8 [N,3] or None -> Voxels(coords int32 [M,4], counts
    int32 [M], voxel_of int32 [N], colours uint8 [M,3] or None, origin, scale, bits)"""
    return ops.voxelize(points, colours, bits=bits, origin=origin, scale=scale, merge=merge, times=times)


def devoxelize(coords, origin, scale):
    """the inverse map, q / scale + origin in fp64: coords [M,4] rows (0, x, y, z) or [M,3] (tensor or array) -> float64 [M,3] of the same
    kind, in the units of the cloud that was voxelised"""
    o = [float(v) for v in origin]
    if torch.is_tensor(coords):
        q = coords[:, -3:].to(torch.float64)
        s = torch.tensor(float(scale), dtype=torch.float64, device=q.device)          # (a tensor: a true division, never q * (1 / scale))
        return q / s + torch.tensor(o, dtype=torch.float64, device=q.device)[None, :]
    q = np.asarray(coords)[:, -3:].astype(np.float64)
    return q / np.float64(scale) + np.asarray(o, np.float64)[None, :]


# ------------------------------------------------------------------------------------------------ `_V.bin`
def pack_frame(bits, origin, scale):
    bits, origin, scale = int(bits), [float(v) for v in origin], float(scale)
    _check_frame('frame', bits, origin, scale)
    blob = _FRAME.pack(MAGIC, VERSION, bits, origin[0], origin[1], origin[2], scale)
    return blob + struct.pack('<I', ops.crc32(blob))


def _check_frame(what, bits, origin, scale):
    if not 1 <= bits <= 20:
        raise PcgcError(f'{what}: bits {bits} outside 1 .. 20')
    if len(origin) != 3 or not all(math.isfinite(v) for v in origin):
        raise PcgcError(f'{what}: origin {list(origin)} is not three finite numbers')
    if not (math.isfinite(scale) and scale > 0):
        raise PcgcError(f'{what}: scale {scale} is not finite and positive')


def unpack_frame(blob, what='_V.bin'):
    """the bytes of a `_V.bin` -> (bits, origin (x, y, z), scale).  PcgcError on another length, a bad magic, version or CRC, bits outside
    1 .. 20, and an origin or scale that is not finite (the scale: and positive)."""
    if len(blob) != FRAME_BYTES:
        raise PcgcError(f'{what}: {len(blob)} bytes; a frame has {FRAME_BYTES}')
    magic, version, bits, ox, oy, oz, scale = _FRAME.unpack_from(blob, 0)
    if magic != MAGIC:
        raise PcgcError(f'{what}: not a voxel frame (magic {magic!r})')
    if version != VERSION:
        raise PcgcError(f'{what}: version {version}; this reader knows version {VERSION}')
    if struct.unpack_from('<I', blob, _FRAME.size)[0] != ops.crc32(blob[:_FRAME.size]):
        raise PcgcError(f'{what}: CRC-32 mismatch (damaged)')
    _check_frame(what, bits, (ox, oy, oz), scale)
    return bits, (ox, oy, oz), scale


def write_frame(path, bits, origin, scale):
    with open(path, 'wb') as f:
        f.write(pack_frame(bits, origin, scale))


def read_frame(path):
    with open(path, 'rb') as f:
        return unpack_frame(f.read(), path)


def frame_bits(prefix):
    """bits of `_V.bin` of one voxelised cloud"""
    return os.path.getsize(prefix + SUFFIX) * 8


# ------------------------------------------------------------------------------------------------ files
def check_bits(bits):
    if isinstance(bits, bool) or not isinstance(bits, (int, np.integer)) or not 1 <= bits <= 20:
        raise ValueError(f'--voxelize / --bits {bits!r}: an integer in 1 .. 20')
    return int(bits)


def voxelize_file(filedir, out, frame_path, bits, merge='mean', origin=None, scale=None, device=None):
    """raw PLY (ASCII or binary, float coordinates, several points per voxel) -> the voxelised ASCII PLY `out` (integer text, with colours
    when the input has them) and the frame `frame_path`; -> (Voxels, rows read)"""
    from .data_utils import read_ply_with_colours, write_ply_ascii_geo, write_ply_ascii_geo_rgb
    from .sparse import require_gpu
    bits = check_bits(bits)
    device = torch.device('cuda') if device is None else device
    require_gpu(device)
    xyz, rgb = read_ply_with_colours(filedir)
    v = voxelize(torch.from_numpy(xyz).to(device), None if rgb is None else torch.from_numpy(rgb).to(device), bits=bits, origin=origin,
                 scale=scale, merge=merge)
    xyz_v = v.coords[:, 1:].cpu().numpy()
    if rgb is None:
        write_ply_ascii_geo(out, xyz_v)
    else:
        write_ply_ascii_geo_rgb(out, xyz_v, v.colours.cpu().numpy())
    write_frame(frame_path, v.bits, v.origin, v.scale)
    return v, len(xyz)


def describe(n, v):
    """the one line the tools print: rows in, voxels out, the largest count, the frame"""
    largest = int(v.counts.max().item()) if len(v.counts) else 0
    return (f'voxelize:\t {n} points -> {len(v.counts)} voxels at {v.bits} bits, largest count {largest}, '
            f'origin {v.origin[0]!r},{v.origin[1]!r},{v.origin[2]!r} scale {v.scale!r}')


def in_front(filedir, outdir, bits, merge='mean'):
    """`--voxelize B` of coder.py and attributes.py: the raw file voxelised into `<prefix>_vox.ply` and `<prefix>_V.bin`, prefix = outdir /
    the file's name -> (the path of `_vox.ply`, which the flow then takes as its --filedir; prefix)"""
    os.makedirs(outdir, exist_ok=True)
    prefix = os.path.join(outdir, os.path.split(filedir)[-1].split('.')[0])
    v, n = voxelize_file(filedir, prefix + '_vox.ply', prefix + SUFFIX, bits, merge)
    print(describe(n, v))
    print(f'{SUFFIX}:\t {frame_bits(prefix)} bits (the frame; not part of the sums below)')
    return prefix + '_vox.ply', prefix


def write_ply_units(path, xyz, rgb=None):
    """ASCII PLY with `property double x/y/z` as text that reads back to the same float64 and, when given, uchar red green blue"""
    import pandas as pd
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    frame = pd.DataFrame({c: xyz[:, j] for j, c in enumerate('xyz')})
    head = 'ply\nformat ascii 1.0\nelement vertex %d\n' % len(xyz) + ''.join(f'property double {c}\n' for c in 'xyz')
    if rgb is not None:
        rgb = np.asarray(rgb).reshape(-1, 3)
        if rgb.dtype != np.uint8 or len(rgb) != len(xyz):
            raise ValueError(f'write_ply_units: colours must be uint8 [{len(xyz)},3]')
        for j, c in enumerate(('red', 'green', 'blue')):
            frame[c] = rgb[:, j].astype(np.int64)
        head += ''.join(f'property uchar {c}\n' for c in ('red', 'green', 'blue'))
    with open(path, 'w', newline='') as f:
        f.write(head + 'end_header\n')
        frame.to_csv(f, sep=' ', header=False, index=False, float_format='%.17g', lineterminator='\n')


def write_units(prefix, decoded_ply):
    """`--devoxelize`: the decoded cloud `decoded_ply` (voxel coordinates, colours or none) in the input's units by `<prefix>_V.bin` ->
    `<prefix>_dec_units.ply`"""
    from .data_utils import read_ply_ascii_with_colours
    _, origin, scale = read_frame(prefix + SUFFIX)
    xyz, rgb = read_ply_ascii_with_colours(decoded_ply)
    write_ply_units(prefix + '_dec_units.ply', devoxelize(xyz, origin, scale), rgb)
    return prefix + '_dec_units.ply'


# ------------------------------------------------------------------------------------------------ CLI
def parse_origin(text):
    try:
        v = tuple(float(t) for t in text.split(','))
    except ValueError:
        v = ()
    if len(v) != 3:
        import argparse
        raise argparse.ArgumentTypeError(f'origin is x,y,z, got {text!r}')
    return v


def parser():
    import argparse
    p = argparse.ArgumentParser(description='voxelise a raw PLY (ASCII or binary) on the GPU', formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('--filedir', required=True, help='input PLY: float coordinates in any unit, ASCII or binary, with or without red green blue')
    p.add_argument('--bits', type=int, required=True, help='bit depth of the lattice, 1 .. 20 (vox10: 10)')
    p.add_argument('--merge', choices=MERGES, default='mean', help='colour of a voxel: the mean of its points (a half rounds up) or its first point')
    p.add_argument('--out', default=None, help='output ASCII PLY (default: the input name + _vox.ply); the frame goes next to it as _V.bin')
    p.add_argument('--origin', type=parse_origin, default=None, help='x,y,z of voxel (0, 0, 0) instead of the per-axis minimum')
    p.add_argument('--scale', type=float, default=None, help='voxels per unit instead of (2^bits - 1) / the largest extent')
    from . import clean
    clean.add_arguments(p)
    return p


def main(argv=None):
    p = parser()
    args = p.parse_args(argv)
    if not 1 <= args.bits <= 20:
        p.error(f'--bits {args.bits}: 1 .. 20')
    from . import clean
    clean.check_arguments(p, args)
    stem = os.path.splitext(args.filedir)[0]
    out = args.out or stem + '_vox.ply'
    prefix = os.path.splitext(out)[0]
    prefix = prefix[:-4] if prefix.endswith('_vox') else prefix
    v, n = voxelize_file(args.filedir, out, prefix + SUFFIX, args.bits, args.merge, args.origin, args.scale)
    print(describe(n, v))
    if args.clean is not None:                           # `<prefix>_clean.ply` next to the voxelised file
        print(clean.describe(clean.clean_file(out, os.path.splitext(out)[0] + '_clean.ply', args.clean_r2, args.clean[0], args.clean[1],
                                              args.keep_largest)))
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
