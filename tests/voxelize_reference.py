"""The definition of voxelising a raw point cloud: numpy, integers wherever possible.  csrc/voxelize.hip, include/pcgc_hip.h
and pcgcv2_amd/voxelize.py follow it, and the device tests hold every output to equality with it.

Frame.  With origin and scale both None, origin[a] is the minimum of axis a taken in fp64 (a zero is +0), e the largest per-axis extent
(max - min) and scale = (2^B - 1) / e in fp64, 1.0 when e == 0.  The caller may give either or both instead: a missing origin is the
minimum, a missing scale comes from the extents of the data.  A row with a NaN or an infinity is an error that names the count; so is a
scale that is not finite and positive (extents below 2^B / 1.8e308 have none).

Quantiser.  q[a] = rint((float64(p[a]) - origin[a]) * scale): the subtraction and the product each rounded once to fp64, ties to even.
A q outside [0, 2^B - 1] (possible with a caller-given frame only) is an error that names the count.

Voxels.  The distinct q in the codec's canonical order, z most significant (array2vector's order).  coords int32 [M,4] with column 0 = 0,
counts int32 [M], voxel_of int32 [N] (the output row of every input row), colours uint8 [M,3] or None.  merge = 'mean': per channel
floor((2 sum + count) / (2 count)) over 64-bit integer sums, which rounds a half up and does not depend on the row order; 'first': the
colour of the voxel's lowest input row.
"""
from collections import namedtuple

import numpy as np

Voxels = namedtuple('Voxels', 'coords counts voxel_of colours origin scale bits')
MERGES = ('mean', 'first')


def _check(points, colours, bits, merge):
    points = np.asarray(points)
    if points.dtype not in (np.float32, np.float64):
        raise ValueError(f'points must be float32 or float64, got {points.dtype}')
    if points.ndim != 2 or points.shape[1] != 3:
        raise ValueError(f'points must be [N,3], got {points.shape}')
    if isinstance(bits, bool) or not isinstance(bits, (int, np.integer)) or not 1 <= bits <= 20:
        raise ValueError(f'bits {bits!r}: an integer in 1 .. 20')
    if merge not in MERGES:
        raise ValueError(f'merge {merge!r}: one of {MERGES}')
    if colours is not None:
        colours = np.asarray(colours)
        if colours.dtype != np.uint8 or colours.shape != points.shape:
            raise ValueError(f'colours must be uint8 [{len(points)},3], got {colours.dtype} {colours.shape}')
    return points.astype(np.float64), colours


def frame(points, bits, origin=None, scale=None):
    """-> (origin float64 [3], scale float) of finite points [N,3] (float64), N >= 1"""
    lo, hi = points.min(0) + 0.0, points.max(0) + 0.0
    if origin is None:
        origin = lo
    origin = np.asarray(origin, np.float64).reshape(3)
    if scale is None:
        e = float((hi - lo).max())
        with np.errstate(over='ignore'):
            scale = float(np.float64((1 << bits) - 1) / np.float64(e)) if e != 0 else 1.0
    scale = float(scale)
    if not np.isfinite(origin).all():
        raise ValueError(f'origin {origin.tolist()} is not finite')
    if not (np.isfinite(scale) and scale > 0):
        raise ValueError(f'scale {scale} is not finite and positive')
    return origin, scale


def voxelize(points, colours=None, bits=10, origin=None, scale=None, merge='mean'):
    p, colours = _check(points, colours, bits, merge)
    n = len(p)
    if n == 0:
        o = np.zeros(3) if origin is None else np.asarray(origin, np.float64).reshape(3)
        return Voxels(np.zeros((0, 4), np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32),
                      None if colours is None else np.zeros((0, 3), np.uint8), o, 1.0 if scale is None else float(scale), int(bits))
    bad = int(np.count_nonzero(~np.isfinite(p).all(1)))
    if bad:
        raise ValueError(f'{bad} of {n} rows hold a NaN or an infinity')
    origin, scale = frame(p, bits, origin, scale)
    with np.errstate(over='ignore', invalid='ignore'):
        q = np.rint((p - origin[None, :]) * np.float64(scale))
    outside = int(np.count_nonzero(~((q >= 0) & (q <= (1 << bits) - 1)).all(1)))
    if outside:
        raise ValueError(f'{outside} of {n} rows fall outside [0, 2^{bits} - 1] in the frame given')
    q = q.astype(np.int64)
    key = (q[:, 2] << 40) | (q[:, 1] << 20) | q[:, 0]
    order = np.argsort(key, kind='stable')
    sk = key[order]
    head = np.ones(n, bool)
    head[1:] = sk[1:] != sk[:-1]
    rank = np.cumsum(head) - 1
    m = int(rank[-1]) + 1
    voxel_of = np.empty(n, np.int32)
    voxel_of[order] = rank
    hk = sk[head]
    coords = np.stack([np.zeros(m, np.int64), hk & 0xFFFFF, (hk >> 20) & 0xFFFFF, hk >> 40], 1).astype(np.int32)
    counts = np.bincount(voxel_of, minlength=m).astype(np.int32)
    out = None
    if colours is not None and merge == 'first':
        out = colours[order[head]]
    elif colours is not None:
        sums = np.zeros((m, 3), np.int64)
        np.add.at(sums, voxel_of, colours.astype(np.int64))
        c = counts.astype(np.int64)[:, None]
        out = ((2 * sums + c) // (2 * c)).astype(np.uint8)
    return Voxels(coords, counts, voxel_of, out, origin, scale, int(bits))


def devoxelize(coords, origin, scale):
    """the position of a voxel in the input's units: q / scale + origin in fp64; coords [M,4] rows (0, x, y, z) or [M,3] -> float64 [M,3]"""
    q = np.asarray(coords)
    q = q[:, -3:].astype(np.float64)
    return q / np.float64(scale) + np.asarray(origin, np.float64).reshape(1, 3)
