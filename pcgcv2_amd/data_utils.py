"""Tensor / IO helpers of the encode/decode path (reference data_utils.py:19-48,55-118)."""
import os
import numpy as np
import torch

from . import ops
from .sparse import SparseTensor, sparse_collate, CoordMap


def read_ply_ascii_geo(filedir):
    """data_utils.py:19-34: every line whose tokens all parse as floats is a data row; keep columns 0:3 as int.
    Parsed natively (pcgc_ply_read_ascii_geo): the reference's per-line Python loop takes seconds at ~10^6 points."""
    from ._lib import lib, PcgcError
    path = os.fsencode(filedir)
    n = int(lib().pcgc_ply_read_ascii_geo(path, None, 0))
    if n == -1:
        raise FileNotFoundError(filedir)
    if n < 0:
        raise PcgcError(f'{filedir}: malformed PLY data rows')
    out = np.empty((n, 3), dtype=np.int32)
    if int(lib().pcgc_ply_read_ascii_geo(path, out.ctypes.data, n)) != n:
        raise PcgcError(f'{filedir}: file changed while reading')
    return out.astype('int')


def write_ply_ascii_geo(filedir, coords):
    """data_utils.py:36-48: ASCII PLY, `property float x/y/z`, integer text (native writer)."""
    from ._lib import lib, PcgcError
    coords = np.ascontiguousarray(np.asarray(coords).astype('int'), dtype=np.int32).reshape(-1, 3)
    if int(lib().pcgc_ply_write_ascii_geo(os.fsencode(filedir), coords.ctypes.data, len(coords))) != 0:
        raise PcgcError(f'cannot write {filedir}')


def write_ply_ascii_geo_normals(filedir, coords, normals):
    """ASCII PLY with `property float x/y/z/nx/ny/nz` (what pc_error.read_ply_ascii_with_normals parses): integer coordinate text, the
    normals as float32 with 9 significant digits (they read back to the same float32)."""
    import pandas as pd
    coords = np.asarray(coords).reshape(-1, 3)
    normals = np.asarray(normals, dtype=np.float32).reshape(-1, 3)
    if len(coords) != len(normals):
        raise ValueError(f'{len(coords)} points but {len(normals)} normals')
    if not np.array_equal(coords, np.rint(coords)):
        raise ValueError('write_ply_ascii_geo_normals: coordinates must be integers (a voxelised cloud)')
    frame = pd.DataFrame(coords.astype(np.int64))
    for j in range(3):
        frame[3 + j] = normals[:, j].astype(np.float64)
    with open(filedir, 'w', newline='') as f:
        f.write('ply\nformat ascii 1.0\nelement vertex %d\n' % len(coords))
        f.write(''.join(f'property float {c}\n' for c in ('x', 'y', 'z', 'nx', 'ny', 'nz')))
        f.write('end_header\n')
        frame.to_csv(f, sep=' ', header=False, index=False, float_format='%.9g', lineterminator='\n')


_RGB = ('red', 'green', 'blue')


def _ply_vertex_header(path):
    """-> (names of the vertex properties in file order, vertex count, number of header lines) of an ASCII PLY"""
    names, n, skip = [], 0, 0
    with open(path, 'rb') as f:
        in_vertex = False
        for line in f:
            skip += 1
            t = line.decode('ascii', 'replace').split()
            if not t:
                continue
            if t[0] == 'element':
                in_vertex = t[1] == 'vertex'
                if in_vertex:
                    n = int(t[2])
            elif t[0] == 'property' and in_vertex:
                names.append(t[-1])
            elif t[0] == 'end_header':
                break
    return names, n, skip


def ply_has_colours(path):
    """True iff the ASCII PLY's vertex element declares red, green and blue (header scan only)"""
    try:
        names = _ply_vertex_header(path)[0]
    except OSError:
        return False
    return all(c in names for c in _RGB)


def read_ply_ascii_with_colours(path):
    """ASCII PLY -> (coordinates float64 [n,3], colours uint8 [n,3] or None): the vertex properties x y z and, when present, red green
    blue, wherever they sit among the columns"""
    import pandas as pd
    names, n, skip = _ply_vertex_header(path)
    if not all(c in names for c in 'xyz'):
        raise ValueError(f'{path}: no x / y / z vertex properties')
    data = pd.read_csv(path, sep=r'\s+', header=None, skiprows=skip, nrows=n, dtype=np.float64, engine='c').to_numpy()
    xyz = np.ascontiguousarray(data[:, [names.index(c) for c in 'xyz']])
    if not all(c in names for c in _RGB):
        return xyz, None
    rgb = data[:, [names.index(c) for c in _RGB]]
    if rgb.size and (rgb.min() < 0 or rgb.max() > 255 or not np.array_equal(rgb, np.rint(rgb))):
        raise ValueError(f'{path}: red / green / blue are not 8-bit integers')
    return xyz, np.ascontiguousarray(rgb.astype(np.uint8))


_PLY_TYPES = {'char': 'i1', 'int8': 'i1', 'uchar': 'u1', 'uint8': 'u1', 'short': 'i2', 'int16': 'i2', 'ushort': 'u2', 'uint16': 'u2',
              'int': 'i4', 'int32': 'i4', 'uint': 'u4', 'uint32': 'u4', 'float': 'f4', 'float32': 'f4', 'double': 'f8', 'float64': 'f8'}
_PLY_FORMATS = {'ascii': None, 'binary_little_endian': '<', 'binary_big_endian': '>'}


def _ply_header(path):
    """-> (format, elements, header bytes) of a PLY of any format; elements: [(name, count, [(property, type or None for a list)])] in
    file order.  ValueError for a file that is no PLY, has no end_header or names an unknown format."""
    fmt, elements, size = None, [], 0
    with open(path, 'rb') as f:
        if f.readline().strip() != b'ply':
            raise ValueError(f'{path}: not a PLY file')
        f.seek(0)
        for line in f:
            size += len(line)
            t = line.decode('ascii', 'replace').split()
            if not t:
                continue
            if t[0] == 'format' and len(t) >= 2:
                fmt = t[1]
            elif t[0] == 'element' and len(t) == 3:
                elements.append((t[1], int(t[2]), []))
            elif t[0] == 'property' and elements and len(t) >= 3:
                elements[-1][2].append((t[-1], None if t[1] == 'list' else t[1]))
            elif t[0] == 'end_header':
                break
        else:
            raise ValueError(f'{path}: no end_header')
    if fmt not in _PLY_FORMATS:
        raise ValueError(f'{path}: format {fmt!r}; one of {sorted(_PLY_FORMATS)}')
    return fmt, elements, size


def _ply_row_dtype(path, element, order):
    name, _, props = element
    fields = []
    for prop, kind in props:
        if kind is None:
            raise ValueError(f'{path}: element {name!r} has a list property ({prop!r}) and stands in front of the vertices: '
                             'its size cannot be known without reading it; write the vertex element first')
        if kind not in _PLY_TYPES:
            raise ValueError(f'{path}: property {prop!r} of element {name!r} has the unknown type {kind!r}')
        fields.append((prop, order + _PLY_TYPES[kind]))
    if len({p for p, _ in fields}) != len(fields):
        raise ValueError(f'{path}: element {name!r} names a property twice')
    return np.dtype(fields)


def read_ply_with_colours(path):
    """A PLY of any format -> (coordinates float64 [n,3], colours uint8 [n,3] or None), as read_ply_ascii_with_colours gives them for an
    ASCII file.  binary_little_endian and binary_big_endian: the vertex element is read through a numpy structured dtype built from the
    header (char uchar short ushort int uint float double and their int8 .. float64 names, in any column order); elements behind the
    vertices are ignored; ValueError for an element with a list property in front of them and for a file that ends inside them."""
    fmt, elements, at = _ply_header(path)
    if fmt == 'ascii':
        return read_ply_ascii_with_colours(path)
    order = _PLY_FORMATS[fmt]
    for element in elements:
        if element[0] == 'vertex':
            break
        at += element[1] * _ply_row_dtype(path, element, order).itemsize
    else:
        raise ValueError(f'{path}: no vertex element')
    n, row = element[1], _ply_row_dtype(path, element, order)
    names = row.names or ()
    if not all(c in names for c in 'xyz'):
        raise ValueError(f'{path}: no x / y / z vertex properties')
    have = os.path.getsize(path) - at
    if n < 0 or have < n * row.itemsize:
        raise ValueError(f'{path}: {n} vertices of {row.itemsize} bytes declared, {max(have, 0)} bytes behind the header (cut short)')
    data = np.fromfile(path, dtype=row, count=n, offset=at)
    xyz = np.stack([data[c].astype(np.float64) for c in 'xyz'], 1) if n else np.zeros((0, 3), np.float64)
    if not all(c in names for c in _RGB):
        return np.ascontiguousarray(xyz), None
    rgb = np.stack([data[c].astype(np.float64) for c in _RGB], 1) if n else np.zeros((0, 3), np.float64)
    if rgb.size and (rgb.min() < 0 or rgb.max() > 255 or not np.array_equal(rgb, np.rint(rgb))):
        raise ValueError(f'{path}: red / green / blue are not 8-bit integers')
    return np.ascontiguousarray(xyz), np.ascontiguousarray(rgb.astype(np.uint8))


def write_ply_ascii_geo_rgb(filedir, coords, rgb):
    """ASCII PLY with `property float x/y/z` and `property uchar red/green/blue`, integer text (native writer): what mpeg-pcc-dmetric's
    `-c 1` and read_ply_ascii_with_colours read; read_ply_ascii_geo reads its coordinates."""
    from ._lib import lib, PcgcError
    coords = np.ascontiguousarray(np.asarray(coords).astype('int'), dtype=np.int32).reshape(-1, 3)
    rgb = np.asarray(rgb)
    if rgb.dtype != np.uint8:
        raise ValueError(f'write_ply_ascii_geo_rgb: colours must be uint8, got {rgb.dtype}')
    rgb = np.ascontiguousarray(rgb).reshape(-1, 3)
    if len(rgb) != len(coords):
        raise ValueError(f'{len(coords)} points but {len(rgb)} colours')
    if int(lib().pcgc_ply_write_ascii_geo_rgb(os.fsencode(filedir), coords.ctypes.data, rgb.ctypes.data, len(coords))) != 0:
        raise PcgcError(f'cannot write {filedir}')


def _h5py():
    try:
        import h5py
    except ImportError as e:
        raise ImportError('h5py is not installed: the .h5 patch files of the reference need it (PLY files do not)') from e
    return h5py


def read_h5_geo(filedir):
    """data_utils.py:6-10: dataset 'data', columns 0:3 as int."""
    with _h5py().File(filedir, 'r') as h:
        pc = h['data'][:]
    return pc[:, 0:3].astype('int')


def write_h5_geo(filedir, coords):
    """data_utils.py:12-17: dataset 'data' as uint8 (coordinates past 255 wrap, as in the reference)."""
    data = np.asarray(coords).astype('uint8')
    with _h5py().File(filedir, 'w') as h:
        h.create_dataset('data', data=data, shape=data.shape)


def array2vector(array, step):
    """data_utils.py:55-61 (host-side; the device path is ops.sort_zyx)."""
    array = torch.as_tensor(array).long().cpu()
    step = int(step)
    return sum(array[:, i] * (step ** i) for i in range(array.shape[-1]))


def _coords_of(t):
    """(coordinate tensor, the level it belongs to or None) of a tensor / SparseTensor / CoordMap"""
    if isinstance(t, SparseTensor):
        return t.C, t.cmap
    if isinstance(t, CoordMap):
        return t.C, t
    return torch.as_tensor(t), None


def isin_mask(data, ground_truth, or_mask=None):
    """isin on device as the uint8 mask the pruning and loss kernels read (pcgc_hash_contains), OR-ed with `or_mask` in the same launch.
    `ground_truth` given as a SparseTensor / CoordMap is probed through the level's own (cached) hash table; a bare [M, 4] tensor gets a
    table of its own."""
    a, _ = _coords_of(data)
    b, level = _coords_of(ground_truth)
    a = a.to(torch.int32).contiguous()
    if a.dim() != 2 or a.shape[1] != 4 or b.dim() != 2 or b.shape[1] != 4:
        raise ValueError('isin on device expects [N, 4] coordinates (batch, x, y, z)')
    if level is not None:
        table = level.table if len(level) else None
    else:
        b = b.to(device=a.device, dtype=torch.int32).contiguous()
        if b.shape[0]:
            ops.check_coords(b, 'isin: ground truth')          # (a row the key cannot hold would silently never match)
        table = ops.HashTable(b, 1) if b.shape[0] else None
    return ops.hash_contains(a, table, or_mask=or_mask)


def isin(data, ground_truth):
    """data_utils.py:63-75: boolean vector, True where a row of `data` (int coordinates [N, D]) occurs in `ground_truth`: the reference's
    Decoder.prune_voxel (autoencoder.py:241-243) and loss.py use it.  Rows on the GPU are looked up in the ground truth's coordinate hash
    (isin_mask; pass the SparseTensor instead of its `.C` to re-use the level's table); CPU tensors take the reference's host route."""
    a, _ = _coords_of(data)
    if a.is_cuda:
        return isin_mask(data, ground_truth).bool()
    dev = a.device
    a, b = a.long().cpu(), _coords_of(ground_truth)[0].long().cpu()
    step = int(max(a.max(), b.max())) + 1
    return torch.isin(array2vector(a, step), array2vector(b, step)).to(dev)


def istopk(data, nums, rho=1.0):
    """data_utils.py:77-89 on device: per batch item b, mask of its int(min(rows_b, nums[b] * rho)) largest values (the reference
    loops over the items on the host; here the items are contiguous row segments of one tensor)."""
    if len(nums) == 1:
        k = int(min(len(data), nums[0] * rho))
        return ops.topk_mask(data.F, k).bool()
    rows = data.cmap.batch_rows
    keep = [int(min(r, n * rho)) for r, n in zip(rows, nums)]
    return ops.topk_mask_segments(data.F, rows, keep).bool()


def sort_spare_tensor(sparse_tensor):
    """data_utils.py:91-101: rows ordered by (z, y, x, batch)."""
    perm = ops.sort_zyx(sparse_tensor.C)
    coords = ops.gather_coords(sparse_tensor.C, perm)
    feats = ops.gather_feats(sparse_tensor.F, perm)
    return SparseTensor(feats, coordinate_map=CoordMap(coords, sparse_tensor.cmap.stride, unique=True))


def load_sparse_tensor(filedir, device):
    """data_utils.py:103-110."""
    coords = torch.tensor(read_ply_ascii_geo(filedir)).int()
    feats = torch.ones((len(coords), 1)).float()
    coords, feats = sparse_collate([coords], [feats])
    return SparseTensor(features=feats, coordinates=coords, tensor_stride=1, device=device)


def scale_sparse_tensor(x, factor):
    """data_utils.py:112-118: (C*factor).round().int() in fp32, then re-collate (dedups)."""
    coords = ops.coords_scale(x.C, factor)
    feats = torch.ones((coords.shape[0], 1), dtype=torch.float32, device=coords.device)
    return SparseTensor(features=feats, coordinates=coords, tensor_stride=1, device=x.device)
