"""Voxelising a raw cloud, the parts that need no GPU: the definition (tests/voxelize_reference.py) against an independent statement, its
ties, means and default frame; `_V.bin` and every refusal of it; the binary PLY reader on files the test writes itself; CLI parsing."""
import struct
import zlib

import numpy as np
import pytest

import voxelize_reference as V
from pcgcv2_amd import attributes, coder, data_utils, voxelize as vox
from pcgcv2_amd._lib import PcgcError


# ---- the definition ----------------------------------------------------------------------------------------------------------------------
def _independent(points, colours, bits, merge):
    """np.unique(axis=0) and a Python dictionary of sums: nothing shared with the definition but the quantiser formula"""
    p = np.asarray(points).astype(np.float64)
    origin = p.min(0)
    e = (p.max(0) - origin).max()
    scale = ((1 << bits) - 1) / e if e else 1.0
    q = np.rint((p - origin) * scale).astype(np.int64)
    uniq, inverse = np.unique(q[:, ::-1], axis=0, return_inverse=True)          # lexicographic in (z, y, x)
    inverse = inverse.reshape(-1)
    sums, first = {}, {}
    for i, v in enumerate(inverse.tolist()):
        c = [int(k) for k in colours[i]]
        s = sums.setdefault(v, [0, 0, 0, 0])
        s[0] += 1
        s[1] += c[0]
        s[2] += c[1]
        s[3] += c[2]
        first.setdefault(v, c)
    counts = [sums[v][0] for v in range(len(uniq))]
    if merge == 'first':
        cols = [first[v] for v in range(len(uniq))]
    else:                                                                      # round(mean) with halves up, in exact integers
        cols = [[(2 * sums[v][k] + sums[v][0]) // (2 * sums[v][0]) for k in (1, 2, 3)] for v in range(len(uniq))]
    return uniq[:, ::-1], np.array(counts), inverse, np.array(cols), origin, scale


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('merge', ['mean', 'first'])
@pytest.mark.parametrize('bits,n,seed', [(1, 50, 0), (3, 400, 1), (6, 2000, 2), (10, 3000, 3), (20, 500, 4)])
def test_definition_against_an_independent_statement(dtype, merge, bits, n, seed):
    rng = np.random.default_rng(seed)
    p = (rng.normal(size=(n, 3)) * rng.choice([1e-3, 1.0, 1e4]) + rng.normal(size=3) * 100).astype(dtype)
    p[n // 2:] = p[:n - n // 2]                                               # every voxel met at least twice
    c = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    got = V.voxelize(p, c, bits, merge=merge)
    xyz, counts, inverse, cols, origin, scale = _independent(p, c, bits, merge)
    assert np.array_equal(got.coords[:, 1:], xyz) and not got.coords[:, 0].any() and got.coords.dtype == np.int32
    assert np.array_equal(got.counts, counts) and np.array_equal(got.voxel_of, inverse) and np.array_equal(got.colours, cols)
    assert np.array_equal(got.origin, origin) and got.scale == scale and got.bits == bits
    assert got.counts.sum() == n and got.colours.dtype == np.uint8
    key = (got.coords[:, 3].astype(np.int64) << 40) | (got.coords[:, 2].astype(np.int64) << 20) | got.coords[:, 1]
    assert (np.diff(key) > 0).all()                                           # array2vector's order, z most significant


def test_ties_go_to_even():
    k = np.arange(0, 9, dtype=np.float64)
    p = np.stack([k + 0.5, np.zeros(9), np.zeros(9)], 1)
    got = V.voxelize(p, None, bits=4, origin=(0, 0, 0), scale=1.0)
    assert got.coords[got.voxel_of, 1].tolist() == [0, 2, 2, 4, 4, 6, 6, 8, 8]
    assert got.counts.tolist() == [1, 2, 2, 2, 2] and got.colours is None


def test_means_round_half_up():
    p = np.zeros((5, 3))
    p[2:, 0] = 1.0
    c = np.array([[0, 255, 1], [255, 0, 2], [1, 2, 255], [2, 2, 255], [2, 3, 255]], np.uint8)
    got = V.voxelize(p, c, bits=1, origin=(0, 0, 0), scale=1.0)
    assert got.colours.tolist() == [[128, 128, 2], [2, 2, 255]]               # 127.5 -> 128, 1.5 -> 2; 5/3 -> 2, 7/3 -> 2
    assert V.voxelize(p, c, bits=1, origin=(0, 0, 0), scale=1.0, merge='first').colours.tolist() == [[0, 255, 1], [1, 2, 255]]


@pytest.mark.parametrize('bits', [1, 20])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_default_frame_reaches_both_ends(bits, dtype):
    rng = np.random.default_rng(bits)
    for magnitude in (1e-6, 1.0, 1e9):
        p = (rng.uniform(-1, 1, (64, 3)) * magnitude + magnitude * rng.uniform(-3, 3)).astype(dtype)
        got = V.voxelize(p, None, bits)
        widest = int(np.argmax(p.astype(np.float64).max(0) - p.astype(np.float64).min(0)))
        assert got.coords[:, 1:].min(0).tolist() == [0, 0, 0]
        assert got.coords[:, 1 + widest].max() == (1 << bits) - 1


def test_definition_refusals_and_edges():
    p = np.array([[0.0, 0, 0], [1, 1, 1], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]])
    with pytest.raises(ValueError, match='3 of 5 rows'):
        V.voxelize(p, None, 4)
    with pytest.raises(ValueError, match='2 of 3 rows fall outside'):
        V.voxelize(np.array([[0.0, 0, 0], [16, 0, 0], [-1, 0, 0]]), None, 4, origin=(0, 0, 0), scale=1.0)
    with pytest.raises(ValueError, match='scale'):
        V.voxelize(np.array([[0.0, 0, 0], [1e-310, 0, 0]]), None, 10)          # (2^10 - 1) / 1e-310 is no double
    for bits in (0, 21, True, 2.0):
        with pytest.raises(ValueError):
            V.voxelize(np.zeros((1, 3)), None, bits)
    with pytest.raises(ValueError):
        V.voxelize(np.zeros((1, 3)), None, 4, merge='median')
    with pytest.raises(ValueError):
        V.voxelize(np.zeros((1, 3), np.int32), None, 4)
    one = V.voxelize(np.full((3, 3), 7.25, np.float32), np.full((3, 3), 9, np.uint8), 10)       # e == 0
    assert one.scale == 1.0 and one.coords.tolist() == [[0, 0, 0, 0]] and one.counts.tolist() == [3] and one.origin.tolist() == [7.25] * 3
    none = V.voxelize(np.zeros((0, 3)), np.zeros((0, 3), np.uint8), 10)
    assert none.coords.shape == (0, 4) and none.colours.shape == (0, 3) and none.voxel_of.shape == (0,)
    back = V.devoxelize(one.coords, one.origin, one.scale)
    assert back.tolist() == [[7.25] * 3] and back.dtype == np.float64
    assert np.array_equal(vox.devoxelize(one.coords, one.origin, one.scale), back)


# ---- `_V.bin` ----------------------------------------------------------------------------------------------------------------------------
def _frame(magic=b'PCGV', version=1, bits=10, origin=(1.5, -2.0, 3.25), scale=511.5, crc=None, tail=b''):
    blob = struct.pack('<4sII4d', magic, version, bits, *origin, scale)
    return blob + struct.pack('<I', zlib.crc32(blob) if crc is None else crc) + tail


def test_frame_file_round_trip(tmp_path):
    blob = vox.pack_frame(10, (1.5, -2.0, 3.25), 511.5)
    assert blob == _frame() and len(blob) == 48 == vox.FRAME_BYTES
    assert vox.unpack_frame(blob) == (10, (1.5, -2.0, 3.25), 511.5)
    path = str(tmp_path / 'a_V.bin')
    vox.write_frame(path, 20, (0.0, 1e9, -1e-9), 1e-3)
    assert vox.read_frame(path) == (20, (0.0, 1e9, -1e-9), 1e-3) and vox.frame_bits(str(tmp_path / 'a')) == 384


@pytest.mark.parametrize('fitted', [True, False], ids=['crc_fits', 'crc_left'])
@pytest.mark.parametrize('name,change', [
    ('magic', dict(magic=b'PCGA')), ('version', dict(version=2)), ('bits0', dict(bits=0)), ('bits21', dict(bits=21)),
    ('scale_zero', dict(scale=0.0)), ('scale_negative', dict(scale=-1.0)), ('scale_inf', dict(scale=float('inf'))),
    ('scale_nan', dict(scale=float('nan'))), ('origin_nan', dict(origin=(0.0, float('nan'), 0.0))),
])
def test_frame_file_refusals(name, change, fitted):
    good = _frame()
    bad = _frame(**change) if fitted else _frame(**change)[:-4] + good[-4:]
    with pytest.raises(PcgcError):
        vox.unpack_frame(bad)


def test_frame_file_refusals_of_length_and_crc():
    good = _frame()
    for bad in (good[:-1], good + b'\0', b'', _frame(tail=b'\0\0\0\0'), _frame(crc=0), good[:20] + bytes([good[20] ^ 1]) + good[21:]):
        with pytest.raises(PcgcError):
            vox.unpack_frame(bad)
    for args in ((0, (0, 0, 0), 1.0), (21, (0, 0, 0), 1.0), (10, (0, 0, float('inf')), 1.0), (10, (0, 0, 0), 0.0), (10, (0, 0, 0), float('nan'))):
        with pytest.raises(PcgcError):
            vox.pack_frame(*args)


# ---- binary PLY --------------------------------------------------------------------------------------------------------------------------
_CODES = {'char': 'b', 'uchar': 'B', 'short': 'h', 'ushort': 'H', 'int': 'i', 'uint': 'I', 'float': 'f', 'double': 'd',
          'int8': 'b', 'uint8': 'B', 'int16': 'h', 'uint16': 'H', 'int32': 'i', 'uint32': 'I', 'float32': 'f', 'float64': 'd'}


def _write_ply(path, fmt, columns, rows, before=(), after=b'', after_header=()):
    """columns: [(name, type)]; rows: one tuple per vertex in column order; before: [(element, count, [(name, type)], rows)] written in
    front of the vertices; after / after_header: raw bytes and header lines of what follows them"""
    order = {'binary_little_endian': '<', 'binary_big_endian': '>'}.get(fmt)
    head = ['ply', f'format {fmt} 1.0', 'comment written by the test']
    body = b''
    for name, count, cols, data in before:
        head += [f'element {name} {count}'] + [f'property {t} {c}' for c, t in cols]
        body += b''.join(struct.pack(order + ''.join(_CODES[t] for _, t in cols), *r) for r in data)
    head += [f'element vertex {len(rows)}'] + [f'property {t} {c}' for c, t in columns]
    head += list(after_header) + ['end_header']
    if order is None:
        body = ''.join(' '.join(repr(v) if isinstance(v, float) else str(v) for v in r) + '\n' for r in rows).encode()
    else:
        body += b''.join(struct.pack(order + ''.join(_CODES[t] for _, t in columns), *r) for r in rows) + after
    with open(path, 'wb') as f:
        f.write(('\n'.join(head) + '\n').encode() + body)


def _cloud(n=37, seed=5):
    rng = np.random.default_rng(seed)
    xyz = rng.integers(-2000, 2000, (n, 3)) / 4.0                              # quarters: float32 holds them, and their text is short
    rgb = rng.integers(0, 256, (n, 3))
    return xyz, rgb


@pytest.mark.parametrize('fmt', ['binary_little_endian', 'binary_big_endian'])
@pytest.mark.parametrize('real', ['float', 'double', 'float32', 'float64'])
def test_binary_ply_reads_what_the_ascii_reader_reads(tmp_path, fmt, real):
    xyz, rgb = _cloud()
    if real in ('float', 'float32'):
        xyz = xyz.astype(np.float32).astype(np.float64)
    columns = [('red', 'uchar'), ('z', real), ('x', real), ('nx', 'float'), ('blue', 'uint8'), ('y', real), ('green', 'uchar')]
    rows = [(int(c[0]), float(p[2]), float(p[0]), 0.25, int(c[2]), float(p[1]), int(c[1])) for p, c in zip(xyz, rgb)]
    _write_ply(str(tmp_path / 'b.ply'), fmt, columns, rows)
    _write_ply(str(tmp_path / 'a.ply'), 'ascii', columns, rows)
    got, want = data_utils.read_ply_with_colours(str(tmp_path / 'b.ply')), data_utils.read_ply_with_colours(str(tmp_path / 'a.ply'))
    ascii_only = data_utils.read_ply_ascii_with_colours(str(tmp_path / 'a.ply'))
    for g, w, a in zip(got, want, ascii_only):
        assert g.dtype == w.dtype and np.array_equal(g, w) and np.array_equal(w, a)
    assert np.array_equal(got[0], xyz) and np.array_equal(got[1], rgb) and got[1].dtype == np.uint8 and got[0].dtype == np.float64


@pytest.mark.parametrize('fmt', ['binary_little_endian', 'binary_big_endian'])
@pytest.mark.parametrize('kind', sorted(_CODES))
def test_binary_ply_every_scalar_type(tmp_path, fmt, kind):
    unsigned = kind.startswith('u')
    values = [0, 1, 2, 100, 127] if unsigned else [-127, -1, 0, 5, 127]
    cast = float if _CODES[kind] in 'fd' else int
    columns = [('x', kind), ('pad', 'uchar'), ('y', kind), ('z', kind), ('red', kind), ('green', kind), ('blue', kind)]
    rows = [(cast(v), 7, cast(v) + 0, cast(values[0]), cast(abs(v)), cast(abs(v)), cast(1)) for v in values]
    path = str(tmp_path / 't.ply')
    _write_ply(path, fmt, columns, rows, after_header=['element face 1', 'property list uchar int vertex_indices'],
               after=struct.pack('<Biii', 3, 0, 1, 2))                        # a face element behind the vertices is not looked at
    xyz, rgb = data_utils.read_ply_with_colours(path)
    assert xyz[:, 0].tolist() == values and xyz[:, 1].tolist() == values and xyz[:, 2].tolist() == [values[0]] * 5
    assert rgb[:, 0].tolist() == [abs(v) for v in values] and rgb[:, 2].tolist() == [1] * 5 and rgb.dtype == np.uint8


def test_binary_ply_elements_around_the_vertices(tmp_path):
    xyz, _ = _cloud(9)
    columns = [('x', 'double'), ('y', 'double'), ('z', 'double')]
    rows = [tuple(float(v) for v in p) for p in xyz]
    path = str(tmp_path / 'c.ply')
    camera = ('camera', 2, [('fx', 'float'), ('id', 'short')], [(1.5, 3), (2.5, 4)])
    _write_ply(path, 'binary_big_endian', columns, rows, before=[camera])     # a fixed-size element in front is skipped by its size
    got, colours = data_utils.read_ply_with_colours(path)
    assert np.array_equal(got, xyz) and colours is None
    with open(path, 'wb') as f:                                               # a list element in front of the vertices: refused
        f.write(b'ply\nformat binary_little_endian 1.0\nelement face 1\nproperty list uchar int vertex_indices\nelement vertex 1\n'
                b'property float x\nproperty float y\nproperty float z\nend_header\n' + struct.pack('<Biii', 3, 0, 0, 0) + struct.pack('<fff', 1, 2, 3))
    with pytest.raises(ValueError, match='list property'):
        data_utils.read_ply_with_colours(path)


def test_binary_ply_refusals(tmp_path):
    xyz, rgb = _cloud(5)
    columns = [('x', 'float'), ('y', 'float'), ('z', 'float'), ('red', 'uchar'), ('green', 'uchar'), ('blue', 'uchar')]
    rows = [(float(p[0]), float(p[1]), float(p[2]), int(c[0]), int(c[1]), int(c[2])) for p, c in zip(xyz, rgb)]
    path = str(tmp_path / 'd.ply')
    _write_ply(path, 'binary_little_endian', columns, rows)
    whole = open(path, 'rb').read()
    assert data_utils.read_ply_with_colours(path)[1].tolist() == rgb.tolist()
    open(path, 'wb').write(whole[:-1])                                        # cut by one byte
    with pytest.raises(ValueError, match='cut short'):
        data_utils.read_ply_with_colours(path)
    open(path, 'wb').write(whole.replace(b'binary_little_endian', b'binary_middle_endian'))
    with pytest.raises(ValueError, match='format'):
        data_utils.read_ply_with_colours(path)
    open(path, 'wb').write(whole.replace(b'property float y', b'property half y'))
    with pytest.raises(ValueError, match='unknown type'):
        data_utils.read_ply_with_colours(path)
    open(path, 'wb').write(whole.replace(b'property float z', b'property float w'))
    with pytest.raises(ValueError, match='x / y / z'):
        data_utils.read_ply_with_colours(path)
    open(path, 'wb').write(b'plx\n' + whole[4:])
    with pytest.raises(ValueError, match='not a PLY'):
        data_utils.read_ply_with_colours(path)
    open(path, 'wb').write(whole.replace(b'end_header\n', b'end_headex\n'))
    with pytest.raises(ValueError, match='end_header'):
        data_utils.read_ply_with_colours(path)
    _write_ply(path, 'binary_little_endian', [('x', 'float'), ('y', 'float'), ('z', 'float'), ('red', 'short'), ('green', 'short'), ('blue', 'short')],
               [(0.0, 0.0, 0.0, 256, 0, 0)])
    with pytest.raises(ValueError, match='8-bit'):
        data_utils.read_ply_with_colours(path)


# ---- CLI ---------------------------------------------------------------------------------------------------------------------------------
def test_cli_parsing(capsys):
    args = vox.parser().parse_args(['--filedir', 'raw.ply', '--bits', '10'])
    assert (args.bits, args.merge, args.out, args.origin, args.scale) == (10, 'mean', None, None, None)
    args = vox.parser().parse_args(['--filedir', 'raw.ply', '--bits', '7', '--merge', 'first', '--origin', '1,-2.5,3e2', '--scale', '0.5', '--out', 'v.ply'])
    assert (args.bits, args.merge, args.out, args.origin, args.scale) == (7, 'first', 'v.ply', (1.0, -2.5, 300.0), 0.5)
    for bad in (['--bits', '0'], ['--bits', '21'], ['--bits', '10', '--merge', 'median'], ['--bits', '10', '--origin', '1,2']):
        with pytest.raises(SystemExit):
            vox.main(['--filedir', 'raw.ply'] + bad)
    args = coder._parse_cli(['--filedir', 'raw.ply', '--voxelize', '9', '--merge', 'first', '--devoxelize', '--lossless'])
    assert (args.voxelize, args.merge, args.devoxelize, args.lossless) == (9, 'first', True, True)
    args = coder._parse_cli(['--filedir', 'vox.ply'])                          # without the flag nothing moves
    assert (args.voxelize, args.merge, args.devoxelize, args.res) == (None, 'mean', False, 1024)
    for bad in (['--voxelize', '0'], ['--voxelize', '21'], ['--voxelize', 'ten'], ['--devoxelize']):
        with pytest.raises(SystemExit):
            coder._parse_cli(['--filedir', 'raw.ply'] + bad)
        with pytest.raises(SystemExit):
            attributes.main(['--filedir', 'raw.ply', '--qstep', '0'] + bad)
    capsys.readouterr()
