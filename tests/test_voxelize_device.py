"""Voxelising a raw cloud on the GPU (csrc/voxelize.hip, pcgcv2_amd/voxelize.py): coords, counts, voxel_of, colours and the frame EQUAL to
the numpy definition (tests/voxelize_reference.py), no tolerance, at the smallest shapes at which the kernels can go wrong: the run lengths
around the merge kernel's rows per workgroup, a colour sum past 32 bits, the ends of the lattice, the edges of fp64; then the two CLIs with
`--voxelize` in front of them on a jittered shell."""
import os

import numpy as np
import pytest
import torch

import voxelize_reference as V
from pcgcv2_amd import attributes, coder, ops, synthetic, voxelize as vox
from pcgcv2_amd._lib import lib
from pcgcv2_amd.data_utils import read_ply_ascii_geo, read_ply_ascii_with_colours, read_ply_with_colours

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
T = 256                                                         # pcgc_voxelize_tile_rows(), asserted below


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same(got, want):
    assert got.coords.dtype == torch.int32 and got.counts.dtype == torch.int32 and got.voxel_of.dtype == torch.int32
    assert np.array_equal(got.coords.cpu().numpy(), want.coords)
    assert np.array_equal(got.counts.cpu().numpy(), want.counts)
    assert np.array_equal(got.voxel_of.cpu().numpy(), want.voxel_of)
    if want.colours is None:
        assert got.colours is None
    else:
        assert got.colours.dtype == torch.uint8 and np.array_equal(got.colours.cpu().numpy(), want.colours)
    assert list(got.origin) == want.origin.tolist() and got.scale == want.scale and got.bits == want.bits


def _check(points, colours, bits, **kw):
    want = V.voxelize(points, colours, bits, **kw)
    got = ops.voxelize(_dev(points), _dev(colours), bits, **kw)
    _same(got, want)
    return got, want


def _colours(n, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (n, 3)).astype(np.uint8)


def _runs(lengths, seed=0, shuffle=True):
    """voxel k = (k % 2, k // 2 % 2, k // 4), the k-th in (z, y, x) order, met lengths[k] times, in the unit frame; the rows shuffled, so that
    the sort has to bring the runs together"""
    k = np.repeat(np.arange(len(lengths)), lengths)
    p = np.stack([k % 2, k // 2 % 2, k // 4], 1).astype(np.float64)
    if shuffle:
        p = p[np.random.default_rng(seed).permutation(len(p))]
    return p


UNIT = dict(origin=(0.0, 0.0, 0.0), scale=1.0)


def test_tile_rows():
    assert ops.voxelize_tile_rows() == T == int(lib().pcgc_voxelize_tile_rows())


# ---- row counts --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 2, 3])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_a_few_rows(n, dtype):
    p = np.array([[0.5, -1.0, 2.0], [0.25, 3.0, 2.0], [0.5, -1.0, 2.0]], dtype)[:n]
    _check(p, _colours(n), 5)
    _check(p, None, 1)


@pytest.mark.parametrize('n', [63, 64, 65, 257, 1025, 70001])
@pytest.mark.parametrize('merge', ['mean', 'first'])
def test_all_rows_in_one_voxel(n, merge):
    p = np.full((n, 3), 0.3, np.float32)
    c = _colours(n, n)
    got, _ = _check(p, c, 10, merge=merge)
    assert got.counts.tolist() == [n] and got.scale == 1.0
    got, _ = _check(np.random.default_rng(n).uniform(-0.49, 0.49, (n, 3)), c, 3, merge=merge, **UNIT)       # one voxel of distinct points
    assert got.coords.tolist() == [[0, 0, 0, 0]]


RUNS = {
    'run_T-1': [3, T - 1, 5], 'run_T': [3, T, 5], 'run_T+1': [3, T + 1, 5], 'run_2T+1': [3, 2 * T + 1, 5],
    'whole_tile': [T, T, 1], 'tile_edges': [T - 1, 1, 1, T - 1, 2 * T],
    'three_workgroups': [10, 2 * T, 7], 'three_workgroups_ragged': [T - 1, T + 2, 1],
    'starts_on_a_last_row': [T - 1, 5, 3], 'starts_on_a_last_row_long': [2 * T - 1, 3 * T, 1],
    'singles': [1] * (2 * T + 3), 'pairs': [2] * (T + 1),
}


@pytest.mark.parametrize('name', sorted(RUNS))
@pytest.mark.parametrize('merge', ['mean', 'first'])
def test_runs_around_the_tile(name, merge):
    p = _runs(RUNS[name], seed=len(name))
    got, _ = _check(p, _colours(len(p), 3), 12, merge=merge, **UNIT)
    assert got.counts.tolist() == RUNS[name]
    _check(p, None, 12, **UNIT)
    _check(_runs(RUNS[name], shuffle=False), np.full((len(p), 3), 255, np.uint8), 12, merge=merge, **UNIT)


def test_colour_sum_past_32_bits():
    """one voxel of 16 843 010 rows of colour 255: 255 x 16 843 010 = 2^32 + 254 is the first such sum that does not fit in 32 bits"""
    n = 16_843_010
    assert 255 * n >= 1 << 32 > 255 * (n - 1)
    p = torch.full((n, 3), 1.5, dtype=torch.float32, device=DEV)
    c = torch.full((n, 3), 255, dtype=torch.uint8, device=DEV)
    got = ops.voxelize(p, c, 10)
    assert got.coords.tolist() == [[0, 0, 0, 0]] and got.counts.tolist() == [n] and got.colours.tolist() == [[255, 255, 255]]
    assert got.voxel_of.shape == (n,) and not bool(got.voxel_of.any()) and got.origin == (1.5, 1.5, 1.5) and got.scale == 1.0


# ---- geometry and values -----------------------------------------------------------------------------------------------------------------
def _cloud(n, seed, spread=1.0, offset=0.0, dtype=np.float64):
    rng = np.random.default_rng(seed)
    p = rng.uniform(-1, 1, (n, 3)) * spread + offset
    p[n // 2:] = p[:n - n // 2] + rng.uniform(-1, 1, (n - n // 2, 3)) * spread * 1e-4      # neighbours: most voxels are met twice
    return p.astype(dtype)


@pytest.mark.parametrize('bits', [1, 2, 7, 10, 20])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_random_clouds(bits, dtype):
    p = _cloud(3001, bits, spread=2.5, offset=-7.0, dtype=dtype)
    got, want = _check(p, _colours(len(p), bits), bits)
    assert int(got.coords[:, 1:].max()) == (1 << bits) - 1 and int(got.coords[:, 1:].min()) == 0
    _check(p, _colours(len(p), bits), bits, merge='first')


def test_far_corner_of_the_lattice():
    top = float((1 << 20) - 1)
    p = np.array([[top, top, top], [0, 0, 0], [top, 0, top], [top - 0.4, top + 0.4, top], [0, top, 0], [top, top, 0], [0.5, 1.5, 2.5]])
    got, _ = _check(p, _colours(len(p)), 20, **UNIT)
    assert got.coords[-1].tolist() == [0] + [(1 << 20) - 1] * 3 and got.counts[-1].item() == 2
    _check(p, _colours(len(p)), 20)                             # the default frame: scale = (2^20 - 1) / (2^20 - 1)


@pytest.mark.parametrize('offset', [1e9, -1e9, -123456.789, 1e15])
def test_huge_and_negative_offsets(offset):
    rng = np.random.default_rng(7)
    p = offset + np.rint(rng.uniform(0, 2000, (999, 3))) * 1e-3 if abs(offset) < 1e12 else offset + np.rint(rng.uniform(0, 2000, (999, 3)))
    _check(p, _colours(999, 1), 10)
    _check(p, _colours(999, 1), 10, origin=(offset - 1.0,) * 3, scale=0.5 if abs(offset) >= 1e12 else 250.0)


def test_float32_equals_its_widening():
    p = _cloud(2049, 11, spread=0.37, offset=3.0, dtype=np.float32)
    c = _colours(len(p), 2)
    a = ops.voxelize(_dev(p), _dev(c), 9)
    b = ops.voxelize(_dev(p.astype(np.float64)), _dev(c), 9)
    for x, y in zip(a[:4], b[:4]):
        assert torch.equal(x, y)
    assert a[4:] == b[4:]
    _same(a, V.voxelize(p, c, 9))


def test_denormals():
    tiny = np.float32(1e-45)                                    # the smallest float32 denormal, 2^-149
    p = (np.random.default_rng(3).integers(0, 5000, (700, 3)).astype(np.float32) * tiny).astype(np.float32)
    assert p.max() < np.finfo(np.float32).tiny and p.max() > 0
    got, _ = _check(p, _colours(700, 4), 8)
    assert len(got.counts) > 200
    _check(-p, None, 8)
    j = np.random.default_rng(4).integers(0, 4, (300, 3)).astype(np.float64)
    p64 = j * 2.0 ** -1024                                      # float64 denormals; times 2^1023 they are j / 2: ties among them
    assert p64.max() < np.finfo(np.float64).tiny
    got, _ = _check(p64, _colours(300, 5), 2, origin=(0.0, 0.0, 0.0), scale=2.0 ** 1023)
    assert sorted(set(got.coords[:, 1].tolist())) == [0, 1, 2]
    with pytest.raises(ValueError, match='scale'):              # their default frame has no finite scale
        ops.voxelize(_dev(p64), None, 10)


def test_planar_cloud_and_single_point():
    p = np.zeros((500, 3))
    p[:, 1] = np.random.default_rng(5).uniform(-3, 9, 500)
    p[:, 0], p[:, 2] = 4.25, -1e3
    got, _ = _check(p, _colours(500, 6), 6)
    assert not got.coords[:, [0, 1, 3]].any() and int(got.coords[:, 2].max()) == 63
    got, _ = _check(np.array([[1e9, -2.5, 1e-9]]), _colours(1), 10)
    assert got.scale == 1.0 and got.origin == (1e9, -2.5, 1e-9) and got.coords.tolist() == [[0, 0, 0, 0]]
    got, _ = _check(np.array([[-0.0, 0.0, -0.0], [0.0, -0.0, -0.0]]), None, 10)
    assert str(got.origin) == '(0.0, 0.0, 0.0)'


def test_ties_go_to_even():
    k = np.arange(0, 600, dtype=np.float64)
    p = np.stack([k + 0.5, k[::-1] + 0.5, np.full(600, 2.5)], 1)
    got, _ = _check(p, _colours(600, 7), 10, **UNIT)
    assert not (got.coords[:, 1:] & 1).any()
    _check(p.astype(np.float32), None, 10, **UNIT)
    _check(p * 0.125, None, 10, origin=(0.0, 0.0, 0.0), scale=8.0)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    p = _cloud(1000, 8)
    p[[3, 500, 999]] += 100.0
    frame = V.voxelize(p[np.setdiff1d(np.arange(1000), [3, 500, 999])], None, 8)
    with pytest.raises(ValueError, match=r'3 of 1000 rows fall outside'):
        ops.voxelize(_dev(p), None, 8, origin=frame.origin, scale=frame.scale)
    with pytest.raises(ValueError, match=r'3 of 1000 rows fall outside'):
        V.voxelize(p, None, 8, origin=frame.origin, scale=frame.scale)
    with pytest.raises(ValueError, match=r'1 of 2 rows fall outside'):
        ops.voxelize(_dev(np.array([[0.0, 0, 0], [-0.51, 0, 0]])), None, 8, **UNIT)
    bad = _cloud(777, 9, dtype=np.float32)
    bad[5, 0], bad[5, 1], bad[300, 2], bad[776, 1], bad[12, 0] = np.nan, np.inf, -np.inf, np.inf, np.nan
    for q in (bad, bad.astype(np.float64)):
        with pytest.raises(ValueError, match=r'4 of 777 rows hold a NaN or an infinity'):
            ops.voxelize(_dev(q), _dev(_colours(777)), 8)
        with pytest.raises(ValueError, match=r'4 of 777 rows hold a NaN or an infinity'):
            ops.voxelize(_dev(q), None, 8, **UNIT)
    ok = _dev(_cloud(10, 1))
    for kw in (dict(bits=0), dict(bits=21), dict(bits=True), dict(bits=8, merge='median'), dict(bits=8, scale=0.0), dict(bits=8, scale=float('inf')),
               dict(bits=8, origin=(0.0, float('nan'), 0.0))):
        with pytest.raises(ValueError):
            ops.voxelize(ok, None, **kw)
    with pytest.raises(ValueError):
        ops.voxelize(ok.to(torch.float16), None, 8)
    with pytest.raises(ValueError):
        ops.voxelize(ok, torch.zeros((9, 3), dtype=torch.uint8, device=DEV), 8)
    with pytest.raises(Exception):
        ops.voxelize(ok.cpu(), None, 8)
    L = lib()
    assert L.pcgc_voxelize_bounds(1, 0, 1 << 31, 1, 1, 1, 1 << 20, None) == -2     # refused before any pointer is looked at
    assert L.pcgc_voxelize_quantize(1, 0, 1 << 31, 10, 0.0, 0.0, 0.0, 1.0, 1, 1, 1, None) == -2
    assert L.pcgc_voxelize_heads(1, 1, 1 << 31, 10, 1, 1, 1, 1, 1 << 40, None) == -2
    assert L.pcgc_voxelize_merge(1, 1, 1, 1 << 31, 1, None, 0, 1, 1, 1, None, 1, 1 << 40, None) == -2


def test_no_rows():
    got = ops.voxelize(torch.empty((0, 3), dtype=torch.float32, device=DEV), torch.empty((0, 3), dtype=torch.uint8, device=DEV), 10)
    _same(got, V.voxelize(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8), 10))
    assert got.coords.shape == (0, 4) and got.colours.shape == (0, 3)
    assert ops.voxelize(torch.empty((0, 3), dtype=torch.float64, device=DEV), None, 10).colours is None


# ---- modes, strides, order ---------------------------------------------------------------------------------------------------------------
def test_first_against_mean():
    p = _runs([4, 1, 7, 300], seed=2)
    c = _colours(len(p), 8)
    first, _ = _check(p, c, 4, merge='first', **UNIT)
    mean, _ = _check(p, c, 4, merge='mean', **UNIT)
    assert not torch.equal(first.colours, mean.colours) and torch.equal(first.coords, mean.coords) and torch.equal(first.voxel_of, mean.voxel_of)
    lowest = [int(np.flatnonzero(p[:, 0] + 2 * p[:, 1] + 4 * p[:, 2] == k)[0]) for k in range(4)]
    assert first.colours.tolist() == c[lowest].tolist()


def test_strided_inputs_are_read_right():
    p, c = _cloud(1500, 12, dtype=np.float32), _colours(1500, 9)
    wide_p = torch.zeros((1500, 7), dtype=torch.float32, device=DEV)
    wide_c = torch.full((3000, 4), 9, dtype=torch.uint8, device=DEV)
    wide_p[:, 2:5], wide_c[::2, 1:] = _dev(p), _dev(c)
    view_p, view_c = wide_p[:, 2:5], wide_c[::2, 1:]
    assert not view_p.is_contiguous() and not view_c.is_contiguous()
    _same(ops.voxelize(view_p, view_c, 6), V.voxelize(p, c, 6))
    _same(ops.voxelize(_dev(p).t().contiguous().t(), view_c, 6), V.voxelize(p, c, 6))       # column-major points


def test_row_order_and_repeatability():
    p, c = _cloud(5000, 13), _colours(5000, 10)
    a, _ = _check(p, c, 5)
    again = ops.voxelize(_dev(p), _dev(c), 5)
    for x, y in zip(a[:4], again[:4]):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    assert a[4:] == again[4:] and vox.pack_frame(a.bits, a.origin, a.scale) == vox.pack_frame(again.bits, again.origin, again.scale)
    perm = np.random.default_rng(14).permutation(5000)
    b, _ = _check(p[perm], c[perm], 5)                          # voxel_of is the definition's for the shuffled rows
    assert torch.equal(a.coords, b.coords) and torch.equal(a.counts, b.counts) and torch.equal(a.colours, b.colours) and a[4:] == b[4:]
    assert np.array_equal(b.voxel_of.cpu().numpy(), a.voxel_of.cpu().numpy()[perm])
    back = vox.devoxelize(a.coords, a.origin, a.scale)
    assert back.dtype == torch.float64 and np.array_equal(back.cpu().numpy(), V.devoxelize(a.coords.cpu().numpy(), a.origin, a.scale))


# ---- end to end: a jittered shell in front of the two CLIs ------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def raw_cloud(tmp_path_factory):
    """shell7's voxels, two float32 points in each (in metres, off the origin), with colours, as a binary little-endian PLY"""
    d = tmp_path_factory.mktemp('voxelize')
    cells = synthetic.shell('shell7').numpy().astype(np.float64)
    rng = np.random.default_rng(21)
    p = np.concatenate([cells + rng.uniform(-0.3, 0.3, cells.shape) for _ in range(2)])
    p = ((p - cells.min(0)) * (127.0 / (cells.max(0) - cells.min(0)).max()) * 0.01 + np.array([12.5, -3.0, 0.75])).astype(np.float32)
    order = rng.permutation(len(p))
    p, c = p[order], rng.integers(0, 256, (len(p), 3)).astype(np.uint8)
    rows = np.zeros(len(p), dtype=[('x', '<f4'), ('y', '<f4'), ('z', '<f4'), ('red', 'u1'), ('green', 'u1'), ('blue', 'u1')])
    for j, name in enumerate('xyz'):
        rows[name] = p[:, j]
    for j, name in enumerate(('red', 'green', 'blue')):
        rows[name] = c[:, j]
    path = str(d / 'raw.ply')
    with open(path, 'wb') as f:
        f.write(('ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n'
                 'property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n' % len(p)).encode())
        rows.tofile(f)
    ckpt = str(d / 'synthetic.pth')
    torch.save({'model': synthetic.synthetic_state_dict(gain=50.0)}, ckpt)
    xyz, rgb = read_ply_with_colours(path)
    assert np.array_equal(xyz, p.astype(np.float64)) and np.array_equal(rgb, c)
    return d, path, ckpt, xyz, V.voxelize(xyz, rgb, 7)


def _read_units(path):
    """`_dec_units.ply` through Python's float(), which reads every double back exactly -> (float64 [n,3], uint8 [n,3] or None)"""
    with open(path) as f:
        lines = f.read().split('\n')
    data = np.array([[float(t) for t in line.split()] for line in lines[lines.index('end_header') + 1:] if line], np.float64)
    return data[:, :3], data[:, 3:].astype(np.uint8) if data.shape[1] == 6 else None


def _by_voxel(xyz):
    xyz = np.asarray(xyz).astype(np.int64)
    return np.argsort((xyz[:, 2] << 40) | (xyz[:, 1] << 20) | xyz[:, 0], kind='stable')


def test_attributes_cli_returns_the_merged_colours(raw_cloud, capsys):
    d, raw, _, _, want = raw_cloud
    out = str(d / 'attr')
    attributes.main(['--filedir', raw, '--outdir', out, '--voxelize', '7', '--qstep', '0', '--devoxelize'])
    text = capsys.readouterr().out
    assert f'{len(want.voxel_of)} points -> {len(want.counts)} voxels at 7 bits' in text and '_V.bin:\t 384 bits' in text
    assert vox.read_frame(os.path.join(out, 'raw_V.bin')) == (7, tuple(want.origin.tolist()), want.scale)
    for name in ('raw_vox.ply', 'raw_vox_dec.ply'):             # the voxelised cloud, and what the codec returns at quantiser 0
        xyz, rgb = read_ply_ascii_with_colours(os.path.join(out, name))
        assert np.array_equal(xyz, want.coords[:, 1:]) and np.array_equal(rgb, want.colours)
    units, rgb = _read_units(os.path.join(out, 'raw_dec_units.ply'))
    assert np.array_equal(units, V.devoxelize(want.coords, want.origin, want.scale)) and np.array_equal(rgb, want.colours)
    assert want.counts.max() >= 2 and not np.array_equal(want.colours, V.voxelize(raw_cloud[3], read_ply_with_colours(raw)[1], 7, merge='first').colours)


def test_lossless_cli_returns_the_voxel_set(raw_cloud, capsys):
    d, raw, ckpt, points, want = raw_cloud
    out = str(d / 'lossless')
    coder.main(['--ckptdir', ckpt, '--filedir', raw, '--outdir', out, '--lossless', '--voxelize', '7', '--merge', 'first', '--devoxelize'])
    text = capsys.readouterr().out
    assert 'lossless:\t exact' in text and '_V.bin:\t 384 bits' in text
    voxels = read_ply_ascii_geo(os.path.join(out, 'raw_vox.ply'))
    decoded = read_ply_ascii_geo(os.path.join(out, 'raw_vox_dec.ply'))
    assert np.array_equal(voxels, want.coords[:, 1:])
    assert np.array_equal(decoded[_by_voxel(decoded)], voxels[_by_voxel(voxels)])
    bits, origin, scale = vox.read_frame(os.path.join(out, 'raw_V.bin'))
    units, _ = _read_units(os.path.join(out, 'raw_dec_units.ply'))
    assert len(units) == len(want.counts) and bits == 7
    units = units[_by_voxel(decoded)]                           # row j: the position of voxel j of the definition
    assert np.abs(units[want.voxel_of] - points).max() <= 0.5 / scale          # every input point lies in the cell of its decoded voxel
    assert np.bincount(want.voxel_of, minlength=len(units)).min() >= 1         # and every decoded point has such an input point
