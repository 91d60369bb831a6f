"""Cleaning a voxelised cloud on the GPU (csrc/clean.hip, pcgcv2_amd/clean.py): keep, neighbours, labels, sizes, the kept rows and colours and
every count EQUAL to the numpy definition (tests/clean_reference.py), no tolerance, at the smallest shapes at which the kernels can go
wrong: one and two rows, a folded path whose smallest row sits at its far end, interleaved components, 65 537 singletons, components across
the multiples of a wave and a workgroup, two batch items in one place, the corners of the lattice; then the three CLIs with `--clean`."""
import os

import numpy as np
import pytest
import torch

import clean_reference as R
import scratch_arena as SA
import voxelize_reference as V
from pcgcv2_amd import attributes, clean, coder, ops, synthetic, voxelize as vox
from pcgcv2_amd._lib import PcgcError, lib
from pcgcv2_amd.data_utils import read_ply_ascii_geo, read_ply_ascii_with_colours, write_ply_ascii_geo_rgb

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
FIELDS = ('keep', 'neighbours', 'labels', 'sizes', 'coords', 'colours')


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _rows(xyz, batch=0):
    xyz = np.asarray(xyz, np.int32).reshape(-1, 3)
    return np.concatenate([np.full((len(xyz), 1), batch, np.int32), xyz], 1)


def _colours(n, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (n, 3)).astype(np.uint8)


def _same(got, want):
    assert got.keep.dtype == torch.bool and got.neighbours.dtype == got.labels.dtype == got.sizes.dtype == got.coords.dtype == torch.int32
    for name in FIELDS:
        g, w = getattr(got, name), getattr(want, name)
        if w is None:
            assert g is None, name
        else:
            assert np.array_equal(g.cpu().numpy(), w), name
    assert (got.removed_density, got.removed_component, got.n_components) == (want.removed_density, want.removed_component, want.n_components)
    if want.colours is not None:
        assert got.colours.dtype == torch.uint8


def _check(c, colours=None, **kw):
    want = R.clean(c, colours, **kw)
    got = ops.clean(_dev(c), _dev(colours), **kw)
    _same(got, want)
    assert got.rounds <= len(c) - want.removed_density + 1                      # (the cap of the labelling rounds)
    return got, want


_NAMED = {}


def _named(name, order='raster'):
    """(rows, the definition's result with the defaults), computed once"""
    if (name, order) not in _NAMED:
        c = _rows(synthetic.cloud(name, order=order, seed=3).numpy())
        _NAMED[name, order] = (c, R.clean(c, None))
    return _NAMED[name, order]


# ---- one and two rows ---------------------------------------------------------------------------------------------------------------------
def test_one_row():
    got, _ = _check(_rows([[5, 6, 7]]), _colours(1))
    assert got.labels.tolist() == [0] and got.sizes.tolist() == [1] and got.neighbours.tolist() == [0] and got.n_components == 1
    got, _ = _check(_rows([[5, 6, 7]]), None, min_neighbours=1)
    assert got.labels.tolist() == [-1] and got.coords.shape == (0, 4) and got.n_components == 0


@pytest.mark.parametrize('second,components', [((4, 3, 3), 1), ((3, 3, 4), 1), ((4, 4, 4), 1), ((2, 4, 2), 1), ((5, 3, 3), 2), ((5, 5, 5), 2), ((4, 4, 5), 2)],
                         ids=['face_x', 'face_z', 'corner', 'corner_mixed', 'two_apart', 'two_apart_diagonal', 'two_apart_in_z'])
def test_two_rows(second, components):
    for c in (_rows([(3, 3, 3), second]), _rows([second, (3, 3, 3)])):
        got, _ = _check(c, None, r2=3)
        assert got.n_components == components and got.labels.tolist() == ([0, 0] if components == 1 else [0, 1])
        _check(c, _colours(2), min_component=2)


def test_no_rows():
    got = ops.clean(torch.empty((0, 4), dtype=torch.int32, device=DEV), torch.empty((0, 3), dtype=torch.uint8, device=DEV), min_neighbours=2)
    _same(got, R.clean(np.zeros((0, 4), np.int32), np.zeros((0, 3), np.uint8), min_neighbours=2))
    assert ops.connected_components(torch.empty((0, 4), dtype=torch.int32, device=DEV))[2] == 0


# ---- a folded path ------------------------------------------------------------------------------------------------------------------------
def _snake(n, W=15, H=16):
    """a path of n voxels, one voxel thick, folded into a box: lines along x two apart in y, U-turns through one voxel set diagonally outside
    the line ends, layers two apart in z joined through one voxel set diagonally outside the layer: no two voxels of the path touch
    (26-connectivity) but consecutive ones"""
    out, z, up = [], 0, True
    x_at = 1                                                                   # the end of the line the walk stands on: 1 or W
    while len(out) < n:
        lines = range(H) if up else range(H - 1, -1, -1)
        for t, j in enumerate(lines):
            y = 2 * j + 1
            xs = range(1, W + 1) if x_at == 1 else range(W, 0, -1)
            out += [(x, y, z) for x in xs]
            x_at = W if x_at == 1 else 1
            if t < H - 1:
                out.append((x_at + (1 if x_at == W else -1), y + (1 if up else -1), z))
        out.append((x_at + (1 if x_at == W else -1), y + (1 if up else -1), z + 1))
        z, up = z + 2, not up
    return np.array(out[:n], np.int32)


def test_snake_jumping_works():
    n = 4097
    path = _snake(n)
    c = _rows(path[::-1])                                                      # reversed: the smallest row sits at the far end
    a, b = R._pairs(c[:, 1:].astype(np.int64), R.FORWARD13)
    assert len(a) == n - 1 and np.bincount(np.concatenate([a, b]), minlength=n).max() == 2         # a path graph: propagation alone needs 4 096 rounds
    got, want = _check(c)
    assert want.n_components == 1 and got.labels.unique().tolist() == [0] and got.sizes.unique().tolist() == [n]
    assert got.rounds < n + 1                                                  # the cap was not reached,
    assert got.rounds < n // 4                                                 # and pointer jumping did its work
    print(f'snake of {n}: {got.rounds} rounds')


def _rings():
    """two interleaved spirals in one plane: A holds the square rings of radius 2, 6, 10, ..., B those of radius 4, 8, 12, ...; the rings of A
    are joined along x = 0 on the top side through three-voxel gaps in B's rings, those of B on the bottom side through gaps in A's"""
    a, b, o = [], [], 30
    for k in range(2, 26, 2):
        mine, top_gap = (a, False) if k % 4 == 2 else (b, True)
        for t in range(-k, k + 1):
            for p in ((t, k), (t, -k), (k, t), (-k, t)):
                if abs(p[0]) <= 1 and p[1] == (k if top_gap else -k):
                    continue
                mine.append(p)
        if k + 4 < 26:
            mine += [(0, s * y) for y in range(k, k + 5) for s in ((1,) if not top_gap else (-1,))]
    f = lambda pts: np.unique(np.array([(x + o, y + o, 7) for x, y in pts], np.int32), axis=0)
    return f(a), f(b)


def test_interleaved_spirals_stay_two():
    a, b = _rings()
    assert np.abs(a[:, None, :] - b[None, :, :]).max(2).min() == 2             # never closer than Chebyshev distance 2
    both = np.concatenate([a, b])
    c = _rows(both[np.random.default_rng(5).permutation(len(both))])
    got, want = _check(c, None, r2=4)
    assert want.n_components == 2 and sorted(got.sizes.unique().tolist()) == sorted([len(a), len(b)])
    _check(c, _colours(len(c)), keep_largest=1)


# ---- row counts ---------------------------------------------------------------------------------------------------------------------------
def test_65537_singletons():
    g = np.arange(41) * 2
    xyz = np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3)
    xyz = xyz[np.random.default_rng(6).permutation(len(xyz))[:65537]]
    got, _ = _check(_rows(xyz), None, r2=3)
    assert got.n_components == 65537 and got.sizes.unique().tolist() == [1] and got.rounds == 1
    assert torch.equal(got.labels, torch.arange(65537, dtype=torch.int32, device=DEV)) and not got.neighbours.any()
    got, _ = _check(_rows(xyz), None, min_component=2)
    assert got.coords.shape == (0, 4) and got.removed_component == 65537


def test_components_across_waves_and_workgroups():
    n = 1100
    joined = {63, 127, 255, 256, 511, 767, 1023}                               # row r and row r + 1 touch: pairs across 64, 128, 256, 512, 768, 1024
    gaps = np.array([1 if r in joined else 3 for r in range(n - 1)])
    x = np.concatenate([[0], np.cumsum(gaps)])
    c = _rows(np.stack([x, np.full(n, 2), np.full(n, 2)], 1))
    got, want = _check(c, None, r2=1, min_component=2)
    assert want.n_components == n - len(joined) and got.keep.sum().item() == 2 * len(joined) - 1         # 255-256-257 is one of three
    long = _rows(np.stack([np.arange(700), np.full(700, 9), np.full(700, 9)], 1))                        # one bar across three workgroups,
    both = np.concatenate([long[::-1], c + np.array([0, 0, 20, 0], np.int32)])                           # its rows descending
    _check(both, _colours(len(both)), r2=2, min_component=3, keep_largest=2)


def test_two_batch_items_in_one_place():
    xyz, _ = _named('noisy_s')
    xyz = xyz[::3, 1:]
    c = np.concatenate([_rows(xyz, 0), _rows(xyz[: len(xyz) // 2], 3), _rows(xyz[5:60], 15)])
    c = c[np.random.default_rng(8).permutation(len(c))]
    got, _ = _check(c, _colours(len(c)), r2=9, min_neighbours=1)
    lab = got.labels.cpu().numpy()
    assert (c[lab[lab >= 0], 0] == c[lab >= 0, 0]).all()                       # no component crosses the items
    got, want = _check(c, None, keep_largest=1)                                # the largest of EACH item stays
    assert sorted(np.unique(want.coords[:, 0]).tolist()) == [0, 3, 15] and len(np.unique(want.labels[want.keep])) == 3
    _check(c, None, keep_largest=3, min_component=2)


def test_corners_of_the_lattice_do_not_wrap():
    top = (1 << 20) - 1
    corners = [(x, y, z) for x in (0, top) for y in (0, top) for z in (0, top)]
    inward = [tuple(1 if v == 0 else top - 1 for v in p) for p in corners]     # one voxel diagonally inside each corner
    edge = [(0, 5, 5), (top, 5, 5), (5, 0, 5), (5, top, 5), (5, 5, 0), (5, 5, top), (top, 6, 6), (0, 6, 4)]
    c = _rows(corners + inward + edge)
    for r2 in (1, 64, 3):
        got, want = _check(c, None, r2=r2)
    assert want.n_components == 8 + 6 and want.neighbours.max() == 1           # x = 0 and x = 2^20 - 1 are not adjacent (r2 = 3)
    _check(np.concatenate([c, _rows(corners[:7], 15)]), None, r2=3, min_component=2)       # (batch 15's far corner is the empty key: left out)


# ---- the project's own clouds -------------------------------------------------------------------------------------------------------------
def _partition(c, labels):
    """per voxel, in voxel order: the smallest voxel key of its component"""
    key = (c[:, 3].astype(np.int64) << 40) | (c[:, 2].astype(np.int64) << 20) | c[:, 1]
    least = np.full(len(c), np.iinfo(np.int64).max)
    np.minimum.at(least, labels, key)
    return least[labels][np.argsort(key)]


@pytest.mark.parametrize('name', ['multi_s', 'noisy_s'])
def test_named_clouds_raster_and_shuffled(name):
    parts = []
    for order in ('raster', 'shuffled'):
        c, want = _named(name, order)
        got = ops.clean(_dev(c))
        _same(got, want)
        labels, sizes, n = ops.connected_components(_dev(c))
        assert torch.equal(labels, got.labels) and torch.equal(sizes, got.sizes) and n == got.n_components
        lab = labels.cpu().numpy()
        assert (lab <= np.arange(len(c))).all() and (lab[lab] == lab).all()    # the labels follow the order: the smallest row of each component
        parts.append(_partition(c, lab))
        print(f'{name} {order}: {got.n_components} components in {got.rounds} rounds')
    assert np.array_equal(parts[0], parts[1])                                  # the same components as sets
    assert got.n_components == {'multi_s': 3, 'noisy_s': 843}[name]


@pytest.mark.parametrize('r2', [1, 3, 16, 64])
def test_neighbours_at_every_reach(r2):
    c, _ = _named('noisy_s', 'shuffled')
    got, want = _check(c, None, r2=r2, min_neighbours=3, min_component=4)
    assert want.neighbours.max() > (2, 8, 30, 100)[(1, 3, 16, 64).index(r2)]


def test_min_neighbours_at_and_above_a_rows_count():
    c, base = _named('noisy_s')
    row = int(np.flatnonzero(base.neighbours == 6)[0])
    at, _ = _check(c, None, min_neighbours=6)
    above, _ = _check(c, None, min_neighbours=7)
    assert at.labels[row].item() >= 0 and at.keep[row].item() and above.labels[row].item() == -1 and not above.keep[row].item()
    assert above.removed_density > at.removed_density


def test_identity_with_the_normals_moments():
    for name in ('noisy_s', 'multi_s'):
        c, _ = _named(name, 'shuffled')
        for r2 in (5, 16):
            k = ops.estimate_normals(_dev(c), r2, want_moments=True)[4][:, 0]
            assert torch.equal(ops.clean(_dev(c), r2=r2).neighbours.to(torch.int64), k - 1)


def test_colours_strides_and_repeatability():
    c, _ = _named('noisy_s', 'shuffled')
    rgb = _colours(len(c), 4)
    kw = dict(r2=16, min_neighbours=4, min_component=8, keep_largest=2)
    a, want = _check(c, rgb, **kw)
    assert 0 < len(want.coords) < len(c) and np.array_equal(want.colours, rgb[want.keep])
    b = ops.clean(_dev(c), _dev(rgb), **kw)
    for name in FIELDS:
        assert getattr(a, name).cpu().numpy().tobytes() == getattr(b, name).cpu().numpy().tobytes(), name
    assert a[6:] == b[6:]
    wide = torch.zeros((len(c), 9), dtype=torch.int32, device=DEV)
    wide[:, 3:7] = _dev(c)
    wide_c = torch.zeros((len(c), 4), dtype=torch.uint8, device=DEV)
    wide_c[:, 1:] = _dev(rgb)
    assert not wide[:, 3:7].is_contiguous()
    _same(ops.clean(wide[:, 3:7], wide_c[:, 1:], **kw), want)
    _same(clean.clean(_dev(c), _dev(rgb), **kw), want)


def test_refusals():
    ok = _rows([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0]])
    dup = ok.copy()
    dup[2], dup[3] = dup[0], dup[0]
    with pytest.raises(ValueError, match='2 of 4 rows repeat'):
        ops.clean(_dev(dup))
    with pytest.raises(ValueError, match='2 of 4 rows repeat'):
        ops.connected_components(_dev(dup))
    far = ok.copy()
    far[1, 1], far[2, 3] = 1 << 20, -1
    with pytest.raises(ValueError, match='2 of 4 rows are outside'):
        ops.clean(_dev(far))
    far[0, 0] = 16
    with pytest.raises(ValueError, match='3 of 4 rows are outside'):
        ops.connected_components(_dev(far))
    for kw in (dict(r2=0), dict(r2=65), dict(r2=True), dict(r2=4.0), dict(min_neighbours=-1), dict(min_component=0), dict(keep_largest=-1)):
        with pytest.raises(ValueError, match=list(kw)[0]):
            ops.clean(_dev(ok), **kw)
    with pytest.raises(ValueError, match='colours'):
        ops.clean(_dev(ok), torch.zeros((3, 3), dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match='int32'):
        ops.clean(_dev(ok).to(torch.int64))
    with pytest.raises(PcgcError):
        ops.clean(torch.from_numpy(ok))
    with pytest.raises(ValueError, match='16777217 rows'):
        ops.clean(torch.zeros((1, 1), dtype=torch.int32, device=DEV).expand((1 << 24) + 1, 4))
    nbr = ops.kmap_k3(_dev(ok), 1, ops.HashTable(_dev(ok), 1))
    labels, sizes, n, rounds = ops.components(nbr)
    assert (labels.tolist(), sizes.tolist(), n) == ([0, 0, 0, 0], [4, 4, 4, 4], 1) and rounds >= 2
    need = int(lib().pcgc_components_workspace_bytes(4))
    before = labels.clone()
    out = torch.full((4,), 77, dtype=torch.int32, device=DEV)
    import ctypes
    h = [ctypes.c_int64(7), ctypes.c_int32(7)]
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    rc = lib().pcgc_components(nbr.data_ptr(), 4, out.data_ptr(), out.data_ptr(), *[ctypes.byref(v) for v in h], ws.data_ptr(), need - 1, None)
    torch.cuda.synchronize()
    assert rc == -2 and out.tolist() == [77] * 4 and not ws.any() and [v.value for v in h] == [7, 7] and torch.equal(labels, before)


def test_recycled_scratch_and_guard_bands():
    """one run on fresh memory, one on the blocks an other cloud's run left behind: the same bytes, every guard intact"""
    kw = dict(r2=16, min_neighbours=4, min_component=8, keep_largest=3)
    (a, _), (b, _) = _named('multi_s', 'shuffled'), _named('noisy_s', 'shuffled')
    a = a[:len(b)] if len(a) > len(b) else np.concatenate([a, a[:len(b) - len(a)] + np.array([1, 0, 0, 0], np.int32)])       # as many rows as b
    rgb = _colours(len(b), 2)
    run = lambda c: ops.clean(_dev(c), _dev(rgb), **kw)
    want = R.clean(b, rgb, **kw)
    run(a)
    fresh, rec = SA.Arena(), SA.Arena()
    outs = []
    for arena, cloud in ((fresh, b), (rec, a)):
        with SA.installed(arena):
            outs.append(run(cloud))
        torch.cuda.synchronize()
        arena.finish()
        arena.check()
    sized_by_the_data = ('compact_coords', 'compact_index', 'kmap_k3', 'components', '__init__', 'clean', '_components_of')
    stale = rec.replay(fresh_ok=sized_by_the_data)
    with SA.installed(stale):
        got = run(b)
    torch.cuda.synchronize()
    stale.finish()
    for arena in (fresh, rec, stale):
        arena.check()
    _same(got, want)
    _same(outs[0], want)
    allocs, replayed, _ = stale.stats()
    assert allocs > 20 and replayed >= 15 and all(caller in sized_by_the_data for _, caller, _, _ in stale.served_fresh)


# ---- end to end: the three CLIs ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def noisy_ply(tmp_path_factory):
    d = tmp_path_factory.mktemp('clean')
    c, _ = _named('noisy_s', 'shuffled')
    rgb = _colours(len(c), 11)
    path = str(d / 'noisy.ply')
    write_ply_ascii_geo_rgb(path, c[:, 1:], rgb)
    ckpt = str(d / 'synthetic.pth')
    torch.save({'model': synthetic.synthetic_state_dict(gain=50.0)}, ckpt)
    return d, path, ckpt, c, rgb


def _by_voxel(xyz):
    xyz = np.asarray(xyz).astype(np.int64)
    return np.argsort((xyz[:, 2] << 40) | (xyz[:, 1] << 20) | xyz[:, 0], kind='stable')


def test_clean_cli(noisy_ply, capsys):
    d, path, _, c, rgb = noisy_ply
    want = R.clean(c, rgb, 16, 4, 8, 0)
    out = str(d / 'own_clean.ply')
    assert clean.main(['--filedir', path, '--min_neighbours', '4', '--min_component', '8', '--out', out]) == 0
    text = capsys.readouterr().out
    assert (f'{len(c)} rows in, {want.removed_density} removed by density, {want.removed_component} removed by component, '
            f'{want.n_components} components, {len(want.coords)} rows out') in text and want.removed_density == 480
    xyz, colours = read_ply_ascii_with_colours(out)
    assert np.array_equal(xyz, want.coords[:, 1:]) and np.array_equal(colours, want.colours)
    clean.main(['--filedir', path, '--r2', '9', '--keep_largest', '1'])
    xyz, colours = read_ply_ascii_with_colours(str(d / 'noisy_clean.ply'))
    largest = R.clean(c, rgb, 9, 0, 1, 1)
    assert np.array_equal(xyz, largest.coords[:, 1:]) and np.array_equal(colours, largest.colours) and len(xyz) == 10204
    capsys.readouterr()


def test_voxelize_and_attributes_cli_with_clean(noisy_ply, capsys):
    d, path, _, c, rgb = noisy_ply
    v = V.voxelize(c[:, 1:].astype(np.float64), rgb, 7, origin=(0.0, 0.0, 0.0), scale=1.0)      # noisy_s lives on a 128 grid: the identity
    want = R.clean(v.coords, v.colours, 16, 4, 8, 0)
    assert 0 < len(want.coords) < len(v.coords) == len(c)
    out = str(d / 'v.ply')
    assert vox.main(['--filedir', path, '--bits', '7', '--origin', '0,0,0', '--scale', '1', '--out', out, '--clean', '4,8']) == 0
    assert f'{want.removed_density} removed by density, {want.removed_component} removed by component' in capsys.readouterr().out
    xyz, colours = read_ply_ascii_with_colours(str(d / 'v_clean.ply'))
    assert np.array_equal(xyz, want.coords[:, 1:]) and np.array_equal(colours, want.colours)
    outdir = str(d / 'attr')
    attributes.main(['--filedir', out, '--outdir', outdir, '--clean', '4,8', '--qstep', '0'])
    assert f'{len(want.coords)} rows out' in capsys.readouterr().out
    for name in ('v_clean.ply', 'v_clean_dec.ply'):                           # the cleaned cloud, and what the codec returns at quantiser 0
        xyz, colours = read_ply_ascii_with_colours(os.path.join(outdir, name))
        assert np.array_equal(xyz, want.coords[:, 1:]) and np.array_equal(colours, want.colours), name
    largest = R.clean(c, rgb, 16, 0, 1, 1)                                     # the shuffled file itself, the largest component only
    attributes.main(['--filedir', path, '--outdir', outdir, '--clean', '0,1', '--keep_largest', '1', '--qstep', '0'])
    xyz, colours = read_ply_ascii_with_colours(os.path.join(outdir, 'noisy_clean_dec.ply'))
    o, w = _by_voxel(xyz), _by_voxel(largest.coords[:, 1:])                    # (the codec returns its own row order)
    assert np.array_equal(xyz[o], largest.coords[w, 1:]) and np.array_equal(colours[o], largest.colours[w])
    capsys.readouterr()


def test_coder_cli_codes_the_cleaned_cloud(noisy_ply, capsys):
    d, path, ckpt, c, rgb = noisy_ply
    want = R.clean(c, None, 16, 4, 8, 0)
    outdir = str(d / 'lossless')
    coder.main(['--ckptdir', ckpt, '--filedir', path, '--outdir', outdir, '--lossless', '--clean', '4,8'])
    text = capsys.readouterr().out
    assert 'lossless:\t exact' in text and f'{len(want.coords)} rows out' in text
    cleaned = read_ply_ascii_geo(os.path.join(outdir, 'noisy_clean.ply'))
    decoded = read_ply_ascii_geo(os.path.join(outdir, 'noisy_clean_dec.ply'))
    assert np.array_equal(cleaned, want.coords[:, 1:])
    assert np.array_equal(decoded[_by_voxel(decoded)], cleaned[_by_voxel(cleaned)])         # the coded cloud is the definition's


def test_voxelize_7_then_clean_4_8_follows_the_definition(noisy_ply, capsys):
    """`--voxelize 7` takes the frame from the bounding box: noisy_s, 71 voxels wide, is stretched by 127 / 71, its surface opens up, and by the
    definition no component of the stretched cloud has 8 rows: 922 rows go by density, the other 10 164 by component.  `_vox_clean.ply` is
    the definition's (empty) cloud, and the codec is not started on it."""
    d, path, ckpt, c, rgb = noisy_ply
    v = V.voxelize(c[:, 1:].astype(np.float64), rgb, 7)
    want = R.clean(v.coords, v.colours, 16, 4, 8, 0)
    assert (len(v.coords), want.removed_density, want.removed_component, len(want.coords)) == (11086, 922, 10164, 0)
    for main, argv in ((coder.main, ['--ckptdir', ckpt, '--lossless']), (attributes.main, ['--qstep', '0'])):
        outdir = str(d / ('stretched_' + main.__module__.split('.')[-1]))
        with pytest.raises(ValueError, match='none of the 11086 rows'):
            main(argv + ['--filedir', path, '--outdir', outdir, '--voxelize', '7', '--clean', '4,8'])
        assert '922 removed by density, 10164 removed by component' in capsys.readouterr().out
        xyz, colours = read_ply_ascii_with_colours(os.path.join(outdir, 'noisy_vox.ply'))
        assert np.array_equal(xyz, v.coords[:, 1:]) and np.array_equal(colours, v.colours)
        assert len(read_ply_ascii_geo(os.path.join(outdir, 'noisy_vox_clean.ply'))) == 0
        assert not os.path.exists(os.path.join(outdir, 'noisy_vox_clean_dec.ply'))
    wide = R.clean(v.coords, v.colours, 16, 4, 1, 0)                            # the same stage with M = 1 in front of the colour codec
    outdir = str(d / 'stretched_wide')
    attributes.main(['--filedir', path, '--outdir', outdir, '--voxelize', '7', '--clean', '4,1', '--qstep', '0'])
    for name in ('noisy_vox_clean.ply', 'noisy_vox_clean_dec.ply'):
        xyz, colours = read_ply_ascii_with_colours(os.path.join(outdir, name))
        assert np.array_equal(xyz, wide.coords[:, 1:]) and np.array_equal(colours, wide.colours) and len(xyz) == 11086 - 922, name
    capsys.readouterr()
