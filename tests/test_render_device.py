"""Rendering on the GPU (csrc/render.hip, pcgcv2_amd/render.py): index, depth, mask, image and every metric sum EQUAL to the numpy definition
(tests/render_reference.py), no tolerance, at the smallest shapes at which the kernels can go wrong: no row and one row, rows that share a
pixel at different and at equal depths in both orders, 65 537 rows on one pixel, row counts across the multiples of a wave and of the
splat's workgroup, points across every border, the corners of the coordinate range, two batch items in one place, 64 slices; then the
command lines."""
import math
import os

import numpy as np
import pytest
import torch

import render_reference as R
import scratch_arena as SA
from pcgcv2_amd import coder, ops, render, synthetic
from pcgcv2_amd._lib import PcgcError
from pcgcv2_amd.data_utils import read_ply_ascii_geo, read_ply_ascii_with_colours, write_ply_ascii_geo_rgb

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
FIELDS = ('index', 'depth', 'mask', 'image')


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _rows(xyz, batch=0):
    xyz = np.asarray(xyz, np.int32).reshape(-1, 3)
    return np.concatenate([np.full((len(xyz), 1), batch, np.int32), xyz], 1)


def _colours(n, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (n, 3)).astype(np.uint8)


def _same(got, want):
    assert got.image.dtype == torch.uint8 and got.depth.dtype == got.index.dtype == torch.int32 and got.mask.dtype == torch.bool
    assert got.matrices.dtype == torch.int64 and np.array_equal(got.matrices.cpu().numpy(), want.matrices)
    for name in FIELDS:
        g, w = getattr(got, name).cpu().numpy(), getattr(want, name)
        assert g.shape == w.shape and np.array_equal(g, w), name


def _check(c, colours, views, bits, size, point_size=1, background=(255, 255, 255), B=None):
    want = R.render_views(c, colours, views, bits, size, (point_size - 1) // 2, background, B)
    got = render.render(_dev(c), _dev(colours), views, size, bits, point_size, background, batch_items=B)
    _same(got, want)
    return got, want


# ---- empty and single inputs ------------------------------------------------------------------------------------------------------------
def test_no_rows():
    got, _ = _check(np.zeros((0, 4), np.int32), np.zeros((0, 3), np.uint8), 'faces;30,20', 3, 8, 3, (1, 2, 3))
    assert (got.index == -1).all() and not got.mask.any() and not got.depth.any()
    assert (got.image == torch.tensor([1, 2, 3], dtype=torch.uint8, device=DEV)).all() and got.image.shape == (1, 7, 8, 8, 3)


def test_one_row():
    got, _ = _check(_rows([[5, 6, 7]]), _colours(1), 'faces', 3, 8)
    assert got.mask.sum().item() == 6 and got.index[0, 4, 6, 5].item() == 0 and got.depth[0, 4, 6, 5].item() == 7     # +z: pixel (u, v) = (x, y), d = z
    got, _ = _check(_rows([[5, 6, 7]]), None, 'faces;-40,10', 3, 8, 9)
    assert got.mask[0, 4].sum().item() == 7 * 6                                # 9 x 9 around (5, 6), clipped to 8 x 8


# ---- depth, ties and ordering -------------------------------------------------------------------------------------------------------------
def test_two_rows_on_one_pixel_at_different_depths():
    for c in (_rows([(3, 4, 1), (3, 4, 6)]), _rows([(3, 4, 6), (3, 4, 1)])):
        near = int(np.flatnonzero(c[:, 3] == 1)[0])
        got, _ = _check(c, _colours(2), '+z;-z', 3, 8)
        assert got.index[0, 0, 4, 3].item() == near and got.index[0, 1, 4, 4].item() == 1 - near
        assert got.depth[0, 0, 4, 3].item() == 1 and got.depth[0, 1, 4, 4].item() == 1


def test_equal_depths_keep_the_lower_row():
    for pair in ([(2, 2, 2), (3, 3, 3)], [(3, 3, 3), (2, 2, 2)]):              # half scale: both on pixel (1, 1) at d = 1
        got, _ = _check(_rows(pair), _colours(2), '+z', 3, 4)
        assert got.index[0, 0, 1, 1].item() == 0 and got.mask.sum().item() == 1
    for pair in ([(2, 3, 5), (3, 3, 5)], [(3, 3, 5), (2, 3, 5)]):              # point size 3: the squares overlap in two columns
        got, _ = _check(_rows(pair), _colours(2), '+z', 3, 8, 3)
        cols = {int(pair[r][0]): r for r in (0, 1)}
        assert got.index[0, 0, 3, 2].item() == 0 and got.index[0, 0, 3, 3].item() == 0
        only = {2: 1, 3: 4}                                                    # the column only the row at x = 2 / x = 3 covers
        for x, r in cols.items():
            assert got.index[0, 0, 3, only[x]].item() == r


def test_shuffled_rows_give_the_same_picture():
    pts = synthetic.cloud('shell6').numpy()
    c = _rows(pts)
    n = len(c)
    perm = np.random.default_rng(12).permutation(n)
    views, bits, size, ps = 'faces;30,20;200,-50', 6, 64, 3
    a, want = _check(c, None, views, bits, size, ps)
    b, _ = _check(c[perm], None, views, bits, size, ps)
    for name in ('depth', 'mask', 'image'):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    reverse = R.render_views(c[::-1], None, views, bits, size, 1)
    decided = want.mask & (want.index == n - 1 - reverse.index)               # pixels where one row alone has the least depth
    assert 0 < decided.sum() < want.mask.sum()
    back = np.where(want.mask, perm[np.maximum(b.index.cpu().numpy(), 0)], -1)
    assert np.array_equal(back[decided], want.index[decided])
    rgb = _colours(n, 1)                                                       # distinct voxels, faces at full scale, point size 1: no ties at all
    a, _ = _check(c, rgb, 'faces', bits, size)
    b, _ = _check(c[perm], rgb[perm], 'faces', bits, size)
    assert torch.equal(a.image, b.image) and torch.equal(a.depth, b.depth)


# ---- contention and tile boundaries -------------------------------------------------------------------------------------------------------
def test_65537_rows_on_one_pixel():
    rng = np.random.default_rng(3)
    n = 65537
    c = _rows(np.concatenate([rng.integers(0, 512, (n, 2)), rng.integers(0, 1024, (n, 1))], 1))
    got, want = _check(c, _colours(n, 2), '+z', 10, 2)
    assert want.mask.sum() == 1 and got.index[0, 0, 0, 0].item() == int(np.flatnonzero(c[:, 3] < 512)[0]) and got.depth[0, 0, 0, 0].item() == 0
    c[:, 3] = 700                                                              # all at one depth: row 0 of 65 537
    got, _ = _check(c, None, '+z', 10, 2)
    assert got.index[0, 0, 0, 0].item() == 0


@pytest.mark.parametrize('n', [63, 64, 65, 255, 256, 257, 'rows+1'])
def test_row_counts(n):
    n = ops.render_splat_rows() + 1 if n == 'rows+1' else n
    assert ops.render_splat_rows() == 256
    rng = np.random.default_rng(n)
    c = _rows(rng.integers(0, 32, (n, 3)))
    c[-1, 1:] = (31, 0, 0)                                                     # the last row is seen: alone in its corner, in front
    c[:-1, 2] = np.maximum(c[:-1, 2], 1)
    got, _ = _check(c, _colours(n, n), '+y;+z;30,20', 5, 32, 3)
    assert got.index[0, 0, 31, 31].item() == n - 1


# ---- clipping -----------------------------------------------------------------------------------------------------------------------------
def test_points_across_every_border_stay_inside():
    top = 15
    pts = [(x, y, 5) for x in (0, top) for y in (0, top)] + [(0, 7, 3), (top, 8, 3), (6, 0, 2), (9, top, 2), (8, 8, 9)]
    c = _rows(pts)
    rgb = _colours(len(c), 5)
    want = R.render_views(c, rgb, 'faces;45,30', 4, (16, 24), 4)
    arena = SA.Arena()
    with SA.installed(arena):
        got = render.render(_dev(c), _dev(rgb), 'faces;45,30', (16, 24), 4, 9)
    arena.check()                                                              # nothing outside any buffer
    _same(got, want)
    assert want.mask[0, 4, :5, :9].all() and want.mask[0, 4, 11:, 15:].all() and not want.mask[0, 0].all()


def test_rows_wholly_outside_the_image():
    c = _rows(np.random.default_rng(4).integers(0, 16, (300, 3)))
    M = render.view_matrices('+z;-x', 4, 16)
    M[0, :2, :3] *= 2                                                          # twice the scale: three quarters of the cube leave the image,
    M[0, 0, 3] -= 10 << 16                                                     # and the rest is moved ten pixels to the left
    M[1, 1, 3] += 40 << 16                                                     # every row below the image
    for ps in (1, 9):
        want = R.render_views(c, None, M, 4, 16, (ps - 1) // 2)
        got = render.render(_dev(c), None, M, 16, 4, ps)
        _same(got, want)
        assert 0 < want.mask[0, 0].sum() < (256 if ps == 1 else 257) and not want.mask[0, 1].any()
    far = M.copy()
    far[0, 0, 3] = -(1 << 60)                                                  # u far below -2^31: compared in 64 bits
    far[1, 1, 3] = 1 << 60
    _same(render.render(_dev(c), None, far, 16, 4, 9), R.render_views(c, None, far, 4, 16, 4))


# ---- range and signs ----------------------------------------------------------------------------------------------------------------------
def test_the_corners_of_the_coordinate_range():
    top = (1 << 20) - 1
    c = _rows([(x, y, z) for x in (0, top) for y in (0, top) for z in (0, top)] + [(top // 2, top // 3, top // 5)])
    got, want = _check(c, _colours(len(c), 6), 'faces', 20, 64, 3)
    assert want.mask[0, :6].sum() == 6 * (4 * 4 + 9)                           # four corners of 2 x 2 and the inner point, on every face
    big = np.zeros((1, 3, 4), np.int64)                                        # products of 2^20 x 2^20 x 3 in every row
    big[0, :, :3] = [[1 << 20, -(1 << 20), 1 << 20], [-(1 << 20), 1 << 20, 1 << 20], [1 << 20, 1 << 20, -(1 << 20)]]
    big[0, :, 3] = [-(top << 20) + (20 << 16), -(top << 20) + (30 << 16), 0]
    want = R.render_views(c, None, big, 20, 64, 1)
    _same(render.render(_dev(c), None, big, 64, 20, 3), want)
    assert want.mask.any() and np.abs(want.depth).max() > 1 << 23
    top = (1 << 21) - 1                                                        # the last coordinate the kernel takes
    c = _rows([(x, y, z) for x in (0, top) for y in (0, top) for z in (0, top)])
    _check(c, None, 'faces', 21, 64)


def test_an_oblique_view_has_negative_depths():
    c = _rows(synthetic.cloud('shell6').numpy())
    got, want = _check(c, None, '30,20', 6, 64)
    assert want.depth.min() < 0 and (want.depth[want.mask] < 0).sum() > 100
    assert got.image[got.mask].min().item() >= 55 and got.image[got.mask].max().item() < 255


# ---- batch and shapes ---------------------------------------------------------------------------------------------------------------------
def test_two_batch_items_in_one_place():
    pts = synthetic.cloud('shell6').numpy()
    c = np.concatenate([_rows(pts, 0), _rows(pts[::2] + np.array([0, 0, 1], np.int32), 1)])
    c = c[np.random.default_rng(7).permutation(len(c))]
    rgb = np.where(c[:, :1] == 0, np.uint8(10), np.uint8(200)).repeat(3, 1).astype(np.uint8)
    got, want = _check(c, rgb, 'faces;30,20', 6, 64, 3)
    assert set(np.unique(want.image[0][want.mask[0]])) == {10} and set(np.unique(want.image[1][want.mask[1]])) == {200}
    alone = R.render_views(c[c[:, 0] == 0], rgb[c[:, 0] == 0], 'faces;30,20', 6, 64, 1)
    assert np.array_equal(got.image[0].cpu().numpy(), alone.image[0]) and np.array_equal(got.depth[0].cpu().numpy(), alone.depth[0])
    _check(c, rgb, '+z', 6, 64, B=3)                                           # an item without rows is all background


def test_64_slices_pass_and_65_are_refused():
    c = np.concatenate([_rows(np.random.default_rng(b).integers(0, 8, (20, 3)), b) for b in range(8)])
    got, _ = _check(c, _colours(len(c), 8), 'turntable:8', 3, 8)
    assert got.image.shape == (8, 8, 8, 8, 3)
    _check(c[c[:, 0] == 0], None, 'turntable:64', 3, 8)
    with pytest.raises(ValueError, match='65'):
        render.render(_dev(c), None, 'turntable:5', 8, 3, batch_items=13)
    with pytest.raises(ValueError):
        render.render(_dev(c), None, 'turntable:65', 8, 3)
    M = np.zeros((65, 3, 4), np.int64)
    with pytest.raises(ValueError):
        render.render(_dev(c), None, M, 8, 3)
    with pytest.raises(ValueError, match='65'):
        ops.render(_dev(c[c[:, 0] == 0]), None, M, np.zeros((65, 2), np.int32), 1, 8, 8)


@pytest.mark.parametrize('size', [(5, 12), (33, 7), (1, 1), (1, 40)])
def test_sides_that_differ(size):
    c = _rows(np.random.default_rng(9).integers(0, 16, (200, 3)))
    M = render.view_matrices('+z;30,20', 4, 64)
    M[:, :, :] //= 4                                                           # any integers are a view: 16 x 16 pixels' worth, cut by the image
    want = R.render_views(c, _colours(200, 9), M, 4, size, 1)
    _same(render.render(_dev(c), _dev(_colours(200, 9)), M, size, 4, 3), want)
    assert want.mask.any()
    if min(size) >= 4:
        _check(c, None, '-x;+y', 4, (4, size[1]) if size[0] < size[1] else (size[0], 4), 3)


# ---- colour -------------------------------------------------------------------------------------------------------------------------------
def test_colours_shade_and_background():
    c = _rows(synthetic.cloud('shell6').numpy())
    rgb = _colours(len(c), 10)
    a, want = _check(c, rgb, 'faces', 6, 64, 1, (0, 17, 255))
    assert (want.image[~want.mask] == np.array([0, 17, 255], np.uint8)).all() and np.array_equal(want.image[want.mask], rgb[want.index[want.mask]])
    b, shade = _check(c, None, 'faces', 6, 64, 1, (0, 17, 255))
    assert torch.equal(a.index, b.index) and (shade.image[shade.mask][:, 0] == shade.image[shade.mask][:, 2]).all()
    assert len(np.unique(shade.image[shade.mask])) > 8
    wide = torch.zeros((len(c), 9), dtype=torch.int32, device=DEV)            # strided inputs
    wide[:, 3:7] = _dev(c)
    wide_c = torch.zeros((len(c), 4), dtype=torch.uint8, device=DEV)
    wide_c[:, 1:] = _dev(rgb)
    _same(render.render(wide[:, 3:7], wide_c[:, 1:], 'faces', 64, 6, 1, (0, 17, 255)), want)


def test_refusals():
    ok = _rows([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0]])
    for at, v in (((1, 1), -1), ((2, 3), 1 << 21), ((0, 0), 1), ((3, 0), -1)):
        bad = ok.copy()
        bad[at] = v
        with pytest.raises(ValueError, match='1 of 4 rows are outside'):
            render.render(_dev(bad), None, '+z', 4, 2, batch_items=1)
    for kw in (dict(point_size=2), dict(point_size=11), dict(point_size=True), dict(size=0), dict(size=4097), dict(bits=22), dict(views='up'),
               dict(background=(0, 0, 256)), dict(background=(0, 0))):
        with pytest.raises(ValueError):
            render.render(_dev(ok), None, **{**dict(views='+z', size=4, bits=2), **kw})
    with pytest.raises(ValueError, match='colours'):
        render.render(_dev(ok), torch.zeros((3, 3), dtype=torch.uint8, device=DEV), '+z', 4, 2)
    with pytest.raises(ValueError, match='int32'):
        render.render(_dev(ok).to(torch.int64), None, '+z', 4, 2)
    with pytest.raises(PcgcError):
        render.render(torch.from_numpy(ok), None, '+z', 4, 2)
    a = render.render(_dev(ok), None, '+z', 4, 2)
    b = render.render(_dev(ok), None, '-z', 4, 2)
    with pytest.raises(ValueError, match='different view matrices'):
        render.view_metric(a, b)
    assert render.render(_dev(ok), None).image.shape == (1, 6, 4, 4, 3)        # bits and size from the cloud: 2 bits hold x = 3


# ---- scratch ------------------------------------------------------------------------------------------------------------------------------
def test_recycled_scratch_and_guard_bands():
    """one run on fresh memory, one on the blocks a sibling cloud's run left behind (its z-buffer full of nearer points elsewhere): the same
    bytes, every guard intact.  This is the test that fails when the z-buffer clear is missing or short."""
    pts = synthetic.cloud('shell6').numpy()
    b = _rows(pts[pts[:, 0] < 30])
    a = _rows(63 - pts[pts[:, 0] < 30][:len(b)])                               # as many rows, the other half of the cube
    assert len(a) == len(b)
    rgb = _colours(len(b), 2)

    def run(c):
        r = render.render(_dev(c), _dev(rgb), 'faces;30,20', 64, 6, 3, (3, 2, 1))
        return r, ops.render_metric(r, r)

    want = R.render_views(b, rgb, 'faces;30,20', 6, 64, 1, (3, 2, 1))
    run(a)
    fresh, rec = SA.Arena(), SA.Arena()
    outs = []
    for arena, cloud in ((fresh, b), (rec, a)):
        with SA.installed(arena):
            outs.append(run(cloud))
        torch.cuda.synchronize()
        arena.finish()
        arena.check()
    sibling = outs[1][0].mask.clone()                                         # (the replay writes into the sibling's own blocks)
    stale = rec.replay()
    with SA.installed(stale):
        got, sums = run(b)
    torch.cuda.synchronize()
    stale.finish()
    for arena in (fresh, rec, stale):
        arena.check()
    _same(got, want)
    _same(outs[0][0], want)
    assert not torch.equal(sibling, got.mask)                                  # the sibling's picture differs: stale words would show
    allocs, replayed, _ = stale.stats()
    assert allocs == replayed == 7 and np.array_equal(sums.cpu().numpy(), R.metric_sums(want, want))     # (the sums are cleared too)


# ---- whole cloud --------------------------------------------------------------------------------------------------------------------------
_SHELL7 = {}


def _shell7():
    if not _SHELL7:
        c = _rows(synthetic.cloud('shell7', order='shuffled', seed=1).numpy())
        rgb = np.stack([c[:, 1] * 2, c[:, 2] * 2, 255 - c[:, 3] * 2], 1).astype(np.uint8)
        _SHELL7['c'], _SHELL7['rgb'] = c, rgb
    return _SHELL7['c'], _SHELL7['rgb']


@pytest.mark.parametrize('point_size', [1, 3])
def test_shell7(point_size):
    c, rgb = _shell7()
    got, want = _check(c, rgb, 'faces;35,25', 7, 128, point_size)
    assert want.mask[0, 4].sum() > 2500 and want.mask.all(axis=(0, 2, 3)).sum() == 0
    again = render.render(_dev(c), _dev(rgb), 'faces;35,25', 128, 7, point_size)
    for name in FIELDS:
        assert torch.equal(getattr(got, name), getattr(again, name)), name


# ---- metric -------------------------------------------------------------------------------------------------------------------------------
def _metric(a, b, ra, rb):
    m = render.view_metric(a, b)
    sums, per, mean = R.view_metric(ra, rb)
    assert m['sums'].dtype == np.int64 and np.array_equal(m['sums'], sums)
    for f in render.FIGURES:
        assert m[f].shape == sums.shape[:2] and m[f].tolist() == [[p[f] for p in item] for item in per], f
    assert m['mean'] == mean
    return m


def test_a_rendering_against_itself():
    c, rgb = _shell7()
    a, ra = _check(c, rgb, 'faces;35,25', 7, 64, 3)
    m = _metric(a, a, ra, ra)
    assert m['sums'][..., 2:].sum() == 0 and np.array_equal(m['sums'][..., 0], m['sums'][..., 1]) and (m['sums'][..., 0] > 0).all()
    assert all(math.isinf(m['mean'][f]) for f in render.FIGURES[:5]) and m['mean']['iou'] == 1.0 and (m['iou'] == 1.0).all()


def test_one_voxel_removed_one_recoloured_one_moved():
    ca = _rows([(1, 1, 0), (2, 1, 0), (3, 1, 0), (5, 5, 2)])
    ka = np.array([[7, 7, 7], [10, 20, 30], [100, 100, 100], [1, 2, 3]], np.uint8)
    cb = _rows([(1, 1, 0), (2, 1, 0), (5, 5, 4)])
    kb = np.array([[7, 7, 7], [13, 20, 30], [1, 2, 3]], np.uint8)
    a, ra = _check(ca, ka, '+z', 3, 8)
    b, rb = _check(cb, kb, '+z', 3, 8)
    m = _metric(a, b, ra, rb)
    # U = 4 pixels, I = 3; the removed voxel shows white against (100, 100, 100): 155^2 in every channel and in luma; the recoloured one adds 3^2
    # to R and nothing to luma (Y = 19 for both); the moved one differs in depth by 2
    assert m['sums'][0, 0].tolist() == [4, 3, 155 * 155 + 9, 155 * 155, 155 * 155, 155 * 155, 4, 0]
    assert m['iou'][0, 0] == 0.75 and m['depth_psnr'][0, 0] == 10 * math.log10(8.0 * 8.0 * 3 / 4) and m['psnr_g'][0, 0] == 10 * math.log10(255.0 * 255.0 * 4 / 24025)
    c, rgb = _shell7()
    keep = np.ones(len(c), bool)
    keep[np.random.default_rng(2).integers(0, len(c), 400)] = False
    other = rgb.copy()
    other[::7] ^= 0x55
    a, ra = _check(c, rgb, 'faces;35,25', 7, 128)
    b, rb = _check(c[keep], other[keep], ra.matrices, 7, 128)
    m = _metric(a, b, ra, rb)
    assert 0.9 < m['mean']['iou'] < 1.0 and 5 < m['mean']['psnr_y'] < 60 and (m['sums'][..., 6] > 0).all()


def test_disjoint_masks_and_depths_out_of_range():
    a, ra = _check(_rows([(1, 1, 1), (2, 2, 2)]), None, '+z;-z', 3, 8)
    b, rb = _check(_rows([(6, 6, 1), (5, 1, 2)]), None, '+z;-z', 3, 8)
    m = _metric(a, b, ra, rb)
    assert m['sums'][0, :, :2].tolist() == [[4, 0], [4, 0]] and (m['iou'] == 0).all() and np.isinf(m['depth_psnr']).all() and np.isfinite(m['psnr_y']).all()
    M = np.zeros((1, 3, 4), np.int64)
    M[0, 2, 2] = 1 << 19                                                       # d = 8 z: two voxels 2^16 apart in z differ by 2^19 in depth
    c = _rows([(0, 0, 0)])
    a = render.render(_dev(c), None, M, 2, 17)
    far = _rows([(0, 0, 1 << 16)])
    b = render.render(_dev(far), None, M, 2, 17)
    sums = ops.render_metric(a, b).cpu().numpy()
    assert np.array_equal(sums, R.metric_sums(R.render_views(c, None, M, 17, 2), R.render_views(far, None, M, 17, 2))) and sums[0, 0, 6:].tolist() == [0, 1]
    with pytest.raises(ValueError, match='1 pixels differ in depth'):
        render.view_metric(a, b)
    near = render.render(_dev(_rows([(0, 0, (1 << 16) - 1)])), None, M, 2, 17)
    assert render.view_metric(a, near)['sums'][0, 0, 6:].tolist() == [((1 << 19) - 8) ** 2, 0]


# ---- end to end: the command lines --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp('render')
    c, rgb = _shell7()
    path = str(d / 'shell7.ply')
    write_ply_ascii_geo_rgb(path, c[:, 1:], rgb)
    keep = np.ones(len(c), bool)
    keep[::9] = False
    other = str(d / 'fewer.ply')
    write_ply_ascii_geo_rgb(other, c[keep, 1:], (rgb[keep] // 2).astype(np.uint8))
    ckpt = str(d / 'synthetic.pth')
    torch.save({'model': synthetic.synthetic_state_dict(gain=50.0)}, ckpt)
    return d, path, other, ckpt, c, rgb, keep


def _png(path):
    return R.read_png(open(path, 'rb').read())[0]


def test_render_cli(files, capsys):
    d, path, other, _, c, rgb, keep = files
    views = 'faces;35,25'
    ra = R.render_views(c, rgb, views, 7, 64, 1)
    rb = R.render_views(c[keep], rgb[keep] // 2, views, 7, 64, 1)
    prefix = str(d / 'cli')
    assert render.main(['--filedir', path, '--against', other, '--views', views, '--size', '64', '--point_size', '3', '--out', prefix]) == 0
    lines = capsys.readouterr().out.splitlines()
    for k in range(7):
        assert np.array_equal(_png(f'{prefix}_view{k}.png'), ra.image[0, k]) and np.array_equal(_png(f'{prefix}_against_view{k}.png'), rb.image[0, k])
    _, per, mean = R.view_metric(ra, rb)
    assert [l for l in lines if l.startswith('view ') or l.startswith('mean')] == [render.describe(f'view {k}', per[0][k]) for k in range(7)] + [render.describe('mean', mean)]
    assert f'Y {mean["psnr_y"]:.4f} dB' in lines[-1] and math.isfinite(mean['psnr_y'])
    assert render.main(['--filedir', other, '--sheet']) == 0                   # bits and size from the file, one sheet
    sheet = _png(str(d / 'fewer_sheet.png'))
    alone = R.render_views(c[keep], rgb[keep] // 2, 'faces', 7, 128)
    assert sheet.shape == (2 * 128, 3 * 128, 3) and np.array_equal(sheet[128:, 128:256], alone.image[0, 4])
    capsys.readouterr()


def _normalised(text, outdir):
    return [l.replace(outdir, '<out>') for l in text.splitlines() if ' Time:' not in l and not l.startswith('View ')]


def test_coder_with_and_without_render(files, capsys):
    d, path, _, ckpt, c, rgb, _ = files
    outs, texts = [str(d / 'plain'), str(d / 'seen')], []
    for outdir, extra in zip(outs, ([], ['--render'])):
        coder.main(['--ckptdir', ckpt, '--filedir', path, '--outdir', outdir, '--lossless'] + extra)
        texts.append(capsys.readouterr().out)
    assert _normalised(texts[0], outs[0]) == _normalised(texts[1], outs[1]) and 'View ' not in texts[0]
    plain, seen = sorted(os.listdir(outs[0])), sorted(os.listdir(outs[1]))
    pngs = [f'shell7_{side}_view{k}.png' for side in ('dec', 'in') for k in range(6)]
    assert sorted(set(seen) - set(plain)) == sorted(pngs) and set(plain) <= set(seen)
    for name in plain:
        assert open(os.path.join(outs[0], name), 'rb').read() == open(os.path.join(outs[1], name), 'rb').read(), name
    # lossless without --attributes: _dec.ply has no colours, so both sides are depth shades, and the voxel sets are equal
    shade = R.render_views(c, None, 'faces', 7, 128)
    dec = read_ply_ascii_geo(os.path.join(outs[1], 'shell7_dec.ply'))
    rdec = R.render_views(_rows(dec), None, 'faces', 7, 128)
    for k in range(6):
        assert np.array_equal(_png(os.path.join(outs[1], f'shell7_in_view{k}.png')), shade.image[0, k])
        assert np.array_equal(_png(os.path.join(outs[1], f'shell7_dec_view{k}.png')), rdec.image[0, k])
    _, _, mean = R.view_metric(shade, rdec)
    said = [l for l in texts[1].splitlines() if l.startswith('View ')]
    assert said == [f'View PSNR (Y):\t {mean["psnr_y"]}', f'View depth PSNR:\t {mean["depth_psnr"]}', f'View IoU:\t {mean["iou"]}'] and mean['iou'] == 1.0


def test_coder_render_with_colours_on_the_lossy_path(files, capsys, monkeypatch):
    from pcgcv2_amd import pc_error as pe
    monkeypatch.setattr(pe, '_exe', lambda: None)
    d, path, _, ckpt, c, rgb, _ = files
    outdir = str(d / 'lossy')
    coder.main(['--ckptdir', ckpt, '--filedir', path, '--outdir', outdir, '--res', '128', '--recolour', '--render', '+z;35,25'])
    text = capsys.readouterr().out
    xyz, colours = read_ply_ascii_with_colours(os.path.join(outdir, 'shell7_dec.ply'))
    bits = render.bits_for(c[:, 1:], xyz)                                      # the smallest cube that holds both files
    ra = R.render_views(c, rgb, '+z;35,25', bits, 1 << bits)
    rb = R.render_views(_rows(xyz), colours, '+z;35,25', bits, 1 << bits)
    for k in range(2):
        assert np.array_equal(_png(os.path.join(outdir, f'shell7_in_view{k}.png')), ra.image[0, k])
        assert np.array_equal(_png(os.path.join(outdir, f'shell7_dec_view{k}.png')), rb.image[0, k])
    _, _, mean = R.view_metric(ra, rb)
    assert f'View PSNR (Y):\t {mean["psnr_y"]}\nView depth PSNR:\t {mean["depth_psnr"]}\nView IoU:\t {mean["iou"]}\n' in text
    assert text.index('Colour PSNR (Y)') < text.index('View PSNR (Y)')


def test_sweep_with_views(files, capsys, monkeypatch):
    import pandas as pd
    from pcgcv2_amd import pc_error as pe
    from pcgcv2_amd.test import test as sweep, main
    monkeypatch.setattr(pe, '_exe', lambda: None)
    d, path, _, ckpt, c, rgb, _ = files
    plain = sweep(path, [ckpt], str(d / 's0'), str(d / 'r0'), res=128, verbose=False, metric='device')
    seen = sweep(path, [ckpt, ckpt], str(d / 's1'), str(d / 'r1'), res=128, verbose=False, metric='device', colour=True, views='faces;35,25')
    assert 'view_iou' not in plain.columns and [k for k in seen.columns if k.startswith('view_')] == ['view_depth_psnr', 'view_iou', 'view_psnr_y']
    for k in plain.columns:
        if not k.startswith('time'):
            assert seen[k][0] == plain[k][0], k
    ra = R.render_views(c, rgb, 'faces;35,25', 7, 128)
    for rate in (1, 2):
        xyz, colours = read_ply_ascii_with_colours(str(d / 's1' / f'shell7_r{rate}_dec.ply'))
        _, _, mean = R.view_metric(ra, R.render_views(_rows(xyz), colours, 'faces;35,25', 7, 128))
        assert (seen['view_depth_psnr'][rate - 1], seen['view_iou'][rate - 1], seen['view_psnr_y'][rate - 1]) == (mean['depth_psnr'], mean['iou'], mean['psnr_y'])
    main(['--filedir', path, '--outdir', str(d / 's2'), '--resultdir', str(d / 'r2'), '--res', '128', '--ckpts', ckpt, '--metric', 'device', '--views'])
    assert 'view depth' in capsys.readouterr().out
    cli = pd.read_csv(d / 'r2' / 'shell7.csv')
    shade = R.render_views(c, None, 'faces', 7, 128)
    xyz = read_ply_ascii_geo(str(d / 's2' / 'shell7_r1_dec.ply'))
    _, _, mean = R.view_metric(shade, R.render_views(_rows(xyz), None, 'faces', 7, 128))
    assert 'view_psnr_y' not in cli.columns and cli['view_iou'][0] == pytest.approx(mean['iou'], rel=1e-12)
    assert cli['view_depth_psnr'][0] == pytest.approx(mean['depth_psnr'], rel=1e-12)
    with pytest.raises(ValueError, match="metric='device'"):
        sweep(path, [ckpt], str(d / 's3'), str(d / 'r3'), res=128, verbose=False, views='faces')
    with pytest.raises(SystemExit):
        main(['--filedir', path, '--views', 'faces'])
