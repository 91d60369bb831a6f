"""The host side of the renderer (pcgcv2_amd/render.py), no GPU: the view matrices against literal pictures and against their
restatement in tests/render_reference.py, the oblique matrices' geometry, the range checks, the PNG writer's round trip, the figures formed
from the integer sums, and the command lines' parsing."""
import math
from collections import namedtuple

import numpy as np
import pytest
import torch

import render_reference as R
from pcgcv2_amd import render

# rows 0, 1, 2 of an asymmetric cloud in the cube [0, 4)^3
CLOUD = np.array([[0, 0, 0, 0], [0, 3, 0, 0], [0, 0, 1, 3]], np.int32)
# the row each pixel shows (. = background), size == 2^bits == 4, rows v = 0 .. 3 from the top, columns u = 0 .. 3 from the left
PICTURES = {
    '+x': ('..2.', '....', '....', '...0'),            # looking along +x: u = 3 - y, v = 3 - z; rows 0 and 1 share a pixel, row 0 (x = 0) is in front
    '-x': ('.2..', '....', '....', '1...'),            # looking along -x: u = y, v = 3 - z; row 1 (x = 3) is in front
    '+y': ('2...', '....', '....', '0..1'),            # u = x, v = 3 - z
    '-y': ('...2', '....', '....', '1..0'),            # u = 3 - x, v = 3 - z
    '+z': ('0..1', '2...', '....', '....'),            # u = x, v = y: the lattice's own columns
    '-z': ('1..0', '...2', '....', '....'),            # u = 3 - x, v = y
}


def _picture(index):
    return tuple(''.join('.' if v < 0 else str(v) for v in row) for row in index)


@pytest.mark.parametrize('face', render.FACES)
def test_literal_pictures_pin_the_six_orientations(face):
    M = render.view_matrices(face, 2, 4)
    assert M.dtype == np.int64 and M.shape == (1, 3, 4)
    got = R.render(CLOUD, None, M, render.depth_planes(M, 2), 1, 4, 4)
    assert _picture(got.index[0, 0]) == PICTURES[face]
    k = render.FACES.index(face)
    assert np.array_equal(render.view_matrices('faces', 2, 4)[k], M[0])


def test_depth_of_the_faces_and_the_shade():
    M = render.view_matrices('+x;-x', 2, 4)
    got = R.render(CLOUD, None, M, render.depth_planes(M, 2), 1, 4, 4)
    assert got.depth[0, 0, 3, 3] == 0 and got.depth[0, 1, 3, 0] == 0 and got.depth[0, 1, 0, 1] == 3
    assert render.depth_planes(M, 2).tolist() == [[0, 3], [0, 3]]
    assert got.image[0, 0, 3, 3].tolist() == [255] * 3 and got.image[0, 1, 0, 1].tolist() == [55] * 3       # near 255, far 255 - 200
    assert got.image[0, 0, 0, 0].tolist() == [255] * 3 and not got.mask[0, 0, 0, 0]                         # the (white) background


@pytest.mark.parametrize('views,bits,size', [('faces', 2, 4), ('faces', 10, 256), ('faces', 7, (64, 128)), ('faces', 20, 64), ('faces', 3, 32),
                                             ('30,20;0,0;45,89;-120.5,-33', 7, 128), ('turntable:5', 10, (100, 300)), ('faces;10,80', 6, 64)])
def test_matrices_equal_their_restatement(views, bits, size):
    assert np.array_equal(render.view_matrices(views, bits, size), R.view_matrices(views, bits, size))
    M = render.view_matrices(views, bits, size)
    assert np.array_equal(render.depth_planes(M, bits), R.depth_planes(M, bits))


def test_faces_are_exact_at_half_scale():
    M = render.view_matrices('+z;-z', 3, 4)                                    # 8 columns onto 4 pixels: a shift, no rounding
    x = np.arange(8)
    assert ((M[0, 0, 0] * x + M[0, 0, 3]) >> 16).tolist() == [0, 0, 1, 1, 2, 2, 3, 3]
    assert ((M[1, 0, 0] * x + M[1, 0, 3]) >> 16).tolist() == [3, 3, 2, 2, 1, 1, 0, 0]
    assert ((M[1, 2, 2] * x + M[1, 2, 3]) >> 16).tolist() == [3, 3, 2, 2, 1, 1, 0, 0]
    wide = render.view_matrices('+z', 3, (8, 12))                              # centred in the longer side
    assert (wide[0, 0, 3] >> 16, wide[0, 1, 3] >> 16) == (2, 0)


@pytest.mark.parametrize('bits', [7, 10])
@pytest.mark.parametrize('size', [None, 64, (48, 200)])
def test_oblique_rows_are_orthogonal_and_the_cube_fits(bits, size):
    L = 1 << bits
    size = L if size is None else size
    H, W = (size, size) if isinstance(size, int) else size
    top = L - 1
    corners = np.array([[x, y, z] for x in (0, top) for y in (0, top) for z in (0, top)], np.int64)
    k16 = (min(H, W) / 2.0 - (0.5 + 3.0 * L / 131072.0)) / (math.sqrt(3.0) / 2.0 * L) * 65536.0          # the scale in Q16, before rounding
    for yaw in (0, 45, 89):
        for pitch in (0, 45, 89):
            M = render.view_matrices(f'{yaw},{pitch}', bits, size)[0]
            A = M[:, :3].astype(np.float64)
            # a row is k16 a + e with |a| = 1 and |e_i| <= 1/2: dots within sqrt(3) k16 + 3/4, norms within sqrt(3)/2 of k16
            for i, j in ((0, 1), (0, 2), (1, 2)):
                assert abs(A[i] @ A[j]) <= math.sqrt(3.0) * k16 + 0.75, (yaw, pitch, i, j)
            assert np.abs(np.linalg.norm(A, axis=1) - k16).max() <= math.sqrt(3.0) / 2 + 1e-9
            uvd = (corners @ M[:, :3].T + M[:, 3]) >> 16
            assert uvd[:, 0].min() >= 0 and uvd[:, 0].max() < W and uvd[:, 1].min() >= 0 and uvd[:, 1].max() < H, (yaw, pitch)
            assert uvd[:, 2].min() < 0 < uvd[:, 2].max()                       # d is measured from the cube's centre


def test_orientation_of_the_oblique_views():
    M = render.view_matrices('0,0;0,90;90,0', 7, 128)
    c = np.array([64, 64, 64])
    shift = lambda k, p: ((M[k, :, :3] @ (c + p) + M[k, :, 3]) >> 16) - ((M[k, :, :3] @ c + M[k, :, 3]) >> 16)
    assert shift(0, [20, 0, 0])[0] > 0 and shift(0, [0, 0, 20])[1] < 0 and shift(0, [0, 20, 0])[2] > 0      # 0,0 looks along +y, z up
    assert shift(1, [0, 0, 20])[2] < 0 and shift(1, [0, 20, 0])[1] < 0                                       # pitch 90 looks down: z is in front
    assert shift(2, [0, 20, 0])[0] > 0 and shift(2, [20, 0, 0])[2] < 0                                       # yaw 90 looks along -x


def test_matrices_that_would_overflow_are_refused():
    ok = np.zeros((1, 3, 4), np.int64)
    render.check_matrices(ok)
    for at, value, fine in (((0, 0, 0), (1 << 20) + 1, 1 << 20), ((0, 1, 2), -(1 << 20) - 1, -(1 << 20)), ((0, 2, 3), 1 << 47, (1 << 47) - 1),
                            ((0, 2, 3), -(1 << 47) - 1, -(1 << 47)), ((0, 0, 3), (1 << 60) + 1, 1 << 60)):
        M = ok.copy()
        M[at] = value
        with pytest.raises(ValueError):
            render.check_matrices(M)
        M[at] = fine
        render.check_matrices(M)
    M = ok.copy()
    M[0, 2] = [1 << 20, 1 << 20, 1 << 20, (1 << 47) - 1 - 3 * (1 << 20) * ((1 << 21) - 1)]      # the far corner reaches 2^47 - 1: the last d inside
    render.check_matrices(M)
    M[0, 2, 3] += 1
    with pytest.raises(ValueError, match='d leaves int32'):
        render.check_matrices(M)
    for bad in (ok.astype(np.int32), ok[0], np.zeros((65, 3, 4), np.int64), np.zeros((0, 3, 4), np.int64)):
        with pytest.raises(ValueError):
            render.check_matrices(bad)
    with pytest.raises(ValueError, match='power of two'):
        render.view_matrices('faces', 21, 16)                                  # the scale 2^-17 is not a Q16 number
    with pytest.raises(ValueError, match='power of two'):
        render.view_matrices('+z', 4, 48)
    with pytest.raises(ValueError, match='too small'):
        render.view_matrices('30,20', 21, 16)
    for bits, size in ((0, 4), (22, 4), (4, 0), (4, 4097), (4, (4, 4, 4)), (True, 4)):
        with pytest.raises(ValueError):
            render.view_matrices('faces', bits, size)


def test_view_lists():
    assert render.parse_views('faces') == [('face', f) for f in render.FACES]
    assert len(render.parse_views('faces;30,20')) == 7 and render.parse_views('faces;30,20')[6] == ('oblique', 30.0, 20.0)
    assert render.parse_views('turntable:4') == [('oblique', y, render.TURNTABLE_PITCH) for y in (0.0, 90.0, 180.0, 270.0)]
    assert render.parse_views(['-z', (10, -5)]) == [('face', '-z'), ('oblique', 10.0, -5.0)]
    for bad in ('', 'face', 'turntable:0', 'turntable:65', 'turntable:x', '10', '10,20,30', '10,91', 'nan,0', 'faces;' * 11 + 'faces'):
        with pytest.raises(ValueError):
            render.parse_views(bad)


@pytest.mark.parametrize('shape', [(1, 1), (2, 3), (5, 4), (3, 7)])
def test_png_round_trip(shape, tmp_path):
    image = np.random.default_rng(shape[0] * 10 + shape[1]).integers(0, 256, shape + (3,)).astype(np.uint8)
    data = render.png_bytes(image)
    assert data[:8] == b'\x89PNG\r\n\x1a\n'
    back, kinds = R.read_png(data)
    assert kinds == [b'IHDR', b'IDAT', b'IEND'] and np.array_equal(back, image)
    path = str(tmp_path / 'p.png')
    render.write_png(path, torch.from_numpy(image))
    assert open(path, 'rb').read() == data
    damaged = bytearray(data)
    damaged[-20] ^= 1                                                          # inside IDAT: the reader's CRC check must see it
    with pytest.raises(AssertionError):
        R.read_png(bytes(damaged))
    for bad in (image.astype(np.int32), image[..., :2], image[0], np.zeros((0, 4, 3), np.uint8)):
        with pytest.raises(ValueError):
            render.png_bytes(bad)


def test_sheet_tiles_the_views():
    Fake = namedtuple('Fake', 'image')
    image = torch.arange(2 * 5 * 2 * 3 * 3, dtype=torch.int64).remainder(251).to(torch.uint8).reshape(2, 5, 2, 3, 3)
    s = render.sheet(Fake(image), item=1, background=(9, 8, 7))
    assert s.shape == (2 * 2, 3 * 3, 3) and s.dtype == np.uint8                # five views: three to a row, two rows
    for k in range(5):
        assert np.array_equal(s[k // 3 * 2:(k // 3 + 1) * 2, k % 3 * 3:(k % 3 + 1) * 3], image[1, k].numpy())
    assert (s[2:, 6:] == np.array([9, 8, 7], np.uint8)).all()


def test_figures_from_the_sums():
    sums = np.array([[[10, 5, 0, 40, 10, 20, 5, 0], [0, 0, 0, 0, 0, 0, 0, 0]]], np.int64)
    m = render.metric_from_sums(sums, 64)
    assert m['psnr_r'][0, 0] == math.inf and m['psnr_y'][0, 0] == 10 * math.log10(255.0 * 255.0 * 10 / 20)
    assert m['depth_psnr'][0, 0] == 10 * math.log10(64.0 * 64.0 * 5 / 5) and m['iou'][0, 0] == 0.5
    assert m['iou'][0, 1] == 1.0 and m['psnr_y'][0, 1] == math.inf and m['depth_psnr'][0, 1] == math.inf    # nothing in either picture
    assert m['mean'] == R.figures(sums[0, 0], 64) and m['sums'] is not None
    for f in render.FIGURES:
        assert m[f][0, 0] == R.figures(sums[0, 0], 64)[f]
    sums[0, 1, 7] = 2
    with pytest.raises(ValueError, match='2 pixels differ in depth'):
        render.metric_from_sums(sums, 64)


def test_the_definition_keeps_the_lower_row_among_equal_depths():
    c = np.array([[0, 2, 2, 2], [0, 3, 3, 3], [0, 2, 2, 1]], np.int32)
    got = R.render_views(c, None, '+z', 3, 4)                                  # half scale: rows 0 and 1 share a pixel and a depth
    assert got.index[0, 0, 1, 1] == 2 and got.depth[0, 0, 1, 1] == 0           # row 2 is nearer
    got = R.render_views(c[:2], None, '+z', 3, 4)
    assert got.index[0, 0, 1, 1] == 0 and got.mask.sum() == 1
    got = R.render_views(c[:2][::-1], None, '+z', 3, 4)
    assert got.index[0, 0, 1, 1] == 0


def test_command_lines_parse():
    a = render.parse_args(['--filedir', 'a.ply'])
    assert (a.views, a.size, a.bits, a.point_size, a.out, a.sheet, a.against) == ('faces', None, None, 1, None, False, None)
    a = render.parse_args(['--filedir', 'a.ply', '--against', 'b.ply', '--views', 'turntable:8', '--size', '512', '--point_size', '3', '--out', 'p',
                           '--sheet', '--bits', '10'])
    assert (a.views, a.size, a.bits, a.point_size, a.out, a.sheet, a.against) == ('turntable:8', 512, 10, 3, 'p', True, 'b.ply')
    for bad in (['--views', 'sideways'], ['--views', 'turntable:0'], ['--point_size', '2'], ['--point_size', '11'], ['--size', '0'], ['--size', '4097'],
                ['--bits', '22'], ['--bits', '0']):
        with pytest.raises(SystemExit):
            render.parse_args(['--filedir', 'a.ply'] + bad)
    with pytest.raises(SystemExit):
        render.parse_args([])
    from pcgcv2_amd import coder
    assert coder._parse_cli([]).render is None and coder._parse_cli(['--render']).render == 'faces'
    assert coder._parse_cli(['--render', '30,20;faces', '--lossless']).render == '30,20;faces'
    with pytest.raises(SystemExit):
        coder._parse_cli(['--render', 'sideways'])
