"""Estimated normals without a GPU: the definition (tests/normals_reference.py) on hand-made cases with their moments, validity, eigenvalues
and normal written out; the host side of the feature (ball masks, PLY writer, library exports, command line)."""
import itertools

import numpy as np
import pytest

import normals_reference as nr
from pcgcv2_amd import _lib, data_utils, pc_error


def _rows(xyz, batch=0):
    xyz = np.asarray(xyz, np.int64)
    return np.concatenate([np.full((len(xyz), 1), batch, np.int64), xyz], 1)


def _at(coords, p):
    return int(np.nonzero((coords[:, 1:] == np.asarray(p)).all(1))[0][0])


def test_plane():
    """z = 5 over 13 x 13: the disc of squared radius 16 holds 49 voxels with sum dx^2 = sum dy^2 = 192, nothing along z"""
    c = _rows([(x, y, 5) for x in range(13) for y in range(13)])
    r = nr.estimate_normals(c, 16)
    i = _at(c, (6, 6, 5))
    assert r['moments'][i].tolist() == [49, 0, 0, 0, 192, 192, 0, 0, 0, 0]
    assert r['valid'][i] and r['count'][i] == 49
    assert r['lam'][i, 0] == 0.0 and r['lam'][i, 1] == r['lam'][i, 2] == 49 * 192
    assert r['normals'][i].tolist() == [0.0, 0.0, 1.0]                 # (the row IS the centroid: dot 0, the largest component is made positive)
    assert r['valid'].all() and (r['lam'][:, 0] == 0.0).all()          # every row of a plane, the corners too (k = 17 there)
    assert (np.abs(r['normals'][:, 2]) == 1.0).all()
    j = _at(c, (0, 0, 5))
    assert r['count'][j] == 17 and r['moments'][j, 1] > 0 and r['moments'][j, 3] == 0
    for orient, z in (((6.0, 6.0, 100.0), 1.0), ((6.0, 6.0, -100.0), -1.0), (None, 1.0)):
        assert (nr.estimate_normals(c, 16, orient)['normals'][:, 2] == z).all(), orient


def test_rod_is_rank_one():
    c = _rows([(x, 3, 3) for x in range(13)])
    r = nr.estimate_normals(c, 16)
    i = _at(c, (6, 3, 3))
    assert r['moments'][i].tolist() == [9, 0, 0, 0, 60, 0, 0, 0, 0, 0]
    assert not r['valid'].any()                                        # k >= 3 everywhere, rank 1
    assert r['lam'][i].tolist() == [0.0, 0.0, 540.0]
    assert (r['normals'] == 0.0).all()


def test_single_voxel_and_pair():
    r = nr.estimate_normals(_rows([(7, 8, 9)]), 16)
    assert r['moments'][0].tolist() == [1] + [0] * 9 and not r['valid'][0]
    assert r['lam'][0].tolist() == [0.0, 0.0, 0.0] and r['normals'][0].tolist() == [0.0, 0.0, 0.0]
    pair = _rows([(3, 0, 0), (7, 0, 0)])
    assert nr.estimate_normals(pair, 16)['count'].tolist() == [2, 2]   # |d|^2 = 16: neighbours across the cell border ...
    assert nr.estimate_normals(pair, 15)['count'].tolist() == [1, 1]   # ... and not at 15


def test_filled_block_centre_is_isotropic():
    """the centre of a 9^3 block sees the whole ball: 257 voxels, sum dx^2 = 796 per axis, no mixed term: S = 257 * 796 * I"""
    c = _rows(list(itertools.product(range(9), repeat=3)))
    r = nr.estimate_normals(c, 16)
    i = _at(c, (4, 4, 4))
    assert r['moments'][i].tolist() == [257, 0, 0, 0, 796, 796, 796, 0, 0, 0]
    assert r['valid'][i]
    assert r['lam'][i].tolist() == [257.0 * 796] * 3
    assert abs(np.linalg.norm(r['normals'][i]) - 1.0) < 1e-15          # (any direction is an eigenvector: only its length is defined)
    assert r['gap'][i] == 0.0


def test_duplicates_batches_and_row_order():
    rng = np.random.default_rng(3)
    pts = np.unique(rng.integers(0, 12, (400, 3)), axis=0)
    base = nr.estimate_normals(_rows(pts), 9)
    dup = np.concatenate([_rows(pts), _rows(pts[:50])])
    perm = rng.permutation(len(dup))
    r = nr.estimate_normals(dup[perm], 9)
    src = np.concatenate([np.arange(len(pts)), np.arange(50)])[perm]
    for k in ('moments', 'valid', 'lam', 'normals'):
        assert np.array_equal(r[k], base[k][src]), k
    two = np.concatenate([_rows(pts, 0), _rows(pts + np.array([1, 0, 0]), 1)])
    r2 = nr.estimate_normals(two, 9)
    assert np.array_equal(r2['moments'][:len(pts)], base['moments']) and np.array_equal(r2['moments'][len(pts):], base['moments'])


def test_both_neighbour_searches_of_the_definition_agree():
    rng = np.random.default_rng(8)
    c = _rows(np.unique(rng.integers(0, 20, (1500, 3)), axis=0))
    for r2 in (1, 16, 17, 64):
        assert np.array_equal(nr.estimate_normals(c, r2, method='kdtree')['moments'], nr.estimate_normals(c, r2, method='grid')['moments']), r2


def test_ball_masks_of_the_library():
    """pcgc_normals_ball_masks against its definition: 27 cells up to r2 = 24, 125 beyond; r2 outside 1 .. 64 is an error"""
    lib = _lib.lib()
    bit = np.arange(64)
    pos = np.stack([bit & 3, (bit >> 2) & 3, bit >> 4], 1)
    for r2, side in ((1, 3), (9, 3), (16, 3), (24, 3), (25, 5), (64, 5)):
        n = int(lib.pcgc_normals_ball_masks(r2, None))
        assert n == side ** 3 * 64, r2
        tab = np.zeros(n, np.uint64)
        assert int(lib.pcgc_normals_ball_masks(r2, tab.ctypes.data)) == n
        tab = tab.reshape(side, side, side, 64)                        # [oz, oy, ox, lane]
        c = side // 2
        total = 0
        for oz, oy, ox in itertools.product(range(side), repeat=3):
            off = 4 * (np.array([ox, oy, oz]) - c)
            d = off + pos[None, :, :] - pos[:, None, :]                # [lane, bit, 3]
            want = ((d * d).sum(-1) <= r2).astype(np.uint64) << bit.astype(np.uint64)[None, :]
            want = np.bitwise_or.reduce(want, 1)
            assert np.array_equal(tab[oz, oy, ox], want), (r2, ox, oy, oz)
            total += sum(bin(int(v)).count('1') for v in want)
        r = int(np.sqrt(r2))
        ball = sum(1 for d in itertools.product(range(-r, r + 1), repeat=3) if sum(v * v for v in d) <= r2)
        assert total == 64 * ball                                      # every lane sees the whole ball: no cell is missing
    for bad in (0, -1, 65):
        assert int(lib.pcgc_normals_ball_masks(bad, None)) < 0


def test_exports():
    lib = _lib.lib()
    for name in ('pcgc_normals_ball_masks', 'pcgc_normals_workspace_bytes', 'pcgc_normals_estimate', 'pcgc_set_normals_mapping'):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert len(_lib.SIGNATURES['pcgc_normals_estimate'][1]) == 24
    assert int(lib.pcgc_normals_workspace_bytes(1000)) >= 4 * 1000
    from pcgcv2_amd import ops
    assert callable(ops.estimate_normals) and callable(pc_error.estimate_normals_device)


def test_writer_reader_round_trip(tmp_path):
    rng = np.random.default_rng(1)
    xyz = rng.integers(0, 1024, (500, 3))
    nrm = rng.normal(size=(500, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm[:3] = [[0, 0, 0], [1, 0, 0], [0, -1, 1e-30]]
    path = str(tmp_path / 'n.ply')
    data_utils.write_ply_ascii_geo_normals(path, xyz, nrm)
    assert pc_error.ply_has_normals(path)
    got_xyz, got_nrm = pc_error.read_ply_ascii_with_normals(path)
    assert np.array_equal(got_xyz, xyz)
    assert np.array_equal(got_nrm, nrm.astype(np.float32).astype(np.float64))        # float32 rounding, nothing else
    assert np.array_equal(data_utils.read_ply_ascii_geo(path), xyz)    # (the geometry reader takes the first three columns)
    with pytest.raises(ValueError):
        data_utils.write_ply_ascii_geo_normals(path, xyz, nrm[:10])
    with pytest.raises(ValueError):
        data_utils.write_ply_ascii_geo_normals(path, xyz + 0.5, nrm)


def test_command_line_parsers():
    from pcgcv2_amd import estimate_normals as cli
    a = cli.parser().parse_args(['--filedir', 'in.ply', '--out', 'out.ply'])
    assert (a.filedir, a.out, a.r2, a.orient) == ('in.ply', 'out.ply', 16, 'centroid')
    a = cli.parser().parse_args(['--filedir', 'i', '--out', 'o', '--r2', '9', '--orient', 'none'])
    assert a.r2 == 9 and a.orient is None
    a = cli.parser().parse_args(['--filedir', 'i', '--out', 'o', '--orient', '0,-5.5,1e3'])
    assert a.orient == (0.0, -5.5, 1000.0)
    for bad in ('up', '1,2', '1,2,x'):
        with pytest.raises(SystemExit):
            cli.parser().parse_args(['--filedir', 'i', '--out', 'o', '--orient', bad])
    with pytest.raises(SystemExit):
        cli.parser().parse_args(['--out', 'o'])
    with pytest.raises(SystemExit):
        cli.main(['--filedir', 'i', '--out', 'o', '--r2', '65'])
