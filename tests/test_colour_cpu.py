"""Colours on the host (no GPU): the numpy definition (tests/colour_reference.py) and pc_error.colour_psnr against what mpeg-pcc-dmetric prints
with `-c 1` (tests/golden/colour_metric.npz), coloured PLY I/O, the recolour definition, and the parser of the binary's colour lines."""
import math
import os

import numpy as np
import pytest

import colour_reference as ref
from pcgcv2_amd import pc_error as pe
from pcgcv2_amd.data_utils import (ply_has_colours, read_ply_ascii_geo, read_ply_ascii_with_colours, write_ply_ascii_geo,
                                   write_ply_ascii_geo_rgb)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'colour_metric.npz')


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


def check_against_printed(got, golden, case):
    """six printed digits, as test_native_d2_matches_pc_error_d holds them: the c[k] values to rel 2e-5 / abs 1e-9, the h.c[k] values (integers)
    exactly, the PSNRs to 2e-4, inf where the binary printed inf"""
    for col in ref.COLUMNS:
        want = float(golden[ref.golden_key(case, col)])
        print(case, repr(col), got[col], want)
        if math.isinf(want):
            assert got[col] == want, (case, col)
        elif 'PSNR' in col:
            assert got[col] == pytest.approx(want, abs=2e-4), (case, col)
        elif col.startswith('h.'):
            assert got[col] == want, (case, col)
        else:
            assert got[col] == pytest.approx(want, rel=2e-5, abs=1e-9), (case, col)


def case_of(golden, i):
    return (golden[f'p{i}_a'].astype(np.int64), golden[f'p{i}_ca'], golden[f'p{i}_b'].astype(np.int64), golden[f'p{i}_cb'])


@pytest.mark.parametrize('case', range(4))
def test_numpy_definition_matches_pc_error_d(golden, case):
    assert ref.COLUMNS == pe.COLOUR_COLUMNS and len(ref.COLUMNS) == 36
    check_against_printed(ref.colour_metric(*case_of(golden, case)), golden, case)


@pytest.mark.parametrize('case', range(4))
def test_host_colour_psnr_matches_pc_error_d(golden, case):
    got = pe.colour_psnr(*case_of(golden, case))
    assert list(got) == pe.COLOUR_COLUMNS
    check_against_printed(got, golden, case)


def test_host_colour_psnr_equals_numpy_definition(golden):
    a, ca, b, cb = case_of(golden, 3)
    got, want = pe.colour_psnr(a, ca, b, cb), ref.colour_metric(a, ca, b, cb)
    for col in ref.COLUMNS:
        if col.startswith('h.'):
            assert got[col] == want[col], col
        else:
            assert got[col] == pytest.approx(want[col], rel=1e-12), col


def test_golden_has_zero_and_inf(golden):
    assert float(golden[ref.golden_key(2, 'c[0],    F')]) == 0.0
    assert math.isinf(float(golden[ref.golden_key(2, 'c[0],PSNRF')])) and math.isinf(float(golden[ref.golden_key(2, 'h.c[1],PSNR1')]))


# ---------------------------------------------------------------------------------------------------------------------------- PLY
def test_coloured_ply_round_trips(tmp_path):
    rng = np.random.default_rng(0)
    xyz = rng.integers(0, 1024, size=(257, 3))
    rgb = rng.integers(0, 256, size=(257, 3)).astype(np.uint8)
    rgb[0], rgb[1] = 0, 255
    p = str(tmp_path / 'c.ply')
    write_ply_ascii_geo_rgb(p, xyz, rgb)
    head = open(p).read().split('end_header\n')[0].splitlines()
    assert head == ['ply', 'format ascii 1.0', 'element vertex 257', 'property float x', 'property float y', 'property float z',
                    'property uchar red', 'property uchar green', 'property uchar blue']
    assert open(p).read().split('end_header\n')[1].splitlines()[0] == ' '.join(str(v) for v in list(xyz[0]) + [0, 0, 0])
    got_xyz, got_rgb = read_ply_ascii_with_colours(p)
    assert got_xyz.dtype == np.float64 and got_rgb.dtype == np.uint8
    np.testing.assert_array_equal(got_xyz, xyz)
    np.testing.assert_array_equal(got_rgb, rgb)
    np.testing.assert_array_equal(read_ply_ascii_geo(p), xyz)
    assert ply_has_colours(p)


def test_colours_found_among_other_columns(tmp_path):
    p = str(tmp_path / 'n.ply')
    with open(p, 'w') as f:
        f.write('ply\nformat ascii 1.0\ncomment by hand\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\n'
                'property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n'
                'element face 0\nproperty list uchar int vertex_indices\nend_header\n'
                '1 2 3 0.5 0.5 0.7 10 20 30\n4 5 6 0 0 1 255 0 128\n7 8 9 1 0 0 0 0 0\n')
    xyz, rgb = read_ply_ascii_with_colours(p)
    np.testing.assert_array_equal(xyz, [[1, 2, 3], [4, 5, 6], [7, 8, 9]])
    np.testing.assert_array_equal(rgb, np.array([[10, 20, 30], [255, 0, 128], [0, 0, 0]], np.uint8))
    assert ply_has_colours(p)


def test_geometry_only_ply_has_no_colours(tmp_path):
    p = str(tmp_path / 'g.ply')
    write_ply_ascii_geo(p, np.arange(12).reshape(4, 3))
    assert not ply_has_colours(p)
    assert not ply_has_colours(str(tmp_path / 'missing.ply'))
    xyz, rgb = read_ply_ascii_with_colours(p)
    assert rgb is None
    np.testing.assert_array_equal(xyz, np.arange(12).reshape(4, 3))


def test_writer_refuses_mismatched_colours(tmp_path):
    with pytest.raises(ValueError):
        write_ply_ascii_geo_rgb(str(tmp_path / 'x.ply'), np.zeros((3, 3), int), np.zeros((2, 3), np.uint8))
    with pytest.raises(ValueError):
        write_ply_ascii_geo_rgb(str(tmp_path / 'x.ply'), np.zeros((3, 3), int), np.zeros((3, 3), np.float32))


# ---------------------------------------------------------------------------------------------------------------------------- recolour
@pytest.mark.parametrize('fn', [ref.recolour, pe.recolour], ids=['definition', 'host'])
def test_recolour_of_a_permutation_permutes(fn):
    rng = np.random.default_rng(1)
    s = np.unique(rng.integers(0, 40, size=(700, 3)), axis=0)
    attr = rng.integers(0, 256, size=(len(s), 3)).astype(np.uint8)
    perm = rng.permutation(len(s))
    np.testing.assert_array_equal(fn(s, attr, s[perm]), attr[perm])


@pytest.mark.parametrize('fn', [ref.recolour, pe.recolour], ids=['definition', 'host'])
def test_recolour_midway_target_rounds_half_up(fn):
    # the target between the two sources is chosen by neither (each source is nearer to a target of its own): it averages 255 and 0 -> 128
    s = np.array([[0, 0, 0], [4, 0, 0]])
    attr = np.array([[255, 255], [0, 1]], np.uint8)
    t = np.array([[0, 0, 0], [2, 0, 0], [4, 0, 0]])
    np.testing.assert_array_equal(fn(s, attr, t), np.array([[255, 255], [128, 128], [0, 1]], np.uint8))


def test_host_recolour_equals_definition(golden):
    a, ca, b, _ = case_of(golden, 3)
    np.testing.assert_array_equal(pe.recolour(a, ca, b), ref.recolour(a, ca, b))
    np.testing.assert_array_equal(pe.recolour(b, ca[:len(b), :1], a), ref.recolour(b, ca[:len(b), :1], a))


def test_host_keeps_the_30_lowest_rows():
    # 48 lattice points at squared distance 14 round one centre, rows shuffled: only the 30 lowest rows count
    g = np.stack(np.meshgrid(*[np.arange(-3, 4)] * 3, indexing='ij'), -1).reshape(-1, 3)
    ring = g[(g * g).sum(1) == 14] + 10
    assert len(ring) == 48
    rng = np.random.default_rng(2)
    ring = ring[rng.permutation(48)]
    attr = rng.integers(0, 256, size=(48, 3)).astype(np.uint8)
    centre = np.array([[10, 10, 10]])
    want = ((2 * attr[:30].astype(np.int64).sum(0) + 30) // 60).astype(np.uint8)
    targets = np.concatenate([centre, ring])                   # every source chooses its own copy among the targets, never the centre
    np.testing.assert_array_equal(pe.recolour(ring, attr, targets)[0], want)
    np.testing.assert_array_equal(ref.recolour(ring, attr, targets)[0], want)
    np.testing.assert_array_equal(pe.recolour(ring, attr, targets)[1:], attr)


def test_host_refusals():
    s, attr = np.zeros((2, 3)), np.zeros((2, 3), np.uint8)
    for bad in (lambda: pe.recolour(np.zeros((0, 3)), np.zeros((0, 3), np.uint8), s), lambda: pe.recolour(s, attr, np.zeros((0, 3))),
                lambda: pe.recolour(s, attr[:1], s), lambda: pe.recolour(s, np.zeros((2, 5), np.uint8), s),
                lambda: pe.colour_psnr(s, attr, s, attr[:, :2]), lambda: pe.colour_psnr(s, attr.astype(np.int32), s, attr)):
        with pytest.raises(ValueError):
            bad()


# ---------------------------------------------------------------------------------------------------------------------------- pc_error(color=True)
def test_pc_error_parses_colour_labels_whole(golden, tmp_path, monkeypatch):
    stub = tmp_path / 'pc_error_stub'
    printed = tmp_path / 'printed.txt'
    printed.write_bytes(bytes(golden['p0_stdout']))
    stub.write_text(f'#!/bin/sh\ncat "{printed}"\n')
    stub.chmod(0o755)
    monkeypatch.setattr(pe, '_exe', lambda: str(stub))
    a, ca, b, cb = case_of(golden, 0)
    pa, pb = str(tmp_path / 'a.ply'), str(tmp_path / 'b.ply')
    write_ply_ascii_geo_rgb(pa, a[:5], ca[:5]); write_ply_ascii_geo_rgb(pb, b[:5], cb[:5])
    df = pe.pc_error(pa, pb, res=64, color=True)
    for col in ref.COLUMNS:
        assert df[col][0] == float(golden[ref.golden_key(0, col)]), col
    assert df['h.c[0],    1'][0] != df['c[0],    1'][0]
    assert list(df.columns) == pe.D1_COLUMNS + pe.COLOUR_COLUMNS  # (the same order as the native route)
    assert df['mseF,PSNR (p2point)'][0] == pytest.approx(42.8899)
    plain = pe.pc_error(pa, pb, res=64)
    assert list(plain.columns) == pe.D1_COLUMNS                # the default call is what it was


def test_pc_error_native_colour_route(golden, tmp_path, monkeypatch):
    monkeypatch.setattr(pe, '_exe', lambda: None)
    a, ca, b, cb = case_of(golden, 3)
    pa, pb, pg = str(tmp_path / 'a.ply'), str(tmp_path / 'b.ply'), str(tmp_path / 'g.ply')
    write_ply_ascii_geo_rgb(pa, a, ca); write_ply_ascii_geo_rgb(pb, b, cb); write_ply_ascii_geo(pg, b)
    df = pe.pc_error(pa, pb, res=128, color=True)
    assert list(df.columns) == pe.D1_COLUMNS + pe.COLOUR_COLUMNS
    check_against_printed({c: df[c][0] for c in ref.COLUMNS}, golden, 3)
    assert list(pe.pc_error(pa, pb, res=128).columns) == pe.D1_COLUMNS
    with pytest.raises(ValueError):
        pe.pc_error(pa, pg, res=128, color=True)
