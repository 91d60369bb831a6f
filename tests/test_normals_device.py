"""Estimated normals on the GPU (ops.estimate_normals, csrc/normals.hip) against their definition (tests/normals_reference.py): moments,
count and validity exactly; directions and eigenvalues where the eigen-gap defines them; orientation; a sphere's radial directions;
reproducibility; then the D2 metric, the R-D sweep and the command line on clouds without normals."""
import functools
import itertools
import os

import numpy as np
import pytest
import torch

import normals_reference as nr
from pcgcv2_amd import ops, synthetic
from pcgcv2_amd import pc_error as pe

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
RADII = (1, 9, 16, 64)
GAP = 1e-6                       # rows whose reference eigen-gap (lam1 - lam0) / lam2 is below this have no defined direction


def _rows(xyz, batch=None):
    xyz = np.asarray(xyz, np.int64).reshape(-1, 3)
    b = np.zeros(len(xyz), np.int64) if batch is None else np.asarray(batch, np.int64)
    return np.concatenate([b[:, None], xyz], 1)


def _dev(rows):
    return torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)).to(DEV)


@functools.lru_cache(maxsize=None)
def _cloud(name):
    """named test clouds -> int64 [N,4] rows (read-only)"""
    if name == 'shell7_dup':                                           # 1 000 rows duplicated, all rows shuffled
        base = _cloud('shell7')
        rng = np.random.default_rng(41)
        rows = np.concatenate([base, base[rng.integers(0, len(base), 1000)]])
        rows = rows[rng.permutation(len(rows))]
    elif name == 'two_batch':                                          # batch 1 = batch 0 shifted by (1, 0, 0): they overlap in space
        base = _cloud('shell7')[:, 1:]
        rows = np.concatenate([_rows(base), _rows(base + np.array([1, 0, 0]), np.ones(len(base)))])
    elif name == 'sphere':
        rows = _rows(synthetic._shell_np((32.3, 31.9, 32.1), 20.0))
    else:
        rows = _rows(synthetic.cloud(name).numpy())
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def _ref(name, r2, orient='centroid'):
    return nr.estimate_normals(_cloud(name), r2, orient)


@functools.lru_cache(maxsize=None)
def _got(name, r2, orient='centroid'):
    out = ops.estimate_normals(_dev(_cloud(name)), r2, orient, want_moments=True)
    return tuple(t.cpu().numpy() for t in out)


def _assert_exact(rows, r2, ref=None):
    ref = nr.estimate_normals(rows, r2) if ref is None else ref
    nrm, lam, count, valid, mom = (t.cpu().numpy() for t in ops.estimate_normals(_dev(rows), r2, want_moments=True))
    bad = np.nonzero((mom != ref['moments']).any(1))[0]
    assert len(bad) == 0, (len(bad), rows[bad[:3]].tolist(), mom[bad[:3]].tolist(), ref['moments'][bad[:3]].tolist())
    assert np.array_equal(count, ref['count'])
    assert np.array_equal(valid, ref['valid'])
    assert (nrm[~valid] == 0.0).all()
    return nrm, lam, count, valid, mom


@pytest.mark.parametrize('r2', RADII)
@pytest.mark.parametrize('name', ['shell7', 'noisy_s', 'multi_s', 'solid_ball_s', 'shell7_dup', 'two_batch'])
def test_moments_count_valid_exact(name, r2):
    nrm, lam, count, valid, mom = _got(name, r2)
    ref = _ref(name, r2)
    bad = np.nonzero((mom != ref['moments']).any(1))[0]
    assert len(bad) == 0, (len(bad), _cloud(name)[bad[:3]].tolist(), mom[bad[:3]].tolist(), ref['moments'][bad[:3]].tolist())
    assert count.dtype == np.int32 and np.array_equal(count, ref['count'])
    assert valid.dtype == np.bool_ and np.array_equal(valid, ref['valid'])
    assert (nrm[~valid] == 0.0).all()
    if name == 'solid_ball_s' and r2 == 16:
        assert count.max() == 257                                      # full neighbourhoods
    if name == 'noisy_s':
        assert (count == 1).any()                                      # isolated voxels
    if name == 'multi_s' and r2 == 16:
        assert (valid & (ref['lam'][:, 0] == 0.0)).any() and (~valid & (count >= 3)).any()      # flat sheets (rank 2), rods (rank 1)


def test_two_batches_do_not_see_each_other():
    """every row of either batch has the moments the shell has alone (a cross-batch neighbour would raise k)"""
    alone = _ref('shell7', 16)['moments']
    mom = _got('two_batch', 16)[4]
    assert np.array_equal(mom[:len(alone)], alone) and np.array_equal(mom[len(alone):], alone)


@pytest.mark.parametrize('r2', [1, 16, 64])
def test_corner_voxels_probe_negative_cells(r2):
    """voxels at 0 .. 3 in every corner combination: their neighbour cells lie at negative coordinates and must miss, not wrap"""
    top = (1 << 20) - 1
    for lo in itertools.product((0, top - 3), repeat=3):
        blk = np.array(list(itertools.product(range(4), repeat=3)), np.int64) + np.array(lo)
        _assert_exact(_rows(blk), r2)
    far = np.array([(0, 0, 0), (top, top, top), (0, top, 0), (3, 2, 1), (top - 1, 0, 2)], np.int64)     # (lone voxels at both ends of the range)
    _assert_exact(_rows(far), r2)


def test_pair_across_a_cell_border():
    """(3,0,0) and (7,0,0) are neighbours at r2 = 16 and not at 15; the same pair moved by 0 .. 3 along every axis"""
    for axis in range(3):
        for shift in itertools.product(range(4), repeat=3):
            a = np.array(shift, np.int64)
            b = a.copy()
            a[axis] += 3; b[axis] += 7
            pair = _rows([a, b])
            for r2, k in ((16, 2), (15, 1)):
                count = _assert_exact(pair, r2)[2]
                assert count.tolist() == [k, k], (axis, shift, r2)


def test_arguments_out_of_range_raise():
    c = _dev(_cloud('shell7'))
    for bad in (0, 65, -3, 2.5):
        with pytest.raises((ValueError, ops.PcgcError)):
            ops.estimate_normals(c, bad)
    idx = ops.D2Index(c)
    ball = ops._normals_ball(DEV, 16)
    bufs = [torch.empty(len(c) * 10, dtype=torch.int64, device=DEV) for _ in range(6)]
    for bad in (0, 65):                                                # the C entry point itself refuses: an error code, nothing clamped
        rc = ops.lib().pcgc_normals_estimate(c.data_ptr(), len(c), idx.qs.data_ptr(), idx.perm.data_ptr(), *idx.tables(), ball.data_ptr(), bad, 1,
                                             None, *[b.data_ptr() for b in bufs], 8 * bufs[5].numel(), torch.cuda.current_stream().cuda_stream)
        assert rc < 0 and b'r2' in ops.lib().pcgc_last_error()
    oob = _cloud('shell7').copy()
    oob[5, 1] = -1
    with pytest.raises(ops.PcgcError):
        ops.estimate_normals(_dev(oob))
    oob[5, 1] = 1 << 20
    with pytest.raises(ops.PcgcError):
        ops.estimate_normals(_dev(oob))
    with pytest.raises(ValueError):
        ops.estimate_normals(c, orient='up')
    with pytest.raises(ops.PcgcError):
        ops.estimate_normals(c, index=ops.D2Index(_dev(_cloud('sparse_s'))))


@pytest.mark.parametrize('name,cap', [('shell7', 0.0), ('sparse_s', 0.0), ('noisy_s', 0.05), ('multi_s', 0.01)])
def test_directions_and_eigenvalues(name, cap):
    """Where the reference's eigen-gap is at least 1e-6: |sin| of the angle to the reference eigenvector <= 1e-8 (the eigenvector error is of
    order eps * |S| / gap ~ 2e-16 * 1e6, a decade of margin) and every eigenvalue within 1e-12 lam2.  Below the gap the direction is not
    defined: unit length and validity only.  The share of such rows is capped per cloud."""
    ref = _ref(name, 16)
    nrm, lam, count, valid, _ = _got(name, 16)
    defined = ref['gap'] >= GAP
    left_out = 1.0 - defined.mean()
    print(f'{name}: {len(defined)} rows, {left_out:.4%} below the gap')
    assert left_out <= cap
    scale = np.maximum(ref['lam'][:, 2], 1.0)
    lam_err = np.abs(lam - ref['lam']).max(1) / scale
    print(f'{name}: eigenvalue error / lam2 max {lam_err.max():.3e}')
    assert (lam_err <= 1e-12).all()
    sel = defined & ref['valid']
    sin = np.linalg.norm(np.cross(nrm[sel], ref['normals'][sel]), axis=1)
    print(f'{name}: |sin| max {sin.max():.3e} over {sel.sum()} rows')
    assert (sin <= 1e-8).all()
    assert np.array_equal(valid, ref['valid'])
    assert np.abs(np.linalg.norm(nrm[valid], axis=1) - 1.0).max() <= 4e-16          # unit length: one rounding of the division per component


@pytest.mark.parametrize('orient', ['centroid', (5.0, -7.0, 300.0), None], ids=['centroid', 'viewpoint', 'none'])
@pytest.mark.parametrize('name', ['shell7', 'multi_s'])
def test_orientation(name, orient):
    ref = _ref(name, 16, orient)
    nrm = _got(name, 16, orient)[0]
    sel = ref['valid'] & (ref['gap'] >= GAP) & (np.abs(ref['dot']) > 1e-6)
    assert sel.mean() > 0.5
    agree = (nrm[sel] * ref['normals'][sel]).sum(1)
    assert (agree > 0).all(), int((agree <= 0).sum())
    assert not np.signbit(nrm[nrm == 0.0]).any()                       # no negative zeros


def test_sphere_normals_are_radial():
    """5 025 voxels on a sphere of radius 20: the definition gives a median angle of 0.97 degrees to the radial direction and 4.01 at the 99th
    percentile; the caps (about 1.5 x) catch a wrong eigenvector, not rounding"""
    rows = _cloud('sphere')
    assert len(rows) == 5025
    nrm, _, _, valid, _ = _got('sphere', 16)
    assert valid.all()
    radial = rows[:, 1:] - np.array([32.3, 31.9, 32.1])
    radial /= np.linalg.norm(radial, axis=1, keepdims=True)
    cos = (nrm * radial).sum(1)
    assert (cos > 0).all()
    ang = np.degrees(np.arccos(np.clip(cos, -1, 1)))
    print(f'sphere: median {np.median(ang):.3f} deg, 99th percentile {np.percentile(ang, 99):.3f} deg')
    assert np.median(ang) <= 1.5 and np.percentile(ang, 99) <= 6.0


def test_reproducible_and_independent_of_row_order():
    rows = _cloud('multi_s')
    a = ops.estimate_normals(_dev(rows), 16, want_moments=True)
    b = ops.estimate_normals(_dev(rows), 16, want_moments=True)
    perm = np.random.default_rng(6).permutation(len(rows))
    c = ops.estimate_normals(_dev(rows[perm]), 16, want_moments=True)
    inv = np.argsort(perm)
    for x, y, z in zip(a, b, c):
        x, y, z = x.cpu().numpy(), y.cpu().numpy(), z.cpu().numpy()
        assert x.tobytes() == y.tobytes()
        assert x.tobytes() == np.ascontiguousarray(z[inv]).tobytes()
    dup, base = _got('shell7_dup', 16), _got('shell7', 16)             # duplicates receive their voxel's result, bit for bit
    key = lambda r: (r[:, 3] << 40) | (r[:, 2] << 20) | r[:, 1]
    src = np.searchsorted(key(_cloud('shell7')), key(_cloud('shell7_dup')))
    for x, y in zip(dup, base):
        assert x.tobytes() == np.ascontiguousarray(y[src]).tobytes()


def test_both_mappings_of_the_moments_pass_agree():
    """the process-wide A/B knob: one wave per cell (default) and one thread per voxel give the same bits"""
    rows = _dev(_cloud('multi_s'))
    lib = ops.lib()
    old = lib.pcgc_set_normals_mapping(1)
    try:
        other = [t.cpu().numpy() for t in ops.estimate_normals(rows, 64, want_moments=True)]
    finally:
        lib.pcgc_set_normals_mapping(old)
    for x, y in zip(_got('multi_s', 64), other):
        assert x.tobytes() == y.tobytes()


def _jitter(pts, amp, seed):
    rng = np.random.default_rng(seed)
    return np.unique(np.clip(pts + rng.integers(-amp, amp + 1, size=pts.shape), 0, None), axis=0)


def test_d2_with_estimated_normals():
    a = _cloud('shell7')
    b = _rows(_jitter(a[:, 1:], 1, seed=3))
    ad, bd = _dev(a), _dev(b)
    est = pe.d2_psnr_device(ad, 'estimate', bd, 256)
    nrm, _, _, valid = pe.estimate_normals_device(ad)
    given = pe.d2_psnr_device(ad, nrm, bd, 256)
    assert est['normals_r2'] == 16 and est['normals_invalid'] == 0 and bool(valid.all())
    assert set(est) == set(given) | {'normals_r2', 'normals_invalid'}
    for k in given:
        assert np.float64(est[k]).tobytes() == np.float64(given[k]).tobytes(), k
    assert np.isfinite(est['mseF,PSNR (p2plane)'])
    r9 = pe.d2_psnr_device(ad, {'r2': 9}, bd, 256)
    assert r9['normals_r2'] == 9 and r9['mse1      (p2point)'] == est['mse1      (p2point)']
    with pytest.raises(ValueError):
        pe.d2_psnr_device(ad, 'guess', bd, 256)


def _write_ply(path, pts):
    with open(path, 'w') as f:
        f.write('ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nend_header\n' % len(pts))
        for q in pts:
            f.write('%d %d %d\n' % tuple(q))


def test_sweep_on_a_cloud_without_normals(tmp_path, monkeypatch):
    import pandas as pd
    from pcgcv2_amd.test import test as sweep, main
    monkeypatch.setattr(pe, '_exe', lambda: None)
    pts = _cloud('shell7')[:, 1:]
    ply = tmp_path / 'shell7.ply'
    _write_ply(ply, pts)
    ckpt = tmp_path / 'r1.pth'
    torch.save({'model': synthetic.synthetic_state_dict()}, str(ckpt))
    plain = sweep(str(ply), [str(ckpt)], str(tmp_path / 'o0'), str(tmp_path / 'r0'), res=128, verbose=False, metric='device')
    est = sweep(str(ply), [str(ckpt)], str(tmp_path / 'o1'), str(tmp_path / 'r1'), res=128, verbose=False, metric='device', estimate_normals=16)
    p2plane = [c for c in est.columns if 'p2plane' in c]
    assert len(p2plane) == 6 and np.isfinite(est[p2plane].to_numpy(dtype=np.float64)).all()
    assert est['normals'][0] == 'estimated' and est['normals_r2'][0] == 16
    assert not any('p2plane' in c or c.startswith('normals') for c in plain.columns)        # without the flag: the D1-only frame of today
    assert [c for c in est.columns if c in plain.columns] == list(plain.columns)
    for c in plain.columns:
        if not c.startswith('time'):
            assert est[c][0] == plain[c][0], c
    main(['--filedir', str(ply), '--outdir', str(tmp_path / 'o2'), '--resultdir', str(tmp_path / 'r2'), '--res', '128', '--ckpts', str(ckpt),
          '--metric', 'device', '--estimate_normals'])
    cli = pd.read_csv(tmp_path / 'r2' / 'shell7.csv')
    assert cli['normals'][0] == 'estimated' and cli['normals_r2'][0] == 16
    assert cli['mseF,PSNR (p2plane)'][0] == pytest.approx(est['mseF,PSNR (p2plane)'][0], rel=1e-12)
    with pytest.raises(ValueError, match='no normals'):                # the host metric has no estimator
        sweep(str(ply), [str(ckpt)], str(tmp_path / 'o3'), str(tmp_path / 'r3'), res=128, verbose=False, estimate_normals=16)


def test_command_line_writes_the_normals(tmp_path, capsys):
    from pcgcv2_amd import estimate_normals as cli
    pts = _cloud('shell7')[:, 1:]
    src, out = tmp_path / 'in.ply', tmp_path / 'out.ply'
    _write_ply(src, pts)
    assert cli.main(['--filedir', str(src), '--out', str(out), '--r2', '9', '--orient', 'none']) == 0
    said = capsys.readouterr().out
    assert f'{len(pts)} points' in said and ' ms' in said and '0 rows without' in said
    xyz, nrm = pe.read_ply_ascii_with_normals(str(out))
    assert np.array_equal(xyz, pts)
    want = _got('shell7', 9, None)[0]
    assert np.array_equal(nrm, want.astype(np.float32).astype(np.float64))
    assert pe.ply_has_normals(str(out))
