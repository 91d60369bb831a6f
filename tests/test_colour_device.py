"""Colours on the GPU (csrc/colour.hip): pc_error.recolour_device and colour_psnr_device against the numpy definition of
tests/colour_reference.py and the vendored binary's printed values (tests/golden/colour_metric.npz); then the public surface: the R-D sweep
with colour=True, coder.py --recolour and python -m pcgcv2_amd.recolour."""
import math
import os

import numpy as np
import pytest
import torch

import colour_reference as ref
from pcgcv2_amd import ops, synthetic
from pcgcv2_amd import pc_error as pe
from pcgcv2_amd._lib import PcgcError, lib
from pcgcv2_amd.data_utils import read_ply_ascii_geo, read_ply_ascii_with_colours, write_ply_ascii_geo, write_ply_ascii_geo_rgb

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'colour_metric.npz')


def _dev(xyz, batch=None):
    xyz = np.asarray(xyz, np.int32)
    b = np.zeros(len(xyz), np.int32) if batch is None else np.asarray(batch, np.int32)
    return torch.from_numpy(np.concatenate([b[:, None], xyz], 1)).to(DEV)


def _jitter(pts, amp, seed):
    rng = np.random.default_rng(seed)
    return np.unique(np.clip(pts + rng.integers(-amp, amp + 1, size=pts.shape), 0, None), axis=0).astype(np.int32)


def _colours(n, seed, channels=3):
    return np.random.default_rng(seed).integers(0, 256, size=(n, channels)).astype(np.uint8)


def _smooth(pts, grid):
    t = np.asarray(pts, np.float64) / grid
    rgb = np.stack([255 * t[:, 0], 127.5 * (1 + np.sin(5 * t[:, 1])), 255 * t[:, 2] * t[:, 0]], 1)
    return np.clip(np.rint(rgb), 0, 255).astype(np.uint8)


def _recolour(s, attr, t, bs=None, bt=None):
    return pe.recolour_device(_dev(s, bs), torch.from_numpy(attr), _dev(t, bt)).cpu().numpy()


@pytest.fixture(scope='module')
def shell8():
    return synthetic.shell('shell8').numpy()


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


# ---------------------------------------------------------------------------------------------------------------------------- recolour
@pytest.mark.parametrize('amp', [1, 3])
def test_recolour_shell8_jitter(shell8, amp):
    t = _jitter(shell8, amp, seed=amp)
    attr = _colours(len(shell8), 10 + amp)
    got = _recolour(shell8, attr, t)
    assert got.dtype == np.uint8 and got.shape == (len(t), 3)
    np.testing.assert_array_equal(got, ref.recolour(shell8, attr, t))


def test_recolour_targets_that_receive_nothing(shell8):
    """S is every third point of the shell, T the whole shell jittered: most targets are nobody's nearest and average their own tie set"""
    s = shell8[::3].copy()
    t = _jitter(shell8, 1, seed=7)
    attr = _colours(len(s), 3)
    np.testing.assert_array_equal(_recolour(s, attr, t), ref.recolour(s, attr, t))


def _ring48(centre):
    g = np.stack(np.meshgrid(*[np.arange(-3, 4)] * 3, indexing='ij'), -1).reshape(-1, 3)
    return (g[(g * g).sum(1) == 14] + np.asarray(centre)).astype(np.int32)


def test_recolour_more_than_30_ties_keeps_the_lowest_rows():
    """three rings of 48 points at d2 = 14 round single centres, rows shuffled, in both directions"""
    rng = np.random.default_rng(5)
    centres = [(20, 20, 20), (40, 20, 30), (30, 45, 25)]
    ring = np.concatenate([_ring48(c) for c in centres])
    ring = ring[rng.permutation(len(ring))]
    lone = np.array(centres, np.int32)
    for s, t in ((lone, ring), (ring, lone)):
        attr = _colours(len(s), len(s))
        np.testing.assert_array_equal(_recolour(s, attr, t), ref.recolour(s, attr, t))
    # a centre that no ring point chose (each has its own copy among the targets) averages the 30 lowest of its 48 ties
    t = np.concatenate([lone[:1], ring])
    attr = _colours(len(ring), 77)
    got = _recolour(ring, attr, t)
    own = np.sort(np.nonzero(((ring.astype(np.int64) - lone[0]) ** 2).sum(1) == 14)[0])[:30]
    np.testing.assert_array_equal(got[0], ref.round_half_up_mean(attr[own]).astype(np.uint8))
    np.testing.assert_array_equal(got, ref.recolour(ring, attr, t))


def test_recolour_duplicated_rows_are_points_of_their_own():
    rng = np.random.default_rng(11)
    base_s = rng.integers(0, 14, size=(1500, 3)).astype(np.int32)
    base_t = rng.integers(0, 14, size=(1200, 3)).astype(np.int32)
    s = np.concatenate([base_s, base_s[rng.integers(0, len(base_s), 400)]])[rng.permutation(1900)]
    t = np.concatenate([base_t, base_t[rng.integers(0, len(base_t), 300)], base_t[:5], base_t[:5]])
    t = t[rng.permutation(len(t))]
    attr = _colours(len(s), 12)
    assert ref.max_tie_set(s, t) <= ref.TIES and ref.max_tie_set(t, s) <= ref.TIES
    np.testing.assert_array_equal(_recolour(s, attr, t), ref.recolour(s, attr, t))


def test_recolour_batch_items_do_not_see_each_other():
    """item 1 overlaps item 0 (a cross-item neighbour would be nearer): expected from the definition with item b moved by b * 10^4"""
    sh = synthetic.shell('shell7').numpy()[::2]
    s0, s1 = sh, sh + np.array([1, 0, 0], np.int32)
    t0, t1 = _jitter(sh, 1, seed=1), _jitter(sh, 2, seed=2)
    s, t = np.concatenate([s0, s1]), np.concatenate([t0, t1])
    bs, bt = np.repeat([0, 1], [len(s0), len(s1)]), np.repeat([0, 1], [len(t0), len(t1)])
    attr = _colours(len(s), 13)
    want = ref.recolour(ref.shifted(np.concatenate([bs[:, None], s], 1)), attr, ref.shifted(np.concatenate([bt[:, None], t], 1)))
    np.testing.assert_array_equal(_recolour(s, attr, t, bs, bt), want)
    np.testing.assert_array_equal(want[:len(t0)], ref.recolour(s0, attr[:len(s0)], t0))


@pytest.mark.parametrize('gap', [45, 300])
def test_recolour_far_apart_clouds(gap):
    rng = np.random.default_rng(gap)
    s = np.unique(rng.integers(0, 24, size=(1500, 3)), axis=0).astype(np.int32)
    t = np.unique(rng.integers(0, 24, size=(1300, 3)), axis=0).astype(np.int32) + np.array([gap, 3, 0], np.int32)
    t = np.concatenate([t, s[:20] + 1])                              # (a few near points: both kinds in one call)
    attr = _colours(len(s), gap)
    np.testing.assert_array_equal(_recolour(s, attr, t), ref.recolour(s, attr, t))
    back = _colours(len(t), gap + 1)
    np.testing.assert_array_equal(_recolour(t, back, s), ref.recolour(t, back, s))


@pytest.mark.parametrize('channels', [1, 3, 4])
def test_recolour_one_target_chosen_by_5000_sources(channels):
    """255 * 5000 needs more than 16 bits: a narrow accumulator would wrap"""
    rng = np.random.default_rng(9)
    s = np.unique(rng.integers(0, 40, size=(9000, 3)), axis=0)[:5000].astype(np.int32)
    assert len(s) == 5000
    attr = np.full((5000, channels), 255, np.uint8)
    got = _recolour(s, attr, np.array([[20, 20, 20]], np.int32))
    np.testing.assert_array_equal(got, np.full((1, channels), 255, np.uint8))


@pytest.mark.parametrize('channels', [1, 3, 4])
def test_recolour_channel_counts(channels):
    s = synthetic.shell('shell7').numpy()
    t = _jitter(s, 2, seed=4)[::2]
    attr = _colours(len(s), 20 + channels, channels)
    np.testing.assert_array_equal(_recolour(s, attr, t), ref.recolour(s, attr, t))


def test_recolour_does_not_depend_on_the_row_order_of_the_source():
    s = synthetic.shell('shell7').numpy()
    t = _jitter(s, 2, seed=6)
    assert ref.max_tie_set(s, t) <= ref.TIES and ref.max_tie_set(t, s) <= ref.TIES
    attr = _colours(len(s), 21)
    perm = np.random.default_rng(22).permutation(len(s))
    np.testing.assert_array_equal(_recolour(s[perm], attr[perm], t), _recolour(s, attr, t))


def test_recolour_permutation_and_two_runs(shell8):
    attr = _colours(len(shell8), 23)
    perm = np.random.default_rng(24).permutation(len(shell8))
    np.testing.assert_array_equal(_recolour(shell8, attr, shell8[perm]), attr[perm])
    t = _jitter(shell8, 3, seed=9)
    assert _recolour(shell8, attr, t).tobytes() == _recolour(shell8, attr, t).tobytes()


def test_recolour_accepts_sparse_tensors_and_shared_searches(shell8):
    from pcgcv2_amd.sparse import SparseTensor
    a, b = _dev(shell8), _dev(_jitter(shell8, 1, seed=2))
    xa = SparseTensor(torch.ones((len(a), 1), device=DEV), coordinates=a, tensor_stride=1, device=DEV)
    xb = SparseTensor(torch.ones((len(b), 1), device=DEV), coordinates=b, tensor_stride=1, device=DEV)
    attr = torch.from_numpy(_colours(len(xa.C), 25)).to(DEV)         # (colours of the tensor's own rows)
    want = pe.recolour_device(xa.C, attr, xb.C)
    assert torch.equal(pe.recolour_device(xa, attr, xb), want)
    assert torch.equal(pe.recolour_device(xa.C, attr, xb.C, nn=pe.nn_both(xa.C.contiguous(), xb.C.contiguous())), want)
    np.testing.assert_array_equal(want.cpu().numpy(), ref.recolour(xa.C[:, 1:].cpu().numpy(), attr.cpu().numpy(), xb.C[:, 1:].cpu().numpy()))


def test_recolour_decode_batch_outputs(tmp_path):
    """the decoder's batched outputs recoloured in one call through the batch index equal the items recoloured alone"""
    from pcgcv2_amd.coder import Coder
    from pcgcv2_amd.pcc_model import PCCModel
    from pcgcv2_amd.sparse import SparseTensor, sparse_collate
    sh = synthetic.shell('shell6')
    clouds = [sh, sh + 3]
    coords, feats = sparse_collate(clouds, [torch.ones((len(c), 1)) for c in clouds])
    x = SparseTensor(feats, coordinates=coords, tensor_stride=1, device=DEV)
    model = PCCModel().to(DEV)
    model.load_state_dict(synthetic.synthetic_state_dict())
    coder = Coder(model, str(tmp_path / 'b'))
    coder.encode_batch(x, ['_0', '_1'])
    outs = coder.decode_batch(['_0', '_1'])
    attr = torch.from_numpy(_colours(len(x.C), 30)).to(DEV)
    target = []
    for b, o in enumerate(outs):
        c = o.C.clone()
        c[:, 0] = b
        target.append(c)
    got = pe.recolour_device(x.C, attr, torch.cat(target).contiguous())
    off_s = off_t = 0
    for b, o in enumerate(outs):
        ns, nt = int((x.C[:, 0] == b).sum()), len(o.C)
        src = x.C[off_s:off_s + ns].clone()
        src[:, 0] = 0
        alone = pe.recolour_device(src, attr[off_s:off_s + ns], o.C)
        assert torch.equal(got[off_t:off_t + nt], alone), b
        np.testing.assert_array_equal(alone.cpu().numpy(), ref.recolour(src[:, 1:].cpu().numpy(), attr[off_s:off_s + ns].cpu().numpy(),
                                                                        o.C[:, 1:].cpu().numpy()))
        off_s, off_t = off_s + ns, off_t + nt


# ---------------------------------------------------------------------------------------------------------------------------- metric
def _check_against_printed(got, golden, case):
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


def _same_as_definition(got, want):
    assert list(got) == ref.COLUMNS
    for col in ref.COLUMNS:
        print(repr(col), got[col], want[col])
        if col.startswith('h.'):
            assert got[col] == want[col], col
        elif math.isinf(want[col]):
            assert got[col] == want[col], col
        else:
            assert got[col] == pytest.approx(want[col], rel=1e-12, abs=0), col


def _metric(a, ca, b, cb, **kw):
    return pe.colour_psnr_device(_dev(a), torch.from_numpy(ca), _dev(b), torch.from_numpy(cb), **kw)


@pytest.mark.parametrize('case', range(4))
def test_metric_golden_pairs(golden, case):
    a, ca, b, cb = (golden[f'p{case}_a'].astype(np.int32), golden[f'p{case}_ca'], golden[f'p{case}_b'].astype(np.int32), golden[f'p{case}_cb'])
    got = _metric(a, ca, b, cb)
    _check_against_printed(got, golden, case)
    host = pe.colour_psnr(a, ca, b, cb)
    for col in ref.COLUMNS:                                          # both sum the same integers: not a bit apart
        assert np.float64(got[col]).tobytes() == np.float64(host[col]).tobytes(), col


@pytest.mark.parametrize('amp', [1, 3])
def test_metric_shell8_against_definition(shell8, amp):
    b = _jitter(shell8, amp, seed=amp)
    ca, cb = _colours(len(shell8), 40 + amp), _smooth(b, 256)
    _same_as_definition(_metric(shell8, ca, b, cb), ref.colour_metric(shell8, ca, b, cb))


def test_metric_duplicates_and_ties_against_definition():
    rng = np.random.default_rng(41)
    a = rng.integers(0, 14, size=(1900, 3)).astype(np.int32)
    b = rng.integers(0, 14, size=(1500, 3)).astype(np.int32)
    assert ref.max_tie_set(a, b) <= ref.TIES and ref.max_tie_set(b, a) <= ref.TIES
    ca, cb = _colours(len(a), 42), _colours(len(b), 43)
    _same_as_definition(_metric(a, ca, b, cb), ref.colour_metric(a, ca, b, cb))


def test_metric_per_point_terms(shell8):
    """pcgc_colour_dist's per-point integers against the definition's terms"""
    a = shell8[::5]
    b = _jitter(a, 2, seed=3)
    ca, cb = _colours(len(a), 44), _colours(len(b), 45)
    nn = ops.d2_nn(_dev(a), _dev(b))
    yuv2, rgb2 = ops.colour_dist(torch.from_numpy(ca).to(DEV), torch.from_numpy(cb).to(DEV), nn)
    mean = np.stack([ref.round_half_up_mean(cb[rows]) for rows in ref.tie_sets(a, b)])
    d = ca.astype(np.int64) - mean
    m = np.array([[2126, 7152, 722], [-1146, -3854, 5000], [5000, -4542, -458]], np.int64)
    np.testing.assert_array_equal(yuv2.cpu().numpy(), (d @ m.T) ** 2)
    np.testing.assert_array_equal(rgb2.cpu().numpy(), d * d)
    red = ops.colour_reduce(yuv2, rgb2).cpu().numpy()
    y2 = (d @ m.T) ** 2
    np.testing.assert_array_equal(red[:3], (y2 & 0xFFFFFFFF).sum(0))
    np.testing.assert_array_equal(red[3:6], (y2 >> 32).sum(0))
    np.testing.assert_array_equal(red[6:], (d * d).max(0))


def test_metric_two_runs_and_shared_searches(shell8):
    b = _jitter(shell8, 3, seed=9)
    ca, cb = _colours(len(shell8), 46), _colours(len(b), 47)
    m1, m2 = _metric(shell8, ca, b, cb), _metric(shell8, ca, b, cb)
    a_dev, b_dev = _dev(shell8), _dev(b)
    ia, ib = ops.D2Index(a_dev), ops.D2Index(b_dev)                  # (the searches d2_psnr_device makes)
    m3 = pe.colour_psnr_device(a_dev, torch.from_numpy(ca), b_dev, torch.from_numpy(cb), nn=(ops.d2_nn(a_dev, ib), ops.d2_nn(b_dev, ia)))
    assert list(m1) == list(m2) == list(m3) == ref.COLUMNS
    for col in ref.COLUMNS:
        assert np.float64(m1[col]).tobytes() == np.float64(m2[col]).tobytes() == np.float64(m3[col]).tobytes(), col


def test_d2_with_shared_searches_is_unchanged(shell8):
    b = _dev(_jitter(shell8, 1, seed=1))
    a = _dev(shell8)
    v = shell8 - shell8.mean(0)
    na = torch.from_numpy(v / np.linalg.norm(v, axis=1, keepdims=True))
    m1, m2 = pe.d2_psnr_device(a, na, b, 256), pe.d2_psnr_device(a, na, b, 256, nn=pe.nn_both(a, b))
    assert m1 == m2


# ---------------------------------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope='module')
def coloured_shell7(tmp_path_factory):
    d = tmp_path_factory.mktemp('colour_e2e')
    pts = synthetic.shell('shell7').numpy()
    rgb = _smooth(pts, 128)
    ply = d / 'shell7c.ply'
    write_ply_ascii_geo_rgb(str(ply), pts, rgb)
    ckpts = []
    for i, gain in enumerate((10.0, 50.0)):
        p = d / f'r{i + 1}.pth'
        torch.save({'model': synthetic.synthetic_state_dict(gain=gain)}, str(p))
        ckpts.append(str(p))
    return d, str(ply), pts, rgb, ckpts


def test_sweep_colour_device_equals_host(coloured_shell7, monkeypatch):
    from pcgcv2_amd.test import test as sweep
    d, ply, pts, rgb, ckpts = coloured_shell7
    monkeypatch.setattr(pe, '_exe', lambda: None)
    host = sweep(ply, ckpts, str(d / 'oh'), str(d / 'rh'), res=128, verbose=False, colour=True)
    dev = sweep(ply, ckpts, str(d / 'od'), str(d / 'rd'), res=128, verbose=False, metric='device', colour=True)
    assert list(host.columns) == list(dev.columns)
    assert all(c in dev.columns for c in ref.COLUMNS)
    for r in range(len(ckpts)):
        for col in ref.COLUMNS:
            if col.startswith('h.') or math.isinf(host[col][r]):
                assert dev[col][r] == host[col][r], (r, col)
            else:
                assert dev[col][r] == pytest.approx(host[col][r], rel=1e-12, abs=0), (r, col)
    for out in ('oh', 'od'):
        xyz, got = read_ply_ascii_with_colours(str(d / out / 'shell7c_r2_dec.ply'))
        np.testing.assert_array_equal(got, ref.recolour(pts, rgb, xyz.astype(np.int64)))
    plain = sweep(ply, ckpts[:1], str(d / 'op'), str(d / 'rp'), res=128, verbose=False, metric='device')
    assert not any(c in plain.columns for c in ref.COLUMNS)
    assert read_ply_ascii_with_colours(str(d / 'op' / 'shell7c_r1_dec.ply'))[1] is None


def test_coder_and_recolour_cli(coloured_shell7, capsys):
    from pcgcv2_amd import coder, recolour
    from pcgcv2_amd.pcc_model import PCCModel
    d, ply, pts, rgb, ckpts = coloured_shell7
    coder.main(['--ckptdir', ckpts[1], '--filedir', ply, '--outdir', str(d / 'plain'), '--res', '128'])
    assert 'Colour PSNR' not in capsys.readouterr().out
    plain = (d / 'plain' / 'shell7c_dec.ply').read_bytes()
    model = PCCModel().to(DEV)
    model.load_state_dict(torch.load(ckpts[1], map_location=DEV)['model'])
    decoded = coder.Coder(model, str(d / 'plain' / 'shell7c')).decode().C[:, 1:].cpu().numpy()
    write_ply_ascii_geo(str(d / 'expected.ply'), decoded)
    assert plain == (d / 'expected.ply').read_bytes()                # without the flag: byte for byte the geometry-only file

    coder.main(['--ckptdir', ckpts[1], '--filedir', ply, '--outdir', str(d / 'col'), '--res', '128', '--recolour'])
    printed = capsys.readouterr().out
    xyz, got = read_ply_ascii_with_colours(str(d / 'col' / 'shell7c_dec.ply'))
    np.testing.assert_array_equal(xyz, decoded)
    want = ref.recolour(pts, rgb, decoded)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(read_ply_ascii_geo(str(d / 'col' / 'shell7c_dec.ply')), decoded)
    y = ref.colour_metric(pts, rgb, decoded, want)['c[0],PSNRF']
    line = [l for l in printed.splitlines() if l.startswith('Colour PSNR (Y)')]
    assert len(line) == 1 and float(line[0].split('\t')[-1]) == pytest.approx(y, rel=1e-12)

    m = recolour.main(['--source', ply, '--target', str(d / 'plain' / 'shell7c_dec.ply'), '--out', str(d / 'cli_rgb.ply'), '--metric'])
    xyz, got = read_ply_ascii_with_colours(str(d / 'cli_rgb.ply'))
    np.testing.assert_array_equal(xyz, decoded)
    np.testing.assert_array_equal(got, want)
    assert m['c[0],PSNRF'] == pytest.approx(y, rel=1e-12)
    assert 'Colour PSNR (Y)' in capsys.readouterr().out


# ---------------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals(tmp_path):
    from pcgcv2_amd.test import test as sweep
    s = _dev(np.array([[1, 2, 3], [4, 5, 6]]))
    empty = _dev(np.zeros((0, 3)))
    attr = torch.zeros((2, 3), dtype=torch.uint8)
    bad = [lambda: pe.recolour_device(empty, attr[:0], s), lambda: pe.recolour_device(s, attr, empty),
           lambda: pe.recolour_device(s, attr[:1], s), lambda: pe.recolour_device(s, torch.zeros((2, 5), dtype=torch.uint8), s),
           lambda: pe.recolour_device(s, attr.float(), s), lambda: pe.colour_psnr_device(s, attr, empty, attr[:0]),
           lambda: pe.colour_psnr_device(s, attr, s, attr[:1]), lambda: pe.colour_psnr_device(s, attr[:, :2], s, attr),
           lambda: pe.colour_psnr_device(empty, attr[:0], s, attr)]
    for fn in bad:
        with pytest.raises((ValueError, PcgcError)):
            fn()
    nn = pe.nn_both(s, s)
    with pytest.raises((ValueError, PcgcError)):
        ops.attr_transfer(2, nn[0], torch.zeros((2, 5), dtype=torch.uint8, device=DEV), nn[1])
    with pytest.raises((ValueError, PcgcError)):
        ops.attr_transfer(3, nn[0], attr.to(DEV), nn[1])
    # the library itself refuses what its 32-bit accumulator fields cannot hold, and a channel count it does not know (before touching memory)
    assert lib().pcgc_attr_transfer(None, None, None, 0xFFFFFFFF // 255 + 1, None, None, None, 10, None, 3, None, None, 0, None) == -2
    assert lib().pcgc_attr_transfer(None, None, None, 10, None, None, None, 10, None, 5, None, None, 0, None) == -2
    assert pe.recolour_device(s, attr, s).cpu().tolist() == attr.tolist()      # (and nothing is left broken)
    geo = tmp_path / 'geo.ply'
    write_ply_ascii_geo(str(geo), synthetic.shell('shell6').numpy())
    torch.save({'model': synthetic.synthetic_state_dict()}, str(tmp_path / 'r1.pth'))
    for metric in ('host', 'device'):
        with pytest.raises(ValueError, match='colours'):
            sweep(str(geo), [str(tmp_path / 'r1.pth')], str(tmp_path / 'o'), str(tmp_path / 'r'), res=64, verbose=False, metric=metric, colour=True)
