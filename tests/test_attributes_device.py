"""The colour codec on the GPU (csrc/raht.hip, pcgcv2_amd/attributes.py): every array the kernels produce — tree fields, H, tokens,
contexts, escapes, histogram, the bytes of `_A.bin`, the decoded colours — EQUAL to the numpy definition (tests/raht_reference.py), at the
smallest shapes at which the code can go wrong; both forms of the transform; then AttributeCoder on a shell and coder.py --attributes."""
import os

import numpy as np
import pytest
import torch

import raht_reference as R
from pcgcv2_amd import attributes as at, ops, synthetic
from pcgcv2_amd._lib import PcgcError
from pcgcv2_amd.data_utils import read_ply_ascii_with_colours, write_ply_ascii_geo_rgb

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
T = 1024                                                        # pcgc_raht_tile_leaves(), asserted below
QSTEPS = [(0, 0), (1, 4), (4, 1), (16, 64), (64, 16), (255, 3)]


# ---- geometry --------------------------------------------------------------------------------------------------------------------------------
def _line(n, x0=0):
    x = np.arange(x0, x0 + n, dtype=np.int64)
    return np.stack([x, np.zeros_like(x), np.zeros_like(x)], 1)


def _two_lines(n):
    """101 voxels on one line, the rest far away in z: the root's gap (100) lies inside the first tile, its range is the whole cloud; the
    second line starts at x = 5, so small subtrees straddle the tile boundaries as well"""
    a, b = _line(min(101, n - 1)), _line(n - min(101, n - 1), 5)
    b[:, 2] = 1 << 12
    return np.concatenate([a, b])


def _random_cloud(n, grid, seed):
    rng = np.random.default_rng(seed)
    pts = np.unique(rng.integers(0, grid, size=(3 * n, 3)), axis=0)
    return pts[rng.permutation(len(pts))[:n]].astype(np.int64)


def _chain():
    x = np.array([0] + [1 << i for i in range(20)], np.int64)
    return np.stack([x, np.zeros_like(x), np.zeros_like(x)], 1)


TOP = (1 << 20) - 1
GEOMETRY = {
    'one': lambda: np.array([[7, 8, 9]]),
    'two': lambda: np.array([[7, 8, 9], [1, 2, 3]]),
    'three': lambda: np.array([[7, 8, 9], [1, 2, 3], [1, 2, 2]]),
    'pair_bit59': lambda: np.array([[3, 4, 1 << 19], [3, 4, 0]]),
    'pair_bit0': lambda: np.array([[7, 4, 9], [6, 4, 9]]),
    'block': lambda: np.array([[x, y, z] for z in range(2) for y in range(2) for x in range(2)]) + 6,
    'chain': _chain,
    'corner': lambda: np.array([[TOP, TOP, TOP], [TOP - 1, TOP, TOP], [0, 0, 0], [TOP, 0, TOP], [0, TOP, 0], [TOP, TOP, 0]]),
    'random': lambda: _random_cloud(3000, 48, 4),
}
for _n in (T - 1, T, T + 1, 2 * T + 1):
    GEOMETRY[f'line{_n}'] = lambda n=_n: _line(n)
    GEOMETRY[f'straddle{_n}'] = lambda n=_n: _line(n, 3)       # leaf i is x = i + 3: the subtrees of aligned x straddle every tile boundary
    GEOMETRY[f'leaving{_n}'] = lambda n=_n: _two_lines(n)


def _colours(kind, pts, seed=0):
    n = len(pts)
    if kind == 'equal':
        return np.full((n, 3), 77, np.uint8)
    if kind == 'random':
        return np.random.default_rng(seed).integers(0, 256, (n, 3)).astype(np.uint8)
    _, perm = R.sort_cloud(pts)                                 # 0 / 255 alternating along Morton order, blue against red and green
    i = np.arange(n)
    rgb = np.zeros((n, 3), np.uint8)
    rgb[perm] = np.stack([255 * (i & 1), 255 * (i & 1), 255 * ((i + 1) & 1)], 1).astype(np.uint8)
    return rgb


def _coords(pts):
    pts = np.asarray(pts, np.int32)
    return torch.from_numpy(np.concatenate([np.zeros((len(pts), 1), np.int32), pts], 1)).to(DEV)


def _np(t):
    return t.cpu().numpy()


@pytest.fixture(scope='module')
def definition():
    """the definition's tree per geometry, computed once"""
    cache = {}

    def get(name):
        if name not in cache:
            pts = np.asarray(GEOMETRY[name](), np.int64)
            rng = np.random.default_rng(len(pts))
            pts = pts[rng.permutation(len(pts))]                # (the caller's row order is not the Morton order)
            keys, perm = R.sort_cloud(pts)
            cache[name] = (pts, keys, perm, R.build_tree(keys))
        return cache[name]
    return get


def test_tile_leaves():
    assert ops.raht_tile_leaves() == T


# ---- every array against the definition ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(GEOMETRY))
def test_tree_equals_the_definition(definition, name):
    pts, keys, perm, ref = definition(name)
    tree = ops.raht_tree(_coords(pts))
    assert tree.n == len(pts)
    assert np.array_equal(_np(tree.keys).view(np.uint64), keys) and np.array_equal(_np(tree.perm), perm)
    for field in ('d', 'lo', 'hi', 'left', 'right', 'order', 'w1', 'w2'):
        assert np.array_equal(_np(getattr(tree, field)).astype(np.int64), ref[field]), field
    assert np.array_equal(tree.bucket, ref['bucket'])
    # the crossing list: exactly the gaps whose range crosses a multiple of T, in coding order
    crossing = (ref['lo'] // T) != (ref['hi'] // T)
    want = ref['order'][crossing[ref['order']]]
    assert tree.cross[-1] == want.size and np.array_equal(_np(tree.cross_order)[:want.size], want)
    assert np.array_equal(np.diff(tree.cross), np.bincount(63 - ref['d'][crossing], minlength=64))
    if name.startswith('leaving') and len(pts) > T:
        inside = (np.arange(len(pts) - 1) % T != T - 1) & crossing
        assert inside.any()                                     # a gap inside a tile whose range leaves it
    if name.startswith('straddle') and len(pts) > T:
        assert (ref['d'][crossing] <= 2).any()                  # a small subtree over a tile boundary


@pytest.mark.parametrize('name', sorted(GEOMETRY))
def test_transform_and_tokens_equal_the_definition(definition, name):
    pts, keys, perm, ref = definition(name)
    tree = ops.raht_tree(_coords(pts))
    for kind in ('random', 'equal', 'alternating'):
        rgb = _colours(kind, pts, 5)
        rgb_d = torch.from_numpy(rgb).to(DEV)
        H_ref, dc_ref = R.forward(ref, R.ycocg_forward(rgb[perm]))
        results = {form: ops.raht_forward(tree, rgb_d, form=form) for form in ops.RAHT_FORMS}
        for form, (H, dc) in results.items():
            assert np.array_equal(_np(H), H_ref), (kind, form)
            assert _np(dc).tolist() == dc_ref.tolist(), (kind, form)
        if kind == 'equal':
            assert not H_ref.any()
        if kind == 'alternating' and len(pts) > 2:
            assert np.abs(H_ref).max() == 510
        H = results[ops.RAHT_FORM][0]
        for ql, qc in (QSTEPS if kind == 'random' else QSTEPS[:2]):
            D16 = R.steps(ref, ql, qc)
            k = R.quantize(H_ref, D16)
            tok_r, ctx_r, esc_r, hist_r = R.tokens(ref, k)
            tok, ctx, esc, hist = ops.raht_quantize(tree, H, ql, qc)
            assert np.array_equal(_np(tok), tok_r) and np.array_equal(_np(ctx).view(np.uint16), ctx_r), (kind, ql, qc)
            assert np.array_equal(_np(esc).view(np.uint16), esc_r) and np.array_equal(_np(hist), hist_r), (kind, ql, qc)
            assert np.array_equal(at.contexts(tree.bucket), ctx_r)
            if kind == 'equal':
                assert not tok_r.any()
            if kind == 'alternating' and ql == 0 and len(pts) > 2:
                assert esc_r.size > 0                           # the escape path
            Hh_ref = R.dequantize(k, D16)
            Hh = ops.raht_dequantize(tree, tok, esc, ql, qc)
            assert np.array_equal(_np(Hh), Hh_ref), (kind, ql, qc)
            want = np.zeros((len(pts), 3), np.uint8)
            want[perm] = R.ycocg_inverse(R.inverse(ref, Hh_ref, dc_ref))
            for form in ops.RAHT_FORMS:
                got = _np(ops.raht_inverse(tree, Hh, dc_ref.tolist(), form=form))
                assert np.array_equal(got, want), (kind, ql, qc, form)
            if ql == 0 and qc == 0:
                assert np.array_equal(want, rgb)


@pytest.mark.parametrize('name', ['one', 'two', 'chain', 'corner', f'line{T}', f'straddle{2 * T + 1}', f'leaving{T + 1}', 'random'])
def test_file_equals_the_definition(definition, name, tmp_path):
    pts, keys, perm, ref = definition(name)
    coords = _coords(pts)
    for kind, (ql, qc) in (('random', (0, 0)), ('random', (4, 16)), ('alternating', (1, 1)), ('equal', (255, 255))):
        rgb = _colours(kind, pts, 9)
        blob, rec = R.encode(pts, rgb, ql, qc, ops.rc_encode_ctx, ops.crc32)
        for form in ops.RAHT_FORMS:
            coder = at.AttributeCoder(str(tmp_path / f'{name}_{form}'), form=form)
            record = coder.encode(coords, torch.from_numpy(rgb).to(DEV), ql, None if qc == ql else qc)
            with open(str(tmp_path / f'{name}_{form}') + at.SUFFIX, 'rb') as fh:
                assert fh.read() == blob, (kind, ql, qc, form)
            assert record['bits_A'] == 8 * len(blob)
            assert np.array_equal(_np(coder.decode(coords)), rec), (kind, ql, qc, form)
    if name == 'one':
        assert len(blob) == R.HEAD.size + R.SIZES.size + 4      # DC only, no payload


def test_row_order_and_repeatability(definition, tmp_path):
    pts, keys, perm, ref = definition('random')
    rgb = _colours('random', pts, 21)
    a = at.AttributeCoder(str(tmp_path / 'a'))
    a.encode(_coords(pts), torch.from_numpy(rgb).to(DEV), 4, 7)
    first = open(str(tmp_path / 'a') + at.SUFFIX, 'rb').read()
    a.encode(_coords(pts), torch.from_numpy(rgb).to(DEV), 4, 7)
    assert open(str(tmp_path / 'a') + at.SUFFIX, 'rb').read() == first                  # two runs, the same bytes
    shuffle = np.random.default_rng(22).permutation(len(pts))
    b = at.AttributeCoder(str(tmp_path / 'b'))
    b.encode(_coords(pts[shuffle]), torch.from_numpy(rgb[shuffle]).to(DEV), 4, 7)
    assert open(str(tmp_path / 'b') + at.SUFFIX, 'rb').read() == first                  # shuffled rows, the same bytes
    dec = _np(a.decode(_coords(pts)))
    assert np.array_equal(_np(a.decode(_coords(pts[shuffle]))), dec[shuffle])           # the decode comes back in the given row order
    assert np.array_equal(_np(a.decode(torch.from_numpy(pts[shuffle].astype(np.int32)).to(DEV))), dec[shuffle])     # [N,3] rows too


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals(tmp_path):
    pts = _random_cloud(50, 16, 1)
    rgb = torch.from_numpy(_colours('random', pts)).to(DEV)
    coder = at.AttributeCoder(str(tmp_path / 'r'))
    dup = np.concatenate([pts, pts[:1]])
    with pytest.raises(ValueError, match='duplicate'):
        ops.raht_tree(_coords(dup))
    with pytest.raises(ValueError, match='duplicate'):
        coder.encode(_coords(dup), torch.cat([rgb, rgb[:1]]), 4)
    batch = _coords(pts)
    batch[25:, 0] = 1
    with pytest.raises(ValueError, match='one frame'):
        coder.encode(batch, rgb, 4)
    for bad in (-1, 1 << 20):
        far = pts.copy()
        far[3, 1] = bad
        with pytest.raises(ValueError, match='outside'):
            coder.encode(_coords(far), rgb, 4)
    with pytest.raises(ValueError):
        coder.encode(_coords(pts), rgb, 256)
    with pytest.raises(ValueError):
        coder.encode(_coords(pts), rgb[:-1], 4)
    with pytest.raises(ValueError):
        ops.raht_tree(_coords(pts[:0]))
    assert ops.lib().pcgc_raht_keys(None, (1 << 24) + 1, None, None, None, None, 0, None) == -2      # refused before anything is touched
    assert ops.lib().pcgc_raht_tree(None, (1 << 24) + 1, None, None, None, None, None, None, None, None, None, 0, None) == -2
    assert not os.path.exists(str(tmp_path / 'r') + at.SUFFIX)
    coder.encode(_coords(pts), rgb, 4)
    with pytest.raises(PcgcError, match='points'):
        coder.decode(_coords(pts[:-1]))
    with pytest.raises(PcgcError):
        coder.decode(_coords(_random_cloud(50, 200, 2)))         # another geometry of the same size
    tree = ops.raht_tree(_coords(pts))
    tok = torch.full((3 * 49,), 63, dtype=torch.int16, device=DEV)
    with pytest.raises(PcgcError, match='escape'):
        ops.raht_dequantize(tree, tok, torch.zeros(5, dtype=torch.int16, device=DEV), 1, 1)


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------
def _field(pts_d):
    """the colour field of tools/recolour_time.py"""
    t = pts_d.double() / float(pts_d.max() + 1)
    rgb = torch.stack([255 * t[:, 0], 127.5 * (1 + torch.sin(40 * t[:, 1])), 255 * t[:, 2] * t[:, 0]], 1)
    noise = torch.randint(-12, 13, rgb.shape, device=pts_d.device, generator=torch.Generator(device=pts_d.device).manual_seed(1))
    return (rgb + noise).round().clamp(0, 255).to(torch.uint8)


def test_attribute_coder_on_a_shell(tmp_path):
    pts_d = synthetic.cloud('shell8', device=DEV)
    rgb_d = _field(pts_d)
    pts, rgb = _np(pts_d).astype(np.int64), _np(rgb_d)
    coder = at.AttributeCoder(str(tmp_path / 'shell8'))
    sizes = []
    for q in (0, 8, 32):
        blob, rec = R.encode(pts, rgb, q, q, ops.rc_encode_ctx, ops.crc32)
        record = coder.encode(pts_d, rgb_d, q)
        assert open(str(tmp_path / 'shell8') + at.SUFFIX, 'rb').read() == blob
        dec = _np(coder.decode(pts_d))
        assert np.array_equal(dec, rec)
        if q == 0:
            assert np.array_equal(dec, rgb)
        sizes.append(record['bits_A'])
    assert sizes[0] > sizes[1] > sizes[2]


@pytest.fixture(scope='module')
def coloured_cloud(tmp_path_factory):
    d = tmp_path_factory.mktemp('attr_e2e')
    pts = synthetic.shell('shell7').numpy()
    t = np.asarray(pts, np.float64) / 128
    rgb = np.clip(np.rint(np.stack([255 * t[:, 0], 127.5 * (1 + np.sin(5 * t[:, 1])), 255 * t[:, 2] * t[:, 0]], 1)), 0, 255).astype(np.uint8)
    ply = d / 'shell7c.ply'
    write_ply_ascii_geo_rgb(str(ply), pts, rgb)
    ckpt = d / 'r.pth'
    torch.save({'model': synthetic.synthetic_state_dict(gain=50.0)}, str(ckpt))
    return d, str(ply), pts, rgb, str(ckpt)


def _printed(out, label):
    return [line.split('\t')[-1].strip() for line in out.splitlines() if line.startswith(label)]


def test_coder_attributes_cli(coloured_cloud, capsys):
    from pcgcv2_amd import coder
    d, ply, pts, rgb, ckpt = coloured_cloud
    coder.main(['--ckptdir', ckpt, '--filedir', ply, '--outdir', str(d / 'plain'), '--res', '128'])
    plain = capsys.readouterr().out
    coder.main(['--ckptdir', ckpt, '--filedir', ply, '--outdir', str(d / 'lossy'), '--res', '128', '--attributes', '8'])
    out = capsys.readouterr().out
    psnr = _printed(out, 'Colour PSNR (Y)')
    assert len(psnr) == 1 and np.isfinite(float(psnr[0]))
    bits = _printed(out, 'bits _A.bin')
    assert len(bits) == 1 and int(bits[0]) == 8 * os.path.getsize(str(d / 'lossy' / 'shell7c_A.bin'))
    assert _printed(out, 'bpps:') == _printed(plain, 'bpps:') and _printed(out, 'bits:') == _printed(plain, 'bits:')     # the existing figures
    xyz, got = read_ply_ascii_with_colours(str(d / 'lossy' / 'shell7c_dec.ply'))
    assert got is not None and got.shape == (len(xyz), 3)
    # what a decoder gets: `_A.bin` decoded on the geometry of `_dec.ply`
    again = at.AttributeCoder(str(d / 'lossy' / 'shell7c')).decode(_coords(xyz.astype(np.int64)))
    assert np.array_equal(_np(again), got)


def test_lossless_attributes_zero_returns_the_colours(coloured_cloud, capsys):
    from pcgcv2_amd import coder
    d, ply, pts, rgb, ckpt = coloured_cloud
    coder.main(['--ckptdir', ckpt, '--filedir', ply, '--outdir', str(d / 'exact'), '--lossless', '--attributes', '0'])
    out = capsys.readouterr().out
    assert _printed(out, 'Colour PSNR (Y)') == ['inf']
    assert len(_printed(out, 'bits _A.bin')) == 1
    xyz, got = read_ply_ascii_with_colours(str(d / 'exact' / 'shell7c_dec.ply'))
    a = np.concatenate([xyz.astype(np.int64), got], 1)
    b = np.concatenate([np.asarray(pts, np.int64), rgb], 1)
    assert np.array_equal(a[np.lexsort(a.T[::-1])], b[np.lexsort(b.T[::-1])])
