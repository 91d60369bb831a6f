"""The sparse-conv operators against an independent float64 definition (tests/fp64_reference.py).

Every other conv test compares the HIP kernels with the CPU oracle bit for bit: the same fp32 fmaf chain, but the oracle is this project's
own restatement of MinkowskiEngine.  Here the definition is pinned to torch's dense conv3d / conv_transpose3d, and the oracle (CPU part)
and every kernel family (GPU part) must stay within the running fp32 error bound of it.  A mutation of the definition (mirrored offsets,
swapped cat halves, ...) must break that tolerance: the bound is tight enough to see a wrong convolution."""
import numpy as np
import pytest
import torch

import fp64_reference as R
from oracle import pcgc_oracle as orc
from pcgcv2_amd import conventions, synthetic

# every bound must stay below TIGHT x the stage's largest magnitude: the teeth test shows the mutations far outside such bounds.  (1e-4 is out
# of reach for the worst-case bound itself: g_n alone is 1e-4 at K Cin = 1728, and sum |W| |x| is several times max |y|; the C = 64 blocks of
# the synthetic model reach 5.5e-3 on a solid body, where every row sums all 27 offsets.)
TIGHT = 1e-2


def _with_batch(c, b=0):
    c = np.asarray(c, np.int64)
    return np.concatenate([np.full((len(c), 1), b, np.int64), c], 1)


def _shell4(name):
    return _with_batch(synthetic.shell(name).numpy())


def _cloud4(name):
    return _with_batch(synthetic.cloud(name).numpy())


@pytest.fixture(scope='module')
def sd_np():
    return synthetic.state_dict_to_numpy(synthetic.synthetic_state_dict())


@pytest.fixture
def offset_order_reset():
    yield
    conventions.reset()


def _check(name, got, want, bound, tight=TIGHT, ratios=None):
    r = R.within(got, want, bound)
    assert r <= 1.0, f'{name}: |got - fp64| is {r:.3g} x the fp32 bound'
    if tight is not None:
        assert bound.max() <= tight * max(np.abs(want).max(), 1e-30), f'{name}: bound {bound.max():.3g} vs max |y| {np.abs(want).max():.3g}'
    if ratios is not None:
        ratios[name] = max(ratios.get(name, 0.0), r)
    return r


# ------------------------------------------------------------------------------------------------ the definition pinned to torch
def _pin_clouds():
    rng = np.random.default_rng(7)
    shell = synthetic.shell('shell6').numpy()
    shell = shell - shell.min(0)
    shell = shell[(shell < 10).all(1)]                                     # a corner of shell6 (a small dense grid at stride 4)
    block = np.stack(np.meshgrid(*[np.arange(6)] * 3, indexing='ij'), -1).reshape(-1, 3) + 3
    iso = np.unique(rng.integers(0, 8, (40, 3)) * 3, axis=0)             # isolated voxels: no two within one lattice step
    two = np.unique(rng.integers(0, 7, (150, 3)), axis=0)
    return {'shell6': _with_batch(shell), 'block6': _with_batch(block), 'isolated': _with_batch(iso),
            'two_items': np.concatenate([_with_batch(two, 0), _with_batch(two, 1)])}


def _torch_w(W, n, transpose=False):
    """ME kernel [n^3, Cin, Cout] -> torch weight [Cout, Cin, x, y, z] (conv3d) or [Cin, Cout, x, y, z] (conv_transpose3d), by the offset
    order: index k = a n^2 + b n + c with (c, b, a) = (x, y, z) for 'xyz', (a, b, c) = (x, y, z) for 'zyx'"""
    Wr = torch.from_numpy(np.asarray(W, np.float64)).reshape(n, n, n, W.shape[1], W.shape[2])
    spatial = (2, 1, 0) if conventions.get('kernel_offset_order') == 'xyz' else (0, 1, 2)
    return Wr.permute(*((3, 4) if transpose else (4, 3)), *spatial).contiguous()


def _dense(c, x, unit, size):
    """per batch item: [1, C, size, size, size] float64 grid with x at c / unit"""
    out = {}
    for b in np.unique(c[:, 0]):
        m = c[:, 0] == b
        g = torch.zeros((1, x.shape[1], size, size, size), dtype=torch.float64)
        p = c[m, 1:] // unit
        g[0, :, p[:, 0], p[:, 1], p[:, 2]] = torch.from_numpy(x[m]).T
        out[int(b)] = g
    return out


def _sample(grids, c, unit):
    return np.stack([grids[int(b)][0, :, p[0], p[1], p[2]].numpy() for b, p in zip(c[:, 0], c[:, 1:] // unit)])


@pytest.mark.parametrize('order', ['xyz', 'zyx'])
@pytest.mark.parametrize('stride', [1, 2, 4])
@pytest.mark.parametrize('cloud', ['shell6', 'block6', 'isolated', 'two_items'])
def test_reference_equals_torch_dense_convolutions(cloud, stride, order, offset_order_reset):
    import torch.nn.functional as F
    conventions.set_convention('kernel_offset_order', order)
    rng = np.random.default_rng(stride)
    c = _pin_clouds()[cloud].copy()
    c[:, 1:] *= 2 * stride                                        # a level of tensor stride 2s (the transpose's input) ...
    fine = R.children_coords(c, 2 * stride)                       # ... and its children at stride s: every lattice parity occurs
    size = int(fine[:, 1:].max()) + 4 * stride + 2
    cin, cout = 3, 2
    x = rng.standard_normal((len(fine), cin))
    W3, W2, b = rng.standard_normal((27, cin, cout)), rng.standard_normal((8, cin, cout)), rng.standard_normal((1, cout))
    tb = torch.from_numpy(b[0])
    dense = _dense(fine, x, 1, size)
    # k3 at tensor stride s: dilation s in coordinate units
    y, _ = R.conv3(fine, stride, x, R.zero_bound(x), W3, b)
    want = _sample({k: F.conv3d(g, _torch_w(W3, 3), tb, padding=stride, dilation=stride) for k, g in dense.items()}, fine, 1)
    np.testing.assert_allclose(y, want, rtol=0, atol=1e-12 * np.abs(want).max())
    # k1
    W1 = rng.standard_normal((cin, cout))
    y, _ = R.conv1(x, R.zero_bound(x), W1, b)
    np.testing.assert_allclose(y, x @ W1 + b, rtol=0, atol=1e-12)
    # k2 s2 down from stride s: output o of stride 2s, dilation s is the coarse voxel 2 s o
    coarse, y, _ = R.down(fine, stride, x, R.zero_bound(x), W2, b)
    assert (coarse[:, 1:] % (2 * stride) == 0).all()
    want = _sample({k: F.conv3d(g, _torch_w(W2, 2), tb, stride=2 * stride, dilation=stride) for k, g in dense.items()}, coarse, 2 * stride)
    np.testing.assert_allclose(y, want, rtol=0, atol=1e-12 * np.abs(want).max())
    # the coarse level holds exactly the cells that contain a fine voxel
    cells = {(int(r[0]),) + tuple(int(v) // (2 * stride) for v in r[1:]) for r in fine}
    assert {(int(r[0]),) + tuple(int(v) // (2 * stride) for v in r[1:]) for r in coarse} == cells and len(coarse) == len(cells)
    # k2 s2 generative transpose from stride 2s: in units of s, out[2 i + d] = W[d]^T x[i]
    xc = rng.standard_normal((len(c), cin))
    kids, y, _ = R.up(c, 2 * stride, xc, R.zero_bound(xc), W2, b)
    np.testing.assert_array_equal(kids, fine)
    up = {k: F.conv_transpose3d(g, _torch_w(W2, 2, transpose=True), tb, stride=2) for k, g in _dense(c, xc, 2 * stride, size).items()}
    want = _sample({k: F.pad(g, (0, 2, 0, 2, 0, 2)) for k, g in up.items()}, kids, stride)
    np.testing.assert_allclose(y, want, rtol=0, atol=1e-12 * np.abs(want).max())


def test_reference_lookup_edges():
    """keys at 0 and 2^20 - 1 on every axis, neighbours beyond the range absent, batch items never mixed"""
    top = (1 << 20) - 1
    c = np.array([[0, 0, 0, 0], [0, top, top, top], [1, 0, 0, 0], [0, 1, 0, 0], [3, top, 0, top]], np.int64)
    nbr = R.neighbour_map(c, c, R.offsets(3))
    assert nbr[13].tolist() == [0, 1, 2, 3, 4]
    assert nbr[14, 0] == 3 and nbr[12, 3] == 0 and (nbr[:, 2] >= 0).sum() == 1 and (nbr[:, 1] >= 0).sum() == 1
    np.testing.assert_array_equal(R.lookup(c, c + np.array([0, 1, 0, 0])), [3, -1, -1, -1, -1])       # x = 2^20: absent


# ------------------------------------------------------------------------------------------------ the oracle within the bound
def _rand_w(rng, K, cin, cout):
    return (rng.uniform(-1, 1, (K, cin, cout)) / np.sqrt(K * cin)).astype(np.float32), rng.uniform(-0.1, 0.1, (1, cout)).astype(np.float32)


def _block_params(rng, C):
    sd = {}
    for nm, K, ci, co in (('conv0_0', 27, C, C // 4), ('conv0_1', 27, C // 4, C // 2), ('conv1_0', 1, C, C // 4), ('conv1_1', 27, C // 4, C // 4),
                          ('conv1_2', 1, C // 4, C // 2)):
        W, b = _rand_w(rng, K, ci, co)
        sd[f'b.{nm}.kernel'], sd[f'b.{nm}.bias'] = (W[0] if K == 1 else W), b
    return sd


@pytest.mark.parametrize('stride', [1, 2])
def test_oracle_primitives_within_the_bound(stride):
    rng = np.random.default_rng(stride)
    c4 = _shell4('shell7')
    c4[:, 1:] *= stride
    n = len(c4)
    for cin, cout in ((1, 16), (16, 16), (32, 32), (64, 64), (32, 8), (16, 1), (64, 1), (8, 64)):
        x = rng.standard_normal((n, cin)).astype(np.float32)
        x[rng.random(n) < 0.05] = 0
        W, b = _rand_w(rng, 27, cin, cout)
        _check(f'k3 {cin}->{cout}', orc.conv_gather(orc.kmap_k3(c4, stride), x, W, b), *R.conv3(c4, stride, x, R.zero_bound(x), W, b))
        W1, b1 = _rand_w(rng, 1, cin, cout)
        _check(f'k1 {cin}->{cout}', orc.conv_k1(x, W1[0], b1), *R.conv1(x, R.zero_bound(x), W1[0], b1))
    for cin, cout in ((16, 32), (32, 64), (64, 32)):
        x = rng.standard_normal((n, cin)).astype(np.float32)
        W, b = _rand_w(rng, 8, cin, cout)
        cc, _ = orc.stride2_coords(c4, 2 * stride)
        coarse, y, e = R.down(c4, stride, x, R.zero_bound(x), W, b)
        np.testing.assert_array_equal(cc, coarse)
        _check(f'down {cin}->{cout}', orc.conv_gather(orc.kmap_down(c4, cc, stride), x, W, b), y, e)
    for cin, cout in ((8, 64), (64, 32), (32, 16)):
        cc = R.down_coords(c4, stride)
        x = rng.standard_normal((len(cc), cin)).astype(np.float32)
        W, b = _rand_w(rng, 8, cin, cout)
        kids, y, e = R.up(cc, 2 * stride, x, R.zero_bound(x), W, b)
        np.testing.assert_array_equal(orc.children_coords(cc, 2 * stride), kids)
        _check(f'up {cin}->{cout}', orc.conv_up2(x, W, b), y, e)
    for C in (16, 32, 64):
        sd = _block_params(rng, C)
        x = rng.standard_normal((n, C)).astype(np.float32)
        _check(f'irn {C}', orc.inception_resnet(sd, 'b', orc.Level(c4, stride), x), *R.inception_resnet(sd, 'b', c4, stride, x, R.zero_bound(x)))


def _oracle_encoder_stages(sd, coords):
    """the oracle's encoder_forward, one stage (a fused kernel's worth) at a time -> {stage: fp32 value}, [(coords, value)] of the 3 outputs"""
    st = {}
    lvl, x = orc.Level(coords, 1), np.ones((len(coords), 1), np.float32)
    outs = []
    for i in range(3):
        x = st[f'encoder.conv{i}'] = orc.relu(orc._conv3(sd, f'encoder.conv{i}', lvl, x))
        lvl, x = orc._down(sd, f'encoder.down{i}', lvl, x)
        x = st[f'encoder.down{i}'] = orc.relu(x)
        for j in range(3):
            x = st[f'encoder.block{i}.{j}'] = orc.inception_resnet(sd, f'encoder.block{i}.{j}', lvl, x)
        outs.append((lvl.C, x))
    st['encoder.conv3'] = orc._conv3(sd, 'encoder.conv3', lvl, x)
    return st, [(lvl.C, st['encoder.conv3']), outs[1], outs[0]]


class StageTap:
    """fp64_reference tap: checks each stage against `values[stage]` within its bound and hands that fp32 value on (bound 0)"""

    def __init__(self, values, tight=TIGHT):
        self.values, self.tight, self.ratios = values, tight, {}

    def __call__(self, name, y, e):
        got = self.values[name]
        _check(name, got, y, e, self.tight, self.ratios)
        return got.astype(np.float64), R.zero_bound(got)


@pytest.mark.parametrize('cloud', ['shell7', 'solid_cube_s', 'noisy_s'])
def test_oracle_encoder_within_the_bound(cloud, sd_np):
    c4 = _cloud4(cloud) if cloud.endswith('_s') else _shell4(cloud)
    st, outs = _oracle_encoder_stages(sd_np, c4)
    for (a, fa), (b, fb) in zip(outs, orc.encoder_forward(sd_np, c4, np.ones((len(c4), 1), np.float32))):
        np.testing.assert_array_equal(a, b)                                 # (the stage walk is the oracle's own composition)
        np.testing.assert_array_equal(fa, fb)
    tap = StageTap(st)
    ref = R.encoder_forward(sd_np, c4, np.ones((len(c4), 1)), tap=tap)
    assert len(tap.ratios) == 3 * 5 + 1
    for (a, _), (b, _, _) in zip(outs, ref):
        np.testing.assert_array_equal(a, b)
    # latent symbols: round(y) may differ from the fp64 value's rounding only within the bound of a half-integer
    y, e = R.conv3(outs[0][0], 8, st['encoder.block2.2'], R.zero_bound(st['encoder.block2.2']), sd_np['encoder.conv3.kernel'], sd_np['encoder.conv3.bias'])
    assert R.rounding_mismatch_outside_bound(st['encoder.conv3'], y, e) == 0


def _oracle_decoder_levels(sd, yC, yF, nums):
    """the oracle's decoder_forward, stage by stage -> [(level input coords, level input feats, {stage: value}, mask)], final coords"""
    C_, x, stride = yC, yF, 8
    levels = []
    for l in range(3):
        st = {}
        inp = (C_, x)
        x = st[f'decoder.up{l}'] = orc.relu(orc.conv_up2(x, sd[f'decoder.up{l}.kernel'], sd[f'decoder.up{l}.bias']))
        lvl = orc.Level(orc.children_coords(C_, stride), stride // 2)
        stride //= 2
        x = st[f'decoder.conv{l}'] = orc.relu(orc._conv3(sd, f'decoder.conv{l}', lvl, x))
        for j in range(3):
            x = st[f'decoder.block{l}.{j}'] = orc.inception_resnet(sd, f'decoder.block{l}.{j}', lvl, x)
        cls = st[f'decoder.conv{l}_cls'] = orc._conv3(sd, f'decoder.conv{l}_cls', lvl, x)
        mask = orc.topk_mask(cls[:, 0], nums[l])
        levels.append((inp, st, mask))
        C_, x = lvl.C[mask], x[mask]
    return levels, C_


@pytest.mark.parametrize('cloud', ['shell7', 'noisy_s'])
def test_oracle_decoder_levels_and_topk_within_the_bound(cloud, sd_np):
    c4 = _cloud4(cloud) if cloud.endswith('_s') else _shell4(cloud)
    enc = orc.encode(sd_np, c4.astype(np.int32))
    yC = np.concatenate([np.zeros((len(enc['coords8']), 1), np.int32), enc['coords8'].astype(np.int32)], 1) * 8
    yC = yC[orc.sort_zyx_perm(yC)]
    yF = orc.eb_decompress(orc.pack_eb_params(sd_np), enc['F'], *np.frombuffer(enc['H'][9:17], np.float32), (len(yC), 8))
    nums = np.frombuffer(enc['num_points'], np.int32).tolist()
    levels, final = _oracle_decoder_levels(sd_np, yC, yF, nums)
    np.testing.assert_array_equal(final, orc.decoder_forward(sd_np, yC, yF, nums)[0])
    for l, ((C_, x), st, mask) in enumerate(levels):
        tap = StageTap(st)
        kids, _, _, cls, ecls = R.decoder_level(sd_np, l, C_, 8 >> l, x.astype(np.float64), R.zero_bound(x), tap=tap)
        assert len(tap.ratios) == 6
        assert R.topk_violation(mask, cls, ecls) <= 0, f'level {l}: the pruning mask is no top-k of the fp64 logits'
        assert mask.sum() == min(nums[l], len(mask))


# ------------------------------------------------------------------------------------------------ teeth: a wrong definition is caught
def _mirror(deltas):
    return deltas[::-1]


def test_mutated_definitions_are_caught(sd_np, offset_order_reset):
    """each mutation of the definition must leave the tolerance (the fp32 bound of the true definition) on at least one output, on the
    same clouds the tests above use — and the bound must stay tight"""
    rng = np.random.default_rng(3)
    c4 = _shell4('shell7')
    n = len(c4)
    x16 = rng.standard_normal((n, 16)).astype(np.float32)
    W3, b3 = _rand_w(rng, 27, 16, 16)
    want3 = orc.conv_gather(orc.kmap_k3(c4, 1), x16, W3, b3)
    _, e3 = R.conv3(c4, 1, x16, R.zero_bound(x16), W3, b3)
    caught = {}

    def k3(deltas, b=b3, coords=c4, x=x16, stride=1):
        y, _ = R._conv(R.neighbour_map(coords, coords, deltas), x, R.zero_bound(x), W3, b)
        return y

    caught['mirrored offsets'] = R.within(want3, k3(_mirror(R.offsets(3))), e3)
    conventions.set_convention('kernel_offset_order', 'zyx')
    caught['other offset order'] = R.within(want3, k3(R.offsets(3)), e3)
    conventions.reset()
    caught['dropped bias'] = R.within(want3, k3(R.offsets(3), b=None), e3)
    # dilation 1 on a level of tensor stride 2
    c2 = c4.copy()
    c2[:, 1:] *= 2
    want2 = orc.conv_gather(orc.kmap_k3(c2, 2), x16, W3, b3)
    caught['dilation 1 at stride 2'] = R.within(want2, k3(R.offsets(3), coords=c2), R.conv3(c2, 2, x16, R.zero_bound(x16), W3, b3)[1])
    # transpose children mirrored: child j takes W[7 - j]
    cc = R.down_coords(c4, 1)
    xc = rng.standard_normal((len(cc), 16)).astype(np.float32)
    W2, b2 = _rand_w(rng, 8, 16, 32)
    _, yu, eu = R.up(cc, 2, xc, R.zero_bound(xc), W2, b2)
    caught['mirrored transpose children'] = R.within(orc.conv_up2(xc, W2, b2), R.up(cc, 2, xc, R.zero_bound(xc), W2[::-1], b2)[1], eu)
    # down conv whose origin is shifted by one stride: offsets {-1, 0} instead of {0, 1} from the same coarse voxels
    xd = rng.standard_normal((n, 16)).astype(np.float32)
    coarse, yd, ed = R.down(c4, 1, xd, R.zero_bound(xd), W2, b2)
    shifted, _ = R._conv(R.neighbour_map(coarse, c4, R.offsets(2) - 1), xd, R.zero_bound(xd), W2, b2)
    want_d = orc.conv_gather(orc.kmap_down(c4, orc.stride2_coords(c4, 2)[0], 1), xd, W2, b2)
    caught['down origin shifted by one stride'] = R.within(want_d, shifted, ed)
    # InceptionResNet: swapped cat halves, dropped residual
    sd = _block_params(rng, 32)
    x32 = rng.standard_normal((n, 32)).astype(np.float32)
    want_irn = orc.inception_resnet(sd, 'b', orc.Level(c4, 1), x32)
    y_irn, e_irn = R.inception_resnet(sd, 'b', c4, 1, x32, R.zero_bound(x32))
    caught['swapped cat halves'] = R.within(want_irn, np.concatenate([y_irn[:, 16:] - x32[:, 16:] + x32[:, :16], y_irn[:, :16] - x32[:, :16] + x32[:, 16:]], 1), e_irn)
    caught['dropped residual'] = R.within(want_irn, y_irn - x32, e_irn)
    missed = {k: v for k, v in caught.items() if not v > 1.0}
    assert not missed, f'mutations inside the tolerance: {missed}'
    for name, (want, e) in {'k3': (want3, e3), 'up': (yu, eu), 'down': (yd, ed), 'irn': (y_irn, e_irn)}.items():
        assert e.max() <= TIGHT * np.abs(want).max(), name


# ================================================================================================ GPU: every kernel family vs the definition
ROWS = (1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 1023, 1025)
PARENTS = (1, 2, 3, 127, 128, 129)
GPU_RATIOS = {}                                  # family -> largest |got - fp64| / bound seen (printed at the end of the GPU session)


def _dev():
    return torch.device('cuda:0')


def _t(a, dt=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(_dev())


@pytest.fixture
def gpu_path():
    """the dispatch record, the forced families and the offset order come back after each test"""
    from pcgcv2_amd import ops
    keep = ops.PATH
    yield ops
    ops.configure(keep)
    ops.set_conv_impl(-1)
    ops.set_up2_impl(2)
    ops.set_rows_q4_variant(0)
    ops.PROFILE.reset(enabled=False)


def _features(rng, n, c, kind='mixed'):
    """standard normal, about 5 % exact-zero rows and some rows scaled to ~1e4 (latent magnitudes at gain 50)"""
    x = rng.standard_normal((n, c)).astype(np.float32)
    if kind == 'mixed':
        x[rng.random(n) < 0.05] = 0
        x[rng.random(n) < 0.02] *= 1e4
    return x


def _poisoned(x, extra=8):
    """x as a column slice of a wider buffer whose other columns, and 64 rows past n, are NaN"""
    n, c = x.shape
    buf = torch.full((n + 64, c + extra), float('nan'), device=_dev())
    buf[:n, :c] = _t(x)
    return buf[:n, :c]


def _gpu_check(family, got, want, bound, oracle=None):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert np.isfinite(got).all(), f'{family}: non-finite output'
    r = _check(family, got, want, bound, tight=None)
    GPU_RATIOS[family] = max(GPU_RATIOS.get(family, 0.0), r)
    if oracle is not None:
        np.testing.assert_array_equal(got, oracle, err_msg=f'{family}: differs from the oracle')


def _edge_clouds():
    """small legal levels: isolated voxels, a solid cube, three batch items with identical xyz, coordinates at 0 and 2^20 - 1"""
    top = (1 << 20) - 1
    rng = np.random.default_rng(11)
    corner = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 1], [top, top, top], [top - 1, top, top], [top, 0, top], [0, top, 0], [top, top, 0]])
    same = np.unique(rng.integers(100, 112, (400, 3)), axis=0)
    return {'noisy_s': _cloud4('noisy_s')[:6000], 'solid_cube_s': _cloud4('solid_cube_s'), 'edges': _with_batch(corner),
            'three_items': np.concatenate([_with_batch(same, b) for b in (1, 2, 3)])}


def _prefix(n, cloud='shell9'):
    c = _shell4(cloud)[:n]
    assert len(c) == n
    return c


@pytest.mark.gpu
@pytest.mark.parametrize('impl,K,cin,cout', [(0, 27, 16, 16), (0, 8, 32, 64), (0, 1, 64, 16), (0, 27, 1, 16), (2, 27, 16, 16), (2, 27, 32, 32),
                                             (2, 27, 64, 64), (6, 27, 32, 8), (6, 27, 16, 16), (6, 27, 16, 4)],
                         ids=lambda v: str(v))
def test_gather_families_vs_fp64(impl, K, cin, cout, gpu_path):
    from pcgcv2_amd._lib import lib
    ops = gpu_path
    family = {0: 'gather valu', 2: 'gather mfma', 6: 'gather row_split'}[impl]
    rng = np.random.default_rng(impl * 100 + cin + cout)
    W, b = _rand_w(rng, K, cin, cout)
    Wt = _t(W[0] if K == 1 else W)
    levels = [(f'{n} rows', _prefix(n)) for n in ROWS] + list(_edge_clouds().items())
    ops.set_conv_impl(impl)
    for name, c4 in levels:
        if K == 8:
            coarse = R.down_coords(c4, 1)
            nbr = R.neighbour_map(coarse, c4, R.offsets(2))
        else:
            nbr = R.k3_map(c4, 1) if K == 27 else np.arange(len(c4))[None]
        x = _features(rng, len(c4), cin)
        y, e = R._conv(nbr, x, R.zero_bound(x), W, b)
        got = ops.conv_gather(_t(nbr, torch.int32), _poisoned(x), Wt, _t(b))
        torch.cuda.synchronize()
        launched = lib().pcgc_last_conv_impl()
        if K == 27 and cin > 1:
            assert launched == impl, (name, launched)
        _gpu_check(family, got, y, e, orc.conv_gather(nbr.astype(np.int32), x, W, b))


@pytest.mark.gpu
def test_unit_conv_vs_fp64(gpu_path):
    ops = gpu_path
    rng = np.random.default_rng(5)
    W, b = _rand_w(rng, 27, 1, 16)
    for name, c4 in [(f'{n} rows', _prefix(n)) for n in ROWS] + list(_edge_clouds().items()):
        nbr = R.k3_map(c4, 1)
        ones = np.ones((len(c4), 1), np.float32)
        y, e = R._conv(nbr, ones, R.zero_bound(ones), W, b)
        got = ops.conv_gather_unit(_t(nbr, torch.int32), _t(W), _t(b))
        _gpu_check('unit', got, y, e, orc.conv_gather(nbr.astype(np.int32), ones, W, b))


def _profiled(ops, fn):
    ops.PROFILE.reset(enabled=True)
    try:
        out = fn()
        torch.cuda.synchronize()
        names = {ops.PROFILE.name_of(d['kernel']) for d in ops.PROFILE.detail()}
    finally:
        ops.PROFILE.reset(enabled=False)
    return out, names


@pytest.mark.gpu
@pytest.mark.parametrize('family', ['rows_conv', 'packed64', 'rows_down'])
def test_rows_and_packed_conv_families_vs_fp64(family, gpu_path):
    ops = gpu_path
    rng = np.random.default_rng(len(family))
    cin, cout, K = {'rows_conv': (32, 32, 27), 'packed64': (64, 64, 27), 'rows_down': (32, 64, 8)}[family]
    W, b = _rand_w(rng, K, cin, cout)
    table = ops.child_conv_table(_t(W))
    levels = [(f'{n} rows', _prefix(n if family != 'rows_down' else 8 * n, 'shell9' if n < 20000 else 'shell10')) for n in ROWS]
    levels += list(_edge_clouds().items()) + [('large', _prefix(150000, 'shell10'))]
    for name, c4 in levels:
        x = _features(rng, len(c4), cin)
        if family == 'rows_down':
            coarse = R.down_coords(c4, 1)
            nbr = R.neighbour_map(coarse, c4, R.offsets(2))
            call = lambda: ops.conv_down_rows(_t(nbr, torch.int32), _poisoned(x), table, _t(b), cout)
            want_name = f'k_rows_down<{cin // 16}, {cout // 16}>'
        else:
            nbr = R.k3_map(c4, 1)
            call = (lambda: ops.conv_rows(_t(nbr, torch.int32), _poisoned(x), table, _t(b), cout)) if family == 'rows_conv' else \
                   (lambda: ops.conv_packed64(_t(nbr, torch.int32), _poisoned(x), table, _t(b)))
            want_name = 'k_rows_conv<2, 2>' if family == 'rows_conv' else 'k_conv_packed64'
        got, names = _profiled(ops, call)
        assert names == {want_name}, names
        y, e = R._conv(nbr, x, R.zero_bound(x), W, b)
        _gpu_check(family, got, y, e, orc.conv_gather(nbr.astype(np.int32), x, W, b) if len(c4) <= 20000 else None)


@pytest.mark.gpu
@pytest.mark.parametrize('impl', [0, 1, 2], ids=['valu', 'mfma', 'mfma_lds_table'])
@pytest.mark.parametrize('cin,cout', [(8, 64), (64, 32), (32, 16)])
def test_conv_up2_impls_vs_fp64(impl, cin, cout, gpu_path):
    ops = gpu_path
    rng = np.random.default_rng(impl + cin)
    W, b = _rand_w(rng, 8, cin, cout)
    ops.set_up2_impl(impl)
    for n in ROWS + (300000,):
        c = R.down_coords(_shell4('shell9') if n < 300000 else _shell4('shell10'), 1)[:n]
        x = _features(rng, len(c), cin)
        kids, y, e = R.up(c, 2, x, R.zero_bound(x), W, b)
        got = ops.conv_up2(_poisoned(x), _t(W), _t(b))
        _gpu_check(f'conv_up2 {["valu", "mfma", "mfma_lds_table"][impl]}', got, y, e, orc.conv_up2(x, W, b) if len(c) <= 20000 else None)


def _block(rng, C):
    from pcgcv2_amd.autoencoder import InceptionResNet
    blk = InceptionResNet(C).to(_dev())
    sd = _block_params(rng, C)
    with torch.no_grad():
        for nm in ('conv0_0', 'conv0_1', 'conv1_0', 'conv1_1', 'conv1_2'):
            getattr(blk, nm).kernel.copy_(_t(sd[f'b.{nm}.kernel']))
            getattr(blk, nm).bias.copy_(_t(sd[f'b.{nm}.bias']))
    return blk, sd


IRN_FAMILIES = {
    # family: (C, PathConfig changes, kernel names the launch must show (None: no bracketed kernel — the five-conv composition), rows_q4 variant)
    'rows64': (64, dict(ROWS_IRN64_MIN=1), {'k_rows_irn_a64', 'k_rows_irn_b64'}, 0),
    'rows32': (32, dict(ROWS_IRN32_MIN=1, ROWS_Q4=False), {'k_rows_irn_a32', 'k_rows_irn_b32'}, 0),
    'rows32q4 v0': (32, dict(ROWS_Q4_MIN=1), {'k_rows_q4_a32', 'k_rows_q4_b32'}, 0),
    'rows32q4 v1': (32, dict(ROWS_Q4_MIN=1), {'k_rows_q4_a32', 'k_rows_q4_b32'}, 1),
    'rows32q4 v2': (32, dict(ROWS_Q4_MIN=1), {'k_rows_q4_a32', 'k_rows_q4_b32'}, 2),
    'rows32q4 v3': (32, dict(ROWS_Q4_MIN=1), {'k_rows_q4_a32', 'k_rows_q4_b32'}, 3),
    'valu 16': (16, dict(), {'k_irn_a_split<16>', 'k_irn_b_split<16>'}, 0),
    'valu 64': (64, dict(ROWS_IRN64=False), {'k_irn_a<64, 16>', 'k_irn_b<64, 16>'}, 0),
    'unfused 32': (32, dict(FUSE_IRN=False), None, 0),
}


@pytest.mark.gpu
@pytest.mark.parametrize('family', list(IRN_FAMILIES))
def test_inception_resnet_families_vs_fp64(family, gpu_path):
    from pcgcv2_amd import dispatch
    from pcgcv2_amd.sparse import CoordMap, SparseTensor
    ops = gpu_path
    C, changes, kernels, variant = IRN_FAMILIES[family]
    rng = np.random.default_rng(C + variant)
    blk, sd = _block(rng, C)
    ops.configure(**changes)
    ops.set_rows_q4_variant(variant)
    fam = family.split(' ')[0]
    levels = [(f'{n} rows', _prefix(n)) for n in ROWS] + list(_edge_clouds().items())
    if fam == 'rows32':
        levels += [('32768 rows', _prefix(32768, 'shell10')), ('32769 rows', _prefix(32769, 'shell10'))]      # both sides of ROWS32_DEEP_MAX
    if family == 'rows32q4 v0':
        levels += [('large', _prefix(ops.PathConfig().ROWS_Q4_MIN, 'shell10'))]                               # the product's own gate
    for name, c4 in levels:
        want_fam = fam if fam != 'unfused' else 'unfused'
        assert dispatch.select('irn', (C,), len(c4)).family == want_fam, (name, dispatch.select('irn', (C,), len(c4)).family)
        x = _features(rng, len(c4), C)
        xs = SparseTensor(_t(x), coordinate_map=CoordMap(_t(c4, torch.int32), 1, unique=True))
        with torch.no_grad():
            got, names = _profiled(ops, lambda: blk(xs).F)
        if kernels is not None:
            assert names == kernels, (name, names)
        y, e = R.inception_resnet(sd, 'b', c4, 1, x, R.zero_bound(x))
        _gpu_check(f'irn {family}', got, y, e, orc.inception_resnet(sd, 'b', orc.Level(c4.astype(np.int32), 1), x) if len(c4) <= 40000 else None)


def _children(n_parents, cloud='shell9'):
    """(parent CoordMap, children CoordMap, children coords) of the first n_parents rows of a cloud's stride-2 level"""
    from pcgcv2_amd.sparse import CoordMap
    pc = R.down_coords(_shell4(cloud), 1)[:n_parents]
    assert len(pc) == n_parents
    parent = CoordMap(_t(pc, torch.int32), 2, unique=True)
    kids = parent.up()
    kc = kids.C.cpu().numpy().astype(np.int64)
    np.testing.assert_array_equal(kc, R.children_coords(pc, 2))
    return parent, kids, kc


CHILD_FAMILIES = ['child conv 16', 'child conv 32', 'cls 16', 'cls 32', 'cls 64', 'child irn 16', 'child irn 32', 'child_q4 cls', 'child_q4 irn']


@pytest.mark.gpu
@pytest.mark.parametrize('family', CHILD_FAMILIES)
def test_children_families_vs_fp64(family, gpu_path):
    ops = gpu_path
    rng = np.random.default_rng(len(family))
    C = int(family.split(' ')[-1]) if family[-1].isdigit() else 16
    big = family in ('child_q4 irn', 'child_q4 cls')
    sizes = [(n, 'shell9') for n in PARENTS] + ([(ops.PathConfig().CHILD_Q4_MIN_PARENTS, 'shell10')] if big else [])
    if family.startswith('child irn') or family == 'child_q4 irn':
        blk, sd = _block(rng, C)
        params = [p for m in (blk.conv0_0, blk.conv0_1, blk.conv1_0, blk.conv1_1, blk.conv1_2) for p in (m.kernel, m.bias)]
        tables = ops.child_irn_tables(params)
        q4 = ops.child_q4_tables(params) if family == 'child_q4 irn' else None
        names = {'k_child_q4<0, 8, 2>', 'k_child_irn_b<16>'} if q4 is not None else {f'k_child_irn_a<{C}>', f'k_child_irn_b<{C}>'}
    else:
        cout = 1 if 'cls' in family else C
        W, b = _rand_w(rng, 27, C, cout)
    for n_p, cloud in sizes:
        parent, kids, kc = _children(n_p, cloud)
        x = _features(rng, len(kc), C)
        if 'irn' in family:
            call = lambda: ops.irn_block_child(parent.k3, _t(x), params, tables, q4_table=q4)
            y, e = R.inception_resnet(sd, 'b', kc, 1, x, R.zero_bound(x))
            oracle = (lambda: orc.inception_resnet(sd, 'b', orc.Level(kc.astype(np.int32), 1), x))
        else:
            if family == 'child_q4 cls':
                call, names = (lambda: ops.cls_child_q4(parent.k3, _poisoned(x), ops.child_q4_cls_table(_t(W)), _t(b))), None
            else:
                table = ops.child_cls_table(_t(W)) if cout == 1 else ops.child_conv_table(_t(W))
                call = lambda: ops.conv_child(parent.k3, _poisoned(x), table, _t(b), cout)
                names = {f'k_child_cls<{C // 16}>' if cout == 1 else f'k_child_conv<{C // 16}, {C // 16}>'}
            y, e = R.conv3(kc, 1, x, R.zero_bound(x), W, b)
            oracle = (lambda: orc.conv_gather(R.k3_map(kc, 1).astype(np.int32), x, W, b))
        got, launched = _profiled(ops, call)
        if names is not None:
            assert launched == names, launched
        _gpu_check(family, got, y, e, oracle() if len(kc) <= 20000 else None)


@pytest.mark.gpu
@pytest.mark.parametrize('cloud', ['shell8', 'noisy_s'])
def test_encoder_and_decoder_through_the_modules_vs_fp64(cloud, gpu_path, sd_np):
    """the product's encoder layer by layer and each decoder level, every stage on the product's own input to it; the product's pruning
    masks must be valid top-k selections of the fp64 logits up to the bound"""
    from pcgcv2_amd.pcc_model import PCCModel
    from pcgcv2_amd.sparse import SparseTensor
    c4 = _cloud4(cloud) if cloud.endswith('_s') else _shell4(cloud)
    model = PCCModel().to(_dev())
    model.load_state_dict(synthetic.synthetic_state_dict())
    seen = {}

    def hook(name):
        def f(mod, args, out):
            seen[name] = (args[0], out)
        return f
    handles = []
    for part, names in (('encoder', [f'conv{i}' for i in range(4)] + [f'down{i}' for i in range(3)] + [f'block{i}.{j}' for i in range(3) for j in range(3)]),
                        ('decoder', [f'{k}{l}' for l in range(3) for k in ('up', 'conv')] + [f'conv{l}_cls' for l in range(3)] +
                         [f'block{l}.{j}' for l in range(3) for j in range(3)])):
        for nm in names:
            handles.append(model.get_submodule(f'{part}.{nm}').register_forward_hook(hook(f'{part}.{nm}')))
    try:
        x = SparseTensor(torch.ones((len(c4), 1)), coordinates=_t(c4, torch.int32), tensor_stride=1, device=_dev())
        with torch.no_grad():
            y = model.encoder(x)[0]
            yq = SparseTensor(torch.round(y.F), coordinate_map=y.cmap)
            model.decoder(yq, [[n] for n in (len(seen['encoder.block1.2'][1].F), len(seen['encoder.block0.2'][1].F), len(c4))])
        torch.cuda.synchronize()
    finally:
        for h in handles:
            h.remove()
    vals = {k: out.F.cpu().numpy() for k, (_, out) in seen.items()}
    tap = StageTap(vals)
    enc = R.encoder_forward(sd_np, c4, np.ones((len(c4), 1)), tap=tap)
    np.testing.assert_array_equal(enc[0][0], seen['encoder.conv3'][1].C.cpu().numpy())
    assert len(tap.ratios) == 16
    GPU_RATIOS['encoder stages'] = max(tap.ratios.values())
    for l in range(3):
        inp = seen[f'decoder.up{l}'][0]
        C_, F_ = inp.C.cpu().numpy().astype(np.int64), inp.F.cpu().numpy()
        tap = StageTap(vals)
        kids, _, _, cls, ecls = R.decoder_level(sd_np, l, C_, 8 >> l, F_.astype(np.float64), R.zero_bound(F_), tap=tap)
        np.testing.assert_array_equal(kids, seen[f'decoder.conv{l}_cls'][1].C.cpu().numpy())
        GPU_RATIOS[f'decoder level {l}'] = max(tap.ratios.values())
        if l < 2:
            kept = R.lookup(kids, seen[f'decoder.up{l + 1}'][0].C.cpu().numpy().astype(np.int64))
            assert (kept >= 0).all()
            mask = np.zeros(len(kids), bool)
            mask[kept] = True
            assert R.topk_violation(mask, cls, ecls) <= 0, f'decoder level {l}: the product mask is no top-k of the fp64 logits'


@pytest.mark.gpu
def test_zz_report_gpu_ratios():
    """(prints the largest error / bound ratio per family: the record the PR body reports)"""
    for k in sorted(GPU_RATIOS):
        print(f'fp64 ratio {k:28s} {GPU_RATIOS[k]:.3e}')
