"""GPU tests of the backward pass (csrc/grad.hip, pcgcv2_amd/grad.py, loss.bce / loss.bits, trainer.py) against the fp64 definition of
tests/grad_reference.py, which tests/test_grad_cpu.py pins to the reference's own gradients.

Operators, exact: integer-valued x, gy and W in [-4, 4] on levels of at most 2^18 rows keep every sum below 2^24, so fp32 is exact in any
order and gW, gb, gx must EQUAL the definition.  Operators, real data: within fp64_reference's bound g_n (|A| . |B|), n = the number of
terms (gW: the offset's pair count; gb: the row count; gx: K Cout + 1).  Leaf gradients (BCE, bottleneck) are rounded once from fp64:
u |value| BOUND_SLACK."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import descent_case
import fp64_reference as R
import grad_reference as G
from pcgcv2_amd import conventions, grad, loss, ops, synthetic
from pcgcv2_amd.sparse import CoordMap, SparseTensor, sparse_collate

DEV = torch.device('cuda:0')
U = R.U

# every (K, Cin, Cout) of the 227-key layout
K3_SHAPES = [(1, 16), (32, 8), (8, 16), (8, 8), (32, 32), (64, 16), (16, 32), (16, 16), (64, 64), (64, 1), (32, 1), (16, 1), (16, 4), (4, 8), (4, 4)]
K1_SHAPES = [(32, 8), (8, 16), (64, 16), (16, 32), (16, 4), (4, 8)]
DOWN_SHAPES = [(16, 32), (32, 64), (64, 32)]
UP_SHAPES = [(8, 64), (64, 32), (32, 16)]


def _t(a, dt=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(DEV)


def _ints(rng, shape):
    return rng.integers(-4, 5, size=shape).astype(np.float32)


def _cmap(names, first=None):
    """the coordinate level of one named cloud (optionally its first rows only) or of a batch of several"""
    clouds = [synthetic.cloud(nm) for nm in names]
    if first is not None:
        clouds = [c[:first] for c in clouds]
    coords, _ = sparse_collate(clouds, [torch.ones((len(c), 1)) for c in clouds])
    return CoordMap(coords.to(DEV).contiguous(), 1, unique=True)


def _strided(a, pad, rng):
    """device copy of a [n, C] as a column slice of a wider buffer filled with other values"""
    n, C = a.shape
    wide = _t(rng.normal(size=(n, C + 2 * pad)).astype(np.float32))
    wide[:, pad:pad + C] = _t(a)
    return wide[:, pad:pad + C]


# ------------------------------------------------------------------------------------------------ the definition, from a map
def def_wgrad(nbr, x, gy):
    """gW [K, Cin, Cout], gb [Cout], pair counts [K] in fp64 from the present pairs of nbr [K, n_out]"""
    K = nbr.shape[0]
    gW = np.zeros((K, x.shape[1], gy.shape[1]))
    for k in range(K):
        o = np.nonzero(nbr[k] >= 0)[0]
        gW[k] = x[nbr[k, o]].astype(np.float64).T @ gy[o].astype(np.float64)
    return gW, gy.astype(np.float64).sum(0), (nbr >= 0).sum(1)


def def_wgrad_bound(nbr, x, gy):
    K = nbr.shape[0]
    mag = np.zeros((K, x.shape[1], gy.shape[1]))
    for k in range(K):
        o = np.nonzero(nbr[k] >= 0)[0]
        n = max(len(o), 1)
        mag[k] = R.BOUND_SLACK * (n * U / (1 - n * U)) * (np.abs(x[nbr[k, o]]).astype(np.float64).T @ np.abs(gy[o]).astype(np.float64))
    n = max(len(gy), 1)
    return mag, R.BOUND_SLACK * (n * U / (1 - n * U)) * np.abs(gy).astype(np.float64).sum(0)


def def_xgrad(nbr, n_in, gy, W, bound=False):
    """gx[i] = sum over pairs (k, o) with nbr[k][o] = i of gy[o] W[k]^T — the adjoint, written as a scatter-add on purpose: the device
    computes it as a gather through a transposed map.  (For a fixed k no input row occurs twice — test_kmap_invert asserts it — so the
    indexed += adds every pair.)"""
    gx = np.zeros((n_in, W.shape[1]))
    g64, W64 = (np.abs(gy), np.abs(W)) if bound else (gy, W)
    g64, W64 = g64.astype(np.float64), W64.astype(np.float64)
    for k in range(nbr.shape[0]):
        o = np.nonzero(nbr[k] >= 0)[0]
        gx[nbr[k, o]] += g64[o] @ W64[k].T
    if bound:
        n = nbr.shape[0] * W.shape[2] + 1
        return R.BOUND_SLACK * (n * U / (1 - n * U)) * gx
    return gx


def _check(got, want, bound, what):
    got = got.detach().cpu().numpy().astype(np.float64).reshape(want.shape)
    if bound is None:
        assert np.array_equal(got, want), f'{what}: {int((got != want).sum())} of {want.size} entries differ'
    else:
        r = R.within(got, want, bound)
        assert r <= 1.0, f'{what}: error / bound = {r:.3g}'
        return r


def _conv_case(nbr_dev, n_in, Cin, Cout, rng, exact, kind, strided=False):
    """one gather convolution's three gradients on the device against the definition; nbr_dev None: k1"""
    n_out = nbr_dev.shape[1] if nbr_dev is not None else n_in
    nbr = nbr_dev.cpu().numpy().astype(np.int64) if nbr_dev is not None else np.arange(n_in)[None]
    K = nbr.shape[0]
    gen = _ints if exact else (lambda r, s: r.normal(size=s).astype(np.float32))
    x, gy, W = gen(rng, (n_in, Cin)), gen(rng, (n_out, Cout)), gen(rng, (K, Cin, Cout))
    xd, gd = (_strided(x, 4, rng), _strided(gy, 8, rng)) if strided else (_t(x), _t(gy))
    gW, gb = ops.conv_wgrad(nbr_dev, xd, gd)
    wW, wb, _ = def_wgrad(nbr, x, gy)
    bW, bb = (None, None) if exact else def_wgrad_bound(nbr, x, gy)
    tag = f'{kind} {Cin}->{Cout} n={n_out}'
    _check(gW, wW, bW, tag + ' gW')
    _check(gb, wb, bb, tag + ' gb')
    m = grad._Map(kind, nbr_dev, n_in)
    Wd = _t(W if K > 1 else W[0])
    gx = ops.conv_gather(m.transposed(), gd, grad.transposed_kernel(Wd, kind), None, n_out=n_in)
    _check(gx, def_xgrad(nbr, n_in, gy, W), None if exact else def_xgrad(nbr, n_in, gy, W, bound=True), tag + ' gx')


# ------------------------------------------------------------------------------------------------ operators
@pytest.fixture(scope='module')
def levels():
    """noisy cloud with holes and salt (absent neighbours), its strided level, and a batch of two items"""
    a = _cmap(['noisy_s'])
    b = _cmap(['noisy_s', 'shell6'])
    return {'noisy': a, 'batch': b}


@pytest.mark.parametrize('exact', [True, False], ids=['exact', 'real'])
def test_k3_gradients_every_shape(levels, exact):
    rng = np.random.default_rng(1)
    cm = levels['noisy']
    nbr = cm.k3
    assert int((nbr < 0).sum()) > 0 and len(cm) <= 1 << 18
    for Cin, Cout in K3_SHAPES:
        _conv_case(nbr, len(cm), Cin, Cout, rng, exact, 'k3')


@pytest.mark.parametrize('exact', [True, False], ids=['exact', 'real'])
def test_k1_down_up_gradients_every_shape(levels, exact):
    rng = np.random.default_rng(2)
    cm = levels['batch']
    assert len(cm.batch_rows) == 2
    coarse, down = cm.down()
    for Cin, Cout in K1_SHAPES:
        _conv_case(None, len(coarse), Cin, Cout, rng, exact, 'k1')
    for Cin, Cout in DOWN_SHAPES:
        _conv_case(down, len(cm), Cin, Cout, rng, exact, 'down', strided=True)
    gen = _ints if exact else (lambda r, s: r.normal(size=s).astype(np.float32))
    n = len(coarse)
    upm = G.up_map(n)
    for Cin, Cout in UP_SHAPES:
        x, gy, W = gen(rng, (n, Cin)), gen(rng, (8 * n, Cout)), gen(rng, (8, Cin, Cout))
        wW, wb, _ = def_wgrad(upm, x, gy)
        bW, bb = (None, None) if exact else def_wgrad_bound(upm, x, gy)
        gW, gb = ops.conv_up2_wgrad(_t(x), _t(gy))
        _check(gW, wW, bW, f'up {Cin}->{Cout} gW'); _check(gb, wb, bb, f'up {Cin}->{Cout} gb')
        gx = ops.conv_gather(ops.kmap_up_inverse(n, DEV), _t(gy), grad.transposed_kernel(_t(W), 'up'), None)
        _check(gx, def_xgrad(upm, n, gy, W), None if exact else def_xgrad(upm, n, gy, W, bound=True), f'up {Cin}->{Cout} gx')
        # the pruned ("pending rows") input: input row p is row rows[p] of a candidates' tensor
        n_cand = n + 37
        rows = np.sort(rng.choice(n_cand, size=n, replace=False)).astype(np.int32)
        cand = gen(rng, (n_cand, Cin))
        gW2, gb2 = ops.conv_up2_wgrad(_strided(cand, 4, rng), _strided(gy, 4, rng), rows=_t(rows))
        wW2, wb2, _ = def_wgrad(upm, cand[rows], gy)
        bW2, bb2 = (None, None) if exact else def_wgrad_bound(upm, cand[rows], gy)
        _check(gW2, wW2, bW2, f'up rows {Cin}->{Cout} gW'); _check(gb2, wb2, bb2, f'up rows {Cin}->{Cout} gb')


def test_k3_gradients_off_the_tile_grids():
    """row counts 1, 15, 16, 17, 4097 and both sides of the end of a workgroup's range; large values at the range ends would show a row
    counted twice or not at all"""
    rng = np.random.default_rng(3)
    rpg = ops.conv_wgrad_rows_per_group(27, 2000, 16, 16)
    assert rpg == ops.conv_wgrad_rows_per_group(27, rpg + 1, 16, 16)
    for n in (1, 15, 16, 17, 4097, rpg - 1, rpg, rpg + 1, 2 * rpg + 3):
        cm = _cmap(['noisy_s'], first=n)
        assert len(cm) == n
        for Cin, Cout in ((16, 16), (8, 4), (1, 16), (64, 1)):
            _conv_case(cm.k3, n, Cin, Cout, rng, True, 'k3')
        _conv_case(None, n, 32, 8, rng, True, 'k1')


def test_gradients_on_a_large_level():
    """a level of 2^17 .. 2^18 rows: every workgroup of the grid and the second stage's whole depth"""
    rng = np.random.default_rng(4)
    cm = _cmap(['shell9'])
    assert (1 << 17) < len(cm) <= (1 << 18)
    for Cin, Cout in ((16, 16), (64, 64)):
        _conv_case(cm.k3, len(cm), Cin, Cout, rng, True, 'k3')
    _conv_case(cm.k3, len(cm), 32, 32, rng, False, 'k3')


@pytest.mark.parametrize('order', ['xyz', 'zyx'])
def test_k3_mirror_in_both_offset_orders(order):
    """the definition's own map (binary search, offsets in the convention's order) is its own transpose under k <-> 26 - k, equals the
    device's map under the convention's permutation, and the gradients agree in the checkpoint's layout"""
    conventions.set_convention('kernel_offset_order', order)
    try:
        rng = np.random.default_rng(5)
        cm = _cmap(['noisy_s'], first=3000)
        c = cm.C.cpu().numpy()
        dmap = R.neighbour_map(c, c, R.offsets(3))
        perm = conventions.offset_permutation(27)
        perm = np.arange(27) if perm is None else perm
        assert np.array_equal(dmap, cm.k3.cpu().numpy()[perm])
        for k in range(27):
            o = np.nonzero(dmap[k] >= 0)[0]
            assert np.array_equal(dmap[26 - k, dmap[k, o]], o)
        x, gy, W = _ints(rng, (len(c), 16)), _ints(rng, (len(c), 8)), _ints(rng, (27, 16, 8))      # W: the checkpoint's layout
        gW, _ = ops.conv_wgrad(cm.k3, _t(x), _t(gy))
        assert np.array_equal(gW.cpu().numpy()[perm], def_wgrad(dmap, x, gy)[0])
        gx = ops.conv_gather(cm.k3, _t(gy), grad.transposed_kernel(_t(W[perm]), 'k3'), None)
        assert np.array_equal(gx.cpu().numpy(), def_xgrad(dmap, len(c), gy, W))
    finally:
        conventions.reset()


def test_kmap_invert(levels):
    cm = levels['batch']
    coarse, down = cm.down()
    kids = coarse.up()
    cases = [('k3', cm.k3, len(cm)), ('down', down, len(cm)), ('up', _t(G.up_map(len(coarse)).astype(np.int32)), len(coarse)),
             ('children k3', kids.k3, len(kids))]
    for name, nbr, n_in in cases:
        inv = ops.kmap_invert(nbr, n_in).cpu().numpy()
        m = nbr.cpu().numpy()
        want = np.full((m.shape[0], n_in), -1, np.int64)
        for k in range(m.shape[0]):
            o = np.nonzero(m[k] >= 0)[0]
            assert len(np.unique(m[k, o])) == len(o), f'{name}: offset {k} is not injective'
            want[k, m[k, o]] = o
        assert np.array_equal(inv, want), name
    assert np.array_equal(ops.kmap_up_inverse(5, DEV).cpu().numpy(), ops.kmap_invert(_t(G.up_map(5).astype(np.int32)), 5).cpu().numpy())


def test_relu_bwd_and_scatter_rows_equal_numpy():
    rng = np.random.default_rng(6)
    n, C = 4099, 12
    y = rng.normal(size=(n, C)).astype(np.float32)
    y[::7, 3] = -0.0; y[1::7, 5] = 0.0; y[2::7, 1] = np.float32(1e-41); y[3::7, 2] = np.float32(-1e-41); y[4::7, 0] = np.float32(2 ** -149)
    g = rng.normal(size=(n, C)).astype(np.float32)
    want = np.where(y > 0, g, np.float32(0))
    assert (want[2::7, 1] == g[2::7, 1]).all()
    for yd, gd in ((_t(y), _t(g)), (_strided(y, 4, rng), _strided(g, 2, rng))):
        assert np.array_equal(ops.relu_bwd(gd, yd).cpu().numpy(), want)
    out = torch.full((n, C + 6), 7.0, device=DEV)
    ops.relu_bwd(_t(g), _t(y), out=out[:, 3:3 + C])
    assert np.array_equal(out[:, 3:3 + C].cpu().numpy(), want) and bool((out[:, :3] == 7).all()) and bool((out[:, 3 + C:] == 7).all())
    for C in (1, 8, 12):
        n_out = 9001
        orig = np.sort(rng.choice(n_out, size=n, replace=False)).astype(np.int32)
        gy = rng.normal(size=(n, C)).astype(np.float32)
        want = np.zeros((n_out, C), np.float32)
        want[orig] = gy
        assert np.array_equal(ops.scatter_rows(_t(gy), _t(orig), n_out).cpu().numpy(), want)
        assert np.array_equal(ops.scatter_rows(_strided(gy, 4, rng), _t(orig), n_out).cpu().numpy(), want)
    # adjoint of the product's own gather: <gather(x), g> = <x, scatter(g)>
    x = _t(rng.normal(size=(n_out, 8)).astype(np.float32))
    got = ops.gather_rows(x, _t(orig)).cpu().numpy()
    assert np.array_equal(got, x.cpu().numpy()[orig])


# ------------------------------------------------------------------------------------------------ leaves
@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'eval_loss.npz')), np.load(os.path.join(golden_dir, 'grad_loss.npz'))


def test_bce_gradient_rounded_once(golden):
    ev, _ = golden
    for i in range(int(ev['n_bce'])):
        z, t = ev[f'e{i}_logits'], ev[f'e{i}_isin']
        for scale in (1.0, 0.37 / len(z)):
            want = scale * G.bce_gradient(z, t)
            got = ops.bce_logits_bwd(_t(z), _t(t.astype(np.uint8)), scale=scale)
            assert got.shape == (len(z), 1)
            # one fp32 rounding of the value, plus the definition's own error: it forms sigmoid(z) - t in fp64, one ulp of 1.0 (2^-52)
            # absolute where sigmoid saturates against t = 1 (the device evaluates -sigmoid(-z) there)
            bound = R.BOUND_SLACK * (U * np.abs(want) + 2.0 ** -52 * scale / G.LN2)
            assert R.within(got.cpu().numpy().ravel(), want, bound) <= 1.0
        zs = _strided(z.reshape(-1, 1), 3, np.random.default_rng(0))
        assert torch.equal(ops.bce_logits_bwd(zs, _t(t.astype(np.uint8))), ops.bce_logits_bwd(_t(z), _t(t.astype(np.uint8))))


def test_bottleneck_gradient_rounded_once(golden):
    ev, gg = golden
    hit = False
    for i in range(int(ev['n_bottleneck'])):
        p, y = ev[f'b{i}_params'], ev[f'b{i}_y']
        for scale in (1.0, 1.0 / 786432):
            gy, gp = ops.eb_likelihood_bwd(_t(y), _t(p), bound=1e-9, scale=scale)
            wy, wp, _ = G.eb_gradients(p, y)
            # the device decides "below the bound" on the fp32 likelihood its forward stores; the definition on the fp64 value: exclude
            # the elements on which the two can differ (none in these cases; asserted)
            lik64 = ev[f'b{i}_lik64']
            assert not ((lik64 > 1e-9 * (1 - 1e-6)) & (lik64 < 1e-9 * (1 + 1e-6)) & (lik64 != 1e-9)).any()
            assert R.within(gy.cpu().numpy(), scale * wy, R.BOUND_SLACK * U * np.abs(scale * wy)) <= 1.0, (i, 'latent')
            assert R.within(gp.cpu().numpy(), scale * wp, R.BOUND_SLACK * U * np.abs(scale * wp)) <= 1.0, (i, 'parameters')
            # ... and within 1e-6 of the reference's own fp64 gradients
            np.testing.assert_allclose(gp.cpu().numpy(), scale * gg[f'b{i}_gparams'], rtol=1e-6, atol=0)
        if str(ev[f'b{i}_kind']) == 'tails':
            clamped = ev[f'b{i}_lik32'] == np.float32(1e-9)
            hit = hit or (clamped.any() and bool((gy.cpu().numpy()[clamped] == 0).all()))
    assert hit, 'no case reached the likelihood bound'


# ------------------------------------------------------------------------------------------------ whole model
@pytest.fixture(scope='module')
def sd():
    return synthetic.synthetic_state_dict()


def _model(sd):
    from pcgcv2_amd.pcc_model import PCCModel
    m = PCCModel().to(DEV)
    m.load_state_dict(sd)
    return m


def _input(names):
    clouds = [synthetic.cloud(nm) for nm in names]
    coords, feats = sparse_collate(clouds, [torch.ones((len(c), 1)) for c in clouds])
    return SparseTensor(feats, coordinates=coords, tensor_stride=1, device=DEV)


def _gen(seed=77):
    return torch.Generator(device=DEV).manual_seed(seed)


def _step_grads(model, x, record=None):
    model.zero_grad(set_to_none=True)
    out = model.forward_train(x, generator=_gen(), record=record)
    total, _, _ = loss.sum_loss(out, len(x))
    total.backward()
    return out, total, {k: p.grad.clone() for k, p in model.named_parameters()}


@pytest.mark.parametrize('names', [['shell8'], ['shell7', 'noisy_s']], ids=['one', 'batch2'])
def test_forward_train_equals_forward_and_gradients_reproduce(sd, names):
    model = _model(sd)
    x = _input(names)
    assert len(x) <= 1 << 17
    ref = model(x, training=True, generator=_gen())
    out, total, g1 = _step_grads(model, x)
    assert set(out) == set(ref)
    assert torch.equal(out['likelihood'], ref['likelihood']) and torch.equal(out['prior'].F, ref['prior'].F)
    assert torch.equal(out['out'].C, ref['out'].C)
    for a, b in zip(out['out_cls_list'], ref['out_cls_list']):
        assert a.F.grad_fn is not None and torch.equal(a.F, b.F) and torch.equal(a.C, b.C)
    for a, b in zip(out['ground_truth_list'], ref['ground_truth_list']):
        assert torch.equal(a.F, b.F) and torch.equal(a.C, b.C)
    for a, b in zip(loss.kept_masks(out), loss.kept_masks(ref)):
        assert torch.equal(a, b)
    # the value of sum_loss is the expression of trainer.py:127-134 on the forward's losses
    want = sum(float(loss.get_bce(c, t)) / len(c) for c, t in zip(ref['out_cls_list'], ref['ground_truth_list'])) + float(loss.get_bits(ref['likelihood'])) / len(x)
    assert abs(float(total.detach()) - want) <= 1e-5 * abs(want)
    # 224 distinct parameters, every one with a finite gradient (a layer whose ReLU is dead on this cloud legitimately gets zeros; the
    # layers at both ends of the chain do not); a second run gives the same bits
    assert len(g1) == 224 and len(model.state_dict()) == 227
    for k, g in g1.items():
        assert bool(torch.isfinite(g).all()), k
    for k in ('encoder.conv0.kernel', 'encoder.conv3.kernel', 'decoder.up0.kernel', 'decoder.conv0_cls.kernel', 'decoder.conv2_cls.bias',
              'entropy_bottleneck._matrices.0', 'entropy_bottleneck._factors.0'):
        assert bool((g1[k] != 0).any()), k
    _, _, g2 = _step_grads(model, x)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    # the three aliased keys of the bottleneck's last layer are the same tensors: one gradient, not two
    eb = model.entropy_bottleneck
    for alias, lst in (('matrix', eb._matrices), ('bias', eb._biases), ('factor', eb._factors)):
        assert getattr(eb, alias) is lst[3] and getattr(eb, alias).grad is lst[3].grad
    only = torch.autograd.grad(loss.bits(model.forward_train(x, generator=_gen())['likelihood']), list(eb._matrices))
    packed = eb.packed_params(DEV)
    direct = ops.eb_likelihood_bwd(out['prior'].F.detach(), packed)[1]
    assert torch.equal(only[3].reshape(-1), direct[21 * 8:24 * 8])


def test_descent_and_checkpoint(sd, tmp_path):
    """Twenty Adam steps (tests/descent_case.py) on one small cloud, the noise re-seeded identically at every step: sum_loss after the steps
    is below sum_loss before.  The fp64 definition through the same steps (its own noise draw) goes from 3.910617 to 2.547253, a drop
    of 34.86 % (test_grad_cpu.py::test_definition_descends asserts at least 5 %), so rounding cannot decide the sign.
    Then the coder, on the updated model, still agrees with itself (the derived weight tables were rebuilt), and a checkpoint written by
    Trainer.save_model loads strictly into a fresh model and reproduces the same `_F.bin`."""
    from pcgcv2_amd.coder import Coder
    from pcgcv2_amd.trainer import Trainer, TrainingConfig
    from pcgcv2_amd.pcc_model import PCCModel
    model = _model(sd)
    x = _input([descent_case.CLOUD])
    coder = Coder(model=model, filename=str(tmp_path / 'before'))
    coder.encode(x)                                              # (fills every derived-table cache with the OLD weights)
    trainer = Trainer(TrainingConfig(logdir=str(tmp_path / 'log'), ckptdir=str(tmp_path / 'ckpt'), init_ckpt='', alpha=1., beta=1.,
                                     lr=descent_case.LR, check_time=1e9), model)
    opt = trainer.set_optimizer()
    losses = []
    for _ in range(descent_case.STEPS + 1):
        losses.append(trainer.step(x, opt if len(losses) < descent_case.STEPS else None, generator=_gen())['sum_loss'])
    print(f'device: sum_loss {losses[0]:.6f} -> {losses[-1]:.6f}')
    assert losses[-1] < losses[0]
    coder = Coder(model=model, filename=str(tmp_path / 'after'))
    coder.encode(x)
    dec = coder.decode(rho=1)
    assert open(str(tmp_path / 'after_F.bin'), 'rb').read() != open(str(tmp_path / 'before_F.bin'), 'rb').read()
    # a model that never held the old weights (no derived table to go stale) codes the same bytes and decodes the same cloud
    path = trainer.save_model()
    ckpt = torch.load(path, map_location='cpu')
    assert set(ckpt) == {'model'} and len(ckpt['model']) == 227
    fresh = PCCModel().to(DEV)
    fresh.load_state_dict(ckpt['model'], strict=True)
    coder2 = Coder(model=fresh, filename=str(tmp_path / 'fresh'))
    coder2.encode(x)
    assert open(str(tmp_path / 'fresh_F.bin'), 'rb').read() == open(str(tmp_path / 'after_F.bin'), 'rb').read()
    assert torch.equal(coder2.decode(rho=1).C, dec.C)
    # ... and the decoder of the updated model, teacher-free, returns a cloud of the input's size
    assert len(dec) == len(x)


# ------------------------------------------------------------------------------------------------ whole model against the definition's VJPs
# Every operator's vector-Jacobian products are evaluated by the definition AT THE DEVICE'S RECORDED FORWARD POINT: inputs, ReLU masks and
# kept sets come from `record`, the cotangent of every layer is the gradient that reached its output on the device (record[..]['gy']).
# Each operator is thus judged on its own inputs with fp64_reference's bound for its own sum (as fp64_reference's `tap` does forward), and
# the chain is closed by checking that the gradient reaching every tensor is the sum of its consumers' input gradients (+ the rounding of
# that sum).  Maps are the definition's own (binary search on the recorded coordinates).
MUTATIONS = ('offsets not mirrored', 'W not transposed', 'ReLU mask dropped', 'bias gradient omitted', '1/len(out_cls) -> 1/len(x)',
             'clamp gradient passed through')


class _Definition:
    def __init__(self, model, x, record, mutation=None, maps=None):
        self.model, self.x, self.rec, self.mut = model, x, record, mutation
        self.params = dict(model.named_parameters())
        self.maps = {} if maps is None else maps
        self.worst = {}

    def np(self, t):
        return t.detach().cpu().numpy().astype(np.float64)

    def map_of(self, e):
        cm, kind = e['coords'], e['kind']
        key = (id(cm), kind)
        if key not in self.maps:
            c = cm.C.cpu().numpy().astype(np.int64)
            if kind == 'k3':
                self.maps[key] = R.neighbour_map(c, c, R.offsets(3) * cm.stride)
            elif kind == 'k1':
                self.maps[key] = np.arange(len(c))[None]
            elif kind == 'down':
                self.maps[key] = R.neighbour_map(e['out_coords'].C.cpu().numpy().astype(np.int64), c, R.offsets(2) * cm.stride)
            else:
                self.maps[key] = G.up_map(len(c))
        return self.maps[key]

    def note(self, family, got, want, bound):
        r = R.within(self.np(got).reshape(want.shape), want, bound)
        self.worst[family] = max(self.worst.get(family, 0.0), r)
        return r

    def layer(self, name):
        """checks the layer's parameter gradients; -> (gx, its bound) of the definition"""
        e = self.rec[name]
        nbr = self.map_of(e)
        x, g = self.np(e['x']), self.np(e['gy'])
        if e['relu'] and self.mut != 'ReLU mask dropped':
            g = g * (self.np(e['y']) > 0)
        W = self.np(self.params[name + '.kernel'])
        W = W[None] if W.ndim == 2 else W
        gW, gb, _ = def_wgrad(nbr, x, g)
        bW, bb = def_wgrad_bound(nbr, x, g)
        if self.mut == 'bias gradient omitted':
            gb = np.zeros_like(gb)
        fam = e['kind'] + (' first layer' if x.shape[1] == 1 else '')
        self.note(fam + ' gW', self.params[name + '.kernel'].grad, gW, bW)
        self.note(fam + ' gb', self.params[name + '.bias'].grad, gb, bb)
        if x.shape[1] == 1 and name == 'encoder.conv0':
            return None
        if self.mut == 'offsets not mirrored' and e['kind'] == 'k3':
            nbr = nbr[::-1]
        if self.mut == 'W not transposed' and W.shape[1] == W.shape[2]:
            W = W.transpose(0, 2, 1)
        return def_xgrad(nbr, x.shape[0], g, W), def_xgrad(nbr, x.shape[0], g, W, bound=True)

    def close(self, family, got, parts):
        """the gradient reaching a tensor = the sum of its consumers' contributions, added in fp32 in some order"""
        want = sum(p[0] for p in parts)
        e = sum(p[1] for p in parts)
        bound = R.BOUND_SLACK * (e + (len(parts) - 1) * U * (sum(np.abs(p[0]) for p in parts) + e))
        return self.note(family, got, want, bound)

    def block_out_grad(self, b):
        return torch.cat([self.rec[b + '.conv0_1']['gy'], self.rec[b + '.conv1_2']['gy']], 1)

    def block(self, b):
        """the five layers of one InceptionResNet; -> the parts that reach its input"""
        a = self.layer(b + '.conv0_1'); self.close('chain', self.rec[b + '.conv0_0']['gy'], [a])
        c = self.layer(b + '.conv1_2'); self.close('chain', self.rec[b + '.conv1_1']['gy'], [c])
        c = self.layer(b + '.conv1_1'); self.close('chain', self.rec[b + '.conv1_0']['gy'], [c])
        go = self.np(self.block_out_grad(b))
        return [self.layer(b + '.conv0_0'), self.layer(b + '.conv1_0'), (go, np.zeros_like(go))]

    def blocks(self, prefix, tail_parts):
        """three blocks whose last output receives tail_parts; -> the parts that reach the first block's input"""
        self.close('chain', self.block_out_grad(prefix + '.2'), tail_parts)
        parts = self.block(prefix + '.2')
        self.close('chain', self.block_out_grad(prefix + '.1'), parts)
        parts = self.block(prefix + '.1')
        self.close('chain', self.block_out_grad(prefix + '.0'), parts)
        return self.block(prefix + '.0')

    def run(self, alpha=1.0, beta=1.0):
        rec, n = self.rec, len(self.x)
        # leaves
        up_parts = None
        for l in (2, 1, 0):
            e = rec[f'decoder.conv{l}_cls']
            logits = self.np(e['y']).ravel()
            truth = G.isin(e['coords'].C.cpu().numpy(), [rec['encoder.block1.2.conv1_2'], rec['encoder.block0.2.conv1_2'], None][l]['coords'].C.cpu().numpy()
                           if l < 2 else self.x.C.cpu().numpy())
            scale = alpha / (n if self.mut == '1/len(out_cls) -> 1/len(x)' else len(logits))
            want = scale * G.bce_gradient(logits, truth)
            # (two roundings: the fp32 scale autograd hands the leaf, the value; + the definition's own sigmoid(z) - t, see test_bce_gradient_rounded_once)
            self.note('bce leaf', e['gy'], want.reshape(-1, 1), R.BOUND_SLACK * (2 * U * np.abs(want) + 2.0 ** -52 * scale / G.LN2).reshape(-1, 1))
            tail = [self.layer(f'decoder.conv{l}_cls')]
            if up_parts is not None:                      # the kept rows feed the next stage's transpose: scatter back to the candidates
                keep = np.nonzero(rec[f'decoder.prune{l}']['mask'].cpu().numpy())[0]
                full = [np.zeros_like(tail[0][0]) for _ in range(2)]
                full[0][keep], full[1][keep] = up_parts
                tail.append(tuple(full))
            parts = self.blocks(f'decoder.block{l}', tail)
            self.close('chain', rec[f'decoder.conv{l}']['gy'], parts)
            self.close('chain', rec[f'decoder.up{l}']['gy'], [self.layer(f'decoder.conv{l}')])
            rec[f'decoder.up{l}'].setdefault('kind', 'up')
            up_parts = self.layer(f'decoder.up{l}')
        eb = rec['entropy_bottleneck']
        packed = self.model.entropy_bottleneck.packed_params(DEV).cpu().numpy()
        gy, gp, _ = G.eb_gradients(packed, eb['x'].cpu().numpy(), passthrough=self.mut == 'clamp gradient passed through')
        gy, gp = beta / n * gy, beta / n * gp
        got = torch.cat([p.grad.reshape(-1) for lst in (self.model.entropy_bottleneck._matrices, self.model.entropy_bottleneck._biases,
                                                        self.model.entropy_bottleneck._factors) for p in lst])
        self.note('bottleneck parameters', got, gp, 2 * R.BOUND_SLACK * U * np.abs(gp))
        self.close('chain', rec['encoder.conv3']['gy'], [up_parts, (gy, 2 * R.BOUND_SLACK * U * np.abs(gy))])
        parts = [self.layer('encoder.conv3')]
        for i in (2, 1, 0):
            parts = self.blocks(f'encoder.block{i}', parts)
            self.close('chain', rec[f'encoder.down{i}']['gy'], parts)
            self.close('chain', rec[f'encoder.conv{i}']['gy'], [self.layer(f'encoder.down{i}')])
            parts = [self.layer(f'encoder.conv{i}')]
        return self.worst


def test_every_gradient_within_the_definitions_bound_and_mutations_fall_outside(sd):
    """(c) and (e): every parameter's gradient and every link of the chain lies within the bound of the definition's VJPs at the recorded
    forward point; each of the six mutated definitions falls outside it on at least one tensor family.  Largest error / bound ratios
    observed are printed (DESIGN §8b records them)."""
    sd = dict(sd)
    for k in ('encoder.conv3.kernel', 'encoder.conv3.bias'):       # a wider latent: some elements must reach the likelihood bound
        sd[k] = sd[k] * 16
    model = _model(sd)
    x = _input(['shell6', 'noisy_s'])
    record, maps = {}, {}
    _step_grads(model, x, record=record)
    lik = record['entropy_bottleneck']['likelihood']
    assert bool((lik == np.float32(1e-9)).any()), 'no latent element reaches the likelihood bound: the clamp mutation could not show'
    worst = _Definition(model, x, record, maps=maps).run()
    print('error / bound per family:', {k: round(v, 4) for k, v in worst.items()})
    assert len(record) >= 75
    for fam, r in worst.items():
        assert r <= 1.0, (fam, r)
    for mut in MUTATIONS:
        w = _Definition(model, x, record, mutation=mut, maps=maps).run()
        out = {k: v for k, v in w.items() if v > 1.0}
        print(f'mutation {mut!r}: outside the bound on', {k: float(f'{v:.3g}') for k, v in out.items()})
        assert out, mut
