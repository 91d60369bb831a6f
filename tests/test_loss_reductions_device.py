"""GPU tests of the loss and rate reductions (csrc/loss.hip: pcgc_bce_logits, pcgc_eb_likelihood, pcgc_neg_log2_sum; csrc/grad.hip:
pcgc_bce_logits_bwd, pcgc_eb_likelihood_bwd) at the sizes training runs them at and at channel counts other than 8, against the fp64
definitions of tests/eval_reference.py and tests/grad_reference.py.

Sums.  The device adds fp64 terms in a fixed order: per thread, per workgroup into a slab slot, then ONE workgroup over the slots with a
stride of 256.  Its double is held to er.sum_bound of the exactly added (math.fsum) terms of the definition: the fp64 bound of a sum of
m terms in any order plus E ulp per term for the device's exp / log1p / log2.  tests/test_loss_reductions_cpu.py shows that on these very
inputs a dropped or double-counted workgroup, final partial workgroup or second trip of the last stage lies far outside that bound (it
uses 16 ulp per term; E is smaller), and holds the definition's own functions to 2 ulp of mpmath.

E is measured, not chosen: test_measured_allowance compares the device with the numpy definition on single terms — every value of
er.BCE_VALUES under both truth values, and 1 000 single-element -log2 sums.  Largest deviation seen on an MI355X: 1 ulp for the BCE term
(at x = 745, t = 1, where the term is exp(-745), one fp64 denormal unit; every other value is reproduced to the bit or to 1 ulp) and
1 ulp for -log2 (MEASURED below); E is twice that, 2 ulp."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import eval_reference as er
import fp64_reference as R
import grad_reference as G
from pcgcv2_amd import loss, ops, synthetic
from pcgcv2_amd.sparse import SparseTensor, sparse_collate

DEV = torch.device('cuda:0')
U = R.U
ONE_ROUNDING = 2.0 ** -23
BOUND32 = np.float32(1e-9)
LN2 = float(np.log(2.0))
MEASURED = {'bce term': 1.0, '-log2 term': 1.0}                  # largest |device - definition| in ulp (fp64), one MI355X
E = 2.0 * max(MEASURED.values())
CHANNELS = (8,) + er.OTHER_CHANNELS


def _t(a, dt=None):
    t = torch.as_tensor(np.ascontiguousarray(a), dtype=dt)
    if t.numel() == 0:                                           # (numpy gives an empty array zero strides; torch's own are row-major)
        t = torch.empty(t.shape, dtype=t.dtype)
    return t.to(DEV)


def _d(t):
    return float(t.item())


def _ulps(got, want):
    return abs(got - want) / float(np.spacing(abs(want)))


def _shifted(a, by=1):
    """device copy of a 1-D array as the [by:] view of a longer buffer: the same values at a pointer that is off the vector alignment"""
    buf = torch.zeros(len(a) + by, dtype=torch.as_tensor(a[:0]).dtype, device=DEV)
    buf[by:] = _t(a)
    return buf[by:]


def _wide(a, pad=2, extra_rows=0, fill=None, rng=None):
    """device copy of a [n, C] as columns pad .. pad + C of a wider (and longer) buffer of other values"""
    n, C = a.shape
    if fill is None:
        wide = _t((rng or np.random.default_rng(0)).normal(size=(n + extra_rows, C + 2 * pad)).astype(np.float32))
    else:
        wide = torch.full((n + extra_rows, C + 2 * pad), fill, dtype=torch.float32, device=DEV)
    wide[:n, pad:pad + C] = _t(a)
    return wide[:n, pad:pad + C]


@pytest.fixture(scope='module')
def b3_params(golden_dir):
    return np.load(os.path.join(golden_dir, 'eval_loss.npz'))['b3_params']


@pytest.fixture(scope='module')
def channels(golden_dir):
    return np.load(os.path.join(golden_dir, 'loss_channels.npz'))


# ------------------------------------------------------------------------------------------------ the allowance E
def _bce_term_deviations():
    out = []
    for x in er.BCE_VALUES:
        for t in (0, 1):
            got = _d(ops.bce_logits(_t(np.array([x], np.float32)), _t(np.array([t], np.uint8)))[0])
            want = float(er.bce_terms([x], [t])[0]) / LN2
            out.append((_ulps(got, want) if want else (0.0 if got == 0 else np.inf), float(x), t, got, want))
    return out


def test_measured_allowance():
    dev = _bce_term_deviations()
    worst_bce = max(dev)
    lik = er.likelihood_samples()
    want = -np.log2(lik.astype(np.float64))
    lik_d = _t(lik)
    got = np.array([_d(ops.neg_log2_sum(lik_d[i:i + 1].reshape(1, 1))) for i in range(len(lik))])
    d = np.abs(got - want) / np.spacing(np.abs(want))
    print(f'largest deviation from the definition: bce term {worst_bce[0]:.3f} ulp at x = {worst_bce[1]!r}, t = {worst_bce[2]}; '
          f'-log2 term {d.max():.3f} ulp at {lik[int(d.argmax())]!r}; E = {E}')
    # a deviation above 8 ulp is a finding to explain from the code, not a tolerance to widen
    assert worst_bce[0] <= 8 and d.max() <= 8
    assert worst_bce[0] <= MEASURED['bce term'] and d.max() <= MEASURED['-log2 term']
    assert E == 2.0 * max(MEASURED.values()) and E < 16


# ------------------------------------------------------------------------------------------------ a. BCE sums and counts
@pytest.mark.parametrize('n', er.BCE_SIZES)
def test_bce_sum_and_counts_at_the_reduction_edges(n):
    x, t, p = er.bce_case(n)
    terms = er.bce_terms(x, t)
    want, bound = er.exact_sum(terms) / LN2, er.sum_bound(terms, E) / LN2
    want_counts = er.counts(p, t)
    assert sum(want_counts) == n
    wide = torch.zeros((n, 3), dtype=torch.float32, device=DEV)
    wide[:, 1] = _t(x)
    layouts = {'dense': (_t(x), _t(t), _t(p)), 'column': (wide[:, 1:2], _t(t), _t(p)), 'shifted logits': (_shifted(x), _t(t), _t(p)),
               'shifted masks': (_t(x), _shifted(t), _shifted(p))}
    if n:
        assert layouts['dense'][0].data_ptr() % 16 == 0 and layouts['shifted logits'][0].data_ptr() % 16 == 4
        assert layouts['dense'][1].data_ptr() % 4 == 0 and layouts['shifted masks'][1].data_ptr() % 4 == 1
    first = None
    for name, (lx, lt, lp) in layouts.items():
        bce, counts = ops.bce_logits(lx, lt, lp)
        got = _d(bce)
        if first is None:
            first = got
            print(f'{n} rows: |error| / bound = {abs(got - want) / bound if bound else 0.0:.3e}')
            assert abs(got - want) <= bound
        assert got == first, name                                # the same partition, the same order: the same double
        assert tuple(counts.tolist()) == want_counts, name
        assert tuple(ops.bce_logits(None, lt, lp)[1].tolist()) == want_counts, name
    # without a prediction mask every row counts as "predicted absent": FN and TN only
    assert tuple(ops.bce_logits(_t(x), _t(t))[1].tolist()) == er.counts(np.zeros(n, bool), t)
    if n == max(er.BCE_SIZES):
        assert loss.get_cls_metrics(_t(p), _t(t)) == er.cls_metrics(p, t)
        assert loss.get_cls_metrics(_t(p != 0), _t(t != 0)) == er.cls_metrics(p, t)


# ------------------------------------------------------------------------------------------------ b. BCE values
def _bce_gradient_check(x, t, strided_too=True):
    for scale in (1.0, 0.37 / len(x)):
        want = scale * G.bce_gradient(x, t != 0)
        got = ops.bce_logits_bwd(_t(x), _t(t), scale=scale)
        assert got.shape == (len(x), 1)
        # the leaf bound of test_grad_device.py::test_bce_gradient_rounded_once
        bound = R.BOUND_SLACK * (U * np.abs(want) + 2.0 ** -52 * scale / G.LN2)
        ratio = R.within(got.cpu().numpy().ravel(), want, bound)
        assert ratio <= 1.0, (scale, ratio)
        if strided_too:
            assert torch.equal(ops.bce_logits_bwd(_wide(x.reshape(-1, 1), pad=3), _t(t), scale=scale), got)
    return ratio


def test_bce_values_one_at_a_time():
    """every value alone (n = 1: the term is the sum) under both truth values, within E ulp of the definition; then all of them in one
    gradient call, dense and as a strided column"""
    dev = _bce_term_deviations()
    worst = max(dev)
    print(f'largest deviation {worst[0]:.3f} ulp at x = {worst[1]!r}, t = {worst[2]} (E = {E})')
    for u, x, t, got, want in dev:
        assert u <= E, (x, t, got, want)
        assert np.isfinite(got) and got >= 0
    x = np.repeat(er.BCE_VALUES, 2)
    t = np.tile(np.array([0, 255], np.uint8), len(er.BCE_VALUES))
    ratio = _bce_gradient_check(x, t)
    print(f'gradient at the values: |error| / bound = {ratio:.3e}')
    g = ops.bce_logits_bwd(_t(x), _t(t)).cpu().numpy().ravel()
    big = np.abs(x) >= 745
    assert np.array_equal(g[big], np.where((x[big] > 0) == (t[big] != 0), 0.0, np.sign(x[big]) / LN2).astype(np.float32))


def test_bce_gradient_beyond_one_trip():
    x, t, _ = er.bce_case(262145)
    print(f'262 145 rows: |error| / bound = {_bce_gradient_check(x, t, strided_too=False):.3e}')


# ------------------------------------------------------------------------------------------------ c. likelihood and bits
def _check_likelihood_and_bits(params, y, lik64, what):
    n, C = y.shape
    yd, pd = _t(y), _t(params)
    lik_t, bits_t = ops.eb_likelihood(yd, pd, bound=1e-9, want_likelihood=True, want_bits=True)
    lik = lik_t.cpu().numpy()
    assert lik.shape == (n, C) and lik.dtype == np.float32
    if n:
        assert float(np.max(np.abs(lik.astype(np.float64) - lik64) / lik64)) <= ONE_ROUNDING, what
    at_bound = lik64 == 1e-9
    assert np.all(lik >= BOUND32) and np.all(lik[at_bound] == BOUND32), what
    bits = _d(bits_t)
    terms = -np.log2(lik.astype(np.float64))                     # of the likelihood as the device stored it
    want, bound = er.exact_sum(terms), er.sum_bound(terms, E)
    assert np.isfinite(bits) and abs(bits - want) <= bound, what
    # the fused rate without a stored likelihood, and the rate of the stored tensor: the same double
    assert _d(ops.eb_likelihood(yd, pd, bound=1e-9, want_likelihood=False, want_bits=True)[1]) == bits, what
    assert _d(ops.neg_log2_sum(lik_t)) == bits, what
    # columns of a wider buffer of NaNs with 64 rows of NaNs past the end: nothing outside [n, C] is read
    nan_view = _wide(y, pad=2, extra_rows=64, fill=float('nan'))
    lik_v, bits_v = ops.eb_likelihood(nan_view, pd, bound=1e-9, want_likelihood=True, want_bits=True)
    assert torch.equal(lik_v, lik_t) and _d(bits_v) == bits, what
    assert _d(ops.neg_log2_sum(_wide(lik, pad=3, extra_rows=64, fill=float('nan')))) == bits, what
    return abs(bits - want) / bound if bound else 0.0, at_bound


@pytest.mark.parametrize('C', CHANNELS)
def test_likelihood_and_bits_at_the_reduction_edges(b3_params, C):
    params = er.tile_channels(b3_params, C)
    lik_all = er.likelihood(params, er.latent_case(max(er.lik_rows(C)), C))
    worst = 0.0
    for n in er.lik_rows(C):
        ratio, _ = _check_likelihood_and_bits(params, er.latent_case(n, C), lik_all[:n], (C, n))
        worst = max(worst, ratio)
    print(f'C = {C}, rows {er.lik_rows(C)}: largest |bits error| / bound = {worst:.3e}')


def _bottleneck(params, C):
    from pcgcv2_amd.entropy_model import EntropyBottleneck
    eb = EntropyBottleneck(C)
    with torch.no_grad():
        for lst, vals in zip((eb._matrices, eb._biases, eb._factors), er.eb_unpack(params, C)):
            for p, v in zip(lst, vals):
                p.copy_(torch.from_numpy(v.astype(np.float32)))
    return eb.to(DEV)


@pytest.mark.parametrize('C', er.OTHER_CHANNELS)
def test_bottleneck_module_at_other_channel_counts(channels, C):
    params, y, lik64 = channels[f'c{C}_params'], channels[f'c{C}_y'], channels[f'c{C}_lik64']
    eb = _bottleneck(params, C)
    assert np.array_equal(eb.packed_params(DEV).cpu().numpy(), params)
    ratio, at_bound = _check_likelihood_and_bits(eb.packed_params(DEV).cpu().numpy(), y, lik64, C)
    assert at_bound.any()
    out, lik_t = eb(_t(y), quantize_mode=None)
    lik = lik_t.cpu().numpy()
    assert torch.equal(out, _t(y)) and torch.equal(lik_t, ops.eb_likelihood(_t(y), _t(params))[0])
    np.testing.assert_array_equal(np.maximum(eb._likelihood(_t(y)).cpu().numpy(), BOUND32), lik)
    # against the reference's fp64 bits: every stored likelihood is within 2^-23 relative, so every term within 2^-23 / ln 2
    bits64 = float(channels[f'c{C}_bits64'])
    got = loss.get_bits(lik_t)
    assert got.dtype == torch.float32 and _d(got) == float(np.float32(_d(ops.neg_log2_sum(lik_t))))
    assert abs(_d(ops.neg_log2_sum(lik_t)) - bits64) <= R.BOUND_SLACK * y.size * ONE_ROUNDING / LN2
    print(f'C = {C}: |bits error| / bound = {ratio:.3e}')


# ------------------------------------------------------------------------------------------------ d. bottleneck gradient
def _near_the_bound(lik64):
    """elements on which "below the bound" decided on the fp32 likelihood (device) and on the fp64 one (definition) can differ"""
    return (lik64 > 1e-9 * (1 - 1e-6)) & (lik64 < 1e-9 * (1 + 1e-6)) & (lik64 != 1e-9)


@pytest.mark.parametrize('C', CHANNELS)
def test_bottleneck_gradient_at_the_reduction_edges(b3_params, C):
    params = er.tile_channels(b3_params, C)
    base, _ = er.gradient_case(er.GRAD_BASE_ROWS, C)
    lik_base = er.likelihood(params, base)
    assert not _near_the_bound(lik_base).any() and (lik_base == 1e-9).any()
    abs_rows = np.abs(G.eb_row_gradients(params, base))         # [2 049, 44 C]: |d rate of base row i / d parameter|
    worst_y = worst_p = 0.0
    for n in er.grad_rows(C):
        y, idx = er.gradient_case(n, C)
        wy, wp, _ = G.eb_gradients(params, y)
        A = np.bincount(idx, minlength=er.GRAD_BASE_ROWS).astype(np.float64) @ abs_rows
        at_bound = lik_base[idx] == 1e-9
        assert n < 8 or at_bound.any()
        for scale in (1.0, 1.0 / 786432):
            first = None
            for feats in (_t(y), _wide(y, pad=3, extra_rows=5, rng=np.random.default_rng(n))):
                gy_t, gp_t = ops.eb_likelihood_bwd(feats, _t(params), bound=1e-9, scale=scale)
                gy, gp = gy_t.cpu().numpy(), gp_t.cpu().numpy()
                assert gy.shape == (n, C) and gp.shape == (44 * C,)
                if first is None:
                    first = (gy_t, gp_t)
                    assert np.all(gy[at_bound] == 0), (C, n)
                    if n == 0:
                        assert np.all(gp == 0)
                    ry = R.within(gy, scale * wy, R.BOUND_SLACK * U * np.abs(scale * wy))
                    rp = R.within(gp, scale * wp, R.BOUND_SLACK * (U * np.abs(scale * wp) + (n + E) * 2.0 ** -53 * scale * A))
                    assert ry <= 1.0 and rp <= 1.0, (C, n, scale, ry, rp)
                    worst_y, worst_p = max(worst_y, ry), max(worst_p, rp)
                else:                                            # a strided latent: the same gradients, bit for bit
                    assert torch.equal(gy_t, first[0]) and torch.equal(gp_t, first[1]), (C, n, scale)
    print(f'C = {C}, rows {er.grad_rows(C)}: largest |error| / bound: latent {worst_y:.3e}, parameters {worst_p:.3e}')


@pytest.mark.parametrize('C', er.OTHER_CHANNELS)
def test_bottleneck_gradient_against_the_reference_at_other_channel_counts(channels, C):
    params, y = channels[f'c{C}_params'], channels[f'c{C}_y']
    lik64 = channels[f'c{C}_lik64']
    assert not _near_the_bound(lik64).any()
    for scale in (1.0, 1.0 / 786432):
        for feats in (_t(y), _wide(y, pad=1)):
            gy, gp = ops.eb_likelihood_bwd(feats, _t(params), bound=1e-9, scale=scale)
            # the tolerance test_grad_device.py::test_bottleneck_gradient_rounded_once uses against the reference
            np.testing.assert_allclose(gp.cpu().numpy(), scale * channels[f'c{C}_gparams'], rtol=1e-6, atol=0)
            np.testing.assert_allclose(gy.cpu().numpy(), scale * channels[f'c{C}_gy'], rtol=1e-6, atol=0)
            assert np.all(gy.cpu().numpy()[lik64 == 1e-9] == 0)
    # through the module and autograd: loss.bits on the likelihood of a forward-train style leaf
    eb = _bottleneck(params, C)
    plist = [p for lst in (eb._matrices, eb._biases, eb._factors) for p in lst]
    from pcgcv2_amd import grad
    yq = _t(y).requires_grad_(True)
    grads = torch.autograd.grad(grad.Bits.apply(yq, 1.0, 1e-9, *plist), [yq] + plist)
    np.testing.assert_allclose(torch.cat([g.reshape(-1) for g in grads[1:]]).cpu().numpy(), channels[f'c{C}_gparams'], rtol=1e-6, atol=0)
    np.testing.assert_allclose(grads[0].cpu().numpy(), channels[f'c{C}_gy'], rtol=1e-6, atol=0)


# ------------------------------------------------------------------------------------------------ e. the training scalar
@pytest.fixture(scope='module')
def model():
    from pcgcv2_amd.pcc_model import PCCModel
    m = PCCModel().to(DEV)
    m.load_state_dict(synthetic.synthetic_state_dict())
    return m


def _input(names):
    clouds = [synthetic.cloud(nm) for nm in names]
    coords, feats = sparse_collate(clouds, [torch.ones((len(c), 1)) for c in clouds])
    return SparseTensor(feats, coordinates=coords, tensor_stride=1, device=DEV)


def _gen(seed=77):
    return torch.Generator(device=DEV).manual_seed(seed)


def _np(t):
    return t.detach().cpu().numpy()


def _definition(out, teacher_forced):
    """per level the BCE in bits, and the rate in bits, from the DEVICE's logits, coordinates and stored likelihood, added exactly"""
    bces = []
    for cls, gt in zip(out['out_cls_list'], out['ground_truth_list']):
        truth = er.isin(_np(cls.C), _np(gt.C))
        assert not teacher_forced or int(truth.sum()) == len(gt)     # (then every true voxel is a candidate)
        bces.append(er.exact_sum(er.bce_terms(_np(cls.F), truth)) / LN2)
    return bces, er.exact_sum(-np.log2(_np(out['likelihood']).astype(np.float64)))


def test_training_scalar_against_the_definition(model, tmp_path):
    from pcgcv2_amd.trainer import Trainer, TrainingConfig
    x = _input(['shell7', 'noisy_s'])
    out = model.forward_train(x, generator=_gen())
    total, bces, bpp = loss.sum_loss(out, len(x))
    want_bces, want_bits = _definition(out, True)
    want = sum(b / len(c) for b, c in zip(want_bces, out['out_cls_list'])) + want_bits / len(x)
    # every part is rounded once to fp32 and the four positive parts are added in fp32
    got_total = float(total.detach())
    print(f'sum_loss {got_total:.8f}, definition {want:.8f}: |error| / (8 u want) = {abs(got_total - want) / (8 * U * want):.3e}')
    assert abs(got_total - want) <= 8 * U * want
    for got, b, c in zip(bces, want_bces, out['out_cls_list']):
        assert abs(float(got) - b / len(c)) <= 8 * U * b / len(c)
    assert abs(float(bpp) - want_bits / len(x)) <= 8 * U * want_bits / len(x)
    trainer = Trainer(TrainingConfig(logdir=str(tmp_path / 'log'), ckptdir=str(tmp_path / 'ckpt'), init_ckpt='', alpha=1., beta=1.,
                                     lr=1e-4, check_time=1e9), model)
    rec = trainer.step(x, None, generator=_gen())
    assert torch.equal(rec['out_set']['likelihood'], out['likelihood'])
    assert abs(rec['sum_loss'] - want) <= 8 * U * want
    assert abs(rec['bpp'] - want_bits / len(x)) <= 8 * U * want_bits / len(x)


def test_evaluate_against_the_definition(model):
    x = _input(['shell7'])
    n = len(x)
    rec = loss.evaluate(model, x)
    out = model(x, training=False)
    want_bces, want_bits = _definition(out, False)
    for got, b in zip(rec['bces'], want_bces):
        assert abs(got - b / n) <= 8 * U * b / n
    assert abs(rec['bpp'] - want_bits / n) <= 8 * U * want_bits / n
    assert abs(rec['bce'] - sum(want_bces) / n) <= 8 * U * sum(want_bces) / n
    metrics = []
    for cls, gt in zip(out['out_cls_list'], out['ground_truth_list']):
        logits, k = _np(cls.F)[:, 0], len(gt)
        v = np.sort(logits + np.float32(0))[::-1]
        assert 0 < k < len(v) and v[k - 1] != v[k], 'a tie straddles the top-k threshold'
        metrics.append(er.cls_metrics(er.topk_mask(logits, k), er.isin(_np(cls.C), _np(gt.C))))
    assert rec['metrics'] == metrics
