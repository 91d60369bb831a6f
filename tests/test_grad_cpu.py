"""The fp64 definition of the training graph's gradients (tests/grad_reference.py), pinned on the CPU before tests/test_grad_device.py
judges the device by it: torch.autograd.gradcheck on a cloud of a few dozen points, and the reference's own fp64 gradients of get_bits
(through Low_bound.backward) and get_bce (tests/golden/grad_loss.npz, made by tests/golden/make_golden_grad.py) to 1e-12 relative."""
import os

import numpy as np
import pytest
import torch

import grad_reference as G
import fp64_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
TOL = 1e-12


def small_cloud(seed=3, n=40, extent=12, items=1):
    rng = np.random.default_rng(seed)
    out = []
    for b in range(items):
        c = np.unique(rng.integers(0, extent, size=(n, 3)), axis=0)
        c = c[np.lexsort((c[:, 0], c[:, 1], c[:, 2]))]
        out.append(np.concatenate([np.full((len(c), 1), b), c], 1))
    return np.concatenate(out).astype(np.int64)


def small_state_dict(seed=11):
    from pcgcv2_amd.synthetic import synthetic_state_dict
    return G.state_dict_f64(synthetic_state_dict(seed=seed, gain=4.0))


def _rel(got, want):
    scale = np.abs(want).max()
    return float(np.abs(got - want).max() / scale) if scale else float(np.abs(got).max())


def test_golden_bottleneck_gradients():
    ev, gg = np.load(os.path.join(GOLDEN, 'eval_loss.npz')), np.load(os.path.join(GOLDEN, 'grad_loss.npz'))
    kinds = set()
    for i in range(int(gg['n_bottleneck'])):
        gy, gp, b = G.eb_gradients(ev[f'b{i}_params'], ev[f'b{i}_y'])
        kinds.add(str(ev[f'b{i}_kind']))
        assert abs(b - float(ev[f'b{i}_bits64'])) <= TOL * abs(b)
        assert _rel(gy, gg[f'b{i}_gy']) <= TOL, (i, 'latent')
        # per tensor of the 12: a relative figure over the whole packed vector would hide the small ones
        off = 0
        for t in G.eb_unpack(torch.from_numpy(gg[f'b{i}_gparams'])):
            n = t.numel()
            assert _rel(gp[off:off + n], gg[f'b{i}_gparams'][off:off + n]) <= TOL, (i, off)
            off += n
        if str(ev[f'b{i}_kind']) == 'tails':
            clamped = ev[f'b{i}_lik64'] == 1e-9
            assert clamped.any() and (gg[f'b{i}_gy'][clamped] == 0).all() and (gy[clamped] == 0).all()
    assert kinds == {'int', 'noisy', 'tails'}


def test_golden_bce_gradient():
    ev, gg = np.load(os.path.join(GOLDEN, 'eval_loss.npz')), np.load(os.path.join(GOLDEN, 'grad_loss.npz'))
    assert int(gg['n_bce']) >= 3
    for i in range(int(gg['n_bce'])):
        g = G.bce_gradient(ev[f'e{i}_logits'], ev[f'e{i}_isin'], ln2=G.LN2_REFERENCE)
        assert _rel(g, gg[f'e{i}_glogits']) <= TOL


def test_clamp_passthrough_is_a_different_gradient():
    ev = np.load(os.path.join(GOLDEN, 'eval_loss.npz'))
    i = [j for j in range(int(ev['n_bottleneck'])) if str(ev[f'b{j}_kind']) == 'tails'][0]
    a = G.eb_gradients(ev[f'b{i}_params'], ev[f'b{i}_y'])[1]
    b = G.eb_gradients(ev[f'b{i}_params'], ev[f'b{i}_y'], passthrough=True)[1]
    assert not np.allclose(a, b, rtol=1e-6, atol=0)


def test_gradcheck_operators():
    rng = np.random.default_rng(5)
    c = small_cloud()
    nbr = R.neighbour_map(c, c, R.offsets(3))
    assert (nbr < 0).any() and (nbr >= 0).sum() > len(c)
    x = torch.tensor(rng.normal(size=(len(c), 3)), requires_grad=True)
    W = torch.tensor(rng.normal(size=(27, 3, 2)), requires_grad=True)
    b = torch.tensor(rng.normal(size=(2,)), requires_grad=True)
    assert torch.autograd.gradcheck(lambda x, W, b: G.conv(nbr, x, W, b), (x, W, b))
    p = torch.tensor(np.load(os.path.join(GOLDEN, 'eval_loss.npz'))['b3_params'].astype(np.float64), requires_grad=True)
    y = torch.tensor(rng.normal(0, 3, size=(7, 8)), requires_grad=True)
    assert torch.autograd.gradcheck(lambda p, y: G.bits(G.likelihood(G.eb_unpack(p), y)), (p, y))
    z = torch.tensor(rng.normal(0, 3, size=(9,)), requires_grad=True)
    mask = rng.random(9) < 0.5
    assert torch.autograd.gradcheck(lambda z: G.bce_bits(z, mask), (z,))


def test_gradcheck_whole_model():
    """sum_loss of the whole model on a cloud of a few dozen points, with respect to a sample of its parameters (every kind of layer);
    the kept sets are constants of the graph and are held fixed by the small finite-difference step (asserted: no logit near a top-k
    threshold would be the alternative; gradcheck itself fails if a set flips)"""
    c = small_cloud(items=2)
    sd = small_state_dict()
    n8 = len(R.down_coords(R.down_coords(R.down_coords(c, 1), 2), 4))
    noise = torch.tensor(np.random.default_rng(1).uniform(-0.5, 0.5, size=(n8, 8)))
    names = ['encoder.conv0.kernel', 'encoder.down1.kernel', 'encoder.block1.1.conv1_0.kernel', 'encoder.block2.0.conv0_1.bias',
             'encoder.conv3.kernel', 'entropy_bottleneck._matrices.1', 'entropy_bottleneck._factors.3', 'entropy_bottleneck._biases.0',
             'decoder.up0.kernel', 'decoder.up1.bias', 'decoder.block1.2.conv1_1.kernel', 'decoder.conv2_cls.kernel', 'decoder.conv0_cls.bias']
    leaves = [sd[n] for n in names]

    def f(*vals):
        s = dict(sd)
        s.update(zip(names, vals))
        return G.model_loss(s, c, noise)[0]
    # fast mode: the directional derivative along a random vector over all entries of the listed tensors at once (entry by entry would be
    # tens of thousands of forward passes)
    assert torch.autograd.gradcheck(f, leaves, eps=1e-6, atol=1e-6, rtol=1e-4, nondet_tol=0.0, fast_mode=True)


def test_definition_descends():
    """the fp64 definition through the steps of the device descent test (test_grad_device.py::test_descent): Adam, the reference's
    default learning rate 8e-4, weight decay 1e-4, the same noise at every step, one small cloud.  Its own drop must be at least 5 % of
    the initial loss, so that rounding cannot decide the sign of the device's drop."""
    import descent_case as D
    first, last = D.definition_descent()
    print(f'definition: sum_loss {first:.6f} -> {last:.6f} ({100 * (first - last) / first:.2f} % drop)')
    assert first - last >= 0.05 * first
