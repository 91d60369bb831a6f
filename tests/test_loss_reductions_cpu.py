"""What tests/test_loss_reductions_device.py relies on, settled without a GPU: the fp64 definitions at channel counts other than 8
against the reference's own answers (tests/golden/loss_channels.npz), the channel tiling, the accuracy of the definition's per-term
functions against mpmath, and the TEETH of the device file's bounds: on the very inputs and sizes the kernels are run at, dropping or
double-counting one workgroup's terms, the final partial workgroup, or every slab slot a second trip of the last stage adds, moves the sum
by more than the bound the device's sum is held to."""
import os

import mpmath
import numpy as np
import pytest
import torch

import eval_reference as er
import fp64_reference as R
import grad_reference as G

TOL = 1e-12
TEETH_ULPS = 16                                                  # the device file's per-term allowance E is far below this (asserted there)


@pytest.fixture(scope='module')
def channels(golden_dir):
    return np.load(os.path.join(golden_dir, 'loss_channels.npz'))


@pytest.fixture(scope='module')
def b3_params(golden_dir):
    return np.load(os.path.join(golden_dir, 'eval_loss.npz'))['b3_params']


def _rel(got, want):
    scale = np.abs(want).max()
    return float(np.abs(got - want).max() / scale) if scale else float(np.abs(got).max())


# ------------------------------------------------------------------------------------------------ definitions at C != 8
def test_definitions_match_the_reference_at_other_channel_counts(channels):
    assert tuple(channels['channels'].tolist()) == er.OTHER_CHANNELS
    for C in er.OTHER_CHANNELS:
        p, y, ref = channels[f'c{C}_params'], channels[f'c{C}_y'], channels[f'c{C}_lik64']
        assert p.shape == (44 * C,) and y.shape == (67, C) and p.dtype == np.float32 and y.dtype == np.float32
        lik = er.likelihood(p, y)
        assert float(np.max(np.abs(lik - ref) / ref)) <= TOL
        at_bound = ref == 1e-9
        assert at_bound.any() and not at_bound.all() and np.all(lik[at_bound] == 1e-9) and np.all(lik >= 1e-9)
        bits64 = float(channels[f'c{C}_bits64'])
        assert abs(er.bits(lik) - bits64) <= TOL * bits64
        assert abs(er.exact_sum(-np.log2(lik)) - bits64) <= TOL * bits64
        gy, gp, b = G.eb_gradients(p, y)
        assert abs(b - bits64) <= TOL * bits64
        assert _rel(gy, channels[f'c{C}_gy']) <= TOL
        assert np.all(gy[at_bound] == 0) and np.all(channels[f'c{C}_gy'][at_bound] == 0)
        off = 0
        for t in G.eb_unpack(torch.from_numpy(channels[f'c{C}_gparams']), C):    # per tensor: one figure over the vector would hide the small ones
            n = t.numel()
            assert _rel(gp[off:off + n], channels[f'c{C}_gparams'][off:off + n]) <= TOL, (C, off)
            off += n


def test_tile_channels_repeats_the_columns_bit_for_bit(b3_params):
    y8 = er.latent_case(33, 8)
    lik8 = er.likelihood(b3_params, y8)
    assert np.array_equal(er.tile_channels(b3_params, 8), b3_params)
    for C in er.OTHER_CHANNELS:
        p = er.tile_channels(b3_params, C)
        assert p.dtype == np.float32 and p.shape == (44 * C,)
        cols = np.arange(C) % 8
        assert np.array_equal(er.likelihood(p, y8[:, cols]), lik8[:, cols])
        for a, b in zip(sum(er.eb_unpack(p, C), []), sum(er.eb_unpack(b3_params, 8), [])):
            assert np.array_equal(a, b[cols])


def test_row_gradients_are_the_jacobian_of_the_per_row_rate(b3_params):
    """grad_reference.eb_row_gradients (one backward pass) against torch.autograd.functional.jacobian of the per-row rate"""
    for C in (3, 8):
        p = er.tile_channels(b3_params, C)
        y, _ = er.gradient_case(12, C)
        assert (er.likelihood(p, y) == 1e-9).any()
        yt = torch.tensor(y.astype(np.float64))

        def row_rate(pt):
            return -torch.log2(G.likelihood(G.eb_unpack(pt, C), yt)).sum(1)
        J = torch.autograd.functional.jacobian(row_rate, torch.tensor(p.astype(np.float64))).numpy()
        rows = G.eb_row_gradients(p, y)
        assert rows.shape == J.shape == (12, 44 * C)
        assert np.abs(rows - J).max() <= TOL * np.abs(J).max()
        assert _rel(rows.sum(0), G.eb_gradients(p, y)[1]) <= TOL


# ------------------------------------------------------------------------------------------------ per-term accuracy of the definition
def _ulps(got, true):
    """|got - true| in units of the spacing of fp64 at `true` (an mpmath number)"""
    return float(abs(mpmath.mpf(float(got)) - true) / mpmath.mpf(float(np.spacing(abs(float(true))))))


def test_definition_terms_are_within_two_ulp_of_mpmath():
    mpmath.mp.dps = 50
    worst = 0.0
    for x in er.BCE_VALUES:
        for t in (0, 1):
            v = mpmath.mpf(float(x))
            true = (v if v > 0 else 0) - v * t + mpmath.log1p(mpmath.exp(-abs(v)))
            worst = max(worst, _ulps(er.bce_terms([x], [t])[0], true))
    print(f'bce_terms: {worst:.3f} ulp')
    assert worst <= 2.0
    lik = er.likelihood_samples()
    assert lik.dtype == np.float32 and len(lik) == 1000 and lik.min() == np.float32(1e-9) and lik.max() == np.float32(0.1)
    got = -np.log2(lik.astype(np.float64))
    worst = max(_ulps(g, -mpmath.log(mpmath.mpf(float(v)), 2)) for g, v in zip(got, lik))
    print(f'-log2: {worst:.3f} ulp')
    assert worst <= 2.0


# ------------------------------------------------------------------------------------------------ teeth
def _mutations_move_the_sum(terms, block, what):
    """every drop / double count of one block's terms, of the final partial block and of the slots from index 256 on changes the exactly
    added sum by more than the bound.  -> (smallest change, bound)"""
    m = terms.size
    bound = er.sum_bound(terms, TEETH_ULPS)
    if m == 0:
        return np.inf, bound
    assert terms.min() > bound, what                             # (so does every non-empty set of terms: they are all positive)
    total = er.exact_sum(terms)
    starts = np.arange(0, m, block)
    block_sums = np.add.reduceat(terms, starts)
    moved = [block_sums]                                         # any one block; the last entry is the final (partial) block
    if len(starts) > er.SLOTS:
        moved.append(np.array([er.exact_sum(terms[er.SLOTS * block:])]))
    smallest = np.inf
    for d in moved:
        for mutated in (total - d, total + d):                   # dropped, double-counted
            change = np.abs(mutated - total)
            assert np.all(change > bound), what
            smallest = min(smallest, float(change.min()))
    return smallest, bound


def test_bce_sizes_have_teeth():
    for n in er.BCE_SIZES:
        x, t, _ = er.bce_case(n)
        assert len(x) == n and (n < 98 or (np.any((x == 0) & ~np.signbit(x)) and np.any((x == 0) & np.signbit(x))))
        assert n == 0 or (np.abs(x).max() <= 4.0 and set(np.unique(t).tolist()) <= {0, 1, 2, 255})
        smallest, bound = _mutations_move_the_sum(er.bce_terms(x, t), er.BCE_BLOCK_ROWS, f'bce, {n} rows')
        if n == max(er.BCE_SIZES):
            assert set(np.unique(t).tolist()) == {0, 1, 2, 255}
            print(f'bce, {n} rows: smallest term {er.bce_terms(x, t).min():.4f}, smallest change {smallest:.1f}, bound {bound:.2e}')


def test_likelihood_sizes_have_teeth(b3_params):
    for C in (8,) + er.OTHER_CHANNELS:
        p = er.tile_channels(b3_params, C)
        rows = max(er.lik_rows(C))
        lik_all = er.likelihood(p, er.latent_case(rows, C)).astype(np.float32).astype(np.float64)    # as the device stores it
        assert lik_all.max() <= 0.5                              # every term is at least one bit
        for n in er.lik_rows(C):
            assert np.array_equal(er.latent_case(n, C), er.latent_case(rows, C)[:n])
            terms = -np.log2(lik_all[:n]).ravel()
            smallest, bound = _mutations_move_the_sum(terms, er.LIK_BLOCK, f'bits, {n} x {C}')
            if n == rows:
                print(f'bits, {n} x {C}: largest likelihood {lik_all.max():.4f}, smallest term {terms.min():.2f}, '
                      f'smallest change {smallest:.1f}, bound {bound:.2e}')


def test_sum_bound_is_the_documented_expression():
    t = np.array([1.0, -2.0, 3.5])
    assert er.sum_bound(t, 4) == R.BOUND_SLACK * (3 + 4) * 2.0 ** -53 * 6.5
    assert er.exact_sum([1e16, 1.0, -1e16]) == 1.0 and er.exact_sum([]) == 0.0
    assert er.bce_terms([0.0], [255])[0] == np.log(2.0)
