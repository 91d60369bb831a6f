"""The generator of the far-offset levels (tests/far_offsets.py) on the reference alone: its geometry at the true row counts, from index
arithmetic only, and its teeth — the exact emulation of the gather equals the fp64 definition, and every wrong offset rule that can
matter at a case's extent moves a clump output outside the fp64 bound or makes it non-finite.  No device, nothing of size N."""
import numpy as np
import pytest

import far_offsets as F
import fp64_reference as R
from oracle import pcgc_oracle as orc


def _weights(K, cin, cout, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1, 1, (K, cin, cout)) / np.sqrt(K * cin)).astype(np.float32), rng.uniform(-0.1, 0.1, (1, cout)).astype(np.float32)


def _case(name):
    kind, n, rb = F.CASES[name]
    L = F.make_level(n, kind, rb)
    nbr, rows = F.gather_map(L)
    rng = np.random.default_rng(len(name))
    x = rng.standard_normal((len(rows), 16)).astype(np.float32)
    Wk, b = _weights(nbr.shape[0], 16, 16)
    return L, nbr, x, Wk, b


@pytest.mark.parametrize('name', list(F.CASES))
def test_exact_emulation_is_the_definition_and_every_wrong_rule_is_caught(name):
    L, nbr, x, Wk, b = _case(name)
    y, e = R._conv(nbr, x, R.zero_bound(x), Wk, b)
    assert R.within(F.emulate(L, x, Wk, b, 'exact'), y, e) <= 1.0
    assert R.within(orc.conv_gather(nbr.astype(np.int32), x, Wk, b), y, e) <= 1.0          # (the bit-exact answer the device must give)
    tried = 0
    for rule in F.RULES:
        for sentinel in (F.LIMIT, F.GATHER_LIMIT):
            if not F.applicable(rule, L, sentinel) or (rule != 'sentinel_in_range' and sentinel != F.LIMIT):
                continue
            got = F.emulate(L, x, Wk, b, rule, sentinel)
            caught = (not np.isfinite(got).all()) or R.within(np.nan_to_num(got), y, e) > 1.0
            assert caught, f'{name}: rule {rule} (sentinel {sentinel:#x}) stays inside the fp64 bound on every clump output'
            tried += 1
    extent = L.n * L.row_bytes
    assert tried == 2 * (extent > F.SIGN) + (extent > 1 << 32) + (extent >= F.LIMIT + 16) + (extent >= F.GATHER_LIMIT + 16)
    assert tried >= 2                                                                       # every case reaches past the sign bit


def test_row_counts_against_the_thresholds():
    rb = F.ROW_BYTES
    assert F.ROWS_SIGN * rb == 1 << 31 and F.ROWS_SIGN == 8388608
    assert F.ROWS_LIMIT * rb == 0xF0000000 and F.ROWS_LIMIT == 15728640
    assert (F.ROWS_GATHER - 1) * rb < 0xFFFFFFF0 < F.ROWS_GATHER * rb and F.ROWS_GATHER - 1 == 16777215       # the limit lies inside that row
    assert F.CASES['below LIMIT'][1] * rb == 0xF0000000 - rb and F.CASES['at LIMIT'][1] * rb == 0xF0000000
    n_below, n_at = F.CASES['below LIMIT children'][1] // 8, F.CASES['at LIMIT children'][1] // 8
    assert (n_below, n_at) == (1966079, 1966080)
    assert 8 * n_below * rb == 0xF0000000 - 8 * rb and 8 * n_at * rb == 0xF0000000
    assert F.CASES['below GATHER_LIMIT'][1] * rb < 0xFFFFFFF0 <= (F.CASES['below GATHER_LIMIT'][1] + 1) * rb
    assert F.CASES['past 4 GiB'][1] * rb > 1 << 32
    below, above = F.CASES['map gate below'][1], F.CASES['map gate above'][1]
    assert 27 * below * 4 < 0xFFFFFFF0 <= 27 * above * 4 and above == below + 1 and F.CASES['map gate below'][2] == 64
    from pcgcv2_amd import dispatch
    assert dispatch.LIMIT == F.LIMIT


@pytest.mark.parametrize('name', list(F.CASES))
def test_geometry_at_the_true_row_counts(name):
    kind, n, rb = F.CASES[name]
    L = F.make_level(n, kind, rb)
    unit = 8 if kind == 'children' else 1
    (a0, w), (b0, _), (c0, _) = L.windows
    # three disjoint windows: the first rows, around byte offset 2^31, the last rows before the guards
    assert a0 == 0 and a0 + w <= b0 and b0 + w <= c0 and c0 + w == n - F.GUARD
    assert b0 * rb < F.SIGN <= (c0 + w) * rb, 'no clump row on each side of 2^31'
    if c0 == b0 + w:
        assert c0 * rb <= F.SIGN + (w // 2 + unit) * rb                       # (the level ends less than w rows past 2^31: the two straddle together)
    else:
        assert b0 * rb < F.SIGN < (b0 + w) * rb
    rows = L.rows
    assert len(np.unique(rows)) == len(rows) == F.SIDE ** 3 and rows.min() == 0 and rows.max() < n - F.GUARD
    in_window = np.zeros(len(rows), int)
    for s, c in L.windows:
        hit = (rows >= s) & (rows < s + c)
        in_window += hit
        assert hit.sum() >= len(rows) // 3 - unit
    assert (in_window == 1).all()
    assert not np.isin(rows, L.excluded).any() and (L.excluded >= 0).all() and (L.excluded < n).all()
    assert set(range(n - F.GUARD, n)) <= set(L.excluded.tolist())
    # the clump has no neighbour outside itself (its map is computed on the clump alone), interior voxels have all 27
    assert (L.nbr < len(rows)).all() and (L.nbr[13] == np.arange(len(rows))).all()
    assert ((L.nbr >= 0).sum(0) == 27).sum() == (F.SIDE - 2) ** 3
    # almost every clump row gathers from all three windows (nine in ten: a children level deals whole parents, 8 rows that are each other's neighbours)
    win = np.searchsorted([b0, c0], rows, side='right')
    src = np.where(L.nbr >= 0, win[np.maximum(L.nbr, 0)], win[None])
    assert np.mean(np.all([(src == v).any(0) for v in range(3)], 0)) > 0.9


@pytest.mark.parametrize('kind', ['plain', 'children', 'down'])
def test_device_map_of_a_small_level(kind):
    """far_map / far_features at a row count that fits anywhere (the windows clamp): fillers have only the centre entry, the clump's entries
    are its own map re-indexed, the features are the clump's at its rows, zero on fillers and NaN on the guards"""
    L = F.make_level(8 * 1200, kind)
    nbr = F.far_map(L, 'cpu').numpy()
    centre = 13 if kind != 'down' else 0
    if kind == 'children':
        filler = np.setdiff1d(np.arange(L.map_cols), L.parent_rows)
        np.testing.assert_array_equal(nbr[:, L.parent_rows], np.where(L.parent_nbr >= 0, L.parent_rows[np.maximum(L.parent_nbr, 0)], -1))
    else:
        filler = np.setdiff1d(np.arange(L.map_cols), L.rows)
        clump, _ = F.gather_map(L)
        np.testing.assert_array_equal(nbr[:, L.out_rows], np.where(clump >= 0, L.rows[np.maximum(clump, 0)], -1))
    assert (nbr[centre, filler] == filler).all() and (np.delete(nbr[:, filler], centre, 0) == -1).all()
    rng = np.random.default_rng(1)
    x = rng.standard_normal((len(L.rows), 16)).astype(np.float32)
    _, f = F.far_features(L, x, 'cpu', pad_bytes=4096)
    f = f.numpy()
    assert np.isnan(f[L.excluded]).all() and np.isfinite(np.delete(f, L.excluded, 0)).all()
    np.testing.assert_array_equal(f[L.rows], x)
    assert (np.delete(f, np.concatenate([L.rows, L.excluded]), 0) == 0).all()
