"""The select, coordinate and entropy-front-end kernels against exact brute-force definitions (tests/exact_reference.py).

csrc/select.hip, csrc/coords.hip and the front end of csrc/entropy.hip decide WHICH voxels exist and WHICH symbols are coded: an error
there is not a small deviation, it changes the cloud or the stream.  The other tests compare them with the CPU oracle on inputs the codec
itself produces.  Here the definitions are pinned to something that is not this project (torch.topk, np.unique, the reference goldens,
fp64_reference's searchsorted lookup), the oracle (CPU part) and every kernel (GPU part) must EQUAL them — integers and booleans: no
tolerance — on inputs built to reach what the codec's own inputs never reach: a populated tie in each radix pass and in the first / last
bin of a pick thread, denormals and infinities at the threshold, segment ends inside a thread's 8 rows, the 64-descriptor look-back
window, probe chains that wrap, duplicates across a wave boundary, the 2^20 border, batch 15, the int16 alphabet limit.  A mutated
definition (teeth test) must differ on the family that targets it."""
import glob
import os

import numpy as np
import pytest
import torch

import exact_reference as X
import fp64_reference as R
from oracle import pcgc_oracle as orc
from pcgcv2_amd import conventions, synthetic
from pcgcv2_amd._lib import PcgcError

REPORT = {}                                                       # family -> [cases, rows compared]


def _count(family, rows, cases=1):
    rec = REPORT.setdefault(family, [0, 0])
    rec[0] += cases
    rec[1] += int(rows)


def _eq(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f'{what}: shape {got.shape} vs {want.shape}'
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f'{what}: {len(bad)} of {got.size} entries differ, first at {tuple(bad[0])}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}')


@pytest.fixture
def conventions_reset():
    yield conventions
    conventions.reset()
    orc.CONVENTIONS.update(kernel_offset_order='xyz', topk_tie='low', dedup_keep='first')


@pytest.fixture(scope='module')
def select_cases():
    return X.radix_cases() + X.special_values()


def _coord_clouds():
    """[(name, rows, tensor stride)]: every coordinate generator, distinct rows"""
    out = [(f'border_s{s}', X.border_cloud(s), s) for s in (1, 2, 4, 8)]
    out += [('batch_raster', X.batch_cloud(), 1), ('batch_shuffled', X.batch_cloud(shuffle=True), 1), ('collated', X.collated_cloud(), 1)]
    return out


def _dup_clouds():
    """[(name, rows with duplicates)]"""
    c, _ = X.lane_duplicates()
    chain, _ = X.collision_case(1024, 1021, 10, n=400)
    rng = np.random.default_rng(3)
    both = np.concatenate([chain, chain[rng.integers(0, len(chain), 112)]])
    return [('lane_duplicates', c), ('chain_with_repeats', both[rng.permutation(len(both))])]


def _zyx_rows():
    """row k of the 'zyx' map = row ZYX[k] of the 'xyz' map (27 offsets)"""
    a, b = X.offsets(3, 'xyz').tolist(), X.offsets(3, 'zyx').tolist()
    return np.array([a.index(d) for d in b])


# ================================================================================================ CPU: the definitions pinned
def test_definition_topk_pinned_to_torch_and_golden(select_cases, golden_dir):
    for name, v, k in select_cases:
        for tie in ('low', 'high'):
            m = X.topk_mask(v, k, tie)
            assert m.sum() == k
            want = torch.topk(torch.from_numpy(v), k).values.numpy()
            _eq(np.sort(v[m] + np.float32(0)), np.sort(want + np.float32(0)), f'{name}/{tie}: kept multiset vs torch.topk')
    # the issue's own trial: 100 000 values bits(1.5f) + U[0, 1024): 1024 distinct keys that differ only in the last digit
    rng = np.random.default_rng(0)
    v = (np.float32(1.5).view(np.uint32) + rng.integers(0, 1024, 100000).astype(np.uint32)).view(np.float32)
    _eq(np.sort(v[X.topk_mask(v, 40000)]), np.sort(torch.topk(torch.from_numpy(v), 40000).values.numpy()), 'last-digit keys')
    g = np.load(os.path.join(golden_dir, 'ordering.npz'))
    for i in range(4):                                             # the tie rule: the reference's own masks
        _eq(X.topk_mask(g[f't{i}_vals'], int(g[f't{i}_k'])), g[f't{i}_mask'], f'golden t{i}')


def test_definition_sorts_pinned_to_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, 'ordering.npz'))
    for i in range(3):
        _eq(X.sort_zyx(g[f's{i}_coords']), g[f's{i}_argsort'], f'golden s{i}')
    c = X.batch_cloud(shuffle=True)
    order = X.sort_bzyx(c)
    assert (np.diff(c[order][:, 0]) >= 0).all()
    for b in np.unique(c[:, 0]):                                   # every item in the order it has when sorted alone
        rows = np.nonzero(c[:, 0] == b)[0]
        _eq(order[np.isin(order, rows)], rows[X.sort_zyx(c[rows])], f'batch-major item {b}')


@pytest.mark.parametrize('order', ['xyz', 'zyx'])
def test_definition_maps_pinned_to_searchsorted_lookup(order, conventions_reset):
    """dictionary lookup on tuples here, np.searchsorted on linearised keys in fp64_reference.py: two independent statements"""
    conventions.set_convention('kernel_offset_order', order)
    for name, c, s in _coord_clouds():
        _eq(X.k3_map(c, s, order), R.neighbour_map(c, c, R.offsets(3) * s), f'{name}: k3')
        (coarse, parent_of, down), = X.pyramid(c, s, 1, order)
        _eq(coarse, R.down_coords(c, s), f'{name}: coarse rows')
        _eq(down, R.neighbour_map(coarse, c, R.offsets(2) * s), f'{name}: down map (scatter vs lookup)')
        _eq(X.down_map(c, coarse, s, order), down, f'{name}: down map (lookup)')
        _eq(coarse[parent_of], X.quantize(c, 2 * s), f'{name}: parent_of')
        _eq(X.children(coarse, 2 * s, order), R.children_coords(coarse, 2 * s), f'{name}: children')


def test_definition_rounding_dedup_scale_and_hash_pinned():
    for name, x in X.entropy_cases():
        t = torch.round(torch.from_numpy(x))
        _eq(np.rint(x).view(np.uint32), t.numpy().view(np.uint32), f'{name}: np.rint vs torch.round')
        lo, hi = X.round_minmax(x)
        assert lo.tobytes() == (t.min() + 0).numpy().tobytes() and hi.tobytes() == (t.max() + 0).numpy().tobytes(), f'{name}: range'
        sym = X.symbolize(x, lo)
        _eq(sym, (t - float(lo)).to(torch.int16).numpy(), f'{name}: symbols')
        _eq(X.desymbolize(sym, lo), t.numpy() + np.float32(0), f'{name}: round trip')
    for name, c in _dup_clouds():
        kept, holder = X.dedup(c)
        _, first = np.unique(c, axis=0, return_index=True)
        _eq(kept, np.sort(first), f'{name}: dedup first vs np.unique')
        _eq(c[holder], c, f'{name}: holder')
        _, first_rev = np.unique(c[::-1], axis=0, return_index=True)
        _eq(X.dedup(c, 'last')[0], np.sort(len(c) - 1 - first_rev), f'{name}: dedup last')
    # scale: torch multiplies in fp32 by the fp32 factor, then rounds half to even
    for f in SCALE_FACTORS:
        c = _scale_rows(f)
        want = c.copy()
        want[:, 1:] = np.rint(c[:, 1:].astype(np.float32) * np.float32(f)).astype(np.int32)
        _eq(X.scale(c, f), want, f'scale {f}')
    # hash: occupied slots do not depend on the insertion order
    rows, _ = X.collision_case(1024, 1021, 10, n=300)
    keys = X.coord_key(rows)
    assert set(X.occupied_slots(keys, 1024)) == set(X.occupied_slots(keys[::-1], 1024)) and len(X.occupied_slots(keys, 1024)) == 300


SCALE_FACTORS = [0.375, 0.5, 0.75, 1.0 / 3.0, 1.0 / 0.375, 2.0, 1.0 / 0.75, 3.0]


def _scale_rows(f):
    """every x from 0 to the largest whose product stays below 2^20 (strided to <= 2^18 rows, both ends kept), random y, z"""
    top = int(np.floor((X.LIM - 1) / f)) if f > 1 else X.LIM - 1
    while np.rint(np.float32(top) * np.float32(f)) >= X.LIM:
        top -= 1
    x = np.unique(np.concatenate([np.arange(0, top + 1, max(1, (top + 1) >> 18)), np.arange(max(0, top - 4096), top + 1)]))
    rng = np.random.default_rng(int(f * 1000))
    c = np.zeros((len(x), 4), np.int32)
    c[:, 0], c[:, 1], c[:, 2], c[:, 3] = rng.integers(0, 16, len(x)), x, rng.integers(0, top + 1, len(x)), top - x
    return c


# ================================================================================================ CPU: the oracle equals the definitions
def test_oracle_equals_definition_select(select_cases, conventions_reset):
    for tie in ('low', 'high'):
        orc.CONVENTIONS['topk_tie'] = tie
        for name, v, k in select_cases:
            _eq(orc.topk_mask(v, k), X.topk_mask(v, k, tie), f'{name}/{tie}')
            _count('cpu oracle select', len(v))
        for rows, ks, v in _segment_lists():
            off = 0
            for r, k in zip(rows, ks):
                _eq(orc.topk_mask(v[off:off + r], max(k, 0)), X.topk_mask(v[off:off + r], k, tie), f'segment of {r} rows, k {k}/{tie}')
                off += r
            _count('cpu oracle select', len(v))


def test_oracle_equals_definition_coordinates(conventions_reset):
    for name, c in _dup_clouds():
        _eq(orc.unique_first(c), c[X.dedup(c)[0]], f'{name}: unique_first')
        orc.CONVENTIONS['dedup_keep'] = 'last'
        _eq(orc.unique_keep(c), c[X.dedup(c, 'last')[0]], f'{name}: unique_keep last')
        orc.CONVENTIONS['dedup_keep'] = 'first'
        _count('cpu oracle coordinates', len(c))
    for name, c, s in _coord_clouds():
        _eq(orc.unique_first(c), c, f'{name}: distinct rows stay')
        _eq(orc.kmap_k3(c, s), X.k3_map(c, s), f'{name}: kmap_k3')
        fine, st = c, s
        for coarse, parent_of, down in X.pyramid(c, s, 3):
            got_c, got_p = orc.stride2_coords(fine, 2 * st)
            _eq(got_c, coarse, f'{name}: stride2_coords at {2 * st}')
            _eq(got_p, parent_of, f'{name}: parent at {2 * st}')
            _eq(orc.kmap_down(fine, got_c, st), down, f'{name}: kmap_down at {st}')
            _eq(orc.kmap_k3(got_c, 2 * st), X.k3_map(coarse, 2 * st), f'{name}: kmap_k3 at {2 * st}')
            kids = X.children(coarse, 2 * st)
            _eq(orc.children_coords(got_c, 2 * st), kids, f'{name}: children_coords')
            fine, st = got_c, 2 * st
        _count('cpu oracle coordinates', len(c))
    # sort_zyx_perm restates array2vector(C, C.max() + 1), whose int64 key wraps once (C.max() + 1)^4 passes 2^63 — in the reference too
    # (data_utils.py:55-61) — so the oracle is compared where that key is exact: coordinates below 2^15
    rng = np.random.default_rng(5)
    small = np.concatenate([X.collated_cloud(), X.collated_cloud()[::7]])
    small = small[rng.permutation(len(small))]
    assert (small.max() + 1) ** 4 < 2 ** 63
    _eq(orc.sort_zyx_perm(small), X.sort_zyx(small), 'sort_zyx_perm (with repeats: stable)')
    _count('cpu oracle coordinates', len(small))


@pytest.fixture(scope='module')
def eb_params():
    return orc.pack_eb_params(synthetic.state_dict_to_numpy(synthetic.synthetic_state_dict()))


def _oracle_symbols(params, x):
    """the symbols orc.eb_compress codes, read back through orc.eb_decompress -> (values, min_v, max_v)"""
    data, lo, hi = orc.eb_compress(params, x)
    return orc.eb_decompress(params, data, lo, hi, x.shape), lo, hi


def test_oracle_equals_definition_symbols(eb_params):
    for name, x in X.entropy_cases():
        values, lo, hi = _oracle_symbols(eb_params, x)
        want_lo, want_hi = X.round_minmax(x)
        assert np.float32(lo).tobytes() == want_lo.tobytes() and np.float32(hi).tobytes() == want_hi.tobytes(), f'{name}: header range'
        _eq(values, X.desymbolize(X.symbolize(x, want_lo), want_lo), f'{name}: coded values')
        _count('cpu oracle symbols', x.size)


def test_an_uncodable_latent_always_shows_in_the_device_range():
    """the alphabet guard reads only the (min, max) that comes back with the symbols: in the order the device reduces in, a NaN or an
    infinity anywhere in the latent reaches one end of that range, and the order agrees with float order on everything else"""
    for name, x in X.entropy_cases():
        lo, hi = X.device_minmax(x)
        assert (lo, hi) == X.round_minmax(x) and np.isfinite([lo, hi]).all() and hi - lo + 1 < 32768, name
    for name, x in X.unsupported_latents():
        lo, hi = X.device_minmax(x)
        assert not (np.isfinite(lo) and np.isfinite(hi)) or hi - lo + 1 >= 32768, name
        if 'alphabet' not in name:
            assert not np.isfinite(x).all() and not (np.isfinite(lo) and np.isfinite(hi)), name


# ================================================================================================ CPU: teeth
def _mut_topk(v, k, sort_key):
    """top-k by an arbitrary sort key (descending), lower row first among equal keys"""
    order = np.lexsort((np.arange(len(v)), -sort_key.astype(np.float64)))
    m = np.zeros(len(v), bool)
    m[order[:k]] = True
    return m


def test_teeth_every_mutation_differs_from_the_oracle(select_cases, eb_params):
    """Each mutated definition must differ from the oracle on at least one input of the family that targets it: the inputs can tell."""
    v64 = lambda v: (np.asarray(v, np.float32) + np.float32(0)).astype(np.float64)
    tiny = np.float32(1.1754943508222875e-38)
    select_mut = {
        'tie to the higher row': lambda v, k: X.topk_mask(v, k, 'high'),
        '-0 < +0': lambda v, k: _mut_topk(v, k, v.astype(np.float64) - 1e-60 * np.signbit(v)),
        'denormals flushed to zero': lambda v, k: _mut_topk(v, k, np.where(np.abs(v) < tiny, 0.0, v64(v))),
        'keys compared as signed integers': lambda v, k: _mut_topk(v, k, (v + np.float32(0)).view(np.int32)),
        'the lowest 10 bits ignored': lambda v, k: _mut_topk(v, k, (X.order_key(v) & np.uint32(0xFFFFFC00)).astype(np.int64)),
    }
    family = {'tie to the higher row': 'pass', '-0 < +0': 'zero', 'denormals flushed to zero': 'denormal', 'keys compared as signed integers': '-neg',
              'the lowest 10 bits ignored': 'pass2'}
    for mut, fn in select_mut.items():
        cases = [(n, v, k) for n, v, k in select_cases if family[mut] in n]
        assert cases, mut
        caught = [n for n, v, k in cases if not np.array_equal(fn(v, k), orc.topk_mask(v, k))]
        assert caught, f'no {family[mut]} input catches: {mut}'
    # ---- coordinates
    c, _ = X.lane_duplicates()
    assert not np.array_equal(c[X.dedup(c, 'last')[0]], orc.unique_first(c)), 'dedup keeps the last'
    b = X.batch_cloud()
    assert not np.array_equal(X.k3_map(b, 1, key=lambda r: (0,) + tuple(r[1:])), orc.kmap_k3(b, 1)), 'lookup ignores the batch column'
    (coarse, _, _), = X.pyramid(b, 1, 1)
    assert not np.array_equal(X.down_map(b, coarse, 1, key=lambda r: (0,) + tuple(r[1:])), orc.kmap_down(b, coarse, 1)), 'down lookup ignores the batch'
    e = X.border_cloud(1)
    wrap = lambda r: (r[0], r[1] % X.LIM, r[2] % X.LIM, r[3] % X.LIM)
    assert not np.array_equal(X.k3_map(e, 1, key=wrap), orc.kmap_k3(e, 1)), 'lookup wraps modulo 2^20'
    e8 = X.border_cloud(8)
    assert not np.array_equal(X.k3_map(e8, 8, key=wrap), orc.kmap_k3(e8, 8)), 'lookup wraps modulo 2^20 (stride 8)'
    col = X.collated_cloud()
    assert not np.array_equal(X.k3_map(col, 1, 'zyx'), orc.kmap_k3(col, 1)), 'offset order zyx for xyz'
    (coarse, _, down), = X.pyramid(col, 1, 1)
    assert not np.array_equal(X.pyramid(col, 1, 1, 'zyx')[0][2], orc.kmap_down(col, coarse, 1)), 'offset order zyx for xyz (down)'
    kids = X.children(coarse, 2)
    mirrored = kids.reshape(-1, 8, 4)[:, ::-1].reshape(-1, 4)
    assert not np.array_equal(mirrored, orc.children_coords(coarse, 2)), 'child slot mirrored'
    assert not np.array_equal(down[::-1], orc.kmap_down(col, coarse, 1)), 'child slot mirrored (down)'
    c = col[np.random.default_rng(1).permutation(len(col))]
    xyz = np.lexsort((c[:, 0], c[:, 3], c[:, 2], c[:, 1]))
    assert not np.array_equal(xyz, orc.sort_zyx_perm(c)), 'sort by (x, y, z)'
    # ---- rounding
    x = dict(X.entropy_cases())['halves']
    away = np.trunc(x + np.copysign(np.float32(0.5), x))
    values, lo, _ = _oracle_symbols(eb_params, x)
    assert not np.array_equal(away + np.float32(0), values), 'rounding half away from zero'
    big = dict(X.entropy_cases())['near_2^23-0.5']
    assert not np.array_equal(np.trunc(big + np.float32(0.5)), _oracle_symbols(eb_params, big)[0]), 'rounding half away from zero at 2^23'


# ================================================================================================ segment lists (CPU and GPU parts)
def _segment_lists():
    """[(rows, ks, values)]: segment ends that are not multiples of 8, inside a 64-row word and around a 2048-row tile; empty segments;
    k of 0 / rows / rows + 1 / negative; a segment that is one single value; 16 segments"""
    rng = np.random.default_rng(11)
    rows = [1, 7, 63, 65, 2047, 2049, 0, 0, 5, 9, 4095, 3, 130, 1, 777, 2]
    ks = [1, 3, 0, 65, 1000, 2050, 0, 5, -2, 4, 2048, 3, 64, 0, 389, 1]
    assert len(rows) == 16 and any(r % 8 for r in rows) and sum(rows) % 8
    n = sum(rows)
    v = (np.round(rng.standard_normal(n) * 3) / 2).astype(np.float32)       # heavy ties
    v[rng.random(n) < 0.05] = -0.0
    off = np.concatenate([[0], np.cumsum(rows)])
    v[off[12]:off[13]] = 0.25                                                 # item 12: one single value, 64 of 130 needed
    v[off[10]:off[10] + 2000] = rng.standard_normal(2000).astype(np.float32)  # item 10: mostly distinct
    out = [(rows, ks, v)]
    rows2 = [5, 2043, 11, 2037, 64 * 3 + 1]                                    # ends at 5, 2048, 2059, 4096: on and off the tile boundary
    v2 = (np.round(rng.standard_normal(sum(rows2)) * 2) / 2).astype(np.float32)
    out.append((rows2, [2, 1000, 11, 1, 100], v2))
    return out


# ================================================================================================ GPU part
gpu = pytest.mark.gpu
DEV = torch.device('cuda:0')


def _t(a, dt=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(DEV)


def _n(t):
    return t.cpu().numpy()


def _set_tie(tie):
    conventions.set_convention('topk_tie', tie)
    orc.CONVENTIONS['topk_tie'] = tie


def _views(v):
    """the same logits as a fresh [n, 1] tensor (16-byte aligned, ld 1), as column 1 of an [n, 3] tensor (ld 3) and as flat[1:] (ld 1, base
    4 bytes off a 16-byte boundary): the last two take the scalar loads"""
    n = len(v)
    wide = np.full((n, 3), 1e30, np.float32)
    wide[:, 1] = v
    flat = np.concatenate([[np.float32(-1e30)], v]).astype(np.float32)
    a, b, c = _t(v).reshape(-1, 1), _t(wide)[:, 1:2], _t(flat)[1:].reshape(-1, 1)
    assert a.data_ptr() % 16 == 0 and b.stride(0) == 3 and c.data_ptr() % 16 == 4 and c.stride(0) == 1
    return {'fresh': a, 'column': b, 'offset': c}


def _check_select(ops, v, rows, ks, tie, what, coords=None, parent=None, parent_stride=0, views=False, oracle=True):
    """topk_mask_segments and topk_select (given coordinates, or children of `parent`) against the definition, and the oracle"""
    n = len(v)
    want = X.topk_mask_segments(v, rows, ks, tie)
    if oracle:
        off = 0
        for r, k in zip(rows, ks):
            _eq(orc.topk_mask(v[off:off + r], max(k, 0)), want[off:off + r], f'{what}: oracle')
            off += r
    cand = coords if coords is not None else X.children(parent, parent_stride)
    bits_w, wprefix_w, orig_w, out_w = X.select_outputs(want, cand)
    for view, logits in (_views(v) if views else {'fresh': _t(v).reshape(-1, 1)}).items():
        w = f'{what}/{tie}/{view}'
        _eq(_n(ops.topk_mask_segments(logits, rows, ks)).astype(bool), want, f'{w}: topk_mask_segments')
        if len(rows) == 1:
            _eq(_n(ops.topk_mask(logits, ks[0])).astype(bool), want, f'{w}: topk_mask')
        bits, wprefix, orig, out = ops.topk_select(logits, rows, ks, coords=None if coords is None else _t(coords, torch.int32),
                                                   parent_coords=None if parent is None else _t(parent, torch.int32), parent_stride=parent_stride)
        _eq(_n(bits), bits_w, f'{w}: bitmap (padding bits of the last word clear)')
        _eq(_n(wprefix), wprefix_w, f'{w}: wprefix')
        _eq(_n(orig), orig_w, f'{w}: orig')
        _eq(_n(out), out_w, f'{w}: survivor coordinates')
    _count('select', n)
    return want


@gpu
@pytest.mark.parametrize('tie', ['low', 'high'])
def test_gpu_select_radix_passes_and_special_values(tie, select_cases, conventions_reset):
    from pcgcv2_amd import ops
    _set_tie(tie)
    rng = np.random.default_rng(2)
    for name, v, k in select_cases:
        n = len(v)
        c4 = np.concatenate([rng.integers(0, 16, (n, 1)), rng.integers(0, X.LIM - 1, (n, 3))], 1).astype(np.int32)
        _check_select(ops, v, [n], [k], tie, name, coords=c4, views=True)
        pad = (-n) % 8                                              # the children form has 8 rows per parent: pad with the smallest value
        v8 = np.concatenate([v, np.full(pad, v.min(), np.float32)])
        parent = np.concatenate([rng.integers(0, 16, (len(v8) // 8, 1)), 2 * rng.integers(0, X.LIM // 2 - 1, (len(v8) // 8, 3))], 1).astype(np.int32)
        _check_select(ops, v8, [len(v8)], [k], tie, name + ' (children)', parent=parent, parent_stride=2)


@gpu
@pytest.mark.parametrize('tie', ['low', 'high'])
def test_gpu_select_segments(tie, conventions_reset):
    from pcgcv2_amd import ops
    _set_tie(tie)
    rng = np.random.default_rng(4)
    for rows, ks, v in _segment_lists():
        n = len(v)
        c4 = np.concatenate([np.repeat(np.arange(len(rows)), rows)[:, None], rng.integers(0, X.LIM, (n, 3))], 1).astype(np.int32)
        _check_select(ops, v, rows, ks, tie, f'{len(rows)} segments', coords=c4, views=True)
    # 17 segments are refused on the host side
    rows17, v17 = [3] * 17, np.zeros(51, np.float32)
    with pytest.raises(PcgcError):
        ops.topk_mask_segments(_t(v17).reshape(-1, 1), rows17, [1] * 17)
    with pytest.raises(PcgcError):
        ops.topk_select(_t(v17).reshape(-1, 1), rows17, [1] * 17, coords=_t(np.zeros((51, 4), np.int32)))
    # one 3 M-row item beside 15 items of 1-9 rows: the grid is sized by the largest
    rows = [3, 1, 9, 3000001, 2, 5, 7, 1, 4, 6, 8, 2, 9, 1, 3, 5]
    ks = [2, 1, 4, 1234567, 0, 5, 8, 0, -1, 3, 8, 1, 5, 1, 2, 4]
    n = sum(rows)
    v = (np.round(rng.standard_normal(n) * 200) / 64).astype(np.float32)       # a few thousand distinct values: a tie at the threshold
    c4 = np.concatenate([np.repeat(np.arange(16), rows)[:, None], rng.integers(0, X.LIM, (n, 3))], 1).astype(np.int32)
    _check_select(ops, v, rows, ks, tie, 'giant item beside 15 tiny ones', coords=c4, oracle=False)


@gpu
@pytest.mark.parametrize('tiles', [64, 65, 128, 129, 1700])
def test_gpu_scan_compaction_and_gathers_at_the_lookback_window(tiles, conventions_reset):
    """mask_scan and topk_select walk back 64 tile descriptors at a time: all-kept, none-kept and alternating selections at 64, 65, 128,
    129 and ~1700 tiles (the product's stride-1 level); compaction and gathers on the same rows"""
    from pcgcv2_amd import ops
    rng = np.random.default_rng(tiles)
    n = tiles * 2048 - 5
    assert (n + 2047) // 2048 == tiles
    c4 = np.concatenate([rng.integers(0, 16, (n, 1)), rng.integers(0, X.LIM - 1, (n, 3))], 1).astype(np.int32)
    alt = (np.arange(n) % 2).astype(np.float32)
    ragged = (rng.random(n) < 0.4).astype(np.float32)
    for what, v, k in (('all kept', ragged, n), ('none kept', ragged, 0), ('alternating', alt, n // 2), ('alternating + tie', alt, n // 2 + 10),
                       ('ragged + tie', ragged, int(ragged.sum()) + 12345)):
        for tie in (('low', 'high') if tiles <= 129 or 'tie' in what else ('low',)):   # (each is a 3.5 M-row sort on the host at ~1700 tiles)
            _set_tie(tie)
            want = _check_select(ops, v, [n], [k], tie, f'{tiles} tiles, {what}', coords=c4, oracle=False)
        m = _t(want.astype(np.uint8))                                 # (tie 'high' mask: survivors bunch at the end)
        prefix, total = ops.mask_scan(m)
        _eq(_n(prefix), np.cumsum(want) - want, f'{tiles} tiles, {what}: mask_scan')
        assert int(total.item()) == want.sum()
        kept = int(want.sum())
        _eq(_n(ops.compact_coords(_t(c4), m, prefix, kept)), c4[want], f'{tiles} tiles, {what}: compact_coords')
        _eq(_n(ops.compact_index(m, prefix, kept)), np.nonzero(want)[0], f'{tiles} tiles, {what}: compact_index')
        _count('scan / compaction', n)
    # features: every width and column slices of a 48-wide buffer (at ~1700 tiles: the narrow widths only)
    want = ragged.astype(bool)
    m = _t(want.astype(np.uint8))
    prefix, _ = ops.mask_scan(m)
    orig = ops.compact_index(m, prefix, int(want.sum()))
    perm = rng.permutation(n).astype(np.int32)
    _eq(_n(ops.gather_coords(_t(c4), _t(perm))), c4[perm], f'{tiles} tiles: gather_coords')
    for C in ((1, 3, 4, 8, 48) if tiles <= 129 else (1, 4)):
        f = rng.standard_normal((n, C)).astype(np.float32)
        ft = _t(f)
        _eq(_n(ops.compact_feats(ft, m, prefix, int(want.sum()))), f[want], f'{tiles} tiles: compact_feats C={C}')
        _eq(_n(ops.gather_feats(ft, _t(perm))), f[perm], f'{tiles} tiles: gather_feats C={C}')
        if C % 4 == 0:
            _eq(_n(ops.gather_rows(ft, orig)), f[want], f'{tiles} tiles: gather_rows C={C}')
        if C == 48:
            for lo, hi in ((0, 32), (4, 36), (2, 34), (1, 4), (5, 6), (3, 48)):
                view = ft[:, lo:hi]                                   # columns 2..34: whole float4s per row, base 8 bytes off -> the scalar kernel
                _eq(_n(ops.compact_feats(view, m, prefix, int(want.sum()))), f[want][:, lo:hi], f'{tiles} tiles: compact_feats columns {lo}..{hi}')
            assert ft[:, 2:34].data_ptr() % 16 == 8 and (34 - 2) % 4 == 0 and ft.stride(0) % 4 == 0
            _eq(_n(ops.gather_rows(ft[:, 4:36], orig)), f[want][:, 4:36], f'{tiles} tiles: gather_rows columns 4..36')
            with pytest.raises(PcgcError):                             # (documented: gather_rows needs 16-byte aligned rows)
                ops.gather_rows(ft[:, 2:34], orig)
        _count('scan / compaction', n * C)


@gpu
def test_gpu_select_nan_logits_keep_the_structure(conventions_reset):
    """A NaN logit means a broken model; torch.topk (NaN largest), the oracle's argsort (NaN last) and the kernel's keys (+NaN above +inf,
    -NaN below -inf: DESIGN.md §3) disagree about it, so only the structure is required: exactly k survivors per item, bitmap, wprefix, orig
    and coordinates mutually consistent, finite rows ranked correctly among themselves."""
    from pcgcv2_amd import ops
    rng = np.random.default_rng(8)
    rows, ks = [700, 1301, 64], [100, 1000, 64]
    n = sum(rows)
    v = (np.round(rng.standard_normal(n) * 4) / 2).astype(np.float32)
    nan_rows = rng.choice(n, 40, replace=False)
    v[nan_rows[:20]] = np.nan
    v[nan_rows[20:]] = -np.float32(np.nan)
    c4 = np.concatenate([np.repeat(np.arange(3), rows)[:, None], rng.integers(0, X.LIM, (n, 3))], 1).astype(np.int32)
    for tie in ('low', 'high'):
        _set_tie(tie)
        bits, wprefix, orig, out = ops.topk_select(_t(v).reshape(-1, 1), rows, ks, coords=_t(c4))
        mask = np.unpackbits(_n(bits), bitorder='little')
        assert not mask[n:].any()
        mask = mask[:n].astype(bool)
        _eq(_n(ops.topk_mask_segments(_t(v).reshape(-1, 1), rows, ks)).astype(bool), mask, 'mask form = select form')
        b2, w2, o2, c2 = X.select_outputs(mask, c4)
        _eq(_n(wprefix), w2, 'wprefix'); _eq(_n(orig), o2, 'orig'); _eq(_n(out), c2, 'coordinates')
        off = 0
        for r, k in zip(rows, ks):
            seg, m = v[off:off + r], mask[off:off + r]
            assert m.sum() == k
            fin = np.isfinite(seg)
            _eq(m[fin], X.topk_mask(seg[fin], int(m[fin].sum()), tie), 'finite rows ranked among themselves')
            off += r
        _count('select', n)


# ------------------------------------------------------------------------------------------------ hash
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def _check_table(ops, rows, absent, what, distinct):
    n = len(rows)
    keys = X.coord_key(rows)
    for keep in ('first', 'last'):
        table = ops.HashTable(_t(rows), 1, keep_last=keep == 'last')
        assert table.cap == X.hash_capacity(n)
        slots = _n(table.keys).view(np.uint64)
        want = X.occupied_slots(keys, table.cap)
        _eq(np.nonzero(slots != EMPTY)[0], np.array(sorted(want)), f'{what}/{keep}: occupied slots')
        _eq(np.sort(slots[slots != EMPTY]), np.unique(keys), f'{what}/{keep}: every key once')
        home = X.home_slot(slots[slots != EMPTY], table.cap)
        at = np.nonzero(slots != EMPTY)[0]
        for h, a in zip(home.tolist(), at.tolist()):                  # linear probing: no empty slot between a key's home and its slot
            assert all(((h + d) & (table.cap - 1)) in want for d in range((a - h) % table.cap)), f'{what}/{keep}: a key is unreachable'
        keep_m, first = ops.first_occurrence_mask(_t(rows), table, want_rows=True)
        kept, holder = X.dedup(rows, keep)
        _eq(_n(first), holder, f'{what}/{keep}: row held for each key')
        _eq(np.nonzero(_n(keep_m))[0], kept, f'{what}/{keep}: kept rows')
        _eq(_n(ops.hash_contains(_t(rows), table)), np.ones(n, np.uint8), f'{what}/{keep}: present keys found')
        _eq(_n(ops.hash_contains(_t(absent), table)), np.zeros(len(absent), np.uint8), f'{what}/{keep}: absent keys inside the chain')
        if distinct and keep == 'first':
            _eq(_n(ops.kmap_k3(_t(rows), 1, table)), X.k3_map(rows, 1), f'{what}: kmap_k3 (26 absent probes per row)')
        _count('hash', n)


@gpu
def test_gpu_hash_chains_wrap_and_half_full_tables():
    from pcgcv2_amd import ops
    rng = np.random.default_rng(6)
    for cap, home, length, n in ((1024, 5, 12, 12), (1024, 1021, 10, 10), (1024, 1019, 40, 511), (1024, 1021, 9, 512), (2048, 2045, 9, 513),
                                 (4096, 4093, 12, 1500), (4096, 100, 30, 2048)):
        rows, absent = X.collision_case(cap, home, length, n=n)
        _check_table(ops, rows, absent, f'cap {cap} home {home} chain {length} n {n}', distinct=True)
    # the same chains with repeated rows: 511 and 512 rows of 400 distinct keys (capacity 1024)
    for total in (511, 512):
        rows, absent = X.collision_case(1024, 1021, 10, n=400)
        rows = np.concatenate([rows, rows[rng.integers(0, 400, total - 400)]])
        _check_table(ops, rows[rng.permutation(total)], absent, f'{total} rows of 400 keys', distinct=False)
    c, _ = X.lane_duplicates()
    _check_table(ops, c, np.array([[0, 1, 2, 3], [15, X.LIM - 1, X.LIM - 1, X.LIM - 2]], np.int32), 'lane duplicates', distinct=False)
    # n = 2^18 distinct rows: the table is exactly half full (capacity 2^19); a dense block, so the k3 map has neighbours
    n = 1 << 18
    cells = rng.choice(128 ** 3, n, replace=False)
    rows = np.stack([np.zeros(n, np.int64), cells % 128 + 500, cells // 128 % 128, cells // 16384 + X.LIM - 128], 1).astype(np.int32)
    table = ops.HashTable(_t(rows), 1)
    assert table.cap == 2 * n == X.hash_capacity(n)
    slots = _n(table.keys).view(np.uint64)
    _eq(np.nonzero(slots != EMPTY)[0], np.array(sorted(X.occupied_slots(X.coord_key(rows), table.cap))), 'half-full table: occupied slots')
    got = _n(ops.kmap_k3(_t(rows), 1, table))
    _eq(got, orc.kmap_k3(rows, 1), 'half-full table: kmap_k3 vs oracle')
    _eq(got[:, :20000], _k3_of_first(rows, 20000), 'half-full table: kmap_k3 vs definition')
    _count('hash', n)


def _k3_of_first(rows, m):
    """definition map of the first m rows of a cloud (all rows are candidates as neighbours)"""
    return X.neighbour_map(rows[:m], rows, X.offsets(3))


def _pyramid_lane_cloud():
    """distinct stride-1 rows whose stride-2 CELLS repeat in runs over wave and block boundaries (lane_duplicates, each repeat at another
    child slot of the cell): the pyramid's insert has the same consecutive-lane shortcut as the plain one"""
    c, runs = X.lane_duplicates()
    f = c.astype(np.int64)
    f[:, 1:] = (f[:, 1:] >> 1) << 1
    slot = np.zeros(len(f), np.int64)
    for s, L in runs:
        slot[s:s + L] = np.arange(L) % 8
    slot[[len(f) - 1, len(f) - 100]] = 7
    f[:, 1] += slot & 1; f[:, 2] += (slot >> 1) & 1; f[:, 3] += slot >> 2
    _, first = np.unique(f, axis=0, return_index=True)
    again = np.setdiff1d(np.arange(len(f)), first)                   # (a 9th repeat, a far repeat of a full cell): moved to a cell of its own
    f[again, 1:] = np.stack([again * 2, again * 2 + 2, again * 0 + 4], 1)
    assert len(np.unique(f, axis=0)) == len(f) and X.in_range(f).all()
    q = X.quantize(f, 2)
    for s, L in runs:
        assert (q[s:s + min(L, 8)] == q[s]).all()
    return f.astype(np.int32)


# ------------------------------------------------------------------------------------------------ coordinates
@gpu
def test_gpu_pyramid_and_maps_through_every_origin(monkeypatch, conventions_reset):
    from pcgcv2_amd import ops, sparse
    from pcgcv2_amd.sparse import CoordMap
    zyx = _zyx_rows()
    clouds = _coord_clouds() + [('cell_runs', _pyramid_lane_cloud(), 1)]
    rng = np.random.default_rng(12)
    defs = {}
    for gate in (sparse.HASH_LEVEL_MAX, 8):                          # hashed maps, then every map derived through the parent level
        monkeypatch.setattr(sparse, 'HASH_LEVEL_MAX', gate)
        for name, c, s in clouds:
            w = f'{name} (gate {gate})'
            if name not in defs:                                     # (the definitions: once per cloud)
                lv = X.pyramid(c, s, 4)
                fines = [c] + [l[0] for l in lv[:2]]
                kc_ = X.children(lv[2][0], 8 * s)
                keep_ = rng.random(len(kc_)) < 0.45
                kmap_ = X.k3_map(kc_, 4 * s)
                defs[name] = (lv, [X.k3_map(f, s << l) for l, f in enumerate(fines)], X.k3_map(c, s, 'zyx'), kc_, keep_, kmap_, X.prune_map(kmap_, keep_),
                              X.k3_map(kc_[keep_], 4 * s))
            want_levels, want_k3s, want_zyx, kc, keep, kmap, want_pruned, want_survivors = defs[name]
            for levels in (1, 2, 3, 4):
                top = CoordMap(_t(c), s, unique=True)
                top.build_pyramid(levels)
                lvl = top
                for l in range(levels):
                    coarse, down = lvl._down
                    _eq(_n(coarse.C), want_levels[l][0], f'{w}: build_pyramid({levels}) level {l} rows')
                    _eq(_n(lvl._parent_of), want_levels[l][1], f'{w}: build_pyramid({levels}) level {l} parent_of')
                    _eq(_n(down), want_levels[l][2], f'{w}: build_pyramid({levels}) level {l} down')
                    lvl = coarse
            lvl, fine, st = CoordMap(_t(c), s, unique=True), c, s      # level by level, and every level's own k3 map
            for l in range(3):
                k3 = _n(lvl.k3)
                _eq(k3, want_k3s[l], f'{w}: k3 at stride {st}')
                if l == 0:
                    _eq(k3[zyx], want_zyx, f'{w}: k3 with z-fastest offsets')
                    _eq(k3, orc.kmap_k3(fine, st), f'{w}: k3 vs oracle')
                coarse, down = lvl.down()
                _eq(_n(coarse.C), want_levels[l][0], f'{w}: down() level {l} rows')
                _eq(_n(down), want_levels[l][2], f'{w}: down() level {l} map')
                _eq(_n(down), orc.kmap_down(fine, want_levels[l][0], st), f'{w}: down() level {l} vs oracle')
                lvl, fine, st = coarse, want_levels[l][0], 2 * st
            # children of the stride-8s level, their map, then pruned / selected levels through the candidates' map and through the parent's
            logits = np.where(keep, 1.0, -1.0).astype(np.float32)
            _eq(want_pruned, want_survivors, f'{w}: prune_map = map of the survivors')
            for own_map in (True, False):
                kids = lvl.up()
                _eq(_n(kids.C), kc, f'{w}: children rows')
                _eq(_n(kids.C), orc.children_coords(fine, st), f'{w}: children rows vs oracle')
                if own_map:
                    _eq(_n(kids.k3), kmap, f'{w}: children k3')
                m = _t(keep.astype(np.uint8))
                prefix, _ = ops.mask_scan(m)
                pruned = CoordMap(ops.compact_coords(kids.C, m, prefix, int(keep.sum())), st // 2, unique=True, origin=('pruned', kids, m, prefix))
                _eq(_n(pruned.k3), want_pruned, f'{w}: pruned by byte mask (own map {own_map})')
                seg = [8 * r for r in lvl.batch_rows]
                bits, wprefix, orig, out = ops.topk_select(_t(logits).reshape(-1, 1), seg, [int(keep[a:a + r].sum()) for a, r in zip(np.cumsum([0] + seg[:-1]), seg)],
                                                           parent_coords=lvl.C, parent_stride=st)
                _eq(_n(out), kc[keep], f'{w}: selected rows')
                selected = CoordMap(out, st // 2, unique=True, origin=('selected', kids, bits, wprefix, orig))
                _eq(_n(selected.k3), want_pruned, f'{w}: selected by rank bitmap (own map {own_map})')
                assert own_map or kids._k3 is None
                grand = selected.up()
                if len(out) < 3000:
                    _eq(_n(grand.k3), X.k3_map(X.children(kc[keep], st // 2), st // 4), f'{w}: children of the selected level')
            _count('coordinates', len(c))


@gpu
def test_gpu_k3_at_the_real_hash_gate():
    """32 768 rows probe the hash, 32 769 derive the map through the strided pyramid: both sides of sparse.HASH_LEVEL_MAX"""
    from pcgcv2_amd import sparse
    from pcgcv2_amd.sparse import CoordMap
    assert sparse.HASH_LEVEL_MAX == 32768
    grid = np.array([(7, x, y, z) for z in range(33) for y in range(32) for x in range(32)], np.int64)
    grid[:, 1:] += X.LIM - 40                                         # a solid block against the top border, batch 7
    for n in (32768, 32769):
        c = grid[np.random.default_rng(n).permutation(len(grid))[:n]].astype(np.int32)
        got = _n(CoordMap(_t(c), 1, unique=True).k3)
        _eq(got, orc.kmap_k3(c, 1), f'{n} rows vs oracle')
        _eq(got[:, :4000], _k3_of_first(c, 4000), f'{n} rows vs definition')
        _count('coordinates', n)


@gpu
def test_gpu_sorts_scale_and_coordinate_checks():
    from pcgcv2_amd import ops
    c, _ = X.lane_duplicates()
    sorts = [('lane_duplicates', c), ('batch_shuffled', X.batch_cloud(shuffle=True)), ('border', X.border_cloud(1)[::-1].copy())]
    rng = np.random.default_rng(13)
    many = np.concatenate([rng.integers(0, 16, (300000, 1)), rng.integers(X.LIM - 64, X.LIM, (300000, 3))], 1).astype(np.int32)
    many = many[X.in_range(many)]
    sorts.append(('300k rows in the top corner, batches 0-15, many repeats', many))
    for name, rows in sorts:
        _eq(_n(ops.sort_zyx(_t(rows))), X.sort_zyx(rows), f'{name}: sort_zyx (stable)')
        _eq(_n(ops.sort_zyx(_t(rows), batch_major=True)), X.sort_bzyx(rows), f'{name}: batch-major sort (stable)')
        _count('sorts', len(rows))
    for f in SCALE_FACTORS:
        rows = _scale_rows(f)
        got = _n(ops.coords_scale(_t(rows), f))
        _eq(got, X.scale(rows, f), f'coords_scale {f}')
        assert got[:, 1:].max() < X.LIM
        _count('scale', len(rows))
    pad = np.zeros((100000, 4), np.int32)
    pad[:, 1] = np.arange(100000)
    for name, row in X.ILLEGAL_ROWS.items():
        with pytest.raises(PcgcError, match='1 of 1 rows'):
            ops.check_coords(_t(np.array([row], np.int32)))
        with pytest.raises(PcgcError, match='1 of 100001 rows'):
            ops.check_coords(_t(np.concatenate([pad, np.array([row], np.int32)])))
        _count('coordinate checks', 100002)
    every = np.concatenate([pad] + [np.array([r], np.int32) for r in X.ILLEGAL_ROWS.values()])
    with pytest.raises(PcgcError, match=f'{len(X.ILLEGAL_ROWS)} of {len(every)} rows'):
        ops.check_coords(_t(every))
    legal = np.array([[15, X.LIM - 1, X.LIM - 1, X.LIM - 2], [15, 0, 0, 0], [0, X.LIM - 1, X.LIM - 1, X.LIM - 1]], np.int32)
    assert ops.check_coords(_t(legal)) >= 0


# ------------------------------------------------------------------------------------------------ entropy front end
@gpu
def test_gpu_entropy_front_end():
    from pcgcv2_amd import ops
    for name, x in X.entropy_cases():
        lo, hi = X.round_minmax(x)
        want = X.symbolize(x, lo)
        flat = np.concatenate([[np.float32(lo)], x.ravel()]).astype(np.float32)
        off = _t(flat)[1:].reshape(x.shape)                          # contiguous, base 4 bytes off a 16-byte boundary: the unaligned path
        assert off.data_ptr() % 16 == 4 and off.is_contiguous()
        for view, t in (('fresh', _t(x)), ('offset', off)):
            w = f'{name}/{view}'
            mm = _n(ops.round_minmax(t))
            assert mm.tobytes() == np.array([lo, hi], np.float32).tobytes(), f'{w}: round_minmax {mm} vs {(lo, hi)}'
            sym = ops.symbolize(t, lo)
            _eq(_n(sym), want, f'{w}: symbolize')
            _eq(_n(ops.desymbolize(sym, lo)), X.desymbolize(want, lo), f'{w}: desymbolize')
            glo, ghi, gsym = ops.quantize_symbols(t)
            assert (glo.tobytes(), ghi.tobytes()) == (lo.tobytes(), hi.tobytes()), f'{w}: quantize_symbols range'
            _eq(gsym, want, f'{w}: quantize_symbols')
            _count('entropy front end', x.size)
    # per-item ranges: all cases as the items of one batch (each with its own min / max)
    cases = X.entropy_cases()
    allx = np.concatenate([x for _, x in cases])
    ranges, sym = ops.quantize_symbols_segments(_t(allx), [len(x) for _, x in cases])
    off = 0
    for (name, x), (lo, hi) in zip(cases, ranges):
        assert (lo, hi) == X.round_minmax(x), f'{name}: item range'
        _eq(sym[off:off + len(x)], X.symbolize(x, lo), f'{name}: item symbols')
        off += len(x)
    _count('entropy front end', allx.size)


@gpu
def test_gpu_alphabets_round_trip_and_the_int16_guard(tmp_path):
    from pcgcv2_amd import ops
    from pcgcv2_amd.entropy_model import EntropyBottleneck
    eb = EntropyBottleneck(8).to(DEV)
    assert eb.table_mode == 'reference'
    for name in ('alphabet1', 'alphabet2', 'alphabet32767', 'constant', 'halves', 'near_2^23-0.5'):
        x = dict(X.entropy_cases())[name]
        strings, lo, hi = eb.compress(_t(x))
        assert (np.float32(lo[0]), np.float32(hi[0])) == X.round_minmax(x)
        back = eb.decompress(strings, lo, hi, x.shape, 8, device=DEV)
        _eq(_n(back), np.rint(x) + np.float32(0), f'{name}: compress / decompress')
        _count('entropy round trip', x.size)
    # the guard: from the min / max that come back with the symbols, before any table is evaluated or byte written
    for name, x in X.unsupported_latents():
        eb.invalidate()
        for call in (lambda: eb.compress(_t(x)), lambda: ops.quantize_symbols(_t(x)),
                     lambda: ops.quantize_symbols_segments(_t(np.concatenate([np.ones((8, 8), np.float32), x])), [8, len(x)])):
            with pytest.raises(PcgcError, match='range'):
                call()
        assert not eb.__dict__.get('_table_cache'), f'{name}: a table was evaluated'
        _count('entropy guard', x.size)
    x = np.zeros((40, 8), np.float32)
    x[3, 3] = 32766                                                  # 32767 symbols: the largest alphabet passes
    assert ops.quantize_symbols(_t(x))[1] == 32766


@gpu
@pytest.mark.parametrize('poison', [1e5, float('nan'), float('inf')])
def test_gpu_encode_and_encode_batch_refuse_an_uncodable_latent(poison, tmp_path):
    """a latent whose range int16 symbols cannot hold (alphabet >= 32768, NaN, infinity) stops encode and encode_batch with a PcgcError naming
    the range; no feature stream or header is written"""
    from pcgcv2_amd.coder import Coder
    from pcgcv2_amd.pcc_model import PCCModel
    from pcgcv2_amd.sparse import SparseTensor, sparse_collate
    sd = synthetic.synthetic_state_dict()
    bias = sd['encoder.conv3.bias'].clone()
    bias.view(-1)[1] = poison                                        # one latent channel far away / not finite
    sd['encoder.conv3.bias'] = bias
    model = PCCModel().to(DEV)
    model.load_state_dict(sd)
    pts = synthetic.shell('shell6')
    coords = torch.cat([torch.zeros((len(pts), 1), dtype=torch.int32), pts], 1)
    x = SparseTensor(torch.ones((len(pts), 1)), coordinates=coords, tensor_stride=1, device=DEV)
    coder = Coder(model, str(tmp_path / 'one'))
    with pytest.raises(PcgcError, match='range'):
        coder.encode(x)
    c2, f2 = sparse_collate([pts, pts + 3], [torch.ones((len(pts), 1))] * 2)
    xb = SparseTensor(f2, coordinates=c2, tensor_stride=1, device=DEV)
    with pytest.raises(PcgcError, match='range'):
        Coder(model, str(tmp_path / 'two')).encode_batch(xb, ['_a', '_b'])
    torch.cuda.synchronize()
    written = [os.path.basename(p) for p in glob.glob(str(tmp_path / '*'))]
    assert not [p for p in written if p.endswith('F.bin') or p.endswith('H.bin')], written
    _count('entropy guard', len(pts))


def _report(prefix):
    for k in sorted(REPORT):
        if k.startswith('cpu') == (prefix == 'cpu'):
            print(f'exact {k:28s} {REPORT[k][0]:6d} cases {REPORT[k][1]:12d} rows')
            assert REPORT[k][1] > 0


def test_zz_report_cpu_comparisons():
    """(prints, per family, how many cases and rows the oracle was compared on for equality)"""
    _report('cpu')


@gpu
def test_zz_report_gpu_comparisons():
    """(prints, per family, how many cases and rows were compared for equality: the record the PR body reports)"""
    _report('gpu')
