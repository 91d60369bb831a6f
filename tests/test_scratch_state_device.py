"""Every wrapper on recycled scratch and guard-banded buffers (tests/scratch_arena.py).

The other device tests ask whether the returned tensors are right.  These ask what was in the scratch and output memory BEFORE the call and
what was written AROUND it: the wrappers allocate with torch.empty and rely on native clears of exactly the parts the kernels need, and a
test process mostly receives zeroed memory, where a missing or short clear changes nothing.  In production the caching allocator hands back
the previous frame's block: descriptors, tickets, hash slots and partial sums that are legal for the shape and wrong for the data.

Protocol of a case: two sibling inputs A and B of identical shapes and different contents.  (1) warm the caches on A outside the arena;
(2) B through a fresh arena -> want; (3) A through a recording arena; (4) B through the stale replay of (3) -> got.  got must equal want
byte for byte, every guard of the three arenas must be intact, every request of (4) must have been replayed (its sequence of (bytes,
dtype) equals the recorded one), and want must equal the family's existing definition."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import eval_reference as er
import exact_reference as X
import fp64_reference as R
import lossless_reference as lr
import rans_reference as rr
import scratch_arena as SA
from oracle import pcgc_oracle as orc
from pcgcv2_amd import conventions, synthetic
from pcgcv2_amd._lib import PcgcError
from scratch_arena import Arena, ArenaError

DEV = torch.device('cuda:0')
REPORT = {}                 # family -> [cases, allocations, replayed, guard bytes, [data-dependent requests served fresh]]


def _t(a, dt=None):
    t = torch.as_tensor(np.ascontiguousarray(a), dtype=dt)
    if t.numel() == 0:
        t = torch.empty(t.shape, dtype=t.dtype)
    return t.to(DEV)


def _freeze(v):
    """tensors -> numpy copies on the host (a view is copied as the view: bytes past it are not results); containers keep their shape"""
    if torch.is_tensor(v):
        return v.detach().cpu().contiguous().numpy().copy()
    if isinstance(v, dict):
        return {k: _freeze(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_freeze(x) for x in v]
    return v


def _same(got, want, what):
    """byte equality, floats included (NaN payloads and the sign of zero too)"""
    if isinstance(want, dict):
        assert isinstance(got, dict) and got.keys() == want.keys(), what
        for k in want:
            _same(got[k], want[k], f'{what}.{k}')
    elif isinstance(want, list):
        assert isinstance(got, list) and len(got) == len(want), f'{what}: {len(got)} entries vs {len(want)}'
        for i, (g, w) in enumerate(zip(got, want)):
            _same(g, w, f'{what}[{i}]')
    elif isinstance(want, np.ndarray):
        assert isinstance(got, np.ndarray) and got.dtype == want.dtype and got.shape == want.shape, f'{what}: {got.dtype}{got.shape} vs {want.dtype}{want.shape}'
        if got.tobytes() != want.tobytes():
            bad = np.flatnonzero(np.frombuffer(got.tobytes(), np.uint8) != np.frombuffer(want.tobytes(), np.uint8))
            at = int(bad[0]) // max(got.itemsize, 1)
            raise AssertionError(f'{what}: stale scratch changed the result: {len(bad)} bytes differ, the first in element {at} of {got.size}: '
                                 f'{got.ravel()[at]!r} on recycled memory, {want.ravel()[at]!r} on fresh memory')
    elif isinstance(want, float):
        assert isinstance(got, float) and np.float64(got).tobytes() == np.float64(want).tobytes(), f'{what}: {got!r} vs {want!r}'
    else:
        assert type(got) is type(want) and got == want, f'{what}: {got!r} on recycled memory, {want!r} on fresh memory'


def _run(arena, fn, inp):
    with SA.installed(arena):
        out = fn(inp)
    torch.cuda.synchronize()
    frozen = _freeze(out)
    arena.finish()
    arena.check()
    return frozen


def protocol(family, fn, A, B, fresh_ok=(), warm=True):
    """-> want (B's result on fresh memory, frozen), after every assertion that involves the arenas"""
    if warm:
        fn(A)
        torch.cuda.synchronize()
    fresh, rec = Arena(), Arena()
    want = _run(fresh, fn, B)
    _run(rec, fn, A)
    stale = rec.replay(fresh_ok)
    got = _run(stale, fn, B)
    for a in (fresh, rec, stale):
        a.check()
    _same(got, want, family)
    allocs, replayed, guarded = stale.stats()
    assert allocs > 0, f'{family}: the case allocated nothing through the arena'
    assert replayed + len(stale.served_fresh) == allocs and all(c in fresh_ok for _, c, _, _ in stale.served_fresh)
    rec_ = REPORT.setdefault(family, [0, 0, 0, 0, []])
    rec_[0] += 1; rec_[1] += allocs; rec_[2] += replayed; rec_[3] += guarded
    rec_[4] += [f'{c}() request {i}: {a[0]} bytes (recorded {None if r is None else r[0]})' for i, c, a, r in stale.served_fresh]
    return want


def _eq(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f'{what}: shape {got.shape} vs {want.shape}'
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f'{what}: {len(bad)} of {got.size} entries differ from the definition, first at {tuple(bad[0])}: got {got[tuple(bad[0])]}, '
                             f'want {want[tuple(bad[0])]}')


def _sibling(c4, cell, seed):
    """the same shape elsewhere: translated by multiples of `cell` (every strided level up to that cell size keeps its row count), rows permuted"""
    rng = np.random.default_rng(seed)
    out = np.asarray(c4, np.int64).copy()
    out[:, 1:] += cell * rng.integers(1, 40, 3)
    assert X.in_range(out).all()
    return out[rng.permutation(len(out))].astype(np.int32)


@pytest.fixture
def conventions_reset():
    yield
    conventions.reset()
    orc.CONVENTIONS.update(kernel_offset_order='xyz', topk_tie='low', dedup_keep='first')


@pytest.fixture
def ops():
    """the dispatch record and the forced families come back after each test"""
    from pcgcv2_amd import ops
    keep = ops.PATH
    yield ops
    ops.configure(keep)
    ops.set_conv_impl(-1)
    ops.set_up2_impl(2)
    ops.set_rows_q4_variant(0)


# ================================================================================================ teeth: no project kernel
def _sum_into_dirty_scratch(x):
    """a reduction that adds into its scratch without clearing it (through the patched name, as a product module would)"""
    from pcgcv2_amd import ops
    px = ops.torch
    acc = px.empty(4, dtype=torch.float32, device=x.device)
    acc += x.reshape(-1, 4).sum(0)
    return acc


def _writes_row_n(x):
    from pcgcv2_amd import ops
    n = x.shape[0]
    out = ops.torch.empty((n, 4), dtype=torch.float32, device=x.device)
    out.as_strided((n + 1, 4), (4, 1)).copy_(torch.cat([x, x[:1]]))      # row n of `out`: the first 16 bytes of the arena's own guard
    return out


def test_teeth_a_missing_clear_shows_as_a_different_result():
    A, B = _t(np.arange(32, dtype=np.float32)), _t(np.arange(32, dtype=np.float32)[::-1] * 3)
    with pytest.raises(AssertionError, match='stale scratch changed the result'):
        protocol('teeth', _sum_into_dirty_scratch, A, B, warm=False)
    REPORT.pop('teeth', None)


def test_teeth_a_write_of_row_n_damages_the_guard():
    x = _t(np.ones((9, 4), np.float32))
    arena = Arena()
    with SA.installed(arena):
        out = _writes_row_n(x)
    assert torch.equal(out, x)
    with pytest.raises(ArenaError, match=r'allocation 0 \(144 bytes of torch.float32.*after the payload: .*first at offset 0 from'):
        arena.check()


# ================================================================================================ scan, compaction, gathers
SCAN_TILE = 2048


def _scan_fn(ops):
    def fn(i):
        prefix, total = ops.mask_scan(i['m'])
        orig = ops.compact_index(i['m'], prefix, i['kept'])
        return dict(prefix=prefix, total=total, orig=orig, coords=ops.compact_coords(i['c'], i['m'], prefix, i['kept']),
                    feats=ops.compact_feats(i['f'], i['m'], prefix, i['kept']), rows=ops.gather_rows(i['f'], orig),
                    gcoords=ops.gather_coords(i['c'], i['perm']), gfeats=ops.gather_feats(i['f'], i['perm']),
                    select=list(ops.topk_select(i['z'], [i['m'].shape[0]], [i['kept']], coords=i['c'])))     # (its own descriptors and ticket)
    return fn


def _scan_input(n, seed, roll):
    rng = np.random.default_rng(seed)
    base = np.random.default_rng(1).random(n) < 0.4
    base[0], base[-1] = True, False                                   # (n = 3 keeps a survivor)
    mask = np.roll(base, roll)                                        # rolled: the population is the same in A and B
    host = dict(m=mask.astype(np.uint8), c=np.concatenate([rng.integers(0, 16, (n, 1)), rng.integers(0, X.LIM, (n, 3))], 1).astype(np.int32),
                f=rng.standard_normal((n, 8)).astype(np.float32), perm=rng.permutation(n).astype(np.int32))
    dev = {k: _t(v) for k, v in host.items()}
    dev['kept'] = int(mask.sum())
    dev['z'] = _t(np.where(mask, 1.0, -1.0).astype(np.float32)).reshape(-1, 1)
    return host, dev


@pytest.mark.parametrize('tiles', [1, 2, 65])
def test_scan_compaction_and_gathers(tiles, ops):
    """one tile, two, and one tile past the 64-descriptor look-back window, + 3 rows"""
    n = (tiles - 1) * SCAN_TILE + 3
    assert -(-n // SCAN_TILE) == tiles
    _, A = _scan_input(n, 10, 0)
    h, B = _scan_input(n, 11, 1)
    assert A['kept'] == B['kept']
    want = protocol('scan / compaction / gathers', _scan_fn(ops), A, B)
    m = h['m'].astype(bool)
    _eq(want['prefix'], np.cumsum(m) - m, 'mask_scan'); _eq(want['total'], [m.sum()], 'total')
    _eq(want['orig'], np.flatnonzero(m), 'compact_index'); _eq(want['coords'], h['c'][m], 'compact_coords')
    _eq(want['feats'], h['f'][m], 'compact_feats'); _eq(want['rows'], h['f'][m], 'gather_rows')
    _eq(want['gcoords'], h['c'][h['perm']], 'gather_coords'); _eq(want['gfeats'], h['f'][h['perm']], 'gather_feats')
    for name, g, w in zip(('bits', 'wprefix', 'orig', 'coords'), want['select'], X.select_outputs(m, h['c'])):
        _eq(g, w, f'topk_select {name}')


# ================================================================================================ top-k
def _set_tie(tie):
    conventions.set_convention('topk_tie', tie)
    orc.CONVENTIONS['topk_tie'] = tie


def _topk_input(rows, seed):
    n = sum(rows)
    rng = np.random.default_rng(seed)
    v = (np.round(rng.standard_normal(n) * 3) / 2).astype(np.float32)          # heavy ties, some at the threshold
    v[rng.random(n) < 0.05] = -0.0
    c4 = np.concatenate([np.repeat(np.arange(len(rows)), rows)[:, None], rng.integers(0, X.LIM, (n, 3))], 1).astype(np.int32)
    return (v, c4), dict(v=_t(v).reshape(-1, 1), c=_t(c4))


@pytest.mark.parametrize('tie', ['low', 'high'])
@pytest.mark.parametrize('rows, ks', [([4097], [2049]), ([2049], [2048]), ([1301, 703, 2093], [650, 700, 699])], ids=['4097_2049', '2049_2048', '3_segments'])
def test_topk_mask_and_select(rows, ks, tie, ops, conventions_reset):
    """(n, k) around the 2048-row tile and the 4096-row pair; three segments whose ends lie inside a thread's 8 rows; both tie rules"""
    assert len(rows) == 1 or all(np.cumsum(rows)[:-1] % 8)
    _set_tie(tie)

    def fn(i):
        out = dict(seg=ops.topk_mask_segments(i['v'], rows, ks), sel=list(ops.topk_select(i['v'], rows, ks, coords=i['c'])))
        if len(rows) == 1:
            out['mask'] = ops.topk_mask(i['v'], ks[0])
        return out
    _, A = _topk_input(rows, 20)
    (v, c4), B = _topk_input(rows, 21)
    want = protocol(f'top-k ({tie})', fn, A, B)
    mask = X.topk_mask_segments(v, rows, ks, tie)
    _eq(want['seg'].astype(bool), mask, 'topk_mask_segments')
    if len(rows) == 1:
        _eq(want['mask'].astype(bool), mask, 'topk_mask')
    for name, g, w in zip(('bits', 'wprefix', 'orig', 'coords'), want['sel'], X.select_outputs(mask, c4)):
        _eq(g, w, f'topk_select {name}')


# ================================================================================================ sorts
def test_sorts_and_batch_counts(ops):
    n = 4097

    def make(seed):
        rng = np.random.default_rng(seed)
        c = np.concatenate([rng.integers(0, 3, (n, 1)), rng.integers(0, 24, (n, 3)) + 1000 * seed], 1).astype(np.int32)       # repeats: stability shows
        return c, _t(c)
    fn = lambda c: dict(zyx=ops.sort_zyx(c), bzyx=ops.sort_zyx(c, batch_major=True), counts=ops.batch_counts(c))
    _, A = make(30)
    c, B = make(31)
    want = protocol('sorts', fn, A, B)
    _eq(want['zyx'], X.sort_zyx(c), 'sort_zyx'); _eq(want['bzyx'], X.sort_bzyx(c), 'sort_bzyx')
    assert want['counts'] == np.bincount(c[:, 0], minlength=3).tolist()


# ================================================================================================ hash, pyramid, kernel maps
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def _table_contents(table):
    """what of a table is defined: WHICH slots are occupied and WHICH keys are stored.  Which of two colliding keys got the earlier slot of a
    probe chain is decided by the order the lanes' compare-and-swaps arrive in, on fresh memory as on recycled: not compared."""
    keys = table.keys.cpu().numpy().view(np.uint64)
    return dict(slots=np.flatnonzero(keys != EMPTY), keys=np.sort(keys[keys != EMPTY]))


def _coords_fn(ops):
    def fn(i):
        c = i['c']
        table = ops.HashTable(c, 1)
        keep, first = ops.first_occurrence_mask(c, table, want_rows=True)
        k3 = ops.kmap_k3(c, 1, table)
        out = dict(table=_table_contents(table), keep=keep, first=first, k3=k3, found=ops.hash_contains(i['other'], table),
                   found_or=ops.hash_contains(i['other'], table, or_mask=i['or']), none=ops.hash_contains(i['other'], None))
        coarse, parent_of, down = ops.down_level(c, 1)
        out['down_level'] = [coarse, parent_of, down]
        out['pyramid1'] = [list(l) for l in ops.pyramid(c, 1, 1)]
        pyr = ops.pyramid(c, 1, 3)
        out['pyramid3'] = [list(l) for l in pyr]
        # the down maps from a dedup of the quantised rows done step by step
        q = ops.coords_quantize(c, 2)
        tq = ops.HashTable(q, 2)
        keep_q, first_q = ops.first_occurrence_mask(q, tq, want_rows=True)
        prefix_q, _ = ops.mask_scan(keep_q)
        out['down_maps'] = list(ops.down_maps(c, first_q, prefix_q, 1, coarse.shape[0]))
        t2 = ops.HashTable(coarse, 2)
        k3_2 = ops.kmap_k3(coarse, 2, t2)
        out['from_coarse'] = ops.kmap_k3_from_coarse(c, 1, parent_of, k3_2, down)
        # the stride-8 level, its children, and the children pruned four ways
        c8 = pyr[2][0].contiguous()
        t8, nbr8, kids, nbr_kids = ops.level_prepare_children(c8, 8)
        out['prepare'] = [_table_contents(t8), nbr8, kids, nbr_kids]
        out['children_map'] = ops.kmap_k3_children(nbr8)
        out['children'] = ops.coords_children(c8, 8)
        m = i['keep'](kids.shape[0])
        prefix, _ = ops.mask_scan(m)
        kept = i['kept'](kids.shape[0])
        orig = ops.compact_index(m, prefix, kept)
        out['prune'] = ops.kmap_k3_prune(nbr_kids, m, prefix, orig)
        out['prune_parent'] = ops.kmap_k3_prune_parent(nbr8, m, prefix, orig)
        logits = (m.to(torch.float32) * 2 - 1).reshape(-1, 1)
        bits, wprefix, orig2, sel = ops.topk_select(logits, [kids.shape[0]], [kept], parent_coords=c8, parent_stride=8)
        out['select'] = [bits, wprefix, orig2, sel]
        out['prune_sel'] = ops.kmap_k3_prune_sel(nbr_kids, bits, wprefix, orig2)
        out['prune_parent_sel'] = ops.kmap_k3_prune_parent_sel(nbr8, bits, wprefix, orig2)
        return out
    return fn


def _keep_mask(n_kids):
    return np.random.default_rng(n_kids).random(n_kids) < 0.45


@pytest.mark.parametrize('cloud', ['noisy_s', 'shell6'])
def test_hash_pyramid_and_kernel_maps(cloud, ops):
    pts = (synthetic.cloud(cloud) if cloud == 'noisy_s' else synthetic.shell(cloud)).numpy()[:6000]
    base = np.concatenate([np.zeros((len(pts), 1), np.int64), pts], 1)
    assert len(np.unique(base, axis=0)) == len(base)

    def make(c, seed):
        rng = np.random.default_rng(seed)
        other = c.copy()
        other[::3, 1] += 1                                             # a third of the rows moved by a voxel: some present, some absent
        orm = (rng.random(len(c)) < 0.2).astype(np.uint8)
        return dict(c=_t(c, torch.int32), other=_t(other, torch.int32), **{'or': _t(orm)}, keep=lambda nk: _t(_keep_mask(nk).astype(np.uint8)),
                    kept=lambda nk: int(_keep_mask(nk).sum())), other, orm
    A, _, _ = make(_sibling(base, 8, 40), 40)
    c = _sibling(base, 8, 41)
    B, other, orm = make(c, 41)
    want = protocol('hash / pyramid / kernel maps', _coords_fn(ops), A, B)
    n = len(c)
    keys = X.coord_key(c)
    _eq(want['table']['slots'], sorted(X.occupied_slots(keys, X.hash_capacity(n))), 'occupied slots'); _eq(want['table']['keys'], np.unique(keys), 'keys')
    _eq(want['keep'], np.ones(n, np.uint8), 'first-occurrence mask (distinct rows)'); _eq(want['first'], np.arange(n), 'first rows')
    k3 = X.k3_map(c, 1)
    _eq(want['k3'], k3, 'kmap_k3'); _eq(want['from_coarse'], k3, 'kmap_k3_from_coarse')
    present = np.isin(X.coord_key(other), keys)
    _eq(want['found'], present, 'hash_contains'); _eq(want['found_or'], present | (orm != 0), 'hash_contains | mask'); _eq(want['none'], np.zeros(n), 'empty set')
    levels = X.pyramid(c, 1, 3)
    for name, got in (('down_level', [want['down_level']]), ('pyramid(1)', want['pyramid1']), ('pyramid(3)', want['pyramid3'])):
        for l, (g, w) in enumerate(zip(got, levels)):
            for part, gg, ww in zip(('rows', 'parent_of', 'down'), g, w):
                _eq(gg, ww, f'{name} level {l} {part}')
    _eq(want['down_maps'][0], levels[0][1], 'down_maps parent_of'); _eq(want['down_maps'][1], levels[0][2], 'down_maps down')
    c8 = levels[2][0]
    kids = X.children(c8, 8)
    kmap = X.k3_map(kids, 4)
    _eq(want['prepare'][1], X.k3_map(c8, 8), 'level_prepare_children: k3'); _eq(want['prepare'][2], kids, 'level_prepare_children: children')
    _eq(want['prepare'][3], kmap, 'level_prepare_children: children k3'); _eq(want['children_map'], kmap, 'kmap_k3_children')
    _eq(want['children'], kids, 'coords_children')
    _eq(want['prepare'][0]['keys'], np.unique(X.coord_key(c8)), 'level_prepare_children: table keys')
    keep = _keep_mask(len(kids))
    pruned = X.prune_map(kmap, keep)
    for k in ('prune', 'prune_parent', 'prune_sel', 'prune_parent_sel'):
        _eq(want[k], pruned, k)
    for name, g, w in zip(('bits', 'wprefix', 'orig', 'coords'), want['select'], X.select_outputs(keep, kids)):
        _eq(g, w, f'topk_select from parents: {name}')


def test_scan_and_pyramid_after_a_fuller_run(ops):
    """the same row count, other populations: the recorded run keeps every row / spreads over many cells, the replayed one keeps few / fills
    few cells.  The scan, hash and upper-bound output buffers have the sizes they had, and hold more state than this run writes over"""
    n = 64 * SCAN_TILE + 3
    sparse = (np.arange(n) % 97 == 5).astype(np.uint8)
    want = protocol('scan / compaction / gathers', lambda m: list(ops.mask_scan(m)), _t(np.ones(n, np.uint8)), _t(sparse))
    _eq(want[0], np.cumsum(sparse) - sparse, 'mask_scan after an all-kept run'); _eq(want[1], [sparse.sum()], 'total')
    m = 6000
    spread = np.concatenate([np.zeros((m, 1), np.int64), synthetic.cloud('noisy_s').numpy()[:m]], 1).astype(np.int32)
    i = np.arange(m)
    solid = np.stack([i * 0, 200 + i % 20, 300 + i // 20 % 20, 400 + i // 400], 1).astype(np.int32)[np.random.default_rng(3).permutation(m)]
    fn = lambda c: dict(down_level=list(ops.down_level(c, 1)), pyramid=[list(l) for l in ops.pyramid(c, 1, 3)])
    want = protocol('hash / pyramid / kernel maps', fn, _t(spread), _t(solid))
    levels = X.pyramid(solid, 1, 3)
    assert len(levels[0][0]) < len(X.pyramid(spread, 1, 1)[0][0]) // 2
    for name, got in (('down_level', [want['down_level']]), ('pyramid(3)', want['pyramid'])):
        for l, (g, w) in enumerate(zip(got, levels)):
            for part, gg, ww in zip(('rows', 'parent_of', 'down'), g, w):
                _eq(gg, ww, f'{name} after a wider cloud: level {l} {part}')


# ================================================================================================ entropy front end
def test_entropy_front_end(ops, golden_dir):
    n, C, seg = 4099, 8, [1301, 707, 2091]
    params_np = np.load(os.path.join(golden_dir, 'eval_loss.npz'))['b3_params'].astype(np.float32)
    params = _t(params_np)

    def make(seed):
        x = (np.random.default_rng(seed).standard_normal((n, C)) * 3).astype(np.float32)
        x[seed % n] = 11.5                                             # (the same symbol range in A and B: the CDF table has one shape)
        x[(seed * 7) % n] = -12.5
        return x, _t(x)

    def fn(x):
        lo, hi, sym = ops.quantize_symbols(x)
        ranges, seg_sym = ops.quantize_symbols_segments(x, seg)
        s = ops.symbolize(x, lo)
        return dict(lo=float(lo), hi=float(hi), sym=sym, ranges=[[float(a), float(b)] for a, b in ranges], seg_sym=seg_sym, mm=ops.round_minmax(x),
                    symbolize=s, desymbolize=ops.desymbolize(s, lo), cdf=list(ops.cdf_table(params, C, -12.0, 12.0)))
    _, A = make(50)
    x, B = make(51)
    want = protocol('entropy front end', fn, A, B)
    lo, hi = X.round_minmax(x)
    assert (want['lo'], want['hi']) == (float(lo), float(hi)) and want['mm'].tobytes() == np.array([lo, hi], np.float32).tobytes()
    _eq(want['sym'], X.symbolize(x, lo), 'quantize_symbols'); _eq(want['symbolize'], X.symbolize(x, lo), 'symbolize')
    _eq(want['desymbolize'], X.desymbolize(X.symbolize(x, lo), lo), 'desymbolize')
    off = 0
    for r, (a, b) in zip(seg, want['ranges']):
        assert (a, b) == tuple(float(v) for v in X.round_minmax(x[off:off + r]))
        _eq(want['seg_sym'][off:off + r], X.symbolize(x[off:off + r], np.float32(a)), 'item symbols')
        off += r
    q, f = want['cdf']
    assert q.shape == (C, 26)
    _eq(f, orc.cdf_float(params_np, -12.0, 12.0), 'cdf_table (fp32) vs the oracle')


# ================================================================================================ loss reductions
LOSS_E = 2.0                                    # tests/test_loss_reductions_device.py: twice the largest measured term deviation, in ulp
LN2 = float(np.log(2.0))


@pytest.mark.parametrize('n', [1023, 1025])
def test_bce_sum_and_counts(n, ops):
    """either side of the 1024-row block of the BCE pass (er.BCE_SIZES)"""
    assert n in er.BCE_SIZES and abs(n - er.BCE_BLOCK_ROWS) == 1
    x, t, p = er.bce_case(n)
    rng = np.random.default_rng(n)
    truth = np.unique(np.concatenate([rng.integers(0, 16, (n, 1)), rng.integers(0, 12, (n, 3))], 1).astype(np.int32), axis=0)
    table = ops.HashTable(_t(truth), 1)                               # (data_utils.isin on the device: the loss's ground-truth masks)
    qa, qb = (np.concatenate([r.integers(0, 16, (n, 1)), r.integers(0, 12, (n, 3))], 1).astype(np.int32) for r in (np.random.default_rng(n + 1), rng))
    fn = lambda i: list(ops.bce_logits(*i[:3])) + list(ops.bce_logits(None, i[1], i[2])) + [ops.hash_contains(i[3], table), ops.hash_contains(i[3], table, or_mask=i[2])]
    A = (_t(np.roll(x, 5)), _t(np.roll(t, 9)), _t(np.roll(p, 3)), _t(qa))
    want = protocol('loss reductions', fn, A, (_t(x), _t(t), _t(p), _t(qb)))
    found = np.isin(X.coord_key(qb), X.coord_key(truth))
    assert found.any() and not found.all()
    _eq(want[4], found, 'hash_contains'); _eq(want[5], found | (p != 0), 'hash_contains | mask')
    terms = er.bce_terms(x, t)
    assert abs(float(want[0][0]) - er.exact_sum(terms) / LN2) <= er.sum_bound(terms, LOSS_E) / LN2
    assert tuple(want[1].tolist()) == er.counts(p, t) == tuple(want[3].tolist())


@pytest.mark.parametrize('n', [31, 33, 1023, 1025])
def test_likelihood_and_bits(n, ops, golden_dir):
    """C = 8: 248 and 264 elements, either side of the 256-element block of the likelihood and -log2 passes (er.LIK_ROWS_C8), and the row
    counts of the BCE cases (32 blocks and a ragged 33rd)"""
    assert (n in er.LIK_ROWS_C8 and abs(8 * n - er.LIK_BLOCK) == 8) or n in er.BCE_SIZES
    params = np.load(os.path.join(golden_dir, 'eval_loss.npz'))['b3_params']
    y = er.latent_case(n, 8)
    pd = _t(params.astype(np.float32))

    def fn(yd):
        lik, bits = ops.eb_likelihood(yd, pd, bound=1e-9, want_likelihood=True, want_bits=True)
        return dict(lik=lik, bits=bits, fused=ops.eb_likelihood(yd, pd, bound=1e-9, want_likelihood=False, want_bits=True)[1], stored=ops.neg_log2_sum(lik))
    want = protocol('loss reductions', fn, _t(y[::-1].copy()), _t(y))
    lik64 = er.likelihood(params, y)
    assert float(np.max(np.abs(want['lik'].astype(np.float64) - lik64) / lik64)) <= 2.0 ** -23
    terms = -np.log2(want['lik'].astype(np.float64))
    assert abs(float(want['bits'][0]) - er.exact_sum(terms)) <= er.sum_bound(terms, LOSS_E)
    assert want['bits'].tobytes() == want['fused'].tobytes() == want['stored'].tobytes()


# ================================================================================================ occupancy symbols and the device rANS coder
def _packed(ctx, bit=None):
    w = np.asarray(ctx, dtype=np.int64) << 1
    if bit is not None:
        w = w | np.asarray(bit, dtype=np.int64)
    return torch.from_numpy(w.astype(np.int16)).to(DEV)


def _rans_cases():
    out = []
    for S, n in ((4, 64 * 4 * 2 + 1), (1, 65)):
        out.append((f'S{S} cyclic', S, rr.cyclic(n, seed=1), rr.cyclic(n, seed=2)))
        out.append((f'S{S} model-drawn', S, rr.model_drawn(n, seed=1), rr.model_drawn(n, seed=2)))
    n = 64 * 4 * 2 + 1
    # the extreme contexts of test_occ_rans_device.py: A leaves the fullest state behind (16 bits a row), B needs the emptiest
    out.append(('S4 improbable then probable', 4, rr.extreme(n, True), rr.extreme(n, False)))
    out.append(('S4 probable then improbable', 4, rr.extreme(n, False), rr.extreme(n, True)))
    out.append(('S4 only lane 63', 4, rr.extreme(n, False, lanes=range(0, 64, 2)), rr.extreme(n, False, lanes=(63,))))
    return out


@pytest.mark.parametrize('name, S, a, b', _rans_cases(), ids=[c[0].replace(' ', '_') for c in _rans_cases()])
def test_occ_rans_encode_and_decode(name, S, a, b, ops):
    """the payload has exactly its capacity of 8 + 516 K + 4 n bytes (+ up to 7 to the int64 it is allocated in) between its guards, the
    decoder's workspace exactly what the library answers for K chunks and no rows"""
    def fn(i):
        ctx, bit = i
        payload = ops.occ_rans_encode(_packed(ctx, bit), S)
        mask, occupied = ops.occ_rans_decode(_packed(ctx), rr.encode(ctx, bit, S), len(ctx))
        return dict(payload=payload, mask=mask, occupied=occupied)
    want = protocol('occupancy rANS', fn, a, b)
    ctx, bit = b
    assert want['payload'] == rr.encode(ctx, bit, S)
    _eq(want['mask'], bit, 'decoded bits')
    assert want['occupied'] == int(np.sum(bit)) and np.array_equal(rr.decode(ctx, want['payload']), bit)


def test_occ_symbols(ops):
    z, q = lr.special_logits()
    zb = np.concatenate([z, lr.random_logits(1025, 7)[0]]).astype(np.float32)
    za = np.concatenate([z[::-1], lr.random_logits(1025, 8)[0]]).astype(np.float32)
    ta, tb = (np.arange(len(za)) % 3 == 0).astype(np.uint8), (np.arange(len(zb)) % 5 < 2).astype(np.uint8)

    def fn(i):
        packed, sums = ops.occ_symbols(i[0], i[1])
        payload, occupied, cost = ops.occ_rans_encode(packed, 4, sums)
        return dict(packed=packed, sums=sums, contexts=ops.occ_symbols(i[0])[0], payload=payload, occupied=occupied, cost=cost)
    want = protocol('occupancy rANS', fn, (_t(za), _t(ta)), (_t(zb), _t(tb)))
    words = lr.occ_symbols(zb, tb)
    ctx = np.asarray(words[0] if isinstance(words, tuple) else words).astype(np.int64) >> 1
    _eq(want['packed'].view(np.uint16), (ctx << 1) | tb, 'packed words'); _eq(want['contexts'].view(np.uint16), ctx << 1, 'contexts')
    assert want['payload'] == rr.encode(ctx, tb, 4) and want['occupied'] == int(tb.sum()) == int(want['sums'][0])
    assert want['cost'] == round(rr.ideal_bits(ctx, tb) * 65536) == int(want['sums'][1])


# ================================================================================================ the coders end to end
def _model():
    from pcgcv2_amd.pcc_model import PCCModel
    model = PCCModel().to(DEV)
    model.load_state_dict(synthetic.synthetic_state_dict())
    return model


def _cloud_tensor(c4):
    from pcgcv2_amd.sparse import SparseTensor
    return SparseTensor(torch.ones((len(c4), 1)), coordinates=torch.from_numpy(np.ascontiguousarray(c4, dtype=np.int32)), tensor_stride=1, device=DEV)


def _shell7_pair():
    pts = synthetic.shell('shell7').numpy()
    a = np.concatenate([np.zeros((len(pts), 1), np.int64), pts], 1).astype(np.int32)
    b = a.copy()
    b[:, 1:] += np.array([16, 40, 8], np.int32)                         # a translate by multiples of 8: every level keeps its row count
    return a, b


def _rows_sorted(c):
    return c[np.lexsort(c.T[::-1])]


def test_coder_encode_and_decode(tmp_path):
    from pcgcv2_amd.coder import Coder, STREAMS
    model = _model()
    a, b = _shell7_pair()

    def fn(c4):
        coder = Coder(model, str(tmp_path / 'c'))
        coder.encode(_cloud_tensor(c4))
        out = coder.decode()
        torch.cuda.synchronize()
        return dict(files={s: open(str(tmp_path / 'c') + s, 'rb').read() for s in STREAMS}, decoded=out.C)
    want = protocol('Coder', fn, a, b)
    sd = synthetic.state_dict_to_numpy(synthetic.synthetic_state_dict())
    ref = orc.encode(sd, b)
    for k in ('F', 'H', 'num_points'):
        assert want['files'][f'_{k}.bin'] == ref[k], f'{k}.bin differs from the oracle'
    _eq(want['decoded'], orc.decode(sd, ref['coords8'], ref['F'], ref['H'], ref['num_points']), 'decoded cloud vs the oracle')


def test_lossless_coder_device_mode(tmp_path):
    from pcgcv2_amd import lossless
    from pcgcv2_amd.coder import STREAMS
    model = _model()
    a, b = _shell7_pair()

    def fn(c4):
        coder = lossless.LosslessCoder(model, str(tmp_path / 'l'), occupancy_coder='device', chunk_steps=16)
        coder.encode(_cloud_tensor(c4))
        out = coder.decode()
        torch.cuda.synchronize()
        return dict(files={s: open(str(tmp_path / 'l') + s, 'rb').read() for s in STREAMS + (lossless.SUFFIX,)}, decoded=out.C)
    want = protocol('LosslessCoder (device)', fn, a, b)
    ref = orc.encode(synthetic.state_dict_to_numpy(synthetic.synthetic_state_dict()), b)
    for k in ('F', 'H', 'num_points'):
        assert want['files'][f'_{k}.bin'] == ref[k], f'{k}.bin differs from the oracle'
    _eq(_rows_sorted(want['decoded']), _rows_sorted(b), 'lossless: the decoded voxel set is the input set')


# ================================================================================================ convolutions: gather, unit, rows, packed, down, up
import test_fp64_definition as F64              # (its inputs, channel shapes and family tables; nothing of it is collected from here)

CONV_ROWS = (1, 17, 129, 1025)
UP_PARENTS = (1, 3, 129)


_CLOUDS = {}


def _shell9(coarse=False):
    if not _CLOUDS:
        _CLOUDS[False] = F64._shell4('shell9')
        _CLOUDS[True] = R.down_coords(_CLOUDS[False], 1)
    return _CLOUDS[coarse]


def _level(n, seed):
    """n rows of a shell, translated and permuted by `seed`: sibling levels of one shape"""
    return _sibling(_shell9()[:n], 8, seed).astype(np.int64)


def _down_pair(n, seed):
    """a stride-1 level whose stride-2 level has exactly n rows -> (fine rows, down map [8, n])"""
    rng = np.random.default_rng(seed)
    pc = _sibling(_shell9(coarse=True)[:n], 16, seed).astype(np.int64)
    pick = np.random.default_rng(n)                                    # (the same pattern for every seed: siblings have the same fine row count)
    keep = pick.random((n, 8)) < 0.5
    keep[np.arange(n), pick.integers(0, 8, n)] = True                  # every parent keeps a child
    fine = R.children_coords(pc, 2)[keep.ravel()]
    fine = fine[rng.permutation(len(fine))]
    down = R.neighbour_map(R.down_coords(fine, 1), fine, R.offsets(2))
    assert down.shape == (8, n)
    return fine, down


CONV_FAMILIES = {
    # family: (K, Cin, Cout, gather impl or None)
    'gather valu': (27, 16, 16, 0), 'gather mfma': (27, 16, 16, 2), 'gather row_split': (27, 16, 16, 6), 'gather k1': (1, 64, 16, 0),
    'unit': (27, 1, 16, None), 'rows_conv': (27, 32, 32, None), 'packed64': (27, 64, 64, None), 'rows_down': (8, 32, 64, None),
}


@pytest.mark.parametrize('family', list(CONV_FAMILIES))
def test_conv_families(family, ops):
    """rows 1, 17, 129, 1025: below one tile of every kernel, one row past 16 and 128, one past 1024.  Outputs are torch.empty: a row the
    kernel did not write holds zero on fresh memory (not the bias) and the previous level's row on recycled memory; every fifth output row
    has no present neighbour, so a kernel that skips absent work still has to store the bias there"""
    K, cin, cout, impl = CONV_FAMILIES[family]
    rng = np.random.default_rng(len(family))
    W, b = F64._rand_w(rng, K, cin, cout)
    Wt, bt = _t(W[0] if K == 1 else W), _t(b)
    table = ops.child_conv_table(_t(W)) if family in ('rows_conv', 'packed64', 'rows_down') else None
    if impl is not None:
        ops.set_conv_impl(impl)
    for n in CONV_ROWS:
        def make(seed):
            if K == 8:
                c4, nbr = _down_pair(n, seed)
            else:
                c4 = _level(n, seed)
                nbr = R.k3_map(c4, 1) if K == 27 else np.arange(len(c4))[None]
            if K > 1:
                nbr = nbr.copy()
                nbr[:, (seed + 3) % 5::5] = -1                         # every fifth output row has no present neighbour at all: out = bias
            x = np.ones((len(c4), 1), np.float32) if family == 'unit' else F64._features(rng, len(c4), cin)
            return (nbr, x), (_t(nbr, torch.int32), F64._poisoned(x))

        def fn(i):
            nbr, x = i
            if family == 'unit':
                return ops.conv_gather_unit(nbr, Wt, bt)
            if family == 'rows_conv':
                return ops.conv_rows(nbr, x, table, bt, cout)
            if family == 'packed64':
                return ops.conv_packed64(nbr, x, table, bt)
            if family == 'rows_down':
                return ops.conv_down_rows(nbr, x, table, bt, cout)
            return ops.conv_gather(nbr, x, Wt, bt)
        _, A = make(100 + n)
        (nbr, x), B = make(200 + n)
        want = protocol(f'conv: {family}', fn, A, B)
        _eq(want, orc.conv_gather(nbr.astype(np.int32), x, W, b), f'{family}, {n} rows vs the oracle')
        if impl is not None and K == 27:
            assert ops.lib().pcgc_last_conv_impl() == impl, (family, n)


@pytest.mark.parametrize('impl', [0, 1, 2], ids=['valu', 'mfma', 'mfma_lds_table'])
def test_conv_up2(impl, ops):
    rng = np.random.default_rng(impl)
    cin, cout = 64, 32
    W, b = F64._rand_w(rng, 8, cin, cout)
    Wt, bt = _t(W), _t(b)
    ops.set_up2_impl(impl)
    for n in UP_PARENTS:
        xa, xb = F64._features(rng, n, cin), F64._features(rng, n, cin)
        rows = rng.permutation(n + 5)[:n].astype(np.int32)
        wide = F64._features(rng, n + 5, cin)
        fn = lambda i: dict(plain=ops.conv_up2(i[0], Wt, bt), rows=ops.conv_up2(i[1], Wt, bt, rows=i[2]))
        A = (F64._poisoned(xa), _t(wide[::-1].copy()), _t(np.sort(rows)))
        want = protocol(f'conv_up2 impl {impl}', fn, A, (F64._poisoned(xb), _t(wide), _t(rows)))
        _eq(want['plain'], orc.conv_up2(xb, W, b), f'conv_up2, {n} parents vs the oracle')
        _eq(want['rows'], orc.conv_up2(wide[rows], W, b), f'conv_up2 through rows, {n} parents vs the oracle')


# ================================================================================================ fused InceptionResNet blocks, children-level kernels
IRN_ROWS = (17, 129, 1025)
CHILD_PARENTS = (3, 129)


@pytest.mark.parametrize('family', list(F64.IRN_FAMILIES))
def test_inception_resnet_families(family, ops):
    from pcgcv2_amd import dispatch
    from pcgcv2_amd.sparse import CoordMap, SparseTensor
    C, changes, _, variant = F64.IRN_FAMILIES[family]
    rng = np.random.default_rng(C + variant)
    blk, sd = F64._block(rng, C)
    ops.configure(**changes)
    ops.set_rows_q4_variant(variant)
    fam = family.split(' ')[0]
    for n in IRN_ROWS:
        assert dispatch.select('irn', (C,), n).family == fam
        def make(seed):
            c4, x = _level(n, seed), F64._features(rng, n, C)
            return (c4, x), (_t(c4, torch.int32), _t(x))

        def fn(i):
            with torch.no_grad():                                     # the level's own map is built here too: hash, probes, scratch and all
                return blk(SparseTensor(i[1], coordinate_map=CoordMap(i[0], 1, unique=True))).F
        _, A = make(300 + n)
        (c4, x), B = make(400 + n)
        want = protocol(f'irn: {family}', fn, A, B)
        _eq(want, orc.inception_resnet(sd, 'b', orc.Level(c4.astype(np.int32), 1), x), f'irn {family}, {n} rows vs the oracle')


@pytest.mark.parametrize('family', F64.CHILD_FAMILIES)
def test_children_families(family, ops):
    from pcgcv2_amd.sparse import CoordMap
    rng = np.random.default_rng(len(family))
    C = int(family.split(' ')[-1]) if family[-1].isdigit() else 16
    irn = 'irn' in family
    if irn:
        blk, sd = F64._block(rng, C)
        params = [p for m in (blk.conv0_0, blk.conv0_1, blk.conv1_0, blk.conv1_1, blk.conv1_2) for p in (m.kernel, m.bias)]
        tables = ops.child_irn_tables(params)
        q4 = ops.child_q4_tables(params) if family == 'child_q4 irn' else None
    else:
        cout = 1 if 'cls' in family else C
        W, b = F64._rand_w(rng, 27, C, cout)
        bt = _t(b)
        table = ops.child_q4_cls_table(_t(W)) if family == 'child_q4 cls' else ops.child_cls_table(_t(W)) if cout == 1 else ops.child_conv_table(_t(W))
    for n_p in CHILD_PARENTS:
        def make(seed):
            pc = _sibling(_shell9(coarse=True)[:n_p], 16, seed).astype(np.int64)
            parent = CoordMap(_t(pc, torch.int32), 2, unique=True)
            kc = R.children_coords(pc, 2)
            x = F64._features(rng, len(kc), C)
            return (kc, x), (parent.k3, F64._poisoned(x) if not irn else _t(x))

        def fn(i):
            if irn:
                return ops.irn_block_child(i[0], i[1], params, tables, q4_table=q4)
            if family == 'child_q4 cls':
                return ops.cls_child_q4(i[0], i[1], table, bt)
            return ops.conv_child(i[0], i[1], table, bt, cout)
        _, A = make(500 + n_p)
        (kc, x), B = make(600 + n_p)
        want = protocol(f'children: {family}', fn, A, B)
        if irn:
            _eq(want, orc.inception_resnet(sd, 'b', orc.Level(kc.astype(np.int32), 1), x), f'{family}, {n_p} parents vs the oracle')
        else:
            _eq(want, orc.conv_gather(R.k3_map(kc, 1).astype(np.int32), x, W, b), f'{family}, {n_p} parents vs the oracle')


# ================================================================================================ backward pass
import test_grad_device as GD                    # (def_wgrad: the definition from a map, exact on integer-valued data)


def _wgrad_sizes(ops, K, cin, cout):
    return (17, ops.conv_wgrad_rows_per_group(K, 17, cin, cout) + 1)


@pytest.mark.parametrize('kind, K, cin, cout', [('k3', 27, 16, 16), ('k1', 1, 32, 8), ('down', 8, 16, 32)])
def test_conv_wgrad(kind, K, cin, cout, ops):
    """17 rows, and one row more than a workgroup reduces: a second partial sum per entry"""
    rng = np.random.default_rng(K)
    for n in _wgrad_sizes(ops, K, cin, cout):
        def make(seed):
            if kind == 'k1':
                nbr, n_in = None, n
            elif kind == 'down':
                c4, nbr = _down_pair(n, seed)
                n_in = len(c4)
            else:
                nbr, n_in = R.k3_map(_level(n, seed), 1), n
            n_out = n_in if nbr is None else nbr.shape[1]
            x, gy = GD._ints(rng, (n_in, cin)), GD._ints(rng, (n_out, cout))
            return (nbr, x, gy), (None if nbr is None else _t(nbr, torch.int32), _t(x), _t(gy))
        fn = lambda i: list(ops.conv_wgrad(*i)) + [ops.conv_wgrad(*i, want_bias=False)[0]] + ([] if i[0] is None else [ops.kmap_invert(i[0], i[1].shape[0])])
        _, A = make(700 + n)
        (nbr, x, gy), B = make(800 + n)
        want = protocol('backward: conv_wgrad / kmap_invert', fn, A, B)
        m = np.arange(len(x))[None] if nbr is None else nbr
        wW, wb, _ = GD.def_wgrad(m, x, gy)
        _eq(want[0].reshape(wW.shape), wW, f'{kind} gW, {n} rows'); _eq(want[1].ravel(), wb, f'{kind} gb'); _eq(want[2].reshape(wW.shape), wW, f'{kind} gW without bias')
        if nbr is not None:
            inv = np.full((K, len(x)), -1, np.int64)
            for k in range(K):
                o = np.flatnonzero(nbr[k] >= 0)
                inv[k, nbr[k, o]] = o
            _eq(want[3], inv, f'{kind} kmap_invert')


def test_conv_up2_wgrad(ops):
    rng = np.random.default_rng(9)
    cin, cout = 64, 32
    for n in _wgrad_sizes(ops, 8, cin, cout):
        def make():
            wide, gy = GD._ints(rng, (n + 5, cin)), GD._ints(rng, (8 * n, cout))
            rows = rng.permutation(n + 5)[:n].astype(np.int32)
            return (wide, gy, rows), (_t(wide), _t(gy), _t(rows))
        fn = lambda i: list(ops.conv_up2_wgrad(i[0][:n], i[1])) + list(ops.conv_up2_wgrad(i[0], i[1], rows=i[2]))
        _, A = make()
        (wide, gy, rows), B = make()
        want = protocol('backward: conv_up2_wgrad', fn, A, B)
        for base, x in ((0, wide[:n]), (2, wide[rows])):                # (integer-valued data: the sums are exact in any order)
            gW = np.stack([x.astype(np.float64).T @ gy[j::8].astype(np.float64) for j in range(8)])
            _eq(want[base].astype(np.float64), gW, f'conv_up2_wgrad gW ({"rows" if base else "plain"}), {n} parents')
            _eq(want[base + 1].ravel(), gy.astype(np.float64).sum(0), 'conv_up2_wgrad gb')


def test_pointwise_backward_and_scatter(ops, golden_dir):
    rng = np.random.default_rng(12)
    n, C, n_out = 1027, 12, 2051
    params = np.load(os.path.join(golden_dir, 'eval_loss.npz'))['b3_params'].astype(np.float32)
    pd = _t(params)

    def make():
        y, g = rng.normal(size=(n, C)).astype(np.float32), rng.normal(size=(n, C)).astype(np.float32)
        y[::7, 3] = -0.0
        orig = np.sort(rng.choice(n_out, size=n, replace=False)).astype(np.int32)
        z, t = rng.uniform(-4, 4, n).astype(np.float32), (rng.random(n) < 0.4).astype(np.uint8)
        lat = (rng.integers(-14, 15, (n, 8)) + rng.uniform(-0.5, 0.5, (n, 8))).astype(np.float32)
        return (y, g, orig, z, t, lat), tuple(_t(a) for a in (y, g, orig, z, t, lat))
    fn = lambda i: dict(relu=ops.relu_bwd(i[1], i[0]), scatter=ops.scatter_rows(i[1], i[2], n_out), bce=ops.bce_logits_bwd(i[3], i[4], scale=0.37),
                        eb=list(ops.eb_likelihood_bwd(i[5], pd, bound=1e-9, scale=1.0)))
    _, A = make()
    (y, g, orig, z, t, lat), B = make()
    want = protocol('backward: pointwise / scatter / leaves', fn, A, B)
    _eq(want['relu'], np.where(y > 0, g, np.float32(0)), 'relu_bwd')
    scattered = np.zeros((n_out, C), np.float32)
    scattered[orig] = g
    _eq(want['scatter'], scattered, 'scatter_rows')
    wz = 0.37 * GD.G.bce_gradient(z, t != 0)                           # the bounds of test_grad_device.py's leaf tests
    assert R.within(want['bce'].ravel(), wz, R.BOUND_SLACK * (R.U * np.abs(wz) + 2.0 ** -52 * 0.37 / GD.G.LN2)) <= 1.0
    wy, wp, _ = GD.G.eb_gradients(params, lat)
    assert R.within(want['eb'][0], wy, R.BOUND_SLACK * R.U * np.abs(wy)) <= 1.0 and R.within(want['eb'][1], wp, R.BOUND_SLACK * R.U * np.abs(wp)) <= 1.0


def test_forward_train_and_backward():
    """one training step on shell7 and on its translate: the loss and all 224 gradients"""
    from pcgcv2_amd import loss
    model = _model()
    a, b = _shell7_pair()

    def fn(c4):
        model.zero_grad(set_to_none=True)
        x = _cloud_tensor(c4)
        out = model.forward_train(x, generator=torch.Generator(device=DEV).manual_seed(77))
        total, _, _ = loss.sum_loss(out, len(x))
        total.backward()
        return dict(total=total.detach(), likelihood=out['likelihood'].detach(), grads={k: p.grad for k, p in model.named_parameters()})
    want = protocol('forward_train + backward', fn, a, b)
    assert len(want['grads']) == 224 and all(np.isfinite(g).all() for g in want['grads'].values()) and np.isfinite(want['total']).all()
    for k in ('encoder.conv0.kernel', 'encoder.conv3.kernel', 'decoder.up0.kernel', 'decoder.conv0_cls.kernel', 'entropy_bottleneck._matrices.0'):
        assert want['grads'][k].any(), k


# ================================================================================================ D1, the D2 chain, normals, colours
import colour_reference as cr
import normals_reference as nr


def _metric_pair(seed):
    """shell7 against its jittered copy (amp 1), both moved by the same multiple of 8 and each in a row order of its own: every tie set,
    selection list and segment total has the size it has in the sibling, and other contents"""
    rng = np.random.default_rng(seed)
    a = synthetic.shell('shell7').numpy().astype(np.int64)
    b = np.unique(np.clip(a + np.random.default_rng(1).integers(-1, 2, size=a.shape), 0, None), axis=0)
    shift = 8 * rng.integers(1, 20, 3)
    a, b = (a + shift)[rng.permutation(len(a))], (b + shift)[rng.permutation(len(b))]
    v = a - a.mean(0)
    na = (v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-9)).astype(np.float32).astype(np.float64)
    ca, cb = rng.integers(0, 256, (len(a), 3)).astype(np.uint8), rng.integers(0, 256, (len(b), 3)).astype(np.uint8)
    a4, b4 = (np.concatenate([np.zeros((len(p), 1), np.int32), p.astype(np.int32)], 1) for p in (a, b))
    return (a4, na, b4, ca, cb), (_t(a4), _t(na), _t(b4), _t(ca), _t(cb))


def test_metrics_normals_and_colours(ops):
    from pcgcv2_amd import pc_error as pe

    def fn(i):
        a, na, b, ca, cb = i
        out = dict(d1_cells=[list(ops.d1_nn(a, b)), list(ops.d1_nn(b, a))])
        with ops.path(D1_CELLS=False):
            out['d1_probes'] = [list(ops.d1_nn(a, b)), list(ops.d1_nn(b, a))]
        nn = pe.nn_both(a, b)
        out['nn'] = [list(nn[0]), list(nn[1])]
        out['d2'] = pe.d2_psnr_device(a, na, b, 128, nn=nn)
        out['d2_own_search'] = pe.d2_psnr_device(a, na, b, 128)
        out['normals'] = list(ops.estimate_normals(a, r2=16, want_moments=True))
        out['recolour'] = pe.recolour_device(a, ca, b, nn=nn)
        out['colour'] = pe.colour_psnr_device(a, ca, b, cb, nn=nn)
        return out
    _, A = _metric_pair(70)
    (a4, na, b4, ca, cb), B = _metric_pair(71)
    want = protocol('D1 / D2 / normals / colours', fn, A, B)
    d1 = orc.d1_metrics(a4[:, 1:], b4[:, 1:], 128)
    for k in ('d1_cells', 'd1_probes'):
        (s1, m1, u1), (s2, m2, u2) = want[k]
        assert (float(s1[0]) / len(a4), float(s2[0]) / len(b4)) == (d1['mse1'], d1['mse2']) and not u1[0] and not u2[0], k
    host = pe.d2_psnr(a4[:, 1:], na, b4[:, 1:], 128)              # the KD-tree statement of the metric (tests/test_d2_metric_device.py holds the device to it)
    for m in (want['d2'], want['d2_own_search']):
        assert sum(k in m for k in host) >= 18
        for k in (k for k in host if k in m):
            assert m[k] == (host[k] if '(p2point)' in k else pytest.approx(host[k], rel=1e-12, abs=0)), k
    assert want['d2'] == want['d2_own_search']
    ref = nr.estimate_normals(a4, 16)
    nrm, lam, count, valid, mom = want['normals']
    _eq(mom, ref['moments'], 'normals: moments'); _eq(count, ref['count'], 'normals: count'); _eq(valid, ref['valid'], 'normals: valid')
    assert (nrm[~valid] == 0.0).all() and np.isfinite(nrm).all()
    _eq(want['recolour'], cr.recolour(a4, ca, b4), 'attr_transfer')
    definition = cr.colour_metric(a4, ca, b4, cb)
    for col in cr.COLUMNS:
        assert want['colour'][col] == (definition[col] if col.startswith('h.') or np.isinf(definition[col]) else pytest.approx(definition[col], rel=1e-12, abs=0)), col


# ================================================================================================ colour transform (RAHT)
import raht_reference as RR
import test_attributes_device as AT            # (its geometries and colour kinds)


def _raht_fn(ops, ql, qc):
    def fn(i):
        coords, rgb = i
        tree = ops.raht_tree(coords)
        out = dict(tree=[getattr(tree, f) for f in ('keys', 'perm', 'd', 'lo', 'hi', 'left', 'right', 'order')], bucket=tree.bucket.copy(), cross=tree.cross.copy(),
                   n_cross=int(tree.cross[-1]))
        out['cross_order'] = tree.cross_order                          # (a stable sort of all n - 1 gaps: the crossing ones first, every slot written)
        fwd = {form: ops.raht_forward(tree, rgb, form=form) for form in ops.RAHT_FORMS}
        out['forward'] = {form: list(v) for form, v in fwd.items()}
        H, dc = fwd[ops.RAHT_FORM]
        tok, ctx, esc, hist = ops.raht_quantize(tree, H, ql, qc)
        out['quantize'] = [tok, ctx, esc, hist]
        Hh = ops.raht_dequantize(tree, tok, esc, ql, qc)
        out['dequantize'] = Hh
        out['inverse'] = {form: ops.raht_inverse(tree, Hh, dc.tolist(), form=form) for form in ops.RAHT_FORMS}
        return out
    return fn


@pytest.mark.parametrize('name, kind, ql, qc', [(f'line{AT.T + 1}', 'random', 1, 4), (f'leaving{AT.T + 1}', 'random', 1, 4), ('random', 'random', 1, 4),
                                                ('random', 'alternating', 0, 0)])
def test_raht(name, kind, ql, qc, ops):
    assert ops.raht_tile_leaves() == AT.T

    def make(seed, kind):
        rng = np.random.default_rng(seed)
        pts = np.asarray(AT.GEOMETRY[name](), np.int64)
        pts = (pts + 8 * rng.integers(1, 30, 3))[rng.permutation(len(pts))]
        rgb = AT._colours(kind, pts, seed)
        return (pts, rgb), (AT._coords(pts), _t(rgb))
    # with 'alternating' colours B's number of escapes differs from A's: the list is a VIEW of a buffer sized by the shape (3 (n - 1))
    _, A = make(80, 'random')
    (pts, rgb), B = make(81, kind)
    want = protocol('RAHT', _raht_fn(ops, ql, qc), A, B)
    keys, perm = RR.sort_cloud(pts)
    ref = RR.build_tree(keys)
    _eq(want['tree'][0].view(np.uint64), keys, 'keys'); _eq(want['tree'][1], perm, 'perm')
    for f, g in zip(('d', 'lo', 'hi', 'left', 'right', 'order'), want['tree'][2:]):
        _eq(g.astype(np.int64), ref[f], f'tree.{f}')
    _eq(want['bucket'], ref['bucket'], 'bucket')
    crossing = (ref['lo'] // AT.T) != (ref['hi'] // AT.T)
    _eq(want['cross_order'][:want['n_cross']], ref['order'][crossing[ref['order']]], 'cross_order')
    H_ref, dc_ref = RR.forward(ref, RR.ycocg_forward(rgb[perm]))
    for form, (H, dc) in want['forward'].items():
        _eq(H, H_ref, f'H ({form})'); assert dc.tolist() == dc_ref.tolist(), form
    D16 = RR.steps(ref, ql, qc)
    k = RR.quantize(H_ref, D16)
    tok_r, ctx_r, esc_r, hist_r = RR.tokens(ref, k)
    tok, ctx, esc, hist = want['quantize']
    _eq(tok, tok_r, 'tokens'); _eq(ctx.view(np.uint16), ctx_r, 'contexts'); _eq(esc.view(np.uint16), esc_r, 'escapes'); _eq(hist, hist_r, 'histogram')
    assert esc_r.size > 0 or kind != 'alternating'                      # the escape path
    Hh_ref = RR.dequantize(k, D16)
    _eq(want['dequantize'], Hh_ref, 'dequantize')
    back = np.zeros((len(pts), 3), np.uint8)
    back[perm] = RR.ycocg_inverse(RR.inverse(ref, Hh_ref, dc_ref))
    for form, got in want['inverse'].items():
        _eq(got, back, f'inverse ({form})')


# ================================================================================================ meshes -> training clouds
import mesh_reference as mr


@pytest.mark.parametrize('T', [65, 1000])
def test_mesh_cdf_sample_voxelize(T, ops):
    n, resolution, seed, rot = 257, 127, 5, mr.fixed_rotation()

    def make(s):
        verts, faces = mr.random_mesh(T, s, -3.0, 2.0)
        faces[0], faces[T - 1] = (1, 1, 2), (9, 3, 9)                  # zero-area triangles first and last
        verts, faces = np.ascontiguousarray(verts, np.float64), np.ascontiguousarray(faces, np.int32)
        return (verts, faces), (_t(verts), _t(faces))

    def fn(i):
        cdf = ops.mesh_area_cdf(*i)
        tri, pts = ops.mesh_sample(i[0], i[1], cdf, seed, 0, n)
        return dict(cdf=cdf, tri=tri, pts=pts, late=list(ops.mesh_sample(i[0], i[1], cdf, seed, 2 ** 32 - 5, 10)), vox=ops.mesh_voxelize(i[0], i[1], cdf, seed, n, rot, resolution))
    _, A = make(90)
    (verts, faces), B = make(91)
    want = protocol('mesh', fn, A, B)
    cdf = want['cdf']
    ref = mr.fsum_cdf(mr.areas(verts, faces))
    assert (np.abs(cdf - ref) <= (np.arange(T) + 8) * 2.0 ** -52 * ref).all() and (np.diff(cdf) >= 0).all() and cdf[0] == 0 and cdf[T - 1] == cdf[T - 2]
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.int64)
    for (tri, pts), first, m in ((( want['tri'], want['pts']), 0, n), (want['late'], 2 ** 32 - 5, 10)):
        rt, rp = mr.sample(verts, faces, cdf, seed, first, m)
        _eq(tri, rt, 'mesh_sample: triangles'); _eq(bits(pts), bits(rp), 'mesh_sample: points')
    vox = mr.voxelize(verts, faces, cdf, seed, n, rot, resolution)
    _eq(want['vox'], np.concatenate([np.zeros((len(vox), 1), np.int32), vox], 1), 'mesh_voxelize')


# ================================================================================================ undersized scratch is refused, not used
def _undersized_cases(ops):
    from pcgcv2_amd import pc_error as pe
    rng = np.random.default_rng(60)
    n = 2051
    _, scan = _scan_input(n, 61, 0)
    c4 = scan['c']
    v = _t(rng.standard_normal(n).astype(np.float32)).reshape(-1, 1)
    x, t, p = (_t(a) for a in er.bce_case(1025))
    ctx, bit = rr.cyclic(513, seed=3)
    feats = _t(GD._ints(rng, (n, 8)))
    pts = AT._random_cloud(600, 24, 5)
    cloud, cloud2, colours = AT._coords(pts), AT._coords(pts[::-1] + 1), _t(AT._colours('random', pts, 1))
    tree = ops.raht_tree(cloud)
    H, _ = ops.raht_forward(tree, colours)
    verts, faces = mr.random_mesh(65, 3, -3.0, 2.0)
    mesh = (_t(np.ascontiguousarray(verts, np.float64)), _t(np.ascontiguousarray(faces, np.int32)))
    mesh_cdf = ops.mesh_area_cdf(*mesh)
    return {
        'pcgc_scan_workspace_bytes': lambda: ops.mask_scan(scan['m']),
        'pcgc_pyramid_scratch_bytes': lambda: ops.pyramid(c4, 1, 3),
        'pcgc_topk_workspace_bytes': lambda: ops.topk_mask(v, 1000),
        'pcgc_topk_select_workspace_bytes': lambda: ops.topk_select(v, [n], [1000], coords=c4),
        'pcgc_sort_workspace_bytes': lambda: ops.sort_zyx(c4),
        'pcgc_loss_workspace_bytes': lambda: ops.bce_logits(x, t, p),
        'pcgc_occ_workspace_bytes': lambda: ops.occ_symbols(x, t),
        'pcgc_occ_rans_workspace_bytes': lambda: ops.occ_rans_encode(_packed(ctx, bit), 4),
        'pcgc_conv_wgrad_workspace_bytes': lambda: ops.conv_wgrad(None, feats, feats),
        'pcgc_eb_bwd_workspace_bytes': lambda: ops.eb_likelihood_bwd(feats, _t(np.zeros(44 * 8, np.float32))),
        'pcgc_d2_scan_workspace_bytes': lambda: ops._d2_scan(_t(np.ones(n, np.int32))),
        'pcgc_d2_reduce_workspace_bytes': lambda: ops.d2_reduce(_t(np.ones(n, np.int64)), _t(np.ones(n, np.float64))),
        'pcgc_attr_transfer_workspace_bytes': lambda: pe.recolour_device(cloud, colours, cloud2),
        'pcgc_colour_reduce_workspace_bytes': lambda: ops.colour_reduce(_t(np.ones((n, 3), np.int64)), _t(np.ones((n, 3), np.int32))),
        'pcgc_raht_keys_workspace_bytes+pcgc_raht_tree_workspace_bytes': lambda: ops.raht_tree(cloud),
        'pcgc_raht_quantize_workspace_bytes': lambda: ops.raht_quantize(tree, H, 1, 4),
        'pcgc_raht_dequantize_workspace_bytes': lambda: ops.raht_dequantize(tree, _t(np.zeros(3 * (tree.n - 1), np.int16)), _t(np.zeros(0, np.int16)), 1, 4),
        'pcgc_normals_workspace_bytes': lambda: ops.estimate_normals(cloud),
        'pcgc_mesh_cdf_workspace_bytes': lambda: ops.mesh_area_cdf(*mesh),
        'pcgc_mesh_voxelize_workspace_bytes': lambda: ops.mesh_voxelize(mesh[0], mesh[1], mesh_cdf, 5, 257, np.eye(3), 127),
    }


UNDERSIZED = ['pcgc_scan_workspace_bytes', 'pcgc_pyramid_scratch_bytes', 'pcgc_topk_workspace_bytes', 'pcgc_topk_select_workspace_bytes',
              'pcgc_sort_workspace_bytes', 'pcgc_loss_workspace_bytes', 'pcgc_occ_workspace_bytes', 'pcgc_occ_rans_workspace_bytes',
              'pcgc_conv_wgrad_workspace_bytes', 'pcgc_eb_bwd_workspace_bytes', 'pcgc_d2_scan_workspace_bytes', 'pcgc_d2_reduce_workspace_bytes',
              'pcgc_attr_transfer_workspace_bytes', 'pcgc_colour_reduce_workspace_bytes',
              # (raht_tree sizes ONE workspace for both calls by the larger answer: both answer one byte less, the first call refuses)
              'pcgc_raht_keys_workspace_bytes+pcgc_raht_tree_workspace_bytes', 'pcgc_raht_quantize_workspace_bytes', 'pcgc_raht_dequantize_workspace_bytes',
              'pcgc_normals_workspace_bytes', 'pcgc_mesh_cdf_workspace_bytes', 'pcgc_mesh_voxelize_workspace_bytes']


def test_every_sizing_call_of_the_library_is_covered(ops):
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'pcgc_hip.h')).read()
    declared = set(re.findall(r'size_t (pcgc_\w+_(?:workspace|scratch)_bytes)\(', header))
    assert declared == {name for entry in UNDERSIZED for name in entry.split('+')}


@pytest.mark.parametrize('sizing', UNDERSIZED)
def test_undersized_scratch_is_refused(sizing, ops, monkeypatch):
    """the sizing call answers one byte less, the wrapper passes on what it was told: the native size check refuses before any launch"""
    call = _undersized_cases(ops)[sizing]
    call()                                                            # (the call is sound with the true size)
    for name in sizing.split('+'):
        monkeypatch.setattr(ops.lib(), name, (lambda true: lambda *a: int(true(*a)) - 1)(getattr(ops.lib(), name)))
    arena = Arena()
    with SA.installed(arena):
        with pytest.raises(PcgcError, match='too small'):
            call()
    n_after = len(arena.blocks)
    arena.check()
    assert n_after > 0 and len(arena.blocks) == n_after
    refused = arena.blocks[-1].caller                                  # the wrapper whose native call refused: nothing is allocated after it,
    for b in arena.blocks:                                             # and nothing it allocated was written (refused before any launch)
        assert b.caller != refused or not b.payload().any(), f'allocation {b.index} from {b.caller}() was written by a refused call'
    rec = REPORT.setdefault('undersized scratch refused', [0, 0, 0, 0, []])
    rec[0] += 1; rec[1] += n_after; rec[3] += arena.stats()[2]


# ================================================================================================ report
def test_zz_report_scratch_state():
    """(prints, per family: cases, allocations, allocations replayed from the recorded run, bytes guarded, and every data-dependent request
    that was served fresh; a shape-determined request that was not replayed fails its own case)"""
    for k in sorted(REPORT):
        cases, allocs, replayed, guarded, fresh = REPORT[k]
        print(f'scratch state {k:34s} {cases:4d} cases {allocs:7d} allocations {replayed:7d} replayed {guarded:12d} bytes guarded; '
              f'served fresh: {fresh if fresh else "none"}')
        assert cases > 0 and allocs > 0
