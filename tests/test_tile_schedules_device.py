"""The MFMA kernels at the edges of their tile schedules (csrc/tile_sched.h), against the float64 definition and the oracle's bits.

Two properties depend on how a launch is cut into tiles and are reached by the other tests only at whole-frame sizes:

* k_conv_packed64 takes its rows per workgroup R at run time (even, 40 .. 128; pk_rows picks it from the row and CU counts).  Here every R
  is forced (ops.set_packed_rows) on inputs of 1, R - 1, R, R + 1, 2 R + 1 and 5 R + 3 rows: R below and above 64 (the second ballot), R a
  multiple of 16 or not (padding slots, the dummy accumulator row), offsets with every row present, with none, with 1 .. 15, and with more
  than 64 that are no multiple of 16.
* The persistent kernels walk several tiles per wave only once a level has more tiles than resident waves — on 256 CUs from 30-65 k rows.
  With ops.set_sched_cus(1) a grid is 8 workgroups, W = 8 x (waves per workgroup) wave slots, and T = 1, 7, 9, W - 1, W, W + 1, 2 W, 2 W + 1
  work units — each with a full last tile and with a single row in it — reach every round boundary in a few thousand rows.  ops.last_sched()
  must report exactly the T a case was built for (a retuned tile height or wave count fails loudly instead of moving the edges), and the
  2 W + 1 case must give the same bits on 1 CU, on the device's own count and with one tile per wave.

No tolerance of its own: the bound is fp64_reference's, bit equality with the oracle as in test_fp64_definition.py, whose helpers run here."""
import numpy as np
import pytest
import torch

import fp64_reference as R
import test_fp64_definition as D
from oracle import pcgc_oracle as orc

SCHED_W = {}                                     # family -> wave slots W per launched kernel on the 8-workgroup grid (printed at the end)


@pytest.fixture
def sched():
    """ops with the CU count, the packed conv's tile size, the PathConfig and the forced families put back afterwards"""
    from pcgcv2_amd import ops
    keep = ops.PATH
    yield ops
    ops.set_sched_cus(0)
    ops.set_packed_rows(0)
    ops.configure(keep)
    ops.set_conv_impl(-1)
    ops.set_up2_impl(2)
    ops.set_rows_q4_variant(0)
    ops.PROFILE.reset(enabled=False)


_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _cloud(name):
    return _cached(('cloud', name), lambda: D._cloud4(name) if name.endswith('_s') else D._shell4(name))


def _rows(n):
    """the first n rows of a shell (the smallest that has them)"""
    for name in ('shell9', 'shell10'):
        if len(_cloud(name)) >= n:
            return _cloud(name)[:n]
    raise AssertionError(n)


# ================================================================================================ packed conv: every tile size
PACKED_R = list(range(40, 129, 2))
PACKED_NMAX = 5 * 128 + 3


def _packed_weights():
    return _cached('packed W', lambda: D._rand_w(np.random.default_rng(64), 27, 64, 64))


def _isolated(n):
    """n voxels, no two within one lattice step of each other: 26 of the 27 offsets have no present row"""
    g = np.stack(np.meshgrid(*[np.arange(7)] * 3, indexing='ij'), -1).reshape(-1, 3) * 3 + 5
    assert n <= len(g)
    return D._with_batch(g[:n])


def _packed_source(cloud):
    """(coords, k3 map, features) of the first PACKED_NMAX rows of a cloud; a prefix of n rows has the map's first n columns with the
    entries >= n absent"""
    def make():
        c4 = _cloud(cloud)[:PACKED_NMAX] if cloud != 'isolated' else _isolated(2 * 128 + 1)
        return c4, R.neighbour_map(c4, c4, R.offsets(3)), D._features(np.random.default_rng(len(cloud)), len(c4), 64)
    return _cached(('packed', cloud), make)


def _packed_inputs(rows):
    """[(name, map [27, n], features [n, 64])] of tile size `rows`"""
    out = []
    for cloud in ('solid_cube_s', 'noisy_s'):
        c4, full, x = _packed_source(cloud)
        for n in (1, rows - 1, rows, rows + 1, 2 * rows + 1, 5 * rows + 3):
            out.append((f'{cloud}[:{n}]', np.where(full[:, :n] < n, full[:, :n], -1), x[:n]))
    c4, full, x = _packed_source('isolated')
    n = 2 * rows + 1
    out.append((f'isolated[:{n}]', np.where(full[:, :n] < n, full[:, :n], -1), x[:n]))
    return out


def _packed_coverage(rows, inputs):
    """which kinds of (tile, offset) the inputs of a tile size hold, by the present rows of the tile at the offset"""
    kinds = set()
    for _, nbr, _ in inputs:
        n = nbr.shape[1]
        for r0 in range(0, n, rows):
            for cnt in (nbr[:, r0:r0 + rows] >= 0).sum(1):
                if cnt == rows:
                    kinds.add('all')
                if cnt == 0:
                    kinds.add('none')
                if 1 <= cnt <= 15:
                    kinds.add('1..15')
                if cnt > 64 and cnt % 16:
                    kinds.add('>64, ragged')
    return kinds


def test_packed_inputs_cover_the_kernel_edges():
    """(CPU) for every tile size the inputs hold a (tile, offset) with all R rows present, one with none, one with 1 .. 15 present and — above
    R = 64, where the second ballot packs rows 64 .. — one with more than 64 present rows that are no multiple of 16"""
    for rows in PACKED_R:
        inputs = _packed_inputs(rows)
        assert [nbr.shape[1] for _, nbr, _ in inputs] == [1, rows - 1, rows, rows + 1, 2 * rows + 1, 5 * rows + 3] * 2 + [2 * rows + 1]
        kinds = _packed_coverage(rows, inputs)
        want = {'all', 'none', '1..15'} | ({'>64, ragged'} if rows > 64 else set())
        assert want <= kinds, (rows, want - kinds)
        for name, nbr, _ in inputs:
            np.testing.assert_array_equal(nbr[13], np.arange(nbr.shape[1]))              # the centre offset is the row itself
            if name.startswith('isolated'):
                assert (np.delete(nbr, 13, 0) < 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize('rows', PACKED_R)
def test_packed_conv_every_tile_size(rows, sched):
    ops = sched
    W, b = _packed_weights()
    table, bt = ops.child_conv_table(D._t(W)), D._t(b)
    ops.set_packed_rows(rows)
    inputs = _packed_inputs(rows)
    for name, nbr, x in inputs:
        n = nbr.shape[1]
        got, names = D._profiled(ops, lambda: ops.conv_packed64(D._t(nbr, torch.int32), D._poisoned(x), table, bt))
        assert names == {'k_conv_packed64'}, names
        tiles = (n + rows - 1) // rows
        assert ops.last_sched() == (tiles, tiles, rows), (name, ops.last_sched())
        y, e = R._conv(nbr, x, R.zero_bound(x), W, b)
        D._gpu_check('packed64 R = 40 .. 128', got, y, e, orc.conv_gather(nbr.astype(np.int32), x, W, b))
    assert {'all', 'none', '1..15'} | ({'>64, ragged'} if rows > 64 else set()) <= _packed_coverage(rows, inputs)


@pytest.mark.gpu
def test_packed_tuning_refuses_untested_sizes(sched):
    from pcgcv2_amd._lib import lib
    ops = sched
    ops.set_packed_rows(64)
    for bad in (-2, 1, 38, 39, 41, 63, 127, 129, 130, 256):
        assert lib().pcgc_set_packed_tuning(bad, 0) == -1, bad
    assert lib().pcgc_set_packed_tuning(64, 8) == -1
    assert lib().pcgc_set_sched_cus(-1) == -1
    W, b = _packed_weights()
    c4, full, x = _packed_source('noisy_s')
    ops.conv_packed64(D._t(full, torch.int32), D._t(x), ops.child_conv_table(D._t(W)), D._t(b))
    assert ops.last_sched()[2] == 64                                # the refused values changed nothing
    for ok in (0, 40, 128):
        assert lib().pcgc_set_packed_tuning(ok, 4) == 0


# ================================================================================================ persistent kernels: every round boundary
T_CASES = ('1', '7', '9', 'W-1', 'W', 'W+1', '2W', '2W+1')


def _t_value(sym, W):
    return {'1': 1, '7': 7, '9': 9, 'W-1': W - 1, 'W': W, 'W+1': W + 1, '2W': 2 * W, '2W+1': 2 * W + 1}[sym]


def _params_of(blk):
    return [p for m in (blk.conv0_0, blk.conv0_1, blk.conv1_0, blk.conv1_1, blk.conv1_2) for p in (m.kernel, m.bias)]


class Family:
    """A kernel family on a level of n `items` (rows, coarse rows or parents).  kernels: per launched kernel (items per tile, work units per
    tile, persistent?).  run(ops, n) -> (output, [last_sched() of each kernel], thunk -> (fp64 value, bound), oracle thunk, output rows)."""

    def __init__(self, name, kernels, run):
        self.name, self.kernels, self.run = name, kernels, run


def _irn_plain(family):
    C, changes, kernels, variant = D.IRN_FAMILIES[family]
    form, tables_of = {'rows64': ('rows64', 'child_irn_tables'), 'rows32': ('rows32', 'rows_irn32_tables')}.get(family, ('rows32_q4', 'rows_q4_tables'))
    h = {'rows64': 16, 'rows32': 16, 'rows32q4 v0': 64, 'rows32q4 v1': 128, 'rows32q4 v2': 64, 'rows32q4 v3': 64}[family]

    def run(ops, n):
        from pcgcv2_amd import dispatch
        from pcgcv2_amd.sparse import CoordMap, SparseTensor
        rng = np.random.default_rng(C + variant + n)
        blk, sd = D._block(rng, C)
        ops.configure(**changes)
        ops.set_rows_q4_variant(variant)
        c4 = _rows(n)
        assert dispatch.select('irn', (C,), n).family == family.split(' ')[0]
        x = D._features(rng, n, C)
        xs = SparseTensor(D._t(x), coordinate_map=CoordMap(D._t(c4, torch.int32), 1, unique=True))
        params = _params_of(blk)
        with torch.no_grad():
            ops.irn_form_pass(form, xs.cmap.k3, xs.F, params, getattr(ops, tables_of)(params), 1)
            sa = ops.last_sched()
            got, names = D._profiled(ops, lambda: blk(xs).F)
        assert names == kernels, names
        return (got, [sa, ops.last_sched()], (lambda: R.inception_resnet(sd, 'b', c4, 1, x, R.zero_bound(x))),
                (lambda: orc.inception_resnet(sd, 'b', orc.Level(c4.astype(np.int32), 1), x)), n)
    return Family(f'irn {family}', [(h, 1, True)] * 2, run)


def _children(n_p):
    """(parent CoordMap, children coords) of the first n_p rows of a shell's stride-2 level (the smallest shell that has them)"""
    from pcgcv2_amd.sparse import CoordMap
    for name in ('shell9', 'shell10'):
        pc = _cached(('parents', name), lambda: R.down_coords(_cloud(name), 1))
        if len(pc) >= n_p:
            break
    assert len(pc) >= n_p
    parent = CoordMap(D._t(pc[:n_p], torch.int32), 2, unique=True)
    kc = R.children_coords(pc[:n_p], 2)
    np.testing.assert_array_equal(parent.up().C.cpu().numpy(), kc)
    return parent, kc


def _child(family):
    C = int(family.split(' ')[-1]) if family[-1].isdigit() else 16
    irn = 'irn' in family
    kernels = {'child conv 16': [(16, 1, True)], 'child conv 32': [(16, 2, True)], 'cls 16': [(16, 1, True)], 'cls 32': [(16, 1, True)],
               'cls 64': [(16, 1, True)], 'child irn 16': [(16, 1, True)] * 2, 'child irn 32': [(16, 2, True)] * 2,
               'child_q4 cls': [(128, 1, True)], 'child_q4 irn': [(128, 1, True), (16, 1, True)]}[family]

    def run(ops, n_p):
        rng = np.random.default_rng(len(family) + n_p)
        parent, kc = _children(n_p)
        x = D._features(rng, len(kc), C)
        if irn:
            blk, sd = D._block(rng, C)
            params = _params_of(blk)
            tables = ops.child_irn_tables(params)
            q4 = ops.child_q4_tables(params) if family == 'child_q4 irn' else None
            names = {'k_child_q4<0, 8, 2>', 'k_child_irn_b<16>'} if q4 is not None else {f'k_child_irn_a<{C}>', f'k_child_irn_b<{C}>'}
            with torch.no_grad():
                ops.irn_form_pass('child_q4' if q4 is not None else f'child<{C}>', parent.k3, D._t(x), params, (q4, tables[1]) if q4 is not None else tables, 1)
                scheds = [ops.last_sched()]
                got, launched = D._profiled(ops, lambda: ops.irn_block_child(parent.k3, D._t(x), params, tables, q4_table=q4))
            ref = lambda: R.inception_resnet(sd, 'b', kc, 1, x, R.zero_bound(x))
            oracle = lambda: orc.inception_resnet(sd, 'b', orc.Level(kc.astype(np.int32), 1), x)
        else:
            cout = 1 if 'cls' in family else C
            W, b = D._rand_w(rng, 27, C, cout)
            scheds = []
            if family == 'child_q4 cls':
                call, names = (lambda: ops.cls_child_q4(parent.k3, D._poisoned(x), ops.child_q4_cls_table(D._t(W)), D._t(b))), None
            else:
                table = ops.child_cls_table(D._t(W)) if cout == 1 else ops.child_conv_table(D._t(W))
                call = lambda: ops.conv_child(parent.k3, D._poisoned(x), table, D._t(b), cout)
                names = {f'k_child_cls<{C // 16}>' if cout == 1 else f'k_child_conv<{C // 16}, {C // 16}>'}
            got, launched = D._profiled(ops, call)
            ref = lambda: R.conv3(kc, 1, x, R.zero_bound(x), W, b)
            oracle = lambda: orc.conv_gather(R.k3_map(kc, 1).astype(np.int32), x, W, b)
        if names is not None:
            assert launched == names, launched
        return got, scheds + [ops.last_sched()], ref, oracle, len(kc)
    return Family(family, kernels, run)


def _down_level(m):
    """the first m coarse rows of shell10's stride-2 level and the fine rows below them: (map [8, m], fine row count)"""
    def make():
        c = _cloud('shell10')
        coarse = R.down_coords(c, 1)
        q = c.copy()
        q[:, 1:] = q[:, 1:] // 2 * 2
        return c, coarse, R.lookup(coarse, q)
    c, coarse, parent = _cached('down level', make)
    assert m <= len(coarse)
    fine = c[parent < m]
    return R.neighbour_map(coarse[:m], fine, R.offsets(2)), len(fine)


def _plain(family):
    def run(ops, n):
        rng = np.random.default_rng(len(family) + n)
        if family == 'rows_conv':
            W, b = D._rand_w(rng, 27, 32, 32)
            nbr = R.k3_map(_rows(n), 1)
            x = D._features(rng, n, 32)
            call, name = (lambda: ops.conv_rows(D._t(nbr, torch.int32), D._poisoned(x), ops.child_conv_table(D._t(W)), D._t(b), 32)), 'k_rows_conv<2, 2>'
        else:
            W, b = D._rand_w(rng, 8, 32, 64)
            nbr, n_fine = _down_level(n)
            x = D._features(rng, n_fine, 32)
            call, name = (lambda: ops.conv_down_rows(D._t(nbr, torch.int32), D._poisoned(x), ops.child_conv_table(D._t(W)), D._t(b), 64)), 'k_rows_down<2, 4>'
        got, names = D._profiled(ops, call)
        assert names == {name}, names
        return got, [ops.last_sched()], (lambda: R._conv(nbr, x, R.zero_bound(x), W, b)), (lambda: orc.conv_gather(nbr.astype(np.int32), x, W, b)), n
    return Family(family, [(16, 1, True)], run)


def _up2(impl, cin, cout):
    def run(ops, n):
        rng = np.random.default_rng(impl + cin + n)
        W, b = D._rand_w(rng, 8, cin, cout)
        ops.set_up2_impl(impl)
        c = _cached('up2 level', lambda: R.down_coords(_cloud('shell9'), 1))[:n]
        assert len(c) == n
        x = D._features(rng, n, cin)
        got = ops.conv_up2(D._poisoned(x), D._t(W), D._t(b))
        return got, [ops.last_sched()], (lambda: R.up(c, 2, x, R.zero_bound(x), W, b)[1:]), (lambda: orc.conv_up2(x, W, b)), 8 * n
    # (the form with fragments from L2 runs one tile per wave on any grid: its sizes are those of the persistent form of the same shape)
    return Family(f'conv_up2 {["valu", "mfma", "mfma_lds_table"][impl]} {cin}->{cout}', [(16, 1, impl == 2)], run)


FAMILIES = {f.name: f for f in
            [_irn_plain(k) for k in D.IRN_FAMILIES if not k.startswith(('valu', 'unfused'))] + [_child(k) for k in D.CHILD_FAMILIES] +
            [_plain('rows_conv'), _plain('rows_down')] + [_up2(i, ci, co) for i in (1, 2) for ci, co in ((64, 32), (32, 16))]}


def _slots(ops, fam):
    """wave slots W of each kernel of the family on the grid of one CU, read from a first launch (17 tiles of the tallest kernel: more than
    any kernel's workgroup holds, so the grid is the full one)"""
    ops.set_sched_cus(1)
    scheds = fam.run(ops, 17 * max(h for h, _, _ in fam.kernels))[1]
    assert len(scheds) == len(fam.kernels)
    if fam.name.startswith('conv_up2 mfma '):                    # not persistent: the boundaries of the LDS-table form
        scheds = FAMILIES[fam.name.replace('mfma ', 'mfma_lds_table ')].run(ops, 17 * 16)[1]
    W = [wg * nw for _, wg, nw in scheds]
    SCHED_W[fam.name] = W
    return W


def _sizes(fam, W, sym, fill):
    """[(kernel index, work units T, items n)]: T units of kernel k, the last tile full or with a single item in it"""
    out = []
    for k, ((h, q, _), Wk) in enumerate(zip(fam.kernels, W)):
        T = _t_value(sym, Wk)
        for Tq in sorted({max(q, T // q * q), -(-T // q) * q}):      # (half units come in pairs: the even counts on both sides of T)
            tiles = Tq // q
            n = tiles * h if fill == 'full' else (tiles - 1) * h + 1
            if (k, Tq, n) not in out:
                out.append((k, Tq, n))
    return out


def _check_case(ops, fam, W, k, T, n, ratios_key):
    got, scheds, ref, oracle, rows = fam.run(ops, n)
    torch.cuda.synchronize()
    for j, ((h, q, persistent), (units, wgs, nw)) in enumerate(zip(fam.kernels, scheds)):
        assert units == q * ((n + h - 1) // h), (fam.name, j, n, scheds)
        if persistent:
            assert wgs * nw == W[j] or units <= W[j], (fam.name, j, n, scheds, W)
            if units > W[j]:
                assert units > wgs * nw
    assert scheds[k][0] == T, (fam.name, k, T, n, scheds)
    D._gpu_check(ratios_key, got, *ref(), oracle() if rows <= 20000 else None)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize('fill', ['full', 'single'])
@pytest.mark.parametrize('sym', T_CASES)
@pytest.mark.parametrize('family', list(FAMILIES))
def test_persistent_kernels_at_round_boundaries(family, sym, fill, sched):
    ops = sched
    fam = FAMILIES[family]
    W = _slots(ops, fam)
    for k, T, n in _sizes(fam, W, sym, fill):
        got = _check_case(ops, fam, W, k, T, n, f'sched {family}')
        if sym == '2W+1':                                        # the same bits on the device's own grid and with one tile per wave
            for cus in (0, 1 << 20):
                ops.set_sched_cus(cus)
                other, scheds = fam.run(ops, n)[:2]
                assert torch.equal(got, other), (family, n, cus)
                if cus:
                    assert all(units <= wgs * nw for units, wgs, nw in scheds), scheds
            ops.set_sched_cus(1)


@pytest.mark.gpu
def test_rows32_sixteen_wave_instantiation_on_one_cu(sched):
    """32 769 rows: the first size of the 16-wave C = 32 rows kernels (ROWS32_DEEP_MAX + 1), 2 049 tiles on 128 wave slots: 17 rounds"""
    ops = sched
    fam = FAMILIES['irn rows32']
    ops.set_sched_cus(1)
    got, scheds, ref, _, _ = fam.run(ops, 32769)
    assert scheds == [(2049, 8, 16)] * 2, scheds
    D._gpu_check('sched irn rows32', got, *ref())
    ops.set_sched_cus(0)
    assert torch.equal(got, fam.run(ops, 32769)[0])


@pytest.mark.gpu
def test_zz_report_tile_schedule_ratios():
    """(prints the wave slots W of each family on one CU and the largest error / bound ratio of the families of this file: the record the
    PR body reports)"""
    for k in sorted(SCHED_W):
        print(f'sched W {k:36s} {SCHED_W[k]}')
    for k in sorted(D.GPU_RATIOS):
        if k.startswith(('sched ', 'packed64 R')):
            print(f'fp64 ratio {k:36s} {D.GPU_RATIOS[k]:.3e}')
