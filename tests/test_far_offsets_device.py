"""Every conv family that addresses its gathered input with 32-bit buffer offsets, on levels (tests/far_offsets.py) whose rows lie past
byte offset 2^31, end one row below each limit (0xF0000000: rows / packed / children kernels; 0xFFFFFFF0: gather MFMA / row-split and the
fused VALU InceptionResNet) or reach it (the refusal), and the fallback kernels above 4 GiB.  The clump's outputs must lie within the fp64
bound of the definition and equal the oracle, every filler row must equal the one constant row, nothing may be non-finite, the expected
kernel must have run, and no case may hold more than 32 GiB.  One process, one case at a time."""
import functools
import time
import zlib

import numpy as np
import pytest
import torch

import far_offsets as F
import fp64_reference as R
from oracle import pcgc_oracle as orc
from test_fp64_definition import CHILD_FAMILIES, IRN_FAMILIES, _block_params, _features, _gpu_check, _profiled, _rand_w, _t, gpu_path  # noqa: F401

pytestmark = pytest.mark.gpu

MAX_BYTES = 32 << 30
REPORT = {}                                      # test id -> (seconds, peak GiB): the record DESIGN.md §5b carries


class _measured:
    def __init__(self, name):
        self.name = name

    def __enter__(self):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        self.t0 = time.perf_counter()

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated()
        REPORT[self.name] = (time.perf_counter() - self.t0, peak / 2 ** 30)
        print(f'far offsets {self.name:60s} {REPORT[self.name][0]:6.2f} s  peak {REPORT[self.name][1]:6.2f} GiB')
        torch.cuda.empty_cache()
        if exc[0] is None:
            assert peak <= MAX_BYTES, f'{self.name}: peak {peak / 2 ** 30:.1f} GiB'


def _dev():
    return torch.device('cuda:0')


# ------------------------------------------------------------------------------------------------ references on the clump alone (once per family)
CONV_FAMILIES = {
    # family: (kind, K, cin, cout, forced gather impl or None, far out= / residual=)
    'gather mfma': ('plain', 27, 64, 64, 2, True),
    'gather row_split': ('plain', 27, 32, 8, 6, True),
    'gather 16': ('plain', 27, 16, 16, None, True),
    'rows_conv': ('plain', 27, 32, 32, None, True),
    'packed64': ('plain', 27, 64, 64, None, False),
    'rows_down': ('down', 8, 32, 64, None, False),
}
IRN_FAR = ('rows64', 'rows32', 'rows32q4 v0', 'valu 16', 'valu 64')
IRN_ROWS = ('rows64', 'rows32', 'rows32q4 v0')
_PARAM_ORDER = ('conv0_0', 'conv0_1', 'conv1_0', 'conv1_1', 'conv1_2')


def _clump(kind):
    return F.make_level(8 * 1200, kind)          # (the clump and its maps do not depend on the level's size)


def _bounded(name, const, y0, e0):
    assert R.within(const, y0, e0) <= 1.0, f'{name}: the filler row is not the definition of an isolated zero voxel'
    return const


@functools.lru_cache(None)
def _ref(family):
    """-> dict: weights, clump features x, the fp64 value y and bound e, the oracle's answer, the filler row(s) `const`"""
    rng = np.random.default_rng(zlib.crc32(family.encode()))
    one = np.array([[0, 64, 64, 64]], np.int64)
    if family in CONV_FAMILIES:
        kind, K, cin, cout, _, far = CONV_FAMILIES[family]
        L = _clump(kind)
        nbr, _ = F.gather_map(L)
        x = _features(rng, len(L.rows), cin)
        W, b = _rand_w(rng, K, cin, cout)
        y, e = R._conv(nbr, x, R.zero_bound(x), W, b)
        oracle = orc.conv_gather(nbr.astype(np.int32), x, W, b)
        lone = np.full((K, 1), -1, np.int64)
        lone[13 if K == 27 else 0] = 0
        x0 = np.zeros((1, cin), np.float32)
        const = _bounded(family, orc.conv_gather(lone.astype(np.int32), x0, W, b), *R._conv(lone, x0, R.zero_bound(x0), W, b))
        ref = dict(W=W, b=b, x=x, y=y, e=e, oracle=oracle, const=const)
        if far:                                                                 # out = conv + residual (the residual of a filler is zero)
            r = rng.standard_normal(y.shape).astype(np.float32)
            ref['r'] = r
            ref['y'], ref['e'] = R.residual(y, e, r, R.zero_bound(r))
            ref['oracle'] = oracle + r
        return ref
    irn = 'irn' in family or family in IRN_FAR
    children = family in CHILD_FAMILIES
    L = _clump('children' if children else 'plain')
    C = IRN_FAMILIES[family][0] if family in IRN_FAR else (int(family.split(' ')[-1]) if family[-1].isdigit() else 16)
    x = _features(rng, len(L.rows), C)
    lone = R.children_coords(one * 2, 2) if children else one
    x0 = np.zeros((len(lone), C), np.float32)
    if irn:
        sd = _block_params(rng, C)
        y, e = R.inception_resnet(sd, 'b', L.coords, 1, x, R.zero_bound(x))
        oracle = orc.inception_resnet(sd, 'b', orc.Level(L.coords.astype(np.int32), 1), x)
        const = _bounded(family, orc.inception_resnet(sd, 'b', orc.Level(lone.astype(np.int32), 1), x0),
                         *R.inception_resnet(sd, 'b', lone, 1, x0, R.zero_bound(x0)))
        return dict(sd=sd, C=C, x=x, y=y, e=e, oracle=oracle, const=const)
    cout = 1 if 'cls' in family else C
    W, b = _rand_w(rng, 27, C, cout)
    y, e = R.conv3(L.coords, 1, x, R.zero_bound(x), W, b)
    oracle = orc.conv_gather(R.k3_map(L.coords, 1).astype(np.int32), x, W, b)
    const = _bounded(family, orc.conv_gather(R.k3_map(lone, 1).astype(np.int32), x0, W, b), *R.conv3(lone, 1, x0, R.zero_bound(x0), W, b))
    return dict(W=W, b=b, C=C, cout=cout, x=x, y=y, e=e, oracle=oracle, const=const)


def _params(sd):
    return [_t(sd[f'b.{nm}.{part}']) for nm in _PARAM_ORDER for part in ('kernel', 'bias')]


# ------------------------------------------------------------------------------------------------ one launch on a far level
def _untouched(buf, view, width):
    """the pad, the tail and the columns past `width` of a far operand are still NaN"""
    first = view.data_ptr() - buf.data_ptr()
    assert torch.isnan(buf[:first // 4]).all() and torch.isnan(buf[first // 4 + view.numel():]).all(), 'a store outside the payload'
    assert width == view.shape[1] or torch.isnan(view[:, width:]).all(), 'a store outside the output columns'


def _call(ops, family, L, nbr, force=None):
    """-> (callable that launches `family` on the far level -> output [n_out, C], expected kernel names or None, far output (buf, view) or None)"""
    ref = _ref(family)
    dev = _dev()
    if family in CONV_FAMILIES:
        kind, K, cin, cout, _, far = CONV_FAMILIES[family]
        xb, x = F.far_features(L, ref['x'], dev)
        W, b = _t(ref['W']), _t(ref['b'])
        keep = [xb]
        if far:
            rb_, res = F.far_features(L, ref['r'], dev, rows=L.out_rows)
            ob, ov = F.far_buffer(L.n_out, L.row_bytes, dev)
            out = ov[:, :cout]
            keep += [rb_, ob]
        if family.startswith('gather'):
            ops.set_conv_impl(-1 if force is None else force)
            return (lambda: ops.conv_gather(nbr, x, W, b, out=out, residual=res)), None, (ob, ov, keep)
        table = ops.child_conv_table(W)
        if family == 'rows_conv':
            return (lambda: ops.conv_rows(nbr, x, table, b, cout, out=out, residual=res)), {'k_rows_conv<2, 2>'}, (ob, ov, keep)
        if family == 'packed64':
            return (lambda: ops.conv_packed64(nbr, x, table, b)), {'k_conv_packed64'}, (None, None, keep)
        return (lambda: ops.conv_down_rows(nbr, x, table, b, cout)), {f'k_rows_down<{cin // 16}, {cout // 16}>'}, (None, None, keep)
    xb, x = F.far_features(L, ref['x'], dev)
    if family in IRN_FAR:
        params = _params(ref['sd'])
        names = IRN_FAMILIES[family][2]
        if family == 'rows64':
            tables = ops.child_irn_tables(params)
            fn = lambda: ops.irn_block_rows64(nbr, x, params, tables)
        elif family == 'rows32':
            tables = ops.rows_irn32_tables(params)
            fn = lambda: ops.irn_block_rows32(nbr, x, params, tables)
        elif family == 'rows32q4 v0':
            ops.set_rows_q4_variant(0)
            tables = ops.rows_q4_tables(params)
            fn = lambda: ops.irn_block_rows32_q4(nbr, x, params, tables)
        else:
            fn = lambda: ops.irn_block(nbr, x, params)
        return fn, names, (None, None, [xb])
    C = ref['C']
    if 'irn' in family:
        params = _params(ref['sd'])
        tables = ops.child_irn_tables(params)
        q4 = ops.child_q4_tables(params) if family == 'child_q4 irn' else None
        names = {'k_child_q4<0, 8, 2>', 'k_child_irn_b<16>'} if q4 is not None else {f'k_child_irn_a<{C}>', f'k_child_irn_b<{C}>'}
        return (lambda: ops.irn_block_child(nbr, x, params, tables, q4_table=q4)), names, (None, None, [xb])
    W, b, cout = _t(ref['W']), _t(ref['b']), ref['cout']
    if family == 'child_q4 cls':
        table = ops.child_q4_cls_table(W)
        return (lambda: ops.cls_child_q4(nbr, x, table, b)), None, (None, None, [xb])
    table = ops.child_cls_table(W) if cout == 1 else ops.child_conv_table(W)
    names = {f'k_child_cls<{C // 16}>' if cout == 1 else f'k_child_conv<{C // 16}, {C // 16}>'}
    if cout == 1:
        return (lambda: ops.conv_child(nbr, x, table, b, cout)), names, (None, None, [xb])
    ob, ov = F.far_buffer(L.n, L.row_bytes, dev)
    out = ov[:, :cout]
    return (lambda: ops.conv_child(nbr, x, table, b, cout, out=out)), names, (ob, ov, [xb, ob])


def _kind(family):
    return CONV_FAMILIES[family][0] if family in CONV_FAMILIES else ('children' if family in CHILD_FAMILIES else 'plain')


def _case_name(case, family):
    kind = _kind(family)
    return case if kind == 'plain' else f'{case} {kind}'


def _run(ops, case, family, force=None, want_impl=None):
    """one family on one case of F.CASES: the launch and every check of the first row of the table"""
    from pcgcv2_amd._lib import lib
    kind, n, rb = F.CASES[_case_name(case, family)]
    with _measured(f'{case} / {family}' + ('' if force is None else f' forced {force}')):
        L = F.make_level(n, kind, rb)
        nbr = F.far_map(L, _dev())
        fn, names, (ob, ov, keep) = _call(ops, family, L, nbr, force)
        ref = _ref(family)
        if names is None:
            got = fn()
            torch.cuda.synchronize()
        else:
            got, launched = _profiled(ops, fn)
            assert launched == names, launched
        if want_impl is not None:
            assert lib().pcgc_last_conv_impl() in want_impl, lib().pcgc_last_conv_impl()
        assert got.shape[0] == L.n_out
        rows = torch.as_tensor(L.out_rows, device=got.device)
        _gpu_check(f'far {family}', got[rows], ref['y'], ref['e'], ref['oracle'])
        assert F.check_fillers(L, got, ref['const']) == 0, f'{family}: filler rows differ from the constant row'
        if ob is not None:
            _untouched(ob, ov, got.shape[1])
        del got, nbr, fn, ob, ov, keep


def _refused(ops, case, family):
    kind, n, rb = F.CASES[_case_name(case, family)]
    with _measured(f'{case} / {family}'):
        L = F.make_level(n, kind, rb)
        nbr = F.far_map(L, _dev())
        fn, names, (ob, ov, keep) = _call(ops, family, L, nbr)
        with pytest.raises(ops.PcgcError, match='too large'):
            fn()
        torch.cuda.synchronize()
        if ob is not None:
            assert torch.isnan(ob).all(), 'a refused call wrote to its output'
        del nbr, fn, ob, ov, keep


# ------------------------------------------------------------------------------------------------ the cases
SIGN_FAMILIES = ['gather mfma', 'gather row_split', 'rows_conv', 'packed64', 'rows_down', *IRN_FAR, *CHILD_FAMILIES]
LIMIT_FAMILIES = ['rows_conv', 'packed64', 'rows_down', *IRN_ROWS, *CHILD_FAMILIES]


@pytest.mark.parametrize('family', SIGN_FAMILIES)
def test_rows_past_the_sign_bit(family, gpu_path):
    impl = CONV_FAMILIES[family][4] if family in CONV_FAMILIES else None
    _run(gpu_path, 'sign bit', family, force=impl, want_impl=None if impl is None else {impl})


@pytest.mark.parametrize('family', LIMIT_FAMILIES)
def test_last_row_below_the_rows_limit(family, gpu_path):
    _run(gpu_path, 'below LIMIT', family)


@pytest.mark.parametrize('family', LIMIT_FAMILIES)
def test_refused_at_the_rows_limit(family, gpu_path):
    _refused(gpu_path, 'at LIMIT', family)


@pytest.mark.parametrize('family,force', [('gather mfma', None), ('gather mfma', 2), ('gather row_split', None), ('gather row_split', 6)])
def test_last_row_below_the_gather_limit(family, force, gpu_path):
    _run(gpu_path, 'below GATHER_LIMIT', family, force=force, want_impl={CONV_FAMILIES[family][4]})


def test_fused_valu_block_below_the_gather_limit(gpu_path):
    _run(gpu_path, 'below GATHER_LIMIT', 'valu 64')


@pytest.mark.parametrize('family', ['gather mfma', 'gather row_split'])
def test_fallback_past_4_gib(family, gpu_path):
    _run(gpu_path, 'past 4 GiB', family, want_impl={0})


@pytest.mark.parametrize('case,impls', [('map gate below', {2}), ('map gate above', {0, 6})])
def test_map_size_gate(case, impls, gpu_path):
    _run(gpu_path, case, 'gather 16', want_impl=impls)


def test_children_row_stride_refused(gpu_path):
    """an absent neighbour is the offset 0xF0000000 plus up to 7 row strides and 256 bytes: a stride that carries the sum past 2^32 is refused
    (n_p = 2: the tensor itself is far below the size limit)"""
    ops = gpu_path
    ld = (0x10000000 - 256) // 28 // 4 * 4 + 4                    # the first multiple of 4 floats with 7 x 4 ld + 256 > 0x10000000
    assert 7 * 4 * ld + 256 > 0x10000000 >= 7 * 4 * (ld - 4) + 256 and 16 * ld * 4 < 0xF0000000
    with _measured('children row stride'):
        rng = np.random.default_rng(0)
        buf = torch.zeros(16 * ld, device=_dev())
        x = buf.view(16, ld)[:, :16]
        nbr = torch.full((27, 2), -1, dtype=torch.int32, device=_dev())
        nbr[13] = torch.arange(2, dtype=torch.int32, device=_dev())
        W, b = _rand_w(rng, 27, 16, 16)
        out = torch.full((16, 16), float('nan'), device=_dev())
        for call in (lambda: ops.conv_child(nbr, x, ops.child_conv_table(_t(W)), _t(b), 16, out=out),
                     lambda: ops.cls_child_q4(nbr, x, ops.child_q4_cls_table(_t(W[:, :, :1])), _t(b[:, :1]))):
            with pytest.raises(ops.PcgcError, match='row stride too large'):
                call()
        torch.cuda.synchronize()
        assert torch.isnan(out).all()
        del buf, x


def _real_level(n):
    """the plain level of n rows with real coordinates, built on the device: fillers on a spacing-2 lattice (isolated), the clump
    (translated clear of the lattice) at its scattered rows -> (Level, coordinates int32 [n, 4])"""
    L = F.make_level(n, 'plain')
    side = 257                                                                  # 257^3 lattice sites >= every n of the table
    assert side ** 3 >= n
    i = torch.arange(n, dtype=torch.int64, device=_dev())
    c = torch.stack([torch.zeros_like(i), 2 * (i % side), 2 * (i // side % side), 2 * (i // (side * side))], 1).to(torch.int32)
    clump = L.coords.copy()
    clump[:, 1:] += 1024 - clump[:, 1:].min()                                   # lattice coordinates end at 512
    c[torch.as_tensor(L.rows, device=_dev())] = _t(clump, torch.int32)
    return L, c


@pytest.mark.parametrize('n', [F.ROWS_LIMIT, F.ROWS_GATHER + F.W + F.GUARD], ids=['at LIMIT', 'past 4 GiB'])
@pytest.mark.parametrize('module', ['conv', 'irn'])
def test_modules_past_the_limits(module, n, gpu_path):
    """beyond LIMIT the generic kernels take over: MinkowskiConvolution(64, 64) and InceptionResNet(64) on a SparseTensor of real
    coordinates launch what dispatch.select names, and compute the same"""
    from pcgcv2_amd import dispatch
    from pcgcv2_amd._lib import lib
    from pcgcv2_amd.autoencoder import InceptionResNet
    from pcgcv2_amd.nn import MinkowskiConvolution
    from pcgcv2_amd.sparse import CoordMap, SparseTensor
    ops = gpu_path
    ref = _ref('packed64' if module == 'conv' else 'valu 64')
    past = n * F.ROW_BYTES >= F.GATHER_LIMIT
    with _measured(f'modules {"past 4 GiB" if past else "at LIMIT"} / {module}'):
        L, coords = _real_level(n)
        xb, x = F.far_features(L, ref['x'], _dev())
        assert x.is_contiguous() and x.shape[0] * x.stride(0) * 4 >= dispatch.LIMIT
        xs = SparseTensor(x, coordinate_map=CoordMap(coords, 1, unique=True))
        assert torch.equal(xs.cmap.k3, F.far_map(L, _dev())), 'the level of real coordinates is not the level the generator describes'
        if module == 'conv':
            assert dispatch.select('conv3', (64, 64), n, extent=n * 256).family == 'gather'
            mod = MinkowskiConvolution(64, 64, 3).to(_dev())
            with torch.no_grad():
                mod.kernel.copy_(_t(ref['W']))
                mod.bias.copy_(_t(ref['b']))
                got, names = _profiled(ops, lambda: mod(xs).F)
            assert names == {'k3 gather conv Cin=64 Cout=64'}, names
            assert lib().pcgc_last_conv_impl() == (0 if past else 2)
        else:
            want = 'unfused' if past else 'valu'
            assert dispatch.select('irn', (64,), n, extent=n * 256).family == want
            mod = InceptionResNet(64).to(_dev())
            with torch.no_grad():
                for nm in _PARAM_ORDER:
                    getattr(mod, nm).kernel.copy_(_t(ref['sd'][f'b.{nm}.kernel']))
                    getattr(mod, nm).bias.copy_(_t(ref['sd'][f'b.{nm}.bias']))
                got, names = _profiled(ops, lambda: mod(xs).F)
            if past:
                assert names and all(nm.startswith('k3 gather conv') for nm in names), names
            else:
                assert names == IRN_FAMILIES['valu 64'][2], names
        rows = torch.as_tensor(L.out_rows, device=got.device)
        _gpu_check(f'far module {module}', got[rows], ref['y'], ref['e'], ref['oracle'])
        assert F.check_fillers(L, got, ref['const']) == 0, f'{module}: filler rows differ from the constant row'
        _untouched(xb, xb[F.PAD_BYTES // 4:F.PAD_BYTES // 4 + n * F.LD].view(n, F.LD), F.LD)
        del got, xs, x, xb, coords, mod


def test_zz_report_far_offsets():
    """(prints duration and peak memory per case: the record DESIGN.md carries)"""
    for k, (s, g) in REPORT.items():
        print(f'far offsets {k:60s} {s:6.2f} s  peak {g:6.2f} GiB')
