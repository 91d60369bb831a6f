"""Derived weight tables follow weight updates and streams, on the device.

Every kernel family that reads a cached, re-laid-out copy of the weights (MFMA fragment tables of a conv, block tables of an InceptionResNet,
the bottleneck's packed parameters and CDF tables) runs once, then the weights change through one of the routes of
tests/test_weight_updates_cpu.py, then it runs again on the SAME module object.  Before the update the output must equal the CPU oracle on
the old weights, after it the oracle on the new weights, bit for bit, and stay within the fp64 definition's bound; the two oracle results must
differ, so a stale table cannot pass.  Expected values never come from the code under test.

The children-level families are dispatched from 8192 rows on (dispatch.TABLE; no PathConfig field lowers that), so at 3 and 129 parents they
are reached the way nn.py / autoencoder.py reach them: the module's own cache (`_table` / `_tables`) feeding the family's op.

Streams: a table is built by torch ops on the builder's stream.  The deterministic test builds it behind a device-side sleep on stream A and
uses the same module on stream B while A still sleeps: B must have been ordered after the build.
    SLEEP_CYCLES = 100 000 000 cycles of torch.cuda._sleep: measured 41.7 ms on the MI355X (10 M cycles: 4.17 ms) against 0.1-0.4 ms of
    host time for the two module calls (first use after an update, with the table build: 0.04-0.36 ms, 0.89 ms for a process's very first
    block; the second stream's call: 0.02-0.05 ms, 0.17 ms at most): a margin of 40 at the very least, 100-400 typically."""
import gc
import zlib

import numpy as np
import pytest
import torch

import eval_reference as er
import fp64_reference as R
import test_fp64_definition as T
import test_weight_updates_cpu as U
from oracle import pcgc_oracle as orc
from pcgcv2_amd import synthetic

pytestmark = pytest.mark.gpu

SLEEP_CYCLES = 100_000_000
ONE_ROUNDING = 2.0 ** -23
BOUND32 = np.float32(1e-9)
GATES = dict(ROWS_IRN64_MIN=1, ROWS_IRN32_MIN=1, ROWS_Q4_MIN=1, ROWS_CONV_MIN=1, ROWS_DOWN_MIN=1, PACKED_CONV64_MIN=1, CHILD_Q4_MIN_PARENTS=1)
PLAIN = (129, 1025)              # either side of a 16-row and a 64-row tile
PARENTS = (3, 129)
_t, _dev = T._t, T._dev


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


def _bias_only(mod, rng):
    with torch.no_grad():
        for name, p in mod.named_parameters():
            if name.endswith('bias'):
                p.add_(0.25)


ROUTES = dict(U.ROUTES, **{'h bias only': _bias_only})


def _churn(mod):
    """(i) allocate and free blocks of every parameter's size (fp32 and fp16), so that the caching allocator is in the state where a new
    tensor can be handed a block that was just freed; whether it was is not asserted — the outcome is"""
    for p in mod.parameters():
        for dt in (torch.float32, torch.float16):
            blocks = [torch.empty(p.shape, dtype=dt, device=p.device) for _ in range(3)]
            del blocks
    gc.collect()


def _apply(route, mod, rng):
    _churn(mod)
    ROUTES[route](mod, rng)
    _churn(mod)


def _np(t):
    return t.detach().cpu().numpy()


def _set(conv, W, b):
    with torch.no_grad():
        conv.kernel.copy_(_t(W))
        conv.bias.copy_(_t(b))


_LEVELS = {}


def _plain(n):
    if ('plain', n) not in _LEVELS:
        c4 = T._prefix(n)
        _LEVELS['plain', n] = (c4, R.k3_map(c4, 1))
    return _LEVELS['plain', n]


def _kids(n_p):
    """children level of n_p parents -> (parent coords, children coords, children k3 map)"""
    if ('kids', n_p) not in _LEVELS:
        pc = R.down_coords(T._shell4('shell9'), 1)[:n_p]
        kc = R.children_coords(pc, 2)
        _LEVELS['kids', n_p] = (pc, kc, R.k3_map(kc, 1))
    return _LEVELS['kids', n_p]


def _sparse(c4, x, stride=1):
    from pcgcv2_amd.sparse import CoordMap, SparseTensor
    return SparseTensor(_t(x), coordinate_map=CoordMap(_t(c4, torch.int32), stride, unique=True))


def _parent_map(pc):
    from pcgcv2_amd.sparse import CoordMap
    parent = CoordMap(_t(pc, torch.int32), 2, unique=True)
    return parent


# ------------------------------------------------------------------------------------------------ conv families
# family: (kind, cin, cout, K).  kind 'module': MinkowskiConvolution.forward on a plain level with the gates lowered; 'child' / 'q4cls': the
# module's `_table` feeding the children-level op; 'gather <impl>' / 'unit' / 'up2': the controls that hold no table.
CONV_FAMILIES = {
    'child conv 16': ('child', 16, 16, 27), 'child conv 32': ('child', 32, 32, 27), 'cls 16': ('child', 16, 1, 27), 'cls 32': ('child', 32, 1, 27),
    'cls 64': ('child', 64, 1, 27), 'child_q4 cls': ('q4cls', 16, 1, 27), 'packed64': ('module', 64, 64, 27), 'rows_conv': ('module', 32, 32, 27),
    'rows_down 16-32': ('module', 16, 32, 8), 'rows_down 32-64': ('module', 32, 64, 8), 'rows_down 64-32': ('module', 64, 32, 8),
    'gather valu': ('gather 0', 16, 16, 27), 'gather mfma': ('gather 2', 16, 16, 27), 'gather row_split': ('gather 6', 16, 16, 27),
    'unit': ('unit', 1, 16, 27), 'conv_up2 mfma_lds_table': ('up2', 64, 32, 8),
}


def _conv_levels(family, rng):
    """-> [(name, call(conv) -> tensor, want_names or None, oracle(W, b), fp64(W, b) -> (y, e), after(ops))]"""
    from pcgcv2_amd import ops
    from pcgcv2_amd._lib import lib
    kind, cin, cout, K = CONV_FAMILIES[family]
    out = []
    if kind in ('child', 'q4cls'):
        for n_p in PARENTS:
            pc, kc, nbr = _kids(n_p)
            x = T._features(rng, len(kc), cin)
            parent = _parent_map(pc)
            if kind == 'q4cls':
                call = lambda conv, parent=parent, x=x: ops.cls_child_q4(parent.k3, T._poisoned(x), conv._table(ops.child_q4_cls_table), conv.bias)
                names = {'k_child_q4<1, 8, 2>'}
            else:
                build = ops.child_cls_table if cout == 1 else ops.child_conv_table
                call = lambda conv, parent=parent, x=x, build=build: ops.conv_child(parent.k3, T._poisoned(x), conv._table(build), conv.bias, cout)
                names = {f'k_child_cls<{cin // 16}>' if cout == 1 else f'k_child_conv<{cin // 16}, {cin // 16}>'}
            out.append((f'{n_p} parents', call, names, lambda W, b, nbr=nbr, x=x: orc.conv_gather(nbr.astype(np.int32), x, W, b),
                        lambda W, b, kc=kc, x=x: R.conv3(kc, 1, x, R.zero_bound(x), W, b), None))
        return out
    for n in PLAIN:
        c4, nbr = _plain(n)
        if kind == 'up2':
            x = T._features(rng, n, cin)
            call = lambda conv, c4=c4, x=x: conv(_sparse(c4 * np.array([1, 2, 2, 2]), x, 2), relu=False).F
            out.append((f'{n} rows', call, None, lambda W, b, x=x: orc.conv_up2(x, W, b),
                        lambda W, b, c4=c4, x=x: R.up(c4 * np.array([1, 2, 2, 2]), 2, x, R.zero_bound(x), W, b)[1:], None))
            continue
        if K == 8:
            coarse = R.down_coords(c4, 1)
            dmap = R.neighbour_map(coarse, c4, R.offsets(2))
            x = T._features(rng, n, cin)

            def call(conv, c4=c4, x=x, coarse=coarse):
                y = conv(_sparse(c4, x))
                np.testing.assert_array_equal(_np(y.C), coarse)
                return y.F
            out.append((f'{n} rows', call, {f'k_rows_down<{cin // 16}, {cout // 16}>'}, lambda W, b, dmap=dmap, x=x: orc.conv_gather(dmap.astype(np.int32), x, W, b),
                        lambda W, b, dmap=dmap, x=x: R._conv(dmap, x, R.zero_bound(x), W, b), None))
            continue
        if kind == 'unit':
            from pcgcv2_amd.sparse import SparseTensor
            x = np.ones((n, 1), np.float32)

            def call(conv, c4=c4):
                xs = SparseTensor(torch.ones((len(c4), 1)), coordinates=_t(c4, torch.int32), tensor_stride=1, device=_dev())
                assert xs.has_unit_features()
                return conv(xs).F
            names = None
        else:
            x = T._features(rng, n, cin)
            call = lambda conv, c4=c4, x=x: conv(_sparse(c4, x)).F
            names = {'packed64': {'k_conv_packed64'}, 'rows_conv': {'k_rows_conv<2, 2>'}}.get(family)
        after = None
        if kind.startswith('gather'):
            impl = int(kind.split(' ')[1])
            after = lambda impl=impl, n=n: (impl, lib().pcgc_last_conv_impl())
        out.append((f'{n} rows', call, names, lambda W, b, nbr=nbr, x=x: orc.conv_gather(nbr.astype(np.int32), x, W, b),
                    lambda W, b, nbr=nbr, x=x: R._conv(nbr, x, R.zero_bound(x), W, b), after))
    return out


def _make_conv(family, rng):
    from pcgcv2_amd.nn import MinkowskiConvolution, MinkowskiGenerativeConvolutionTranspose
    kind, cin, cout, K = CONV_FAMILIES[family]
    if kind == 'up2':
        conv = MinkowskiGenerativeConvolutionTranspose(cin, cout, 2, 2)
    else:
        conv = MinkowskiConvolution(cin, cout, 2 if K == 8 else 3, 2 if K == 8 else 1)
    conv = conv.to(_dev())
    _set(conv, *T._rand_w(rng, K, cin, cout))
    return conv


def _run_conv_round(ops, family, conv, levels, tag):
    """one pass over the levels with the module's CURRENT weights -> [oracle result per level]"""
    W, b = _np(conv.kernel), _np(conv.bias)
    wants = []
    for name, call, names, oracle, fp64, after in levels:
        with torch.no_grad():
            got, launched = T._profiled(ops, lambda: call(conv))
        if names is not None:
            assert launched == names, (family, tag, name, launched)
        if after is not None:
            want_impl, got_impl = after()
            assert got_impl == want_impl, (family, tag, name, got_impl)
        want = oracle(W, b)
        y, e = fp64(W, b)
        T._gpu_check(f'{family} ({tag})', got, y, e, want)
        wants.append(want)
    return wants


@pytest.mark.parametrize('route', list(ROUTES))
@pytest.mark.parametrize('family', list(CONV_FAMILIES))
def test_conv_families_follow_the_weights(family, route, gpu_path):
    ops = gpu_path
    kind = CONV_FAMILIES[family][0]
    rng = np.random.default_rng(zlib.crc32(family.encode()))
    ops.configure(**GATES)
    if kind.startswith('gather'):
        ops.set_conv_impl(int(kind.split(' ')[1]))
    if kind == 'up2':
        ops.set_up2_impl(2)
    conv = _make_conv(family, rng)
    levels = _conv_levels(family, rng)
    before = _run_conv_round(ops, family, conv, levels, 'before')
    _apply(route, conv, np.random.default_rng(len(route)))
    if kind.startswith('gather'):
        ops.set_conv_impl(int(kind.split(' ')[1]))
    after = _run_conv_round(ops, family, conv, levels, route)
    for a, b in zip(before, after):
        assert not np.array_equal(a, b), f'{family} / {route}: the update does not change the expected output — the case has no teeth'


# ------------------------------------------------------------------------------------------------ InceptionResNet families
IRN_FAMILIES = {
    # family: (C, kind, PathConfig changes on top of GATES, kernel names)
    'rows64': (64, 'module', dict(), {'k_rows_irn_a64', 'k_rows_irn_b64'}),
    'rows32': (32, 'module', dict(ROWS_Q4=False), {'k_rows_irn_a32', 'k_rows_irn_b32'}),
    'rows32q4 v0': (32, 'module', dict(), {'k_rows_q4_a32', 'k_rows_q4_b32'}),
    'child 16': (16, 'child', dict(), {'k_child_irn_a<16>', 'k_child_irn_b<16>'}),
    'child 32': (32, 'child', dict(), {'k_child_irn_a<32>', 'k_child_irn_b<32>'}),
    'child_q4 16': (16, 'child_q4', dict(), {'k_child_q4<0, 8, 2>', 'k_child_irn_b<16>'}),
    'valu 16': (16, 'module', dict(), {'k_irn_a_split<16>', 'k_irn_b_split<16>'}),                  # control: reads the parameters directly
}
CONVS5 = ('conv0_0', 'conv0_1', 'conv1_0', 'conv1_1', 'conv1_2')


def _block_sd(blk):
    sd = {}
    for nm in CONVS5:
        sd[f'b.{nm}.kernel'], sd[f'b.{nm}.bias'] = _np(getattr(blk, nm).kernel), _np(getattr(blk, nm).bias)
    return sd


def _block_params_list(blk):
    return [p for nm in CONVS5 for p in (getattr(blk, nm).kernel, getattr(blk, nm).bias)]


def _irn_levels(family, rng):
    from pcgcv2_amd import ops
    C, kind, _, _ = IRN_FAMILIES[family]
    out = []
    if kind == 'module':
        for n in PLAIN:
            c4, _ = _plain(n)
            x = T._features(rng, n, C)
            out.append((f'{n} rows', c4, x, lambda blk, c4=c4, x=x: blk(_sparse(c4, x)).F))
        return out
    for n_p in PARENTS:
        pc, kc, _ = _kids(n_p)
        x = T._features(rng, len(kc), C)
        parent = _parent_map(pc)

        def call(blk, parent=parent, x=x):
            params = _block_params_list(blk)
            tables = blk._tables('child', ops.child_irn_tables, params)
            q4 = blk._tables('q4', ops.child_q4_tables, params) if kind == 'child_q4' else None
            return ops.irn_block_child(parent.k3, _t(x), params, tables, q4_table=q4)
        out.append((f'{n_p} parents', kc, x, call))
    return out


def _run_irn_round(ops, family, blk, levels, tag):
    names = IRN_FAMILIES[family][3]
    sd = _block_sd(blk)
    wants = []
    for name, c4, x, call in levels:
        with torch.no_grad():
            got, launched = T._profiled(ops, lambda: call(blk))
        assert launched == names, (family, tag, name, launched)
        want = orc.inception_resnet(sd, 'b', orc.Level(c4.astype(np.int32), 1), x)
        y, e = R.inception_resnet(sd, 'b', c4, 1, x, R.zero_bound(x))
        T._gpu_check(f'irn {family} ({tag})', got, y, e, want)
        wants.append(want)
    return wants


@pytest.mark.parametrize('route', list(ROUTES))
@pytest.mark.parametrize('family', list(IRN_FAMILIES))
def test_inception_resnet_families_follow_the_weights(family, route, gpu_path):
    ops = gpu_path
    C, kind, changes, _ = IRN_FAMILIES[family]
    rng = np.random.default_rng(zlib.crc32(family.encode()))
    ops.configure(**dict(GATES, **changes))
    ops.set_rows_q4_variant(0)
    blk, _ = T._block(rng, C)
    levels = _irn_levels(family, rng)
    before = _run_irn_round(ops, family, blk, levels, 'before')
    _apply(route, blk, np.random.default_rng(len(route)))
    after = _run_irn_round(ops, family, blk, levels, route)
    for a, b in zip(before, after):
        assert not np.array_equal(a, b), f'{family} / {route}: no teeth'


# ------------------------------------------------------------------------------------------------ bottleneck
def _eb_dev():
    return U._eb().to(_dev())


def _eb_params(eb):
    return orc.pack_eb_params(U._eb_sd(eb))


def _eb_inputs():
    rng = np.random.default_rng(12)
    y_int = np.rint(rng.normal(0, 3.0, (257, 8))).clip(-9, 7).astype(np.float32)
    y_int[0, 0], y_int[-1, -1] = -9, 7
    return y_int, (rng.standard_normal((1025, 8)) * 3).astype(np.float32)


def _check_bottleneck(eb, tag):
    """likelihood through the module against the fp64 restatement (one rounding) and, at integers, the oracle bit for bit; host_table in the
    three modes against the oracle's tables, the SAME ranges every time; a compress / decompress round through the tables -> what a stale
    copy would change: (likelihood at integers, reference table, device table, bytes)"""
    params = _eb_params(eb)
    y_int, y_real = _eb_inputs()
    _, lik = eb(_t(y_real), quantize_mode=None)
    lik64 = er.likelihood(params, y_real)
    rel = float(np.max(np.abs(_np(lik).astype(np.float64) - lik64) / lik64))
    assert rel <= ONE_ROUNDING, f'{tag}: likelihood {rel:.3e} from the fp64 restatement'
    _, lik_i = eb(_t(y_int), quantize_mode=None)
    want_i = np.maximum(orc.likelihood(params, -9.0, 7.0), BOUND32)[(y_int + 9).astype(np.int64), np.arange(8)[None, :]]
    np.testing.assert_array_equal(_np(lik_i), want_i, err_msg=tag)
    ref = orc.cdf_table_ref32(params, np.float32(-9), np.float32(7))
    dev_table = orc.cdf_u16(orc.cdf_float(params, -9.0, 7.0))
    keep = eb.table_mode
    try:
        for mode, want in (('reference', ref), ('reference-python', ref), ('device', dev_table)):
            eb.table_mode = mode
            for lo, hi, w in ((-9, 7, want), (-2, 3, None)):
                if w is None:
                    w = orc.cdf_table_ref32(params, np.float32(lo), np.float32(hi)) if mode != 'device' else orc.cdf_u16(orc.cdf_float(params, float(lo), float(hi)))
                got = eb.host_table(np.float32(lo), np.float32(hi), _dev())
                np.testing.assert_array_equal(got, w, err_msg=f'{tag}: host_table {mode} [{lo}, {hi}]')
                assert eb.host_table(np.float32(lo), np.float32(hi), _dev()) is got
    finally:
        eb.table_mode = keep
    data, lo, hi = eb.compress(_t(y_int))
    want_bytes, wlo, whi = orc.eb_compress(params, y_int)
    assert data == want_bytes and float(lo[0]) == float(wlo) and float(hi[0]) == float(whi), tag
    back = eb.decompress(data, lo, hi, y_int.shape, 8, device=_dev())
    np.testing.assert_array_equal(_np(back), y_int + np.float32(0))
    return _np(lik_i), ref, dev_table, data


def _differs(a, b):
    """the likelihoods, the reference table and the device table all differ (the bytes then differ too, but need not)"""
    return all(not np.array_equal(x, y) for x, y in zip(a[:3], b[:3]))


@pytest.mark.parametrize('route', list(ROUTES))
def test_bottleneck_follows_every_route(route):
    eb = _eb_dev()
    old = _check_bottleneck(eb, 'before')
    _churn(eb)
    if route == 'h bias only':
        with torch.no_grad():
            eb._biases[1].add_(0.3)
    else:
        U.eb_route(eb, route, np.random.default_rng(len(route)))
    _churn(eb)
    new = _check_bottleneck(eb, route)
    assert _differs(old, new), f'{route}: no teeth'


@pytest.mark.parametrize('key', U.EB_KEYS)
def test_bottleneck_follows_each_of_the_12_tensors(key):
    eb = _eb_dev()
    old = _check_bottleneck(eb, 'before')
    with torch.no_grad():
        eb.get_parameter(key).add_(0.05 if 'bias' not in key.lower() else 0.3)
    new = _check_bottleneck(eb, key)
    assert _differs(old, new), f'{key}: no teeth'


# ------------------------------------------------------------------------------------------------ whole model
DEV = torch.device('cuda:0')
START = dict(seed=4321, gain=30.0)
_ORACLE = {}


def _model(sd):
    from pcgcv2_amd.pcc_model import PCCModel
    m = PCCModel().to(DEV)
    m.load_state_dict(sd)
    return m


def _model_sd_np(model):
    return {k: _np(v) for k, v in model.state_dict().items()}


def _oracle_code(sd_np, cloud):
    """orc.encode + orc.decode of a cloud under these weights, computed once per distinct weights"""
    key = (cloud, zlib.crc32(b''.join(np.ascontiguousarray(sd_np[k]).tobytes() for k in sorted(sd_np))))
    if key not in _ORACLE:
        c4 = T._shell4(cloud).astype(np.int32)
        enc = orc.encode(sd_np, c4)
        _ORACLE[key] = (enc, orc.decode(sd_np, enc['coords8'], enc['F'], enc['H'], enc['num_points']))
    return _ORACLE[key]


def _input(cloud):
    from pcgcv2_amd.sparse import SparseTensor
    c4 = T._shell4(cloud).astype(np.int32)
    return SparseTensor(torch.ones((len(c4), 1)), coordinates=_t(c4, torch.int32), tensor_stride=1, device=DEV)


def _code_and_check(coder, x, cloud, postfix, tag):
    """encode + decode with this Coder / model: the streams and the decoded cloud must be the oracle's under the model's CURRENT weights"""
    enc, dec = _oracle_code(_model_sd_np(coder.model), cloud)
    coder.encode(x, postfix=postfix)
    stem = coder.filename + postfix
    for k in ('F', 'H', 'num_points'):
        assert open(f'{stem}_{k}.bin', 'rb').read() == enc[k], f'{tag}: {k}.bin differs from the oracle under the current weights'
    key = lambda a: a[np.lexsort((a[:, 0], a[:, 1], a[:, 2]))]
    np.testing.assert_array_equal(key(coder.coordinate_coder.decode(postfix=postfix)), key(enc['coords8']), err_msg=f'{tag}: C.bin')
    out = coder.decode(postfix=postfix)
    np.testing.assert_array_equal(_np(out.C), dec, err_msg=f'{tag}: decoded cloud')
    return enc


def _gen(seed=77):
    return torch.Generator(device=DEV).manual_seed(seed)


def _trainer(model, tmp_path):
    from pcgcv2_amd.trainer import Trainer, TrainingConfig
    import logging
    t = Trainer(TrainingConfig(logdir=str(tmp_path / 'log'), ckptdir=str(tmp_path / 'ckpt'), init_ckpt='', alpha=1., beta=1., lr=8e-4, check_time=1e9), model)
    t.logger.setLevel(logging.WARNING)
    return t


def _target():
    """the synthetic weights at gain 50, on the device"""
    return {k: v.to(DEV) for k, v in synthetic.synthetic_state_dict().items()}


def _model_route(route, model, x, tmp_path):
    tgt = _target()
    named = dict(model.named_parameters())
    if route.startswith('a adam'):
        kind = 'default' if route == 'a adam' else route.split(' ')[-1]
        why = U.adam_rejected(kind, DEV)
        if why is not None:
            pytest.skip(f'torch.optim.Adam({kind}=True) is not accepted by this build: {why}')
        opt = torch.optim.Adam(model.parameters(), lr=8e-4, **({} if kind == 'default' else {kind: True}))
        _trainer(model, tmp_path).step(x, opt, generator=_gen())
    elif route == 'b copy_':
        with torch.no_grad():
            for k, p in named.items():
                p.copy_(tgt[k])
    elif route == 'b mul_':
        with torch.no_grad():
            for k, p in named.items():
                if not k.startswith('entropy_bottleneck'):
                    p.mul_(1.03)
            model.entropy_bottleneck._biases[0].mul_(1.03)
    elif route.startswith('c load'):
        model.load_state_dict(tgt, assign=route.endswith('assign'))
    elif route == 'd data=':
        for k, p in named.items():
            p.data = tgt[k].clone()
    elif route == 'd vector_to_parameters':
        torch.nn.utils.vector_to_parameters(torch.cat([tgt[k].reshape(-1) for k in named]), list(named.values()))
    elif route == 'e half float':
        model.half().float()
    elif route == 'f data.mul_ + weights_changed':
        for k, p in named.items():
            if not k.startswith('entropy_bottleneck'):
                p.data.mul_(0.97)
        model.entropy_bottleneck._biases[0].data.mul_(0.97)
        model.weights_changed()
    elif route == 'f data.copy_ + weights_changed':
        for k, p in named.items():
            p.data.copy_(tgt[k])
        model.weights_changed()
    elif route == 'g two updates':
        with torch.no_grad():
            for k, p in named.items():
                p.copy_(0.5 * (p + tgt[k]))
        for k, p in named.items():
            p.data = tgt[k].clone()
    elif route == 'h bias only':
        with torch.no_grad():
            for k, p in named.items():
                if k.endswith('.bias') and not k.startswith('entropy_bottleneck'):
                    p.add_(0.02)
    else:
        raise KeyError(route)


@pytest.mark.parametrize('gates', ['lowered', 'defaults'])
@pytest.mark.parametrize('route', list(ROUTES))
def test_coder_follows_the_weights(route, gates, gpu_path, tmp_path):
    """Coder.encode / decode on shell7, the update, then the SAME Coder and model objects again"""
    from pcgcv2_amd.coder import Coder
    ops = gpu_path
    if gates == 'lowered':
        ops.configure(**GATES)
    model = _model(synthetic.synthetic_state_dict(**START))
    x = _input('shell7')
    coder = Coder(model, str(tmp_path / 'w'))
    old = _code_and_check(coder, x, 'shell7', '_old', 'before')
    _churn(model)
    _model_route(route, model, x, tmp_path)
    _churn(model)
    new = _code_and_check(coder, x, 'shell7', '_new', route)
    assert new['F'] != old['F'], f'{route}: no teeth'
    _code_and_check(coder, x, 'shell7', '_again', route + ' (again)')


@pytest.mark.parametrize('gates', ['lowered', 'defaults'])
def test_train_steps_alternate_with_coding_and_fused_equals_unfused(gates, gpu_path, tmp_path):
    """three rounds of Trainer.step / encode / decode on one model: after every step the fused forward (tables) equals forward_train (the
    unfused graph, no tables) bit for bit for the same generator state, and the coder agrees with the oracle on the updated weights"""
    from pcgcv2_amd.coder import Coder
    ops = gpu_path
    if gates == 'lowered':
        ops.configure(**GATES)
    model = _model(synthetic.synthetic_state_dict())
    x = _input('shell6')
    coder = Coder(model, str(tmp_path / 't'))
    trainer = _trainer(model, tmp_path)
    opt = trainer.set_optimizer()
    seen = [_code_and_check(coder, x, 'shell6', '_0', 'before')['F']]
    model(x, training=True, generator=_gen())                            # (the fused training forward has run with the old weights too)
    for rnd in range(1, 4):
        trainer.step(x, opt, generator=_gen())
        fused = model(x, training=True, generator=_gen())
        unfused = model.forward_train(x, generator=_gen())
        assert torch.equal(fused['likelihood'], unfused['likelihood']) and torch.equal(fused['prior'].F, unfused['prior'].F), rnd
        assert torch.equal(fused['out'].C, unfused['out'].C), rnd
        for a, b in zip(fused['out_cls_list'], unfused['out_cls_list']):
            assert torch.equal(a.C, b.C) and torch.equal(a.F, b.F.detach()), rnd
        seen.append(_code_and_check(coder, x, 'shell6', f'_{rnd}', f'round {rnd}')['F'])
    assert len(set(seen)) == 4, 'a training step left the stream unchanged: no teeth'


# ------------------------------------------------------------------------------------------------ streams, deterministic
def _warm_indices(ops):
    """every weight-independent index tensor the table builders gather through (ops._TABLE_INDEX), built from throwaway weights and complete
    before anything sleeps: the stream test may make a kernel read wrong FLOATS, never an uninitialised index"""
    rng = np.random.default_rng(0)
    for C in (16, 32, 64):
        W = _t(T._rand_w(rng, 27, C, 1)[0])
        ops.child_cls_table(W)
        blk, _ = T._block(rng, C)
        ops.child_irn_tables(_block_params_list(blk))
    ops.child_q4_cls_table(_t(T._rand_w(rng, 27, 16, 1)[0]))
    blk, _ = T._block(rng, 32)
    ops.rows_irn32_tables(_block_params_list(blk))
    ops.rows_q4_tables(_block_params_list(blk))
    torch.cuda.synchronize()


def _poison_fp32(stream, sizes):
    """same-sized fp32 blocks full of NaN, allocated and freed on the building stream: a table that is read before it is written reads NaN"""
    with torch.cuda.stream(stream):
        blocks = [torch.full((n,), float('nan'), dtype=torch.float32, device=DEV) for n in sizes for _ in range(3)]
        stream.synchronize()
        del blocks


@pytest.mark.parametrize('what', ['conv table (rows_conv)', 'irn tables (rows32)', 'packed_params'])
def test_second_stream_is_ordered_after_the_table_build(what, gpu_path):
    ops = gpu_path
    ops.configure(**dict(GATES, ROWS_Q4=False))
    rng = np.random.default_rng(21)
    n = 1025
    c4, nbr = _plain(n)
    _warm_indices(ops)
    if what.startswith('conv'):
        mod = _make_conv('rows_conv', rng)
        x = T._features(rng, n, 32)
        xs = _sparse(c4, x)
        run = lambda: mod(xs).F
        oracle = lambda: orc.conv_gather(nbr.astype(np.int32), x, _np(mod.kernel), _np(mod.bias))
        sizes = [mod.kernel.numel()]
    elif what.startswith('irn'):
        mod, _ = T._block(rng, 32)
        x = T._features(rng, n, 32)
        xs = _sparse(c4, x)
        run = lambda: mod(xs).F
        oracle = lambda: orc.inception_resnet(_block_sd(mod), 'b', orc.Level(c4.astype(np.int32), 1), x)
        sizes = [t.numel() for t in ops.rows_irn32_tables(_block_params_list(mod))]
    else:
        mod = _eb_dev()
        y_int, _ = _eb_inputs()
        yt = _t(y_int)
        run = lambda: mod(yt, quantize_mode=None)[1]
        oracle = lambda: np.maximum(orc.likelihood(_eb_params(mod), -9.0, 7.0), BOUND32)[(y_int + 9).astype(np.int64), np.arange(8)[None, :]]
        sizes = [352, 3, 9, 24]
    with torch.no_grad():
        np.testing.assert_array_equal(_np(run()), oracle())              # first use, old weights: the level's maps and every index now exist
        before = oracle()
        _apply('b copy_' if not what.startswith('packed') else 'b mul_', mod, rng)
        want = oracle()
        assert not np.array_equal(want, before)
        torch.cuda.synchronize()
        A, B = torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)
        _poison_fp32(A, sizes)
        torch.cuda.synchronize()
        built = torch.cuda.Event()
        with torch.cuda.stream(A):
            torch.cuda._sleep(SLEEP_CYCLES)
            out_a = run()                                                # first use after the update: builds the table behind the sleep
            built.record(A)
        with torch.cuda.stream(B):
            out_b = run()
        still_asleep = not built.query()
        torch.cuda.synchronize()
    assert still_asleep, 'precondition: stream A had finished before stream B\'s call returned — the sleep is too short to test anything'
    got_b, got_a = _np(out_b), _np(out_a)
    assert np.isfinite(got_b).all(), f'{what}: stream B read a table that was not written yet'
    np.testing.assert_array_equal(got_b, want, err_msg=f'{what}: stream B')
    np.testing.assert_array_equal(got_a, want, err_msg=f'{what}: stream A')


# ------------------------------------------------------------------------------------------------ streams, threaded
def _units(names):
    return [(f'u{i}', _input(nm)) for i, nm in enumerate(names)]


def _same_files(a_dir, b_dir, units):
    from pcgcv2_amd.coder import STREAMS
    for name, _ in units:
        for suffix in STREAMS:
            assert (a_dir / f'f_{name}{suffix}').read_bytes() == (b_dir / f'f_{name}{suffix}').read_bytes(), (name, suffix)


def test_frames_in_flight_on_a_cold_model_and_after_an_update(gpu_path, tmp_path):
    """shard.code_units(in_flight=4) where no derived table exists yet — one worker builds each, the others find it — and again right after
    the weights changed on the warm model; the sequential baseline comes from a second model object with the same weights"""
    from pcgcv2_amd.coder import Coder
    from pcgcv2_amd import shard
    ops = gpu_path
    ops.configure(**GATES)
    names = ['shell7', 'shell6', 'shell8']
    units = _units(names)
    torch.cuda.synchronize()
    for stage, sd in (('cold', synthetic.synthetic_state_dict(**START)), ('updated', synthetic.synthetic_state_dict())):
        if stage == 'cold':
            model = _model(sd)                                           # never used: every cache is empty
        else:
            with torch.no_grad():                                        # the warm model of the first stage moves to other weights
                for k, p in model.named_parameters():
                    p.copy_(sd[k].to(DEV))
        par, seq = tmp_path / f'{stage}_par', tmp_path / f'{stage}_seq'
        par.mkdir(); seq.mkdir()
        st_par, out_par = shard.code_units(Coder(model, str(par / 'f')), units, in_flight=4)
        torch.cuda.synchronize()
        st_seq, out_seq = shard.code_units(Coder(_model(sd), str(seq / 'f')), units)
        assert st_par.v.tolist() == st_seq.v.tolist(), stage
        _same_files(par, seq, units)
        for name, _ in units:
            assert torch.equal(out_par[name].C, out_seq[name].C), (stage, name)
        enc, dec = _oracle_code(synthetic.state_dict_to_numpy(sd), 'shell7')
        assert (par / 'f_u0_F.bin').read_bytes() == enc['F'], stage
        np.testing.assert_array_equal(_np(out_par['u0'].C), dec)
