"""Derived weight copies follow weight updates: the stamp helper (pcgcv2_amd/derived.py) and the host side of the bottleneck, on CPU tensors.

The kernels read re-laid-out copies of the weights that are cached on the modules.  A cached copy must be rebuilt exactly when the values
it was built from can have changed.  Routes (the GPU file tests the same list on the device):
  (a) an optimizer step (Adam: default, foreach, fused)      (b) p.copy_(w), p.mul_(s) under no_grad
  (c) load_state_dict, default and assign=True               (d) p.data = w, vector_to_parameters
  (e) module.half().float()                                  (f) p.data.mul_(s), p.data.copy_(w) + weights_changed()
  (g) two updates with no use between                        (h) the bias only
Expected tables come from an independent statement of the layout (conv) or from the CPU oracle (bottleneck), never from a cache."""
import gc

import numpy as np
import pytest
import torch

from oracle import pcgc_oracle as orc
from pcgcv2_amd import derived, ops
from pcgcv2_amd.autoencoder import InceptionResNet
from pcgcv2_amd.entropy_model import EntropyBottleneck
from pcgcv2_amd.nn import MinkowskiConvolution


def _conv_table_definition(W):
    """ops.child_conv_table's documented layout, element by element: table[k][n][cb][lane][jj] = W[k][16 cb + 4 jj + (lane >> 4)][16 n + (lane & 15)]"""
    K, cin, cout = W.shape
    k, n, cb, lane, jj = np.meshgrid(np.arange(K), np.arange(cout // 16), np.arange(cin // 16), np.arange(64), np.arange(4), indexing='ij')
    return W[k, 16 * cb + 4 * jj + (lane >> 4), 16 * n + (lane & 15)].reshape(-1)


def adam_rejected(kind, device):
    """None if torch.optim.Adam(<kind>=True) can be constructed for a parameter on `device` in this build, else the constructor's message.
    Only the constructor's rejection is a reason to skip; whatever a step raises afterwards is a failure."""
    if kind == 'default':
        return None
    try:
        torch.optim.Adam([torch.nn.Parameter(torch.zeros(2, device=device))], lr=1e-2, **{kind: True})
    except (RuntimeError, ValueError, TypeError) as e:
        return str(e)
    return None


def _adam(kind):
    def step(mod, rng):
        params = list(mod.parameters())
        why = adam_rejected(kind, params[0].device)
        if why is not None:
            pytest.skip(f'torch.optim.Adam({kind}=True) is not accepted by this build: {why}')
        opt = torch.optim.Adam(params, lr=1e-2, **({} if kind == 'default' else {kind: True}))
        for p in params:
            p.grad = torch.from_numpy(rng.standard_normal(tuple(p.shape)).astype(np.float32)).to(p.device)
        opt.step()
    return step


def _new_like(p, rng):
    return torch.from_numpy((rng.standard_normal(tuple(p.shape)) * 0.1).astype(np.float32)).to(p.device)


def _copy(mod, rng):
    with torch.no_grad():
        for p in mod.parameters():
            p.copy_(_new_like(p, rng))


def _mul(mod, rng):
    with torch.no_grad():
        for p in mod.parameters():
            p.mul_(1.25)


def _load(assign):
    def f(mod, rng):
        sd = {k: _new_like(v, rng) for k, v in mod.state_dict().items()}
        mod.load_state_dict(sd, assign=assign)
    return f


def _data_assign(mod, rng):
    for p in mod.parameters():
        p.data = _new_like(p, rng)


def _vector(mod, rng):
    ps = list(mod.parameters())
    vec = torch.nn.utils.parameters_to_vector(ps)
    torch.nn.utils.vector_to_parameters(vec * 0.5 + 0.01, ps)


def _half_float(mod, rng):
    mod.half().float()


def _data_mul(mod, rng):
    for p in mod.parameters():
        p.data.mul_(0.75)
    mod.weights_changed()


def _data_copy(mod, rng):
    for p in mod.parameters():
        p.data.copy_(_new_like(p, rng))
    mod.weights_changed()


def _twice(mod, rng):
    _copy(mod, rng)
    _data_assign(mod, rng)


ROUTES = {'a adam': _adam('default'), 'a adam foreach': _adam('foreach'), 'a adam fused': _adam('fused'), 'b copy_': _copy, 'b mul_': _mul,
          'c load_state_dict': _load(False), 'c load_state_dict assign': _load(True), 'd data=': _data_assign, 'd vector_to_parameters': _vector,
          'e half float': _half_float, 'f data.mul_ + weights_changed': _data_mul, 'f data.copy_ + weights_changed': _data_copy,
          'g two updates': _twice}


def _churn(p):
    """(i): allocate and free blocks of the parameter's size, so that an allocator that recycles does so"""
    for _ in range(4):
        t = torch.empty_like(p)
        del t
    gc.collect()


@pytest.mark.parametrize('route', list(ROUTES))
def test_conv_table_follows(route):
    rng = np.random.default_rng(len(route))
    torch.manual_seed(1)
    conv = MinkowskiConvolution(32, 32, 3)
    old = conv.kernel.detach().numpy().copy()
    t0 = conv._table(ops.child_conv_table)
    np.testing.assert_array_equal(t0.numpy(), _conv_table_definition(old))
    assert conv._table(ops.child_conv_table) is t0                       # nothing changed: nothing rebuilt
    _churn(conv.kernel)
    ROUTES[route](conv, rng)
    _churn(conv.kernel)
    new = conv.kernel.detach().numpy().copy()
    assert not np.array_equal(new, old)
    want_old, want_new = _conv_table_definition(old), _conv_table_definition(new)
    assert not np.array_equal(want_old, want_new)
    t1 = conv._table(ops.child_conv_table)
    np.testing.assert_array_equal(t1.numpy(), want_new)
    assert conv._table(ops.child_conv_table) is t1
    # a second layout of the same layer has a slot of its own, and follows too
    head = MinkowskiConvolution(16, 1, 3)
    c0 = head._table(ops.child_cls_table).clone()
    q0 = head._table(ops.child_q4_cls_table).clone()
    ROUTES[route](head, rng)
    for build, before in ((ops.child_cls_table, c0), (ops.child_q4_cls_table, q0)):
        got = head._table(build)
        np.testing.assert_array_equal(got.numpy(), build(head.kernel.detach().clone()).numpy())
        assert not torch.equal(got, before)


def test_bias_only_update():
    """(h): the conv tables hold kernels only — a bias update rebuilds nothing there; a fused block's stamp covers all ten parameters"""
    torch.manual_seed(2)
    conv = MinkowskiConvolution(16, 16, 3)
    t0 = conv._table(ops.child_conv_table)
    with torch.no_grad():
        conv.bias.add_(1.0)
    assert conv._table(ops.child_conv_table) is t0
    blk = InceptionResNet(16)
    params = [p for m in (blk.conv0_0, blk.conv0_1, blk.conv1_0, blk.conv1_1, blk.conv1_2) for p in (m.kernel, m.bias)]
    a0 = blk._tables('child', ops.child_irn_tables, params)
    assert blk._tables('child', ops.child_irn_tables, params) is a0
    with torch.no_grad():
        blk.conv1_1.bias.add_(1.0)
    a1 = blk._tables('child', ops.child_irn_tables, params)
    assert a1 is not a0 and all(torch.equal(x, y) for x, y in zip(a0, a1))


@pytest.mark.parametrize('route', list(ROUTES))
@pytest.mark.parametrize('kind', ['child', 'q4', 'rows32', 'rows_q4'])
def test_block_tables_follow(kind, route):
    """the four block-table kinds through InceptionResNet._tables; expected = the builder on detached CLONES of the current weights"""
    C, build = {'child': (16, ops.child_irn_tables), 'q4': (16, ops.child_q4_tables), 'rows32': (32, ops.rows_irn32_tables),
                'rows_q4': (32, ops.rows_q4_tables)}[kind]
    rng = np.random.default_rng(len(route) + C)
    torch.manual_seed(3)
    blk = InceptionResNet(C)
    plist = lambda: [p for m in (blk.conv0_0, blk.conv0_1, blk.conv1_0, blk.conv1_1, blk.conv1_2) for p in (m.kernel, m.bias)]
    flat = lambda t: torch.cat([x.reshape(-1) for x in (t if isinstance(t, tuple) else (t,)) if x is not None])
    fresh = lambda: flat(build([p.detach().clone() for p in plist()]))
    want_old = fresh()
    t0 = blk._tables(kind, build, plist())
    assert torch.equal(flat(t0), want_old) and blk._tables(kind, build, plist()) is t0
    ROUTES[route](blk, rng)
    want_new = fresh()
    assert not torch.equal(want_new, want_old)
    t1 = blk._tables(kind, build, plist())
    assert torch.equal(flat(t1), want_new)
    assert blk._tables(kind, build, plist()) is t1


def test_stamp_changes_exactly_when_values_can_change():
    torch.manual_seed(4)
    p = torch.nn.Parameter(torch.randn(27, 16, 16))
    q = torch.nn.Parameter(torch.randn(1, 16))
    s0 = derived.stamp((p, q))
    # reads, views, detach(), .data reads, autograd bookkeeping: no change
    _ = p.detach().sum(), p.data.abs().max(), p[3], p.reshape(-1)
    (p.sum() + q.sum()).backward()
    p.grad = None
    assert derived.stamp((p, q)) == s0
    with torch.no_grad():
        q.mul_(2)
    s1 = derived.stamp((p, q))
    assert s1 != s0 and s1[:2] == s0[:2]                               # (element 0: the optimizer epoch, then one entry per tensor)
    p.data = torch.randn(27, 16, 16)
    s2 = derived.stamp((p, q))
    assert s2[1] != s1[1] and s2[2] == s1[2] and s2[0] == s1[0]
    # a write through .data is the one route the stamp cannot see (hence weights_changed)
    p.data.mul_(2)
    assert derived.stamp((p, q)) == s2
    assert derived.stamp((p,), device=True)[1][2] == p.device
    # an optimizer step advances the epoch, whether or not the optimizer bumps version counters (a fused one does not)
    other = torch.nn.Parameter(torch.randn(3))
    other.grad = torch.ones(3)
    torch.optim.SGD([other], lr=0.1).step()
    assert derived.stamp((p, q))[0] == s2[0] + 1 and derived.stamp((p, q))[1:] == s2[1:]


def test_entry_alias_keeps_the_old_storage():
    """while an entry lives, the block its stamp names cannot be freed (and so cannot be handed to a new tensor): the alias still reads the
    old values after the parameter moved on, and a same-sized allocation cannot take the address"""
    torch.manual_seed(5)
    conv = MinkowskiConvolution(16, 16, 3)
    old_ptr, old = conv.kernel.data_ptr(), conv.kernel.detach().clone()
    conv._table(ops.child_conv_table)
    entry = conv.__dict__['_child_tables']['child_conv_table']
    assert isinstance(entry, derived.Entry) and entry.alias[0].data_ptr() == old_ptr
    conv.kernel.data = torch.zeros_like(conv.kernel)
    gc.collect()
    held = [torch.empty_like(old) for _ in range(64)]
    assert all(t.data_ptr() != old_ptr for t in held)
    assert torch.equal(entry.alias[0], old)
    # the alias shares the parameter's version counter: an in-place update of the ORIGINAL tensor is seen through it
    blk = InceptionResNet(16)
    params = [p for m in (blk.conv0_0, blk.conv0_1, blk.conv1_0, blk.conv1_1, blk.conv1_2) for p in (m.kernel, m.bias)]
    blk._tables('child', ops.child_irn_tables, params)
    e = blk.__dict__['_derived']['child']
    assert len(e.alias) == 10 and all(a.data_ptr() == p.data_ptr() for a, p in zip(e.alias, params))


def test_weights_changed_reaches_every_level():
    import copy
    from pcgcv2_amd.pcc_model import PCCModel
    torch.manual_seed(6)
    m = PCCModel()
    blk = m.encoder.block0[1]
    params = [p for c in (blk.conv0_0, blk.conv0_1, blk.conv1_0, blk.conv1_1, blk.conv1_2) for p in (c.kernel, c.bias)]
    blk._tables('rows32', ops.rows_irn32_tables, params)
    m.encoder.conv1._table(ops.child_conv_table)
    m.entropy_bottleneck.host_table(-3.0, 3.0, None)
    dup = copy.deepcopy(m)                                              # a copy carries no usable derived entry
    assert dup.encoder.conv1.__dict__['_child_tables']['child_conv_table'].stamp is None
    np.testing.assert_array_equal(dup.encoder.conv1._table(ops.child_conv_table).numpy(), _conv_table_definition(dup.encoder.conv1.kernel.detach().numpy()))
    m.weights_changed()
    assert '_derived' not in blk.__dict__ and '_child_tables' not in m.encoder.conv1.__dict__
    assert not m.entropy_bottleneck.__dict__.get('_table_cache') and m.entropy_bottleneck._hpacked is None
    for mod in (blk, m.encoder.conv1, m.entropy_bottleneck):
        mod.weights_changed()                                           # reachable on the bare modules too


# ------------------------------------------------------------------------------------------------ bottleneck, host side
EB_KEYS = orc.EB_NAMES + ['matrix', 'bias', 'factor']


def _eb_sd(eb):
    return {f'entropy_bottleneck.{k}': v.detach().cpu().numpy() for k, v in eb.state_dict().items()}


def _oracle_table(eb, lo, hi):
    return orc.cdf_table_ref32(orc.pack_eb_params(_eb_sd(eb)), np.float32(lo), np.float32(hi))


def _eb():
    torch.manual_seed(7)
    np.random.seed(7)
    eb = EntropyBottleneck(8)
    with torch.no_grad():
        for f in eb._factors:
            f.uniform_(-0.5, 0.5)
    return eb


def eb_route(eb, route, rng):
    """ROUTES[route] on a bottleneck.  The routes that set new VALUES set the old ones moved by a small random amount (arbitrary values are
    no bottleneck), through the same mechanism."""
    if route.startswith(('b copy_', 'c load', 'd data=', 'f data.copy_', 'g ')):
        # (random replacement values are no bottleneck: move every tensor by a small random amount instead, through the same route)
        base = {k: v.detach().clone() for k, v in eb.state_dict().items()}
        moved = {k: base[k] + 0.05 * torch.from_numpy(rng.standard_normal(tuple(base[k].shape)).astype(np.float32)).to(base[k].device) for k in orc.EB_NAMES}
        for alias, k in (('matrix', '_matrices.3'), ('bias', '_biases.3'), ('factor', '_factors.3')):
            moved[alias] = moved[k]
        if route.startswith('c load'):
            eb.load_state_dict(moved, assign=route.endswith('assign'))
        elif route.startswith('d data='):
            for k in orc.EB_NAMES:
                eb.get_parameter(k).data = moved[k].clone()
        elif route.startswith('f '):
            for k in orc.EB_NAMES:
                eb.get_parameter(k).data.copy_(moved[k])
            eb.weights_changed()
        else:
            with torch.no_grad():
                for k in orc.EB_NAMES:
                    eb.get_parameter(k).copy_(moved[k])
            if route.startswith('g '):
                for k in orc.EB_NAMES:
                    eb.get_parameter(k).data = moved[k] * 1.01
    else:
        ROUTES[route](eb, rng)


@pytest.mark.parametrize('mode', ['reference', 'reference-python'])
@pytest.mark.parametrize('key', EB_KEYS)
def test_host_table_follows_each_of_the_12_tensors(key, mode):
    """each tensor changed alone (the three aliased keys reach the last layer's), the SAME (min_v, max_v) asked again"""
    eb = _eb()
    eb.table_mode = mode
    old = _oracle_table(eb, -9, 7)
    np.testing.assert_array_equal(eb.host_table(np.float32(-9), np.float32(7), None), old)
    p = eb.get_parameter(key)
    with torch.no_grad():
        p.add_(0.05 if 'bias' not in key.lower() else 0.3)
    new = _oracle_table(eb, -9, 7)
    assert not np.array_equal(new, old), key
    got = eb.host_table(np.float32(-9), np.float32(7), None)
    np.testing.assert_array_equal(got, new)
    assert eb.host_table(np.float32(-9), np.float32(7), None) is got       # and cached again
    np.testing.assert_array_equal(eb._host_packed(), orc.pack_eb_params(_eb_sd(eb)))


@pytest.mark.parametrize('mode', ['reference', 'reference-python'])
@pytest.mark.parametrize('route', list(ROUTES))
def test_host_table_follows_every_route(route, mode):
    rng = np.random.default_rng(len(route))
    eb = _eb()
    eb.table_mode = mode
    old = _oracle_table(eb, -6, 6)
    np.testing.assert_array_equal(eb.host_table(np.float32(-6), np.float32(6), None), old)
    np.testing.assert_array_equal(eb.host_table(np.float32(-2), np.float32(3), None), _oracle_table(eb, -2, 3))
    eb_route(eb, route, rng)
    new = _oracle_table(eb, -6, 6)
    assert not np.array_equal(new, old)
    np.testing.assert_array_equal(eb.host_table(np.float32(-6), np.float32(6), None), new)
    np.testing.assert_array_equal(eb.host_table(np.float32(-2), np.float32(3), None), _oracle_table(eb, -2, 3))
    cdf, table = eb.reference_table(np.float32(-6), np.float32(6))
    np.testing.assert_array_equal(table, new)
    np.testing.assert_array_equal(eb.reference_table_native(np.float32(-6), np.float32(6)), new)


@pytest.mark.parametrize('route', ['a adam', 'b mul_', 'c load_state_dict assign', 'd data=', 'e half float', 'f data.mul_ + weights_changed'])
def test_library_table_cache_follows(route, tmp_path):
    """the native side keeps tables per (parameter VALUES, range) — pcgc_table_cache, and the reftable library's per-parameter-set operators:
    coded with the updated parameters, the stream is the oracle's for the NEW table, and decodes"""
    from pcgcv2_amd import entropy_model
    rng = np.random.default_rng(len(route))
    eb = _eb()
    r = 700
    sym = np.clip(np.rint(rng.normal(6, 2.0, size=(r, 8))), 0, 12).astype(np.int16)
    sym[0, 0], sym[-1, -1] = 0, 12
    xyz = rng.permutation(np.unique(rng.integers(0, 40, size=(4 * r, 3)), axis=0))[:r].astype(np.int32)

    def code(stem):
        ops.table_warm(eb._host_packed(), 8)
        ops.items_encode([stem], sym, xyz, [r], [(-6.0, 6.0)], [(r, 2 * r, 3 * r)], eb._host_packed(), 16)
        sb, lb = np.zeros((r, 8), np.int16), np.zeros((r, 4), np.int32)
        ops.frame_decode(stem, 8, eb._host_packed(), sb, lb)
        np.testing.assert_array_equal(sb, sym)
        rows, C, ranges, counts, native = ops.items_probe([stem])
        got, _ = ops.items_decode([stem], rows, C, ranges, native, eb._host_packed())
        np.testing.assert_array_equal(got, sym)
        return open(stem + '_F.bin', 'rb').read()
    entropy_model.table_cache(on=True, clear=True)
    old = orc.rc_encode(_oracle_table(eb, -6, 6), sym)
    assert code(str(tmp_path / 'a')) == old
    ROUTES[route](eb, rng)
    new = orc.rc_encode(_oracle_table(eb, -6, 6), sym)
    assert new != old
    assert code(str(tmp_path / 'b')) == new
    assert code(str(tmp_path / 'c')) == new                                # (now from the caches)
