"""Every convolution family at the value edges of fp32 (tests/value_edges.py), against the oracle and the exact integer chain.

The other device tests vary shapes, memory and weights around ONE kind of values (standard normals, weights of order 1 / sqrt(K Cin)).  Here the
families of tests/test_scratch_state_device.py, forced as that file forces them, at their two smallest shapes, are fed

* the finite classes (denormal, underflow, near_overflow, wide): device bits = oracle bits, and at the smallest shape = the exact chain.  The
  one tolerated difference is -0 against +0 in class `underflow` (an MFMA adds fma(x, 0, -0) = +0 for a padded product that the oracle
  skips); it is counted per family and must occur nowhere else;
* the zero-sign relation: flipping the signs of zero features changes no output bit (on `underflow`: nothing but the sign of zero outputs,
  see tests/test_value_edges_cpu.py) — what makes the difference above harmless for the next layer;
* `nonfinite`: a compact cluster S of rows with +inf, -inf, NaN and an element that overflows in the chain.  Outside the family's footprint
  of S the output equals the oracle bit for bit; inside it, for single convolutions and heads, every element is bit-equal to the oracle,
  non-finite, or +0 after a fused ReLU; for fused blocks nothing is asserted inside.  No family may raise or touch the guard band;
* the ReLU pin: fmaxf(v, 0) maps a NaN pre-activation to +0 where the oracle (np.maximum) and the reference (torch.relu) propagate it.

The plain levels are prefixes of a shell, which are flat at these sizes: their chains run through the nine in-plane offsets (absent ones before,
between and after); the children levels are solid 2 x 2 x 2 blocks and run through all 27.

test_zz_report prints the per-family counts that DESIGN.md §3 records."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import fp64_reference as R
import test_fp64_definition as F64
import test_scratch_state_device as SS          # (CONV_FAMILIES, _level, _down_pair, _sibling, _shell9; nothing of it is collected from here)
import value_edges as V
from oracle import pcgc_oracle as orc

gpu_path = F64.gpu_path

ROWS = (17, 129)
PARENTS = (3, 129)
SEED = 900
ZERO_SIGN = {}              # family -> {class: outputs that are -0 on one side and +0 on the other, device vs oracle}
FLIPPED = {}                # family -> zero outputs whose sign followed the flipped zero features (class underflow)
NONFINITE = {}              # family -> [elements inside the footprint, bit-equal, device non-finite, +0 after ReLU, other, rows outside]
CHAIN = {}                  # (op, class) -> the exact chain's output at the smallest shape: families of one shape share it

# Footprint of a non-finite input row, in Chebyshev distance at the level's stride (rows further away must equal the oracle):
#   per-row and rows kernels gather exactly the 27 neighbours of an output row (conv.hip, rows_irn.hip, conv_packed.hip): 1 per k3 hop;
#   children kernels gather the parent's 4 x 4 x 4 halo, cells -1 .. 2 per axis from the parent's origin (child_kernels.h, "Geometry"), and
#   multiply zero B columns for the children that do not reach a cell: a child at 0 or 1 is up to 2 away from every cell: 2 per k3 hop;
#   a plain convolution is one hop, an InceptionResNet block two (conv0_0 -> conv0_1, conv1_1 behind the pointwise conv1_0).
RADIUS = {'conv': 1, 'irn': 2, 'child conv': 2, 'child irn': 4}
TRUE_RADIUS = {'conv': 1, 'irn': 2, 'child conv': 1, 'child irn': 2}


@pytest.fixture(autouse=True)
def _stop_after_a_fault():
    """non-finite data goes through every kernel here: if one faulted, the session ends instead of launching the next family on that device"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f'the device reports an error after this test, nothing more is launched: {e}', returncode=3)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _np(t):
    torch.cuda.synchronize()
    return t.detach().cpu().contiguous().numpy()


def _guarded(x):
    """-> (the F64._poisoned column slice of x, a check that its guard columns and rows are still NaN)"""
    view = F64._poisoned(x)
    base, (n, c) = view._base, x.shape

    def intact():
        return bool(torch.isnan(base[:, c:]).all() and torch.isnan(base[n:]).all())
    return view, intact


def _differences(got, want):
    """-> (elements whose bits differ only as -0 / +0, elements that differ otherwise); a NaN equals any NaN"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape
    diff = (_bits(got) != _bits(want)) & ~(np.isnan(got) & np.isnan(want))
    zero = diff & (got == 0) & (want == 0)
    return zero, diff & ~zero


# ------------------------------------------------------------------------------------------------ the families, forced as the scratch tests force them
class Family:
    """one family at one shape: .device(x, W) -> (output, guard intact), .oracle(x, W), .chain(x, W), .case(cls) -> (x, W), the geometry of the
    non-finite footprint.  For the fused blocks W is the block's state dict; for `unit` the classes apply to the weights and x is the all-ones
    input."""
    relu = False            # the launch takes relu=


def _conv_family(family, n, ops):
    K, cin, cout, impl = SS.CONV_FAMILIES[family]
    f = Family()
    f.name, f.kind, f.op, f.relu = family, 'conv', (K, cin, cout), True
    if K == 8:
        f.c_in, nbr = SS._down_pair(n, SEED + n)
    else:
        f.c_in = SS._level(n, SEED + n)
        nbr = R.k3_map(f.c_in, 1) if K == 27 else np.arange(n)[None]
    if K > 1:
        nbr = nbr.copy()
        nbr[:, 3::5] = -1                                              # every fifth output row has no present neighbour: out = bias
    f.nbr = nbr
    nbr_d = SS._t(nbr, torch.int32)
    unit = family == 'unit'
    ones = np.ones((n, 1), np.float32)

    def device(x, Wb, relu=False):
        W, b = Wb
        Wt, bt = SS._t(W[0] if K == 1 else W), SS._t(b)
        if impl is not None:
            ops.set_conv_impl(impl)
        if unit:
            return _np(ops.conv_gather_unit(nbr_d, Wt, bt, relu=relu)), True
        xv, intact = _guarded(x)
        if family in ('rows_conv', 'packed64', 'rows_down'):
            table = ops.child_conv_table(SS._t(W))
            out = ops.conv_rows(nbr_d, xv, table, bt, cout, relu=relu) if family == 'rows_conv' else \
                ops.conv_packed64(nbr_d, xv, table, bt, relu=relu) if family == 'packed64' else ops.conv_down_rows(nbr_d, xv, table, bt, cout, relu=relu)
        else:
            out = ops.conv_gather(nbr_d, xv, Wt, bt, relu=relu)
            if K == 27:
                assert ops.lib().pcgc_last_conv_impl() == impl, (family, n)
        return _np(out), intact()
    f.device = device
    f.oracle = lambda x, Wb: orc.conv_gather(nbr.astype(np.int32), ones if unit else x, Wb[0], Wb[1])
    f.chain = lambda x, Wb: V.chain(nbr, ones if unit else x, Wb[0], Wb[1])

    def case(cls):
        if unit:                                                       # the class's features are the 27 x 16 weights; near_overflow on the ones input
            rng = np.random.default_rng(SEED)
            W = V.features(cls, rng, 27, 16)[:, None, :]
            if cls == 'near_overflow':
                W = (W.astype(np.float64) * 2.0 ** np.ceil(np.log2(1e37 / V._max64(nbr, ones, W)))).astype(np.float32)
            return None, (W, V.weights(cls, rng, 27, 1, 16)[1])
        x, W, b = V.case(cls, SEED, len(f.c_in), K, cin, cout, nbr)
        return x, (W, b)
    f.case = case
    f.n_in = len(f.c_in)
    if K == 27:
        f.footprint = lambda S: _within(f.c_in, f.c_in[S], RADIUS['conv'])
    elif K == 8:
        f.footprint = lambda S: np.isin(nbr, S).any(0)
    else:
        f.footprint = lambda S: np.isin(np.arange(n), S)
    f.true_footprint = f.footprint
    return f


def _up2_family(impl, form, n, ops):
    cin, cout = 64, 32
    f = Family()
    f.name, f.kind, f.op, f.relu = f'conv_up2 impl {impl}{" rows=" if form == "rows" else ""}', 'conv', ('up2', cin, cout), True
    rows = np.random.default_rng(n).permutation(n + 5)[:n].astype(np.int32)
    f.n_in = n

    def device(x, Wb, relu=False):
        ops.set_up2_impl(impl)
        Wt, bt = SS._t(Wb[0]), SS._t(Wb[1])
        if form == 'rows':                                             # the level is rows `rows` of a wider buffer whose other rows are NaN
            wide = np.full((n + 5, cin), np.nan, np.float32)
            wide[rows] = x
            return _np(ops.conv_up2(SS._t(wide), Wt, bt, relu=relu, rows=SS._t(rows))), True
        xv, intact = _guarded(x)
        return _np(ops.conv_up2(xv, Wt, bt, relu=relu)), intact()
    f.device = device
    f.oracle = lambda x, Wb: orc.conv_up2(x, Wb[0], Wb[1])
    f.chain = lambda x, Wb: V.up2(x, Wb[0], Wb[1])

    def case(cls):
        x, W, b = V.case(cls, SEED, n, 8, cin, cout)
        return x, (W, b)
    f.case = case
    f.c_in = SS._shell9(coarse=True)[:n]                               # (S: adjacent parents; the footprint is their own children)
    f.footprint = f.true_footprint = lambda S: np.isin(np.arange(8 * n) // 8, S)
    return f


def _within(c_out, c_s, radius, unit=1):
    d = np.abs(c_out[:, None, 1:] - c_s[None, :, 1:]).max(2) // unit
    d = np.where(c_out[:, None, 0] == c_s[None, :, 0], d, 1 << 30)
    return (d <= radius).any(1)


def _load(blk, sd):
    with torch.no_grad():
        for nm in ('conv0_0', 'conv0_1', 'conv1_0', 'conv1_1', 'conv1_2'):
            getattr(blk, nm).kernel.copy_(SS._t(sd[f'b.{nm}.kernel']))
            getattr(blk, nm).bias.copy_(SS._t(sd[f'b.{nm}.bias']))


def _irn_family(family, n, ops, c4=None):
    from pcgcv2_amd import dispatch
    from pcgcv2_amd.sparse import CoordMap, SparseTensor
    C, changes, _, variant = F64.IRN_FAMILIES[family]
    f = Family()
    f.name, f.kind, f.op = f'irn {family}', 'irn', ('irn', C)
    blk, _ = F64._block(np.random.default_rng(0), C)
    ops.configure(**changes)
    ops.set_rows_q4_variant(variant)
    f.c_in = SS._level(n, SEED + n) if c4 is None else c4
    n = len(f.c_in)
    assert dispatch.select('irn', (C,), n).family == family.split(' ')[0]
    k3 = R.k3_map(f.c_in, 1)
    lvl = orc.Level(f.c_in.astype(np.int32), 1)

    def device(x, sd, relu=False):
        _load(blk, sd)
        with torch.no_grad():
            return _np(blk(SparseTensor(SS._t(x), coordinate_map=CoordMap(SS._t(f.c_in, torch.int32), 1, unique=True))).F), True
    f.device = device
    f.oracle = lambda x, sd: orc.inception_resnet(sd, 'b', lvl, x)
    f.chain = lambda x, sd: V.inception_resnet(sd, 'b', k3, x)

    def case(cls):
        sd, x = V.block_case(cls, SEED, n, C, k3)
        return x, sd
    f.case = case
    f.n_in = n
    f.footprint = lambda S: _within(f.c_in, f.c_in[S], RADIUS['irn'])
    f.true_footprint = lambda S: _within(f.c_in, f.c_in[S], TRUE_RADIUS['irn'])
    return f


def _child_family(family, n_p, ops, pc=None):
    from pcgcv2_amd.sparse import CoordMap
    C = int(family.split(' ')[-1]) if family[-1].isdigit() else 16
    irn = 'irn' in family
    f = Family()
    f.name, f.kind = family, 'child irn' if irn else 'child conv'
    cout = 1 if 'cls' in family else C
    f.op = ('child irn', C) if irn else ('child', C, cout)
    f.relu = not irn and cout != 1                                     # (the heads have no fused epilogue: the logits are stored as they are)
    pc = SS._sibling(SS._shell9(coarse=True)[:n_p], 16, SEED + n_p).astype(np.int64) if pc is None else pc
    parent = CoordMap(SS._t(pc, torch.int32), 2, unique=True)
    f.c_in = kc = R.children_coords(pc, 2)
    k3 = R.k3_map(kc, 1)
    f.n_in = len(kc)
    if irn:
        blk, _ = F64._block(np.random.default_rng(0), C)
        params = [p for m in (blk.conv0_0, blk.conv0_1, blk.conv1_0, blk.conv1_1, blk.conv1_2) for p in (m.kernel, m.bias)]
        lvl = orc.Level(kc.astype(np.int32), 1)

        def device(x, sd, relu=False):
            _load(blk, sd)                                             # the tables are derived from the weights: rebuilt after every load
            q4 = ops.child_q4_tables(params) if family == 'child_q4 irn' else None
            return _np(ops.irn_block_child(parent.k3, SS._t(x), params, ops.child_irn_tables(params), q4_table=q4)), True
        f.oracle = lambda x, sd: orc.inception_resnet(sd, 'b', lvl, x)
        f.chain = lambda x, sd: V.inception_resnet(sd, 'b', k3, x)

        def case(cls):
            sd, x = V.block_case(cls, SEED, len(kc), C, k3)
            return x, sd
    else:
        def device(x, Wb, relu=False):
            W, b = Wb
            xv, intact = _guarded(x)
            if family == 'child_q4 cls':
                out = ops.cls_child_q4(parent.k3, xv, ops.child_q4_cls_table(SS._t(W)), SS._t(b))
            else:
                table = ops.child_cls_table(SS._t(W)) if cout == 1 else ops.child_conv_table(SS._t(W))
                out = ops.conv_child(parent.k3, xv, table, SS._t(b), cout, relu=relu)
            return _np(out), intact()
        f.oracle = lambda x, Wb: orc.conv_gather(k3.astype(np.int32), x, Wb[0], Wb[1])
        f.chain = lambda x, Wb: V.chain(k3, x, Wb[0], Wb[1])

        def case(cls):
            x, W, b = V.case(cls, SEED, len(kc), 27, C, cout, k3)
            return x, (W, b)
    f.device, f.case = device, case
    f.footprint = lambda S: _within(kc, kc[S], RADIUS[f.kind])
    f.true_footprint = lambda S: _within(kc, kc[S], TRUE_RADIUS[f.kind])
    return f


UP2 = [(impl, form) for impl in (0, 1, 2) for form in ('plain', 'rows')]
FAMILIES = [('conv', k) for k in SS.CONV_FAMILIES] + [('up2', k) for k in UP2] + [('irn', k) for k in F64.IRN_FAMILIES] + \
           [('child', k) for k in F64.CHILD_FAMILIES]


def _family(group, key, size, ops):
    """size 0: the smallest shape (the exact chain is computed there), 1: the second"""
    if group == 'conv':
        return _conv_family(key, ROWS[size], ops)
    if group == 'up2':
        return _up2_family(key[0], key[1], PARENTS[size], ops)
    if group == 'irn':
        return _irn_family(key, ROWS[size], ops)
    return _child_family(key, PARENTS[size], ops)


def _ids(v):
    return f'{v[0]}-{v[1]}'.replace(' ', '_')


# ------------------------------------------------------------------------------------------------ finite classes and the zero-sign relation
def _zeros_flipped(f, cls, x, W):
    """-> (input with zeros, the same with their signs drawn again), in the features — in the weights for `unit`"""
    rng = np.random.default_rng(SEED + 1)
    if x is None:
        Wz = V.with_zeros(rng, W[0][:, 0])
        return (None, (Wz[:, None], W[1])), (None, (V.flip_zero_signs(rng, Wz)[:, None], W[1]))
    xz = V.with_zeros(rng, x)
    return (xz, W), (V.flip_zero_signs(rng, xz), W)


@pytest.mark.parametrize('group,key', FAMILIES, ids=[_ids(v) for v in FAMILIES])
def test_finite_classes_and_zero_signs(group, key, gpu_path):
    failures = []
    for size in (0, 1):
        f = _family(group, key, size, gpu_path)
        zs = ZERO_SIGN.setdefault(f.name, dict.fromkeys(V.FINITE, 0))
        for cls in V.FINITE:
            x, W = f.case(cls)
            want = f.oracle(x, W)
            if f.name != 'unit' and f.kind in ('conv', 'child conv'):
                V.precondition(cls, want)                              # (the blocks add the residual; `unit` has no products)
            got, intact = f.device(x, W)
            assert intact, f'{f.name} {cls}: guard band written'
            refs = [('the oracle', want)]
            if size == 0:
                if (f.op, cls) not in CHAIN:
                    CHAIN[f.op, cls] = f.chain(x, W)
                refs.append(('the exact chain', CHAIN[f.op, cls]))
                if not np.array_equal(_bits(want), _bits(CHAIN[f.op, cls])):
                    failures.append(f'{f.name} {cls}: the oracle differs from the exact chain')
            for what, ref in refs:
                zero, other = _differences(got, ref)
                print(f'{f.name:28s} {cls:14s} size {size} vs {what:15s}: {int(zero.sum()):6d} -0/+0, {int(other.sum()):6d} other of {got.size}')
                if what == 'the oracle':
                    zs[cls] += int(zero.sum())
                if other.any():
                    i = tuple(np.argwhere(other)[0])
                    failures.append(f'{f.name} {cls} size {size}: {other.sum()} of {got.size} outputs differ from {what}, first at {i}: '
                                    f'{got[i]!r} ({_bits(got)[i]:#010x}) vs {ref[i]!r} ({_bits(ref)[i]:#010x})')
                if zero.any() and cls != 'underflow':
                    failures.append(f'{f.name} {cls} size {size}: {zero.sum()} outputs differ from {what} in the sign of a zero')
            # the relation: the signs of zero features reach no output bit (underflow: nothing but the sign of zero outputs)
            (xz, Wz), (xf, Wf) = _zeros_flipped(f, cls, x, W)
            plain, flipped = f.device(xz, Wz)[0], f.device(xf, Wf)[0]
            zero, other = _differences(flipped, plain)
            if other.any() or (zero.any() and cls != 'underflow'):
                failures.append(f'{f.name} {cls} size {size}: flipping the signs of zero features changed {int(zero.sum())} zero signs and '
                                f'{int(other.sum())} other outputs')
            FLIPPED[f.name] = FLIPPED.get(f.name, 0) + int(zero.sum())
            zero, other = _differences(plain, f.oracle(xz, Wz))
            if other.any() or (zero.any() and cls != 'underflow'):
                failures.append(f'{f.name} {cls} size {size}, zero features: {int(zero.sum())} zero signs and {int(other.sum())} other outputs '
                                'differ from the oracle')
    assert not failures, '\n'.join(failures)


# ------------------------------------------------------------------------------------------------ non-finite rows
def _nearest4(c_in, r0):
    d = np.abs(c_in[:, 1:] - c_in[r0, 1:]).max(1) + (c_in[:, 0] != c_in[r0, 0]) * (1 << 30)
    return np.argsort(d, kind='stable')[:4]


def _cluster(c_in, halo=None):
    """four adjacent input rows: a centre row and the three nearest to it.  The centre is the row nearest to the level's median coordinate;
    with halo = (footprint radius, true radius) it is the row around which most output rows lie in the halo only"""
    if halo is None:
        mid = np.median(c_in[:, 1:], axis=0)
        return _nearest4(c_in, np.argmin(np.abs(c_in[:, 1:] - mid).max(1)))
    count = lambda S: int((_within(c_in, c_in[S], halo[0]) & ~_within(c_in, c_in[S], halo[1])).sum())
    return max((_nearest4(c_in, r0) for r0 in range(0, len(c_in), 8)), key=count)


def _nonfinite_case(f):
    """x ~ N(0, 1) with the cluster; weights U(-2, 2), so that 3.0e38 x w overflows for |w| > 1.14 (43 % of the weights)"""
    rng = np.random.default_rng(SEED + 2)
    if f.kind in ('irn', 'child irn'):
        C = f.op[1]
        sd = {}
        for nm, K, di, do in V._BLOCK:
            W = rng.uniform(-2, 2, (K, C // di, C // do)).astype(np.float32)
            sd[f'b.{nm}.kernel'], sd[f'b.{nm}.bias'] = (W[0] if K == 1 else W), rng.uniform(-0.1, 0.1, (1, C // do)).astype(np.float32)
        return rng.standard_normal((f.n_in, C)).astype(np.float32), sd
    K, cin, cout = (8, f.op[1], f.op[2]) if f.op[0] == 'up2' else (27, f.op[1], f.op[2]) if f.op[0] == 'child' else f.op
    W, b = rng.uniform(-2, 2, (K, cin, cout)).astype(np.float32), rng.uniform(-0.1, 0.1, (1, cout)).astype(np.float32)
    return rng.standard_normal((f.n_in, cin)).astype(np.float32), (W, b)


@pytest.mark.parametrize('group,key', FAMILIES, ids=[_ids(v) for v in FAMILIES])
def test_nonfinite_rows_are_contained(group, key, gpu_path):
    failures = []
    for size in (0, 1):
        f = _family(group, key, size, gpu_path)
        x, W = _nonfinite_case(f)
        if f.name == 'unit':                                           # the all-ones input: four non-finite OFFSETS of the kernel instead
            cnt = (f.nbr >= 0).sum(1)
            ks = np.repeat(np.argsort(np.where(cnt > 0, cnt, 1 << 30), kind='stable')[:2], 2).tolist()     # the two rarest present offsets, two values each
            Wn = V.nonfinite_rows(W[0][:, 0], ks)[:, None]
            x, W = None, (Wn, W[1])
            inside = (f.nbr[ks] >= 0).any(0)
            true_inside = inside
        else:
            if f.op[0] == 8:                                           # the first four fine rows under the middle coarse rows (adjacent by construction)
                cols = f.nbr[:, f.nbr.shape[1] // 2:]
                S = cols.T[cols.T >= 0][:4]
            else:
                S = _cluster(f.c_in, (RADIUS[f.kind], TRUE_RADIUS[f.kind]) if f.kind.startswith('child') else None)
            x = V.nonfinite_rows(x, S)
            inside, true_inside = f.footprint(S), f.true_footprint(S)
        assert inside.any() and (true_inside <= inside).all()
        if size == 1:                                                  # the class's precondition, at the shape that has room for it
            assert (~inside).mean() >= 0.25, f'{f.name}: {(~inside).mean():.2f} of the output rows lie outside the footprint'
            if f.kind.startswith('child'):
                assert (inside & ~true_inside).sum() >= 16, f'{f.name}: {(inside & ~true_inside).sum()} rows in the halo only'
        rec = NONFINITE.setdefault(f.name, [0, 0, 0, 0, 0, 0])
        for relu in ((False, True) if f.relu else (False,)):
            want = f.oracle(x, W)
            want = orc.relu(want) if relu else want
            assert not np.isfinite(want[true_inside]).all(), f'{f.name}: the cluster reached no output'
            got, intact = f.device(x, W, relu=relu)
            if not intact:
                failures.append(f'{f.name} size {size}: guard band written')
            eq = (_bits(got) == _bits(want)) | (np.isnan(got) & np.isnan(want))
            if not eq[~inside].all():
                failures.append(f'{f.name} size {size} relu {relu}: {(~eq[~inside]).sum()} elements OUTSIDE the footprint differ from the oracle')
            nonfin = ~eq & ~np.isfinite(got)
            relu0 = ~eq & ~nonfin & (_bits(got) == 0) & relu
            other = ~eq & ~nonfin & ~relu0
            rec[0] += int(inside.sum()) * got.shape[1]; rec[1] += int(eq[inside].sum()); rec[2] += int(nonfin[inside].sum())
            rec[3] += int(relu0[inside].sum()); rec[4] += int(other[inside].sum()); rec[5] += int((~inside).sum())
            print(f'{f.name:28s} size {size} relu {int(relu)}: inside {int(inside.sum())} rows ({int((inside & ~true_inside).sum())} halo only), '
                  f'equal {int(eq[inside].sum())}, non-finite {int(nonfin[inside].sum())}, +0 after ReLU {int(relu0[inside].sum())}, '
                  f'other {int(other[inside].sum())}')
            if other[inside].any() and f.kind in ('conv', 'child conv'):
                i = tuple(np.argwhere(other & inside[:, None])[0])
                failures.append(f'{f.name} size {size} relu {relu}: {other[inside].sum()} elements inside the footprint are neither the oracle\'s, '
                                f'non-finite nor +0 after ReLU, first at {i}: {got[i]!r} vs {want[i]!r}')
    assert not failures, '\n'.join(failures)


# ------------------------------------------------------------------------------------------------ the ReLU pin
def _fmax_block(sd, k3, x):
    """the block with the device's ReLU, fmaxf(v, 0): NaN -> +0 (the oracle's convolutions, composed here)"""
    relu = lambda v: np.fmax(v, np.float32(0))
    ident = np.arange(len(x), dtype=np.int32)[None]
    c = lambda nm, m, v: orc.conv_gather(m, v, sd[f'b.{nm}.kernel'], sd[f'b.{nm}.bias'])
    k3 = k3.astype(np.int32)
    out0 = c('conv0_1', k3, relu(c('conv0_0', k3, x)))
    out1 = c('conv1_2', ident, relu(c('conv1_1', k3, relu(c('conv1_0', ident, x)))))
    return np.concatenate([out0, out1], 1) + x


SINGLE = [v for v in FAMILIES if v[0] in ('conv', 'up2') or (v[0] == 'child' and v[1].startswith('child conv'))]
BLOCKS = [v for v in FAMILIES if v[0] == 'irn' or (v[0] == 'child' and 'irn' in v[1])]


@pytest.mark.parametrize('group,key', SINGLE, ids=[_ids(v) for v in SINGLE])
def test_relu_maps_a_nan_preactivation_to_plus_zero(group, key, gpu_path):
    """a row that holds a NaN has a NaN pre-activation in every output column (its own centre product); the fused epilogue's fmaxf(v, 0)
    stores +0 there, the oracle's np.maximum and the reference's torch.relu store NaN.  Pinned so that changing it is a deliberate act."""
    f = _family(group, key, 0, gpu_path)
    x, W = _nonfinite_case(f)
    if f.name == 'unit':
        Wn = W[0].copy()
        Wn[13, 0, 5] = np.nan                                          # the centre offset of column 5: every row that has itself
        x, W, rows, cols = None, (Wn, W[1]), np.flatnonzero(f.nbr[13] >= 0), [5]
    else:
        r = int(_cluster(f.c_in)[0])
        x[r, x.shape[1] // 2] = np.nan
        rows = np.flatnonzero(f.footprint([r]) if f.op[0] == 'up2' else (f.nbr == r).any(0) if f.kind == 'conv' else np.arange(f.n_in) == r)
        cols = slice(None)
    want = orc.relu(f.oracle(x, W))
    assert len(rows) and np.isnan(want[rows][:, cols]).all()
    got, intact = f.device(x, W, relu=True)
    assert intact
    assert (_bits(got[rows][:, cols]) == 0).all(), f'{f.name}: relu(NaN) is {got[rows][:, cols].ravel()[:4]}, pinned as +0'
    assert np.isnan(f.device(x, W, relu=False)[0][rows][:, cols]).all()                       # (without the ReLU the NaN is stored)


@pytest.mark.parametrize('group,key', BLOCKS, ids=[_ids(v) for v in BLOCKS])
def test_relu_inside_a_fused_block_erases_a_nan(group, key, gpu_path):
    """an isolated voxel (plain levels) or an isolated parent's eight children (children levels) with one NaN feature: the hidden rows are
    relu(NaN) = +0 on the device, so the output is finite wherever the residual is — the oracle's row is NaN throughout.  The expected row is
    the block composed from the oracle's convolutions with fmax as the ReLU, on the isolated piece alone."""
    if group == 'irn':
        c4 = SS._level(ROWS[0] - 1, SEED)
        far = c4[:1].copy()
        far[0, 1:] = c4[:, 1:].max(0) + 64
        f = _irn_family(key, None, gpu_path, c4=np.concatenate([c4, far]))
        piece = np.array([len(c4)])
    else:
        pc = SS._sibling(SS._shell9(coarse=True)[:PARENTS[0] - 1], 16, SEED).astype(np.int64)
        far = pc[:1].copy()
        far[0, 1:] = pc[:, 1:].max(0) + 64
        f = _child_family(key, None, gpu_path, pc=np.concatenate([pc, far]))
        piece = 8 * len(pc) + np.arange(8)
    assert not _within(f.c_in[:piece[0]], f.c_in[piece], 8).any()
    x, sd = _nonfinite_case(f)
    col = x.shape[1] // 2
    x[piece[0], col] = np.nan
    got, _ = f.device(x, sd)
    assert np.isnan(f.oracle(x, sd)[piece]).all()
    want = _fmax_block(sd, R.k3_map(f.c_in[piece], 1), x[piece])
    finite = np.ones(want.shape, bool)
    finite[0, col] = False                                             # (the residual's own NaN)
    assert np.isfinite(want[finite]).all() and np.isfinite(got[piece][finite]).all() and np.isnan(got[piece[0], col])
    same = _bits(got[piece]) == _bits(want)
    print(f'{f.name}: {int((same & finite).sum())} of {int(finite.sum())} elements of the isolated piece equal the block with fmax')
    if group == 'child' and 'q4' not in key:
        # the MFMA passes on a children level multiply the NaN row by the zero columns of the children that do not reach it: further hidden
        # rows of the conv1 branch become NaN and are erased too (which ones is the kernel's packing).  The conv0 half is the same either
        # way: all eight hidden rows of the parent hold the NaN in their true neighbourhood
        assert same[:, :col].all(), f'{f.name}: conv0 half {got[piece][:, :col]} vs the block with fmax {want[:, :col]}'
    else:
        assert same[finite].all(), f'{f.name}: {got[piece]} vs the block with fmax {want}'
    rest = np.arange(piece[0])
    assert np.array_equal(_bits(got[rest]), _bits(f.oracle(x, sd)[rest]))


# ------------------------------------------------------------------------------------------------ report
def test_zz_report_value_edges():
    """(prints, per family: the -0 / +0 differences against the oracle per finite class, the zero outputs whose sign followed flipped zero
    features, and the categories of the elements inside the non-finite footprint: the record DESIGN.md §3 holds)"""
    for k in sorted(ZERO_SIGN):
        z = ZERO_SIGN[k]
        print(f'value edges {k:28s} -0/+0 vs the oracle: ' + ', '.join(f'{c} {z[c]}' for c in V.FINITE) + f'; flipped zero features: {FLIPPED.get(k, 0)}')
        assert all(z[c] == 0 for c in V.FINITE if c != 'underflow')
    for k in sorted(NONFINITE):
        n, eq, nonfin, relu0, other, outside = NONFINITE[k]
        print(f'value edges {k:28s} non-finite footprint: {n} elements, {eq} equal, {nonfin} non-finite, {relu0} +0 after ReLU, {other} other; '
              f'{outside} rows outside')
        assert eq + nonfin + relu0 + other == n
