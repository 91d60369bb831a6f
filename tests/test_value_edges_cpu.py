"""The oracle's convolutions at the value edges of fp32 against the exact integer chain (tests/value_edges.py): denormals, products that
underflow, partial sums near FLT_MAX and exponent spreads wide enough that the order of the chain decides every bit.  No GPU needed.

Every other conv test draws standard normals and weights of order 1 / sqrt(K Cin): a translation unit built with flushing, or a kernel that
sums in another order, passes them.  Here each class asserts on the definition that it is what its name says, each mutated definition must
differ in bits on the class named for it, and the oracle (C, OpenMP threads, -O2) must equal the definition bit for bit."""
import numpy as np
import pytest

import fp64_reference as R
import test_fp64_definition as F64
import value_edges as V
from oracle import pcgc_oracle as orc

N = 17


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(got, want, what):
    """bit equality; a NaN equals any NaN (the payload is not part of the definition)"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f'{what}: NaNs at other places'
    bad = (_bits(got) != _bits(want)) & ~nan
    assert not bad.any(), f'{what}: {bad.sum()} of {bad.size} outputs differ in bits, first {got[bad][0]!r} vs {want[bad][0]!r}'


@pytest.fixture(scope='module')
def level():
    c4 = F64._prefix(N)
    k3 = R.k3_map(c4, 1)
    present = (k3 >= 0).sum(0)
    assert present.min() >= 1 and present.max() < 27 and (k3[14:] >= 0).any() and (k3[:13] >= 0).any()     # absent offsets before and after present ones
    down = R.neighbour_map(R.down_coords(c4, 1), c4, R.offsets(2))
    return dict(c4=c4, k3=k3, down=down, k1=np.arange(N)[None])


@pytest.fixture(scope='module')
def k3_chain(level):
    """class -> (x, W, b, the definition's output): computed once, shared by the precondition and mutation tests"""
    out = {}
    for i, cls in enumerate(V.FINITE):
        x, W, b = V.case(cls, 10 + i, N, 27, 16, 16, level['k3'])
        out[cls] = (x, W, b, V.chain(level['k3'], x, W, b))
    return out


@pytest.mark.parametrize('cls', V.FINITE)
def test_class_preconditions_hold_on_the_definition(cls, k3_chain, level):
    """measured here: denormal 1.00 of the outputs non-zero denormals, underflow 1.00 of them -0, near_overflow max |y| 1.74e37"""
    x, W, b, y = k3_chain[cls]
    share = V.precondition(cls, y)
    print(f'{cls}: share {share}, max |y| {np.abs(y).max():.3g}')
    if cls == 'underflow':
        assert V.neg_zero(V.chain(level['k3'], x, W, None)).all()            # -0 before the bias too
    if cls == 'wide':
        assert np.isfinite(y).all() and np.log2(np.abs(x).max() / np.abs(x[x != 0]).min()) > 100


@pytest.mark.parametrize('cls', V.FINITE)
@pytest.mark.parametrize('op', ['k27', 'k8', 'k1', 'k27 1->16', 'k27 16->1'])
def test_oracle_conv_gather_equals_the_chain(op, cls, level, k3_chain):
    if op == 'k27':
        x, W, b, want = k3_chain[cls]
        nbr = level['k3']
    else:
        K, cin, cout = {'k8': (8, 16, 8), 'k1': (1, 16, 16), 'k27 1->16': (27, 1, 16), 'k27 16->1': (27, 16, 1)}[op]
        nbr = level['k3' if K == 27 else 'down' if K == 8 else 'k1']
        x, W, b = V.case(cls, 20 + len(op), N, K, cin, cout, nbr)
        want = V.chain(nbr, x, W, b)
    _same_bits(orc.conv_gather(nbr.astype(np.int32), x, W[0] if op == 'k1' else W, b), want, f'{op} {cls}')
    if cls == 'underflow':                                                    # the sign of the zero accumulator itself, before a bias meets it
        _same_bits(orc.conv_gather(nbr.astype(np.int32), x, W[0] if op == 'k1' else W, None), V.chain(nbr, x, W, None), f'{op} {cls}, no bias')


@pytest.mark.parametrize('cls', V.FINITE)
def test_oracle_conv_up2_equals_the_chain(cls):
    x, W, b = V.case(cls, 30, 5, 8, 16, 8)
    _same_bits(orc.conv_up2(x, W, b), V.up2(x, W, b), f'up2 {cls}')


@pytest.mark.parametrize('cls', V.FINITE)
def test_oracle_inception_resnet_equals_the_chain(cls, level):
    """the block composed from the exact chain with NaN-propagating ReLU"""
    sd, x = V.block_case(cls, 40, N, 16, level['k3'])
    want = V.inception_resnet(sd, 'b', level['k3'], x)
    assert np.isfinite(want).all()
    if cls == 'near_overflow':
        assert np.abs(want).max() >= 1e36
    _same_bits(orc.inception_resnet(sd, 'b', orc.Level(level['c4'].astype(np.int32), 1), x), want, f'irn {cls}')


MUTATION_CLASS = {'descending': 'wide', 'per_offset': 'wide', 'no_fma': 'wide', 'flush_inputs': 'denormal', 'flush_results': 'denormal',
                  'padded': 'underflow'}


def test_mutated_definitions_differ_in_bits(level, k3_chain):
    """each wrong convolution a kernel could plausibly compute differs from the exact chain on the class named for it.  Shares of differing
    outputs measured here (17 rows, K = 27, 16 -> 16): descending 0.59, per_offset 0.49, no_fma 0.54, flush_inputs 1.00, flush_results 1.00,
    padded 1.00"""
    assert set(MUTATION_CLASS) == set(V.MUTATIONS)
    shares = {}
    for mut, cls in MUTATION_CLASS.items():
        x, W, b, want = k3_chain[cls]
        shares[mut] = V.differing(V.chain(level['k3'], x, W, b, mutation=mut), want)
        print(f'mutation {mut:14s} on {cls:10s}: {shares[mut]:.2f} of the outputs differ')
    assert all(s > 0 for s in shares.values()), shares
    # the oracle's per-offset convention is one realisation of `per_offset`: it equals that mutation, not the definition
    x, W, b, want = k3_chain['wide']
    orc.CONVENTIONS['accumulate'] = 'per_offset_gemm'
    try:
        gemm = orc.conv_gather(level['k3'].astype(np.int32), x, W, b)
    finally:
        orc.CONVENTIONS['accumulate'] = 'chain'
    _same_bits(gemm, V.chain(level['k3'], x, W, b, mutation='per_offset'), 'per_offset_gemm')
    assert V.differing(gemm, want) > 0


def _zero_sign_only(got, want, what):
    """equal as real numbers; bits may differ only where both are zeros -> the number of such sign differences"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    diff = _bits(got) != _bits(want)
    assert not (diff & ~((got == 0) & (want == 0))).any(), f'{what}: more than the sign of a zero differs'
    return int(diff.sum())


@pytest.mark.parametrize('cls', V.FINITE)
def test_zero_sign_relation_on_the_oracle(cls, level):
    """The accumulator starts at +0, so the sign of a zero FEATURE reaches no output bit: (+-0) w + acc = acc for every acc but -0, and a
    chain that starts at +0 holds -0 only after a negative underflow.  That exception is the class `underflow`: there fma(-0, w, -0) = -0 and
    fma(+0, w, -0) = +0 by the IEEE rule the definition itself follows, so flipping zero features flips the sign of zero OUTPUTS (measured
    here: 32 of 272 at k27) and nothing else.  Asserted: bits unchanged on denormal, near_overflow and wide; on underflow equality as real
    numbers, every differing bit the sign of a zero, and both sides bit-equal to the exact chain"""
    rng = np.random.default_rng(50)
    x, W, b = V.case(cls, 51, N, 27, 16, 16, level['k3'])
    x = V.with_zeros(rng, x)
    xf = V.flip_zero_signs(rng, x)
    assert (_bits(x) != _bits(xf)).any() and np.array_equal(x, xf)
    nbr = level['k3'].astype(np.int32)
    sd, xb = V.block_case(cls, 52, N, 16, level['k3'])
    xb = V.with_zeros(rng, xb)
    lvl = orc.Level(level['c4'].astype(np.int32), 1)
    pairs = [(f'k27 {cls}', orc.conv_gather(nbr, xf, W, b), orc.conv_gather(nbr, x, W, b)),
             (f'k27 {cls}, no bias', orc.conv_gather(nbr, xf, W, None), orc.conv_gather(nbr, x, W, None)),
             (f'k1 {cls}', orc.conv_k1(xf, W[0], b), orc.conv_k1(x, W[0], b)),
             (f'up2 {cls}', orc.conv_up2(xf[:5], W[:8], b), orc.conv_up2(x[:5], W[:8], b)),
             (f'irn {cls}', orc.inception_resnet(sd, 'b', lvl, V.flip_zero_signs(rng, xb)), orc.inception_resnet(sd, 'b', lvl, xb))]
    _same_bits(pairs[0][2], V.chain(nbr, x, W, b), f'k27 {cls} with zeros vs the chain')
    _same_bits(pairs[0][1], V.chain(nbr, xf, W, b), f'k27 {cls} with flipped zeros vs the chain')
    for what, flipped, plain in pairs:
        if cls == 'underflow':
            print(f'{what}: {_zero_sign_only(flipped, plain, what)} zero outputs changed sign')
        else:
            _same_bits(flipped, plain, what)


def test_chain_special_values():
    """the definition's own corners, against values known in closed form"""
    one = np.arange(1)[None]
    f = lambda x, w, **kw: V.chain(one, np.array([x], np.float32), np.array(w, np.float32).reshape(1, len(x), 1), **kw)[0, 0]
    tiny = np.float32(2.0 ** -149)
    assert _bits(f([-1e-30], [1e-30])) == 0x80000000                                  # negative underflow: -0
    assert _bits(f([-1e-30, 0.0], [1e-30, 1.0])) == 0 and _bits(f([-1e-30, 1.0], [1e-30, 0.0])) == 0       # a present zero: (+0)(1) + (-0) = +0 ...
    assert _bits(f([-1e-30, -0.0], [1e-30, 1.0])) == 0x80000000                       # ... and (-0)(1) + (-0) = -0
    assert f([0.5], [tiny]) == 0 and f([0.75], [tiny]) == tiny and f([1.5], [tiny]) == np.float32(2.0 ** -148)     # half to even at the bottom
    assert f([3.0e38, 3.0e38], [1.0, 1.0]) == np.inf and np.isfinite(f([3.0e38], [1.0]))
    assert np.isnan(f([np.inf], [0.0])) and np.isnan(f([np.inf, -np.inf], [1.0, 1.0])) and f([np.inf, 1.0], [-1.0, 5.0]) == -np.inf
    assert np.isnan(f([np.nan], [1.0], relu_out=True)) and _bits(f([-1.0], [1.0], relu_out=True)) == 0
    assert f([1.0, 2.0 ** -24], [1.0, 1.0]) == 1 and f([1.0, 2.0 ** -24, 2.0 ** -24], [1.0, 1.0, 1.0]) == 1       # ties to even, one rounding per step
    assert f([1.0 + 2.0 ** -23], [1.0 + 2.0 ** -23]) == np.float32(1 + 2.0 ** -22)   # 1 + 2^-22 + 2^-46 rounds down; through a rounded product too
    rng = np.random.default_rng(0)
    a = rng.standard_normal(64).astype(np.float32)
    a[:4] = [-0.0, 2.0 ** -149, -3.4028235e38, -np.inf]
    assert np.array_equal(_bits(V.to_float32(list(zip(*V.parts(a))), a.shape)), _bits(a))                          # parts <-> bits round trip
