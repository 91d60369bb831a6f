"""The canonical conv chain of DESIGN.md §3 in exact integer arithmetic, and the value classes that stress it.

Every binary32 is an integer multiple of 2^-149 and every product of two an integer multiple of 2^-298, so a step
acc = round_to_binary32(x * w + acc) is computed exactly in Python integers and rounded ONCE: half to even, denormals kept, overflow to
+-inf, the sign of an exact zero sum by the IEEE rule (-0 only if both addends are -0).  Present neighbours are visited in ascending k, then
ascending ci; absent ones are skipped; the epilogue is + bias, + residual, max(., 0) with NaN propagated.  No library beyond numpy (for the
bit casts) is involved: the chain does not share a rounding, a flush mode or an fma with anything it is compared with.

A value is the pair (m, s): m the signed multiple of 2^-149 (None for NaN, INF for an infinity), s the sign bit (what a zero keeps)."""
import numpy as np

import test_fp64_definition as F64              # (_rand_w: the weight scale every conv test uses)

Q = 149
LIM = 1 << (128 + Q)                             # 2^128 in units of 2^-149: the first magnitude that is no finite binary32
MIN_NORMAL = 1 << 23


class _Inf:
    """an infinity: no arithmetic is defined on it, so the integer fast path raises TypeError and the special cases take over"""

    def __repr__(self):
        return 'INF'


INF = _Inf()
NAN_BITS = 0x7FC00000


# ------------------------------------------------------------------------------------------------ binary32 <-> (m, s)
def parts(a):
    """float32 array -> (M, S): nested lists of the shape of `a`"""
    a = np.ascontiguousarray(a, np.float32)
    bits = a.view(np.uint32).ravel().tolist()
    M, S = [], []
    for u in bits:
        s, e, f = u >> 31, (u >> 23) & 0xFF, u & 0x7FFFFF
        if e == 255:
            m = INF if f == 0 else None
        else:
            m = f if e == 0 else (f | MIN_NORMAL) << (e - 1)
            if s:
                m = -m
        M.append(m)
        S.append(s)

    def shape(flat, dims):
        if len(dims) == 1:
            return flat
        step = len(flat) // dims[0]
        return [shape(flat[i * step:(i + 1) * step], dims[1:]) for i in range(dims[0])]
    return shape(M, a.shape), shape(S, a.shape)


def bits_of(m, s):
    if m is None:
        return NAN_BITS
    if m is INF:
        return (s << 31) | 0x7F800000
    a = -m if m < 0 else m
    if a == 0:
        return s << 31
    s = 1 if m < 0 else 0
    n = a.bit_length()
    if n <= 23:
        return (s << 31) | a
    e = n - 23
    f = a >> (e - 1)
    assert f << (e - 1) == a and e < 255, 'not a binary32'
    return (s << 31) | (e << 23) | (f & 0x7FFFFF)


def to_float32(vals, shape):
    """[(m, s)] in row-major order -> float32 array"""
    return np.array([bits_of(m, s) for m, s in vals], np.uint32).view(np.float32).reshape(shape)


# ------------------------------------------------------------------------------------------------ one rounding
def _round(S, unit):
    """S != 0, an exact value in units of 2^-unit (unit >= 149) -> (m, s), rounded half to even to binary32"""
    a = -S if S < 0 else S
    sh = a.bit_length() - 24
    if sh < unit - Q:
        sh = unit - Q                                                  # below 2^-126 the quantum stays 2^-149: denormals
    if sh > 0:
        r = a >> sh
        rem = a - (r << sh)
        half = 1 << (sh - 1)
        if rem > half or (rem == half and r & 1):
            r += 1
        m = r << (sh - (unit - Q))
    else:
        m = a
    if m >= LIM:
        return INF, int(S < 0)
    return (-m if S < 0 else m), int(S < 0)


def _special_fma(xm, xs, wm, ws, am, as_):
    if xm is None or wm is None or am is None:
        return None, 0
    ps = xs ^ ws
    if xm is INF or wm is INF:
        if (xm is not INF and xm == 0) or (wm is not INF and wm == 0):
            return None, 0                                             # 0 x inf
        if am is INF and as_ != ps:
            return None, 0                                             # inf - inf
        return INF, ps
    return am, as_                                                     # a finite product into an infinite sum


def fma(xm, xs, wm, ws, am, as_):
    """round(x * w + acc), once"""
    try:
        p = xm * wm
        if p:
            S = p + (am << Q)
            if S:
                return _round(S, 2 * Q)
            return 0, 0                                                # exact cancellation: +0 (round to nearest)
        if am == 0:
            return 0, as_ & (xs ^ ws)                                  # (+-0) + (+-0)
        return am, as_
    except TypeError:
        return _special_fma(xm, xs, wm, ws, am, as_)


def add(am, as_, bm, bs):
    """round(a + b)"""
    try:
        S = am + bm
        if S:
            return _round(S, Q)
        if am == 0 and bm == 0:
            return 0, as_ & bs
        return 0, 0
    except TypeError:
        if am is None or bm is None:
            return None, 0
        if am is INF and bm is INF:
            return (INF, as_) if as_ == bs else (None, 0)
        return (am, as_) if am is INF else (bm, bs)


def mul(xm, xs, wm, ws):
    """round(x * w): the product of a multiply-then-add (the no-fma mutation)"""
    try:
        p = xm * wm
        return _round(p, 2 * Q) if p else (0, xs ^ ws)
    except TypeError:
        if xm is None or wm is None:
            return None, 0
        if (xm is not INF and xm == 0) or (wm is not INF and wm == 0):
            return None, 0
        return INF, xs ^ ws


def relu(m, s):
    """max(v, 0), NaN propagated (np.maximum, torch.relu); a zero of either sign gives +0"""
    if m is None:
        return None, 0
    if m is INF:
        return (0, 0) if s else (INF, 0)
    return (m, 0) if m > 0 else (0, 0)


def _flush(m, s):
    if m is not None and m is not INF and -MIN_NORMAL < m < MIN_NORMAL:
        return 0, s
    return m, s


# ------------------------------------------------------------------------------------------------ the chain
MUTATIONS = ('descending', 'per_offset', 'no_fma', 'flush_inputs', 'flush_results', 'padded')


def chain(nbr, x, W, bias=None, residual=None, relu_out=False, mutation=None):
    """nbr [K, n_out] (absent: < 0), x [n_in, Cin], W [K, Cin, Cout] (or [Cin, Cout]), bias [1, Cout], residual [n_out, Cout] -> float32
    [n_out, Cout].  mutation: None (the definition) or one of MUTATIONS, each a wrong convolution a kernel could plausibly compute."""
    assert mutation is None or mutation in MUTATIONS
    nbr = np.asarray(nbr)
    W = np.asarray(W, np.float32)
    if W.ndim == 2:
        W = W[None]
    K, cin, cout = W.shape
    n_out = nbr.shape[1]
    assert nbr.shape[0] == K and np.asarray(x).shape[1] == cin
    XM, XS = parts(x)
    WM, WS = parts(np.ascontiguousarray(W.transpose(0, 2, 1)))       # [k][co][ci]
    if mutation == 'flush_inputs':
        XM = [[_flush(m, 0)[0] for m in r] for r in XM]
        WM = [[[_flush(m, 0)[0] for m in c] for c in k] for k in WM]
    BM, BS = parts(np.asarray(bias, np.float32).reshape(-1)) if bias is not None else (None, None)
    RM, RS = parts(residual) if residual is not None else (None, None)
    zero_m, zero_s = [0] * cin, [0] * cin
    ks = range(K - 1, -1, -1) if mutation == 'descending' else range(K)
    flush_out = mutation == 'flush_results'
    out = []
    nb = nbr.tolist()
    for o in range(n_out):
        rows = [(k, nb[k][o]) for k in ks if nb[k][o] >= 0 or mutation == 'padded']
        for co in range(cout):
            am, as_ = 0, 0
            for k, i in rows:
                xm, xs = (XM[i], XS[i]) if i >= 0 else (zero_m, zero_s)   # (padded: an absent neighbour lands as a row of +0)
                wm, ws = WM[k][co], WS[k][co]
                if mutation == 'per_offset':
                    dm, ds = 0, 0
                    for ci in range(cin):
                        dm, ds = fma(xm[ci], xs[ci], wm[ci], ws[ci], dm, ds)
                    am, as_ = add(am, as_, dm, ds)
                elif mutation == 'no_fma':
                    for ci in range(cin):
                        am, as_ = add(am, as_, *mul(xm[ci], xs[ci], wm[ci], ws[ci]))
                elif flush_out:
                    for ci in range(cin):
                        am, as_ = _flush(*fma(xm[ci], xs[ci], wm[ci], ws[ci], am, as_))
                else:
                    for ci in range(cin):
                        am, as_ = fma(xm[ci], xs[ci], wm[ci], ws[ci], am, as_)
            if BM is not None:
                am, as_ = add(am, as_, BM[co], BS[co])
            if RM is not None:
                am, as_ = add(am, as_, RM[o][co], RS[o][co])
            if relu_out:
                am, as_ = relu(am, as_)
            out.append((am, as_))
    return to_float32(out, (n_out, cout))


def up2(x, W, bias, mutation=None):
    """generative transpose k2 s2: row 8 i + k = chain of x[i] through W[k]"""
    n = len(x)
    ident = np.arange(n)[None]
    out = np.empty((8 * n, W.shape[2]), np.float32)
    for k in range(8):
        out[k::8] = chain(ident, x, W[k], bias, mutation=mutation)
    return out


def inception_resnet(sd, name, nbr, x):
    """cat(conv0_1(relu(conv0_0 x)), conv1_2(relu(conv1_1(relu(conv1_0 x))))) + x, every conv the exact chain, every ReLU NaN-propagating"""
    ident = np.arange(len(x))[None]
    c = lambda nm, m, v, **kw: chain(m, v, sd[f'{name}.{nm}.kernel'], sd[f'{name}.{nm}.bias'], **kw)
    half = sd[f'{name}.conv0_1.kernel'].shape[2]
    out0 = c('conv0_1', nbr, c('conv0_0', nbr, x, relu_out=True), residual=x[:, :half])
    out1 = c('conv1_2', ident, c('conv1_1', nbr, c('conv1_0', ident, x, relu_out=True), relu_out=True), residual=x[:, half:])
    return np.concatenate([out0, out1], 1)


# ------------------------------------------------------------------------------------------------ value classes
FINITE = ('denormal', 'underflow', 'near_overflow', 'wide')


def features(cls, rng, n, c):
    """the features of a finite class: [n, c] float32"""
    if cls == 'denormal':
        k = rng.integers(1, 8_000_000, (n, c)).astype(np.uint32) | (rng.integers(0, 2, (n, c)).astype(np.uint32) << 31)
        return k.view(np.float32)
    if cls == 'underflow':
        return (-rng.uniform(1, 2, (n, c)) * 1e-30).astype(np.float32)
    if cls == 'near_overflow':
        return (rng.standard_normal((n, c)) * 1e19).astype(np.float32)
    if cls == 'wide':
        return (rng.standard_normal((n, c)) * 2.0 ** rng.integers(-60, 61, (n, 1))).astype(np.float32)
    raise KeyError(cls)


def weights(cls, rng, K, cin, cout):
    """-> W [K, cin, cout], bias [1, cout] of a finite class"""
    if cls == 'denormal':
        W, _ = F64._rand_w(rng, K, cin, cout)
        return W, np.zeros((1, cout), np.float32)
    if cls == 'underflow':
        return (rng.uniform(1, 2, (K, cin, cout)) * 1e-30).astype(np.float32), np.full((1, cout), -0.0, np.float32)
    if cls == 'near_overflow':
        return (rng.uniform(-1, 1, (K, cin, cout)) * 5e16).astype(np.float32), rng.uniform(-0.1, 0.1, (1, cout)).astype(np.float32)
    if cls == 'wide':
        return rng.uniform(-1, 1, (K, cin, cout)).astype(np.float32), rng.uniform(-0.1, 0.1, (1, cout)).astype(np.float32)
    raise KeyError(cls)


def _max64(nbr, x, W):
    """max |y| of the convolution in float64 (nbr None: the transpose, every input row through every offset)"""
    x64, W64 = np.asarray(x, np.float64), np.asarray(W, np.float64)
    if nbr is None:
        return float(np.abs(np.einsum('ni,kio->kno', x64, W64)).max())
    y = np.zeros((nbr.shape[1], W.shape[2]))
    for k in range(nbr.shape[0]):
        o = np.flatnonzero(nbr[k] >= 0)
        y[o] += x64[nbr[k, o]] @ W64[k]
    return float(np.abs(y).max())


def to_near_overflow(x, nbr, W):
    """x times the power of two that puts the float64 convolution's max |y| into [1e37, 2e37): the table's scales (1e19 x 5e16) reach 1.4e37 on a
    full 27 x 16 neighbourhood; other shapes and sparser levels get the same output magnitude, 17 x below FLT_MAX (the scaling is exact)"""
    s = 2.0 ** np.ceil(np.log2(1e37 / _max64(nbr, x, W)))
    out = (np.asarray(x, np.float64) * s).astype(np.float32)
    assert np.isfinite(out).all()
    return out


def case(cls, seed, n, K, cin, cout, nbr=None):
    """-> x [n, cin], W [K, cin, cout], bias [1, cout] of a finite class for the map nbr (None: the transpose conv)"""
    rng = np.random.default_rng(seed)
    x = features(cls, rng, n, cin)
    W, b = weights(cls, rng, K, cin, cout)
    if cls == 'near_overflow':
        x = to_near_overflow(x, nbr, W)
    return x, W, b


_BLOCK = (('conv0_0', 27, 1, 4), ('conv0_1', 27, 4, 2), ('conv1_0', 1, 1, 4), ('conv1_1', 27, 4, 4), ('conv1_2', 1, 4, 2))


def block_case(cls, seed, n, C, k3):
    """-> (state dict of one InceptionResNet block under the prefix 'b', x [n, C]) of a finite class.  near_overflow: the class weights sit in
    the two convs that read x (their sums are the ones near FLT_MAX: x is scaled on conv0_0), the later convs carry F64._rand_w so that the
    block stays finite"""
    rng = np.random.default_rng(seed)
    sd = {}
    for nm, K, di, do in _BLOCK:
        W, b = weights(cls, rng, K, C // di, C // do)
        if cls == 'near_overflow' and nm not in ('conv0_0', 'conv1_0'):
            W, b = F64._rand_w(rng, K, C // di, C // do)
        sd[f'b.{nm}.kernel'], sd[f'b.{nm}.bias'] = (W[0] if K == 1 else W), b
    x = features(cls, rng, n, C)
    if cls == 'near_overflow':
        x = to_near_overflow(x, k3, sd['b.conv0_0.kernel'])
    return sd, x


def neg_zero(y):
    return np.asarray(y, np.float32).view(np.uint32) == 0x80000000


def denormal(y):
    a = np.asarray(y, np.float32).view(np.uint32) & 0x7FFFFFFF
    return (a > 0) & (a < MIN_NORMAL)


def precondition(cls, y):
    """asserted on the DEFINITION's output y of a k3 conv of the class: the class is what its name says (the figures: tests/test_value_edges_cpu.py)"""
    y = np.asarray(y, np.float32)
    if cls == 'denormal':
        share = denormal(y).mean()
        assert share >= 0.5, f'denormal: {share:.2f} of the outputs are non-zero denormals'
    elif cls == 'underflow':
        share = neg_zero(y).mean()
        assert share >= 0.5, f'underflow: {share:.2f} of the outputs are -0'
    elif cls == 'near_overflow':
        assert np.isfinite(y).all() and np.abs(y).max() >= 1e37, f'near_overflow: max |y| {np.abs(y).max():.3g}'
        share = None
    else:
        share = None
    return share


def flip_zero_signs(rng, x):
    """x with the sign of every exact-zero feature drawn again (the values are unchanged)"""
    u = np.array(x, np.float32).view(np.uint32)
    z = (u & 0x7FFFFFFF) == 0
    u[z] = rng.integers(0, 2, int(z.sum())).astype(np.uint32) << 31
    return u.view(np.float32)


def with_zeros(rng, x, share=0.15):
    """x with `share` of its elements, and one row in eight entirely, set to +0: what flip_zero_signs acts on"""
    x = np.array(x, np.float32)
    x[rng.random(x.shape) < share] = 0
    x[::8] = 0
    return x


def nonfinite_rows(x, rows):
    """x with rows[0] = +inf in one element, rows[1] = -inf, rows[2] = NaN, rows[3] = one element of 3.0e38 (it overflows in the chain once a
    weight exceeds 1.14 in magnitude or another term joins it); the other elements of those rows stay as they are"""
    x = np.array(x, np.float32)
    c = x.shape[1]
    for r, v, col in zip(rows, (np.inf, -np.inf, np.nan, 3.0e38), (0, c // 3, c // 2, c - 1)):
        x[r, col] = v
    return x


def differing(a, b):
    """share of elements whose BITS differ"""
    return float((np.asarray(a, np.float32).view(np.uint32) != np.asarray(b, np.float32).view(np.uint32)).mean())
