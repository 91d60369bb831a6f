"""A plain float64 definition of the sparse convolutions of PCGCv2, for tests (a helper module, like third_party_vectors.py).

Independent of the oracle and of the product's kernel maps: neighbours are found here by `np.searchsorted` over linearised
(batch, x, y, z) keys, and every operator is written as MinkowskiEngine defines it:

    k3 conv at tensor stride s     out[p] = b + sum_d W[k(d)]^T x[p + s d],  d in {-1, 0, 1}^3, present neighbours only
    k1 conv                        out[p] = b + W^T x[p]
    k2 s2 down conv (stride s)     coarse q = floor(c / 2s) 2s;  out[q] = b + sum_d W[k(d)]^T x[q + s d],  d in {0, 1}^3
    k2 s2 generative transpose     child j of p = p + (s/2) d(j);  out[child j of p] = b + W[j]^T x[p]

k(d) is the kernel offset index of `conventions.get('kernel_offset_order')` ('xyz': x fastest, 'zyx': z fastest).

Every operator takes and returns (value, bound) pairs: `e` bounds |fp32 result - this fp64 value| for ANY fp32 summation order, with or
without FMA (Higham, Accuracy and Stability of Numerical Algorithms, eq. 3.5), given inputs within `e_in` of the values passed:
    conv      e_out = g_n (|W| * (|x| + e_in) + |b|) + |W| * e_in,   g_n = n u / (1 - n u),  n = K Cin + 1,  u = 2^-24
    relu      e unchanged;   cat: the bounds concatenated;   residual add: (e1 + e2) + u (|y| + e1 + e2)
(`*` the same convolution).  BOUND_SLACK covers the second-order terms and the fp64 evaluation itself."""
import numpy as np

from pcgcv2_amd import conventions

U = 2.0 ** -24
BOUND_SLACK = 1.01


# ------------------------------------------------------------------------------------------------ coordinates
def keys(coords):
    """(batch, x, y, z) int rows -> uint64 keys (20 bits per axis, 4 of batch); rows outside [0, 2^20) get the key ABSENT"""
    c = np.asarray(coords, np.int64)
    ok = ((c[:, 1:] >= 0) & (c[:, 1:] < (1 << 20))).all(1) & (c[:, 0] >= 0) & (c[:, 0] < 16)
    cu = np.where(ok[:, None], c, 0).astype(np.uint64)
    k = (cu[:, 0] << np.uint64(60)) | (cu[:, 1] << np.uint64(40)) | (cu[:, 2] << np.uint64(20)) | cu[:, 3]
    return np.where(ok, k, ABSENT)


ABSENT = np.uint64(0xFFFFFFFFFFFFFFFF)


def lookup(coords, query):
    """row of `coords` holding each row of `query`, -1 where there is none (coords: unique rows)"""
    kc, kq = keys(coords), keys(query)
    if len(kc) == 0:
        return np.full(len(kq), -1, np.int64)
    order = np.argsort(kc, kind='stable')
    sk = kc[order]
    pos = np.minimum(np.searchsorted(sk, kq), len(sk) - 1)
    return np.where((sk[pos] == kq) & (kq != ABSENT), order[pos], -1)


def offsets(n):
    """[n^3, 3] offset d(k) per kernel index k of an n x n x n kernel (n = 3: d in {-1,0,1}, n = 2: d in {0,1}), by the offset-order convention"""
    lo = -1 if n == 3 else 0
    k = np.arange(n ** 3)
    fast, mid, slow = k % n + lo, (k // n) % n + lo, k // (n * n) + lo
    if conventions.get('kernel_offset_order') == 'xyz':
        return np.stack([fast, mid, slow], 1)
    return np.stack([slow, mid, fast], 1)


def neighbour_map(coords_out, coords_in, deltas):
    """[K, n_out] rows of coords_in at coords_out + deltas[k] (batch unchanged), -1 = absent"""
    c = np.asarray(coords_out, np.int64)
    out = np.empty((len(deltas), len(c)), np.int64)
    for k, d in enumerate(np.asarray(deltas, np.int64)):
        q = c.copy()
        q[:, 1:] += d
        out[k] = lookup(coords_in, q)
    return out


def down_coords(coords, stride):
    """coarse coordinates of a k2 s2 conv on a level of tensor stride `stride`: floor(c / 2s) 2s, unique, in first-occurrence order"""
    c = np.asarray(coords, np.int64).copy()
    c[:, 1:] = np.floor_divide(c[:, 1:], 2 * stride) * (2 * stride)
    _, first = np.unique(keys(c), return_index=True)
    return c[np.sort(first)]


def children_coords(coords, stride):
    """children of a generative transpose k2 s2 on a level of tensor stride `stride`: row 8 i + j = coords[i] + (stride / 2) d(j)"""
    c = np.asarray(coords, np.int64)
    d = offsets(2) * (stride // 2)
    out = np.repeat(c, 8, axis=0)
    out[:, 1:] += np.tile(d, (len(c), 1))
    return out


# ------------------------------------------------------------------------------------------------ operators: (value, bound)
def _conv(nbr, x, e, W, b):
    """out[o] = b + sum_k W[k]^T x[nbr[k, o]] over present rows, and its bound.  W [K, Cin, Cout]; b [1, Cout] or None."""
    x, e = np.asarray(x, np.float64), np.asarray(e, np.float64)
    W = np.asarray(W, np.float64)
    K, cin, cout = W.shape
    y = np.zeros((nbr.shape[1], cout))
    mag = np.zeros_like(y)                                    # |W| * (|x| + e)
    prop = np.zeros_like(y)                                   # |W| * e
    ax, aW = np.abs(x) + e, np.abs(W)
    for k in range(K):
        rows = np.nonzero(nbr[k] >= 0)[0]
        src = nbr[k, rows]
        y[rows] += x[src] @ W[k]
        mag[rows] += ax[src] @ aW[k]
        prop[rows] += e[src] @ aW[k]
    if b is not None:
        b = np.asarray(b, np.float64).reshape(1, -1)
        y += b
        mag += np.abs(b)
    n = K * cin + 1
    g = n * U / (1 - n * U)
    return y, BOUND_SLACK * (g * mag + prop)


def zero_bound(x):
    return np.zeros(np.shape(x))


_LAST_K3 = [None]


def k3_map(coords, dilation):
    """neighbour_map of a k3 conv; the last one is kept (an InceptionResNet runs three convs on one level)"""
    key = (conventions.get('kernel_offset_order'), int(dilation))
    hit = _LAST_K3[0]
    if hit is None or hit[0] != key or hit[1] is not coords:
        hit = _LAST_K3[0] = (key, coords, neighbour_map(coords, coords, offsets(3) * dilation))
    return hit[2]


def conv3(coords, stride, x, e, W, b, dilation=None):
    """k3 conv at tensor stride `stride` (neighbours at p + dilation d; dilation defaults to the stride, as in ME)"""
    return _conv(k3_map(coords, stride if dilation is None else dilation), x, e, W, b)


def conv1(x, e, W, b):
    W = np.asarray(W)
    nbr = np.arange(len(x))[None]
    return _conv(nbr, x, e, W.reshape(1, *W.shape[-2:]), b)


def down(coords, stride, x, e, W, b):
    """k2 s2 conv -> (coarse coords, value, bound)"""
    coarse = down_coords(coords, stride)
    y, ey = _conv(neighbour_map(coarse, coords, offsets(2) * stride), x, e, W, b)
    return coarse, y, ey


def up(coords, stride, x, e, W, b):
    """k2 s2 generative transpose -> (children coords, value, bound); child j of row i is row 8 i + j"""
    kids = children_coords(coords, stride)
    n = len(coords)
    W = np.asarray(W)
    ys, es = zip(*(_conv(np.arange(n)[None], x, e, W[j:j + 1], b) for j in range(8)))
    y = np.stack(ys, 1).reshape(8 * n, -1)
    return kids, y, np.stack(es, 1).reshape(8 * n, -1)


def relu(y, e):
    return np.maximum(y, 0.0), e


def cat(a, ea, b, eb):
    return np.concatenate([a, b], 1), np.concatenate([ea, eb], 1)


def residual(y1, e1, y2, e2):
    y, e = y1 + y2, e1 + e2
    return y, BOUND_SLACK * (e + U * (np.abs(y) + e))


# ------------------------------------------------------------------------------------------------ the model (autoencoder.py)
def _c3(sd, name, coords, stride, x, e):
    return conv3(coords, stride, x, e, sd[name + '.kernel'], sd[name + '.bias'])


def _c1(sd, name, x, e):
    return conv1(x, e, sd[name + '.kernel'], sd[name + '.bias'])


def inception_resnet(sd, name, coords, stride, x, e):
    """autoencoder.py:52-57: cat(conv0_1(relu(conv0_0 x)), conv1_2(relu(conv1_1(relu(conv1_0 x))))) + x"""
    a = _c3(sd, name + '.conv0_1', coords, stride, *relu(*_c3(sd, name + '.conv0_0', coords, stride, x, e)))
    h = relu(*_c1(sd, name + '.conv1_0', x, e))
    c = _c1(sd, name + '.conv1_2', *relu(*_c3(sd, name + '.conv1_1', coords, stride, *h)))
    return residual(*cat(*a, *c), x, e)


def _keep(name, y, e):
    return y, e


def block(sd, name, coords, stride, x, e, tap=_keep):
    for i in range(3):                                        # make_layer(block_layers=3), autoencoder.py:59-66
        x, e = tap(f'{name}.{i}', *inception_resnet(sd, f'{name}.{i}', coords, stride, x, e))
    return x, e


def encoder_level(sd, i, coords, stride, x, e, tap=_keep, prefix='encoder'):
    """level i of autoencoder.py:138-147: relu(conv_i) -> relu(down_i) -> block_i  ->  (coarse coords, value, bound).
    tap(stage name, value, bound) -> (value, bound) sees every stage a fused kernel computes (a conv with its ReLU, one InceptionResNet)
    and may hand on another input: a test hands on the fp32 value under test with bound 0, so that each stage is checked on its own
    input (bounds propagated through a whole level grow by |W| at every conv and stop being informative)."""
    x, e = tap(f'{prefix}.conv{i}', *relu(*_c3(sd, f'{prefix}.conv{i}', coords, stride, x, e)))
    coarse, y, ey = down(coords, stride, x, e, sd[f'{prefix}.down{i}.kernel'], sd[f'{prefix}.down{i}.bias'])
    x, e = tap(f'{prefix}.down{i}', *relu(y, ey))
    return (coarse,) + block(sd, f'{prefix}.block{i}', coarse, 2 * stride, x, e, tap)


def encoder_forward(sd, coords, x, e=None, stride=1, tap=_keep, prefix='encoder'):
    """autoencoder.py:138-147 -> [(C8, y, e), (C4, out1, e), (C2, out0, e)] like the reference's [out2, out1, out0]"""
    e = zero_bound(x) if e is None else e
    outs = []
    for i in range(3):
        coords, x, e = encoder_level(sd, i, coords, stride, x, e, tap, prefix)
        stride *= 2
        outs.append((coords, x, e))
    y, ey = _c3(sd, f'{prefix}.conv3', coords, stride, x, e)
    tap(f'{prefix}.conv3', y, ey)                             # (the last stage: its fp64 value and bound are returned)
    return [(coords, y, ey), outs[1], outs[0]]


def decoder_level(sd, l, coords, stride, x, e, tap=_keep, prefix='decoder'):
    """level l of autoencoder.py:251-273 before the pruning: relu(up_l) -> relu(conv_l) -> block_l -> conv_l_cls.
    -> (children coords, features, bound, logits, logit bound); the children have tensor stride stride / 2.  tap: as in encoder_level."""
    kids, y, ey = up(coords, stride, x, e, sd[f'{prefix}.up{l}.kernel'], sd[f'{prefix}.up{l}.bias'])
    s = stride // 2
    h = tap(f'{prefix}.up{l}', *relu(y, ey))
    h = tap(f'{prefix}.conv{l}', *relu(*_c3(sd, f'{prefix}.conv{l}', kids, s, *h)))
    f, ef = block(sd, f'{prefix}.block{l}', kids, s, *h, tap=tap)
    cls, ecls = _c3(sd, f'{prefix}.conv{l}_cls', kids, s, f, ef)
    tap(f'{prefix}.conv{l}_cls', cls, ecls)                   # (the last stage: its fp64 value and bound are returned)
    return kids, f, ef, cls, ecls


# ------------------------------------------------------------------------------------------------ checks
def within(got, want, bound):
    """max |got - want| / bound (0 where both are 0; inf where the bound is 0 and they differ) — <= 1 means within the bound"""
    d = np.abs(np.asarray(got, np.float64) - want)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(d == 0, 0.0, d / bound)
    return float(r.max()) if r.size else 0.0


def topk_violation(mask, logits, bound):
    """largest (dropped logit - kept logit - (e_kept + e_dropped)) over every kept / dropped pair; <= 0 means `mask` is a valid top-k of
    the fp64 logits up to the bounds: every kept row's logit + bound >= every dropped row's logit - bound."""
    mask = np.asarray(mask, bool)
    l, e = np.asarray(logits, np.float64).ravel(), np.asarray(bound, np.float64).ravel()
    if mask.all() or not mask.any():
        return -np.inf
    return float((l[~mask] - e[~mask]).max() - (l[mask] + e[mask]).min())


def rounding_mismatch_outside_bound(got, want, bound):
    """number of entries where round(got) != round(want) although want is farther than `bound` from every half-integer"""
    got, want = np.asarray(got), np.asarray(want, np.float64)
    diff = np.rint(got) != np.rint(want)
    dist = np.abs(want - (np.floor(want) + 0.5))
    return int((diff & (dist > bound)).sum())
