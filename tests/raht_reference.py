"""The colour format's definition: integer lifting RAHT on YCoCg-R, its quantiser, tokens, tables and the `_A.bin` container, in numpy
integers.  The kernels (pcgcv2_amd/csrc/raht.hip), DESIGN.md 8j and include/pcgc_hip.h follow THIS file; the device tests hold every array
the kernels produce to equality with what is computed here.  Nothing in here is floating point except `isqrt`'s first guess (corrected to
the exact integer root, and checked against math.isqrt) and the orthonormal fp64 RAHT at the end, which is a yardstick, not the format.

Colour space  YCoCg-R (>> is the arithmetic shift):  Co = R - B; t = B + (Co >> 1); Cg = G - t; Y = t + (Cg >> 1)
              inverse: t = Y - (Cg >> 1); G = Cg + t; B = t - (Co >> 1); R = B + Co; clamp to 0 .. 255
Order         Morton key: bit 3 i + 0 / 1 / 2 = bit i of x / y / z, coordinates in [0, 2^20); distinct voxels, sorted ascending
Tree          gap i (between sorted leaves i and i + 1) is one merge: split bit d = msb(key_i ^ key_{i+1}); range [lo, hi] = the maximal run
              around the gap whose other gaps have a smaller d; w1 = i - lo + 1, w2 = hi - i; children = the gap of largest d in
              [lo, i - 1] and in [i + 1, hi - 1], or a leaf where that run is empty (a child c >= 0 is a gap, c < 0 the leaf ~c)
Lifting       H = a2 - a1; L = a1 + floor(w2 H / (w1 + w2));  inverse a1 = L - floor(w2 H^ / (w1 + w2)); a2 = a1 + H^;  root L = DC
Quantiser     D16 = 16 if Q = 0 else max(16, isqrt(floor(256 Q^2 (w1 + w2) / (w1 w2)))); k = sign(H) floor((32 |H| + D16) / (2 D16));
              H^ = sign(k) floor((|k| D16 + 8) / 16)
Tokens        z = 2 k (k >= 0) or -2 k - 1; token = min(z, 63); token 63 sends z - 63 as 10 raw bits; ctx = 16 channel + min(d // 3, 15);
              coding order: gaps by d descending then index ascending, Y, Co, Cg within a gap
Tables        semi-static, one row of 64 frequencies per context that occurs: 0 where the count is 0, else max(1, floor(count 65536 /
              total)), the difference to 65536 added to (taken from) the most frequent token, lowest index on a tie; token 63 counts as
              seen at least once (see `frequencies`)
`_A.bin`      "PCGA" | u32 version 1 | u32 N | u16 Q_luma | u16 Q_chroma | 3 x i16 DC | u16 R | R x (u16 ctx, 63 x u16 cdf[1..63]) |
              u64 tokens = 3 (N - 1) | u64 payload bytes | u64 escapes | payload (rc_encode_ctx; empty when there is no token) | escapes,
              10 bits each, LSB first, zero-padded to a byte | u32 CRC-32 of all that precedes.  Little endian.
"""
import math
import struct

import numpy as np

MAX_POINTS = 1 << 24
COORD_BITS = 20
ESCAPE = 63
ESCAPE_BITS = 10
CONTEXTS = 48
MAGIC, VERSION = b'PCGA', 1
HEAD = struct.Struct('<4sIIHH3hH')
SIZES = struct.Struct('<3Q')


# ---------------------------------------------------------------------------------------------------------------- colour space
def ycocg_forward(rgb):
    """uint8 [N,3] -> int64 [N,3] (Y, Co, Cg)"""
    rgb = np.asarray(rgb).astype(np.int64)
    r, g, b = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    co = r - b
    t = b + (co >> 1)
    cg = g - t
    y = t + (cg >> 1)
    return np.stack([y, co, cg], 1)


def ycocg_inverse(ycc):
    """int [N,3] -> uint8 [N,3], clamped"""
    ycc = np.asarray(ycc).astype(np.int64)
    y, co, cg = ycc[:, 0], ycc[:, 1], ycc[:, 2]
    t = y - (cg >> 1)
    g = cg + t
    b = t - (co >> 1)
    r = b + co
    return np.clip(np.stack([r, g, b], 1), 0, 255).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------- order
def _spread3(v):
    v = v.astype(np.uint64) & np.uint64(0x1FFFFF)
    v = (v | (v << np.uint64(32))) & np.uint64(0x1F00000000FFFF)
    v = (v | (v << np.uint64(16))) & np.uint64(0x1F0000FF0000FF)
    v = (v | (v << np.uint64(8))) & np.uint64(0x100F00F00F00F00F)
    v = (v | (v << np.uint64(4))) & np.uint64(0x10C30C30C30C30C3)
    v = (v | (v << np.uint64(2))) & np.uint64(0x1249249249249249)
    return v


def morton_keys(xyz):
    """int [N,3] (x, y, z) in [0, 2^20) -> uint64 [N]"""
    xyz = np.asarray(xyz).astype(np.int64)
    if xyz.size and (xyz.min() < 0 or xyz.max() >= 1 << COORD_BITS):
        raise ValueError('coordinates outside [0, 2^20)')
    return _spread3(xyz[:, 0]) | (_spread3(xyz[:, 1]) << np.uint64(1)) | (_spread3(xyz[:, 2]) << np.uint64(2))


def msb(v):
    """index of the highest set bit of uint64 v > 0"""
    v = np.asarray(v, np.uint64).copy()
    r = np.zeros(v.shape, np.int64)
    for s in (32, 16, 8, 4, 2, 1):
        big = v >= (np.uint64(1) << np.uint64(s))
        r += np.where(big, s, 0)
        v = np.where(big, v >> np.uint64(s), v)
    return r


def sort_cloud(xyz):
    """-> (sorted keys, perm): leaf i is row perm[i]"""
    keys = morton_keys(xyz)
    if keys.size > MAX_POINTS:
        raise ValueError('more than 2^24 points')
    perm = np.argsort(keys, kind='stable')
    keys = keys[perm]
    if keys.size > 1 and (keys[1:] == keys[:-1]).any():
        raise ValueError('duplicate voxels')
    return keys, perm.astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------- tree
def naive_merges(keys):
    """siblings merged bit by bit from bit 0 upwards -> int64 [N-1, 4] rows (d, gap, w1, w2) in the order the merges happen
    (bit ascending, position ascending)"""
    keys = np.asarray(keys, np.uint64)
    first = np.arange(keys.size, dtype=np.int64)               # first leaf of each current node
    weight = np.ones(keys.size, np.int64)
    node_key = keys.copy()
    out = []
    for b in range(3 * COORD_BITS):
        if node_key.size < 2:
            break
        up = node_key >> np.uint64(b + 1)
        pair = np.flatnonzero(up[1:] == up[:-1])               # node j and j + 1 are siblings at this bit (never three: keys are distinct)
        if pair.size:
            out.append(np.stack([np.full(pair.size, b, np.int64), first[pair + 1] - 1, weight[pair], weight[pair + 1]], 1))
            weight[pair] += weight[pair + 1]
            keep = np.ones(node_key.size, bool)
            keep[pair + 1] = False
            first, weight, node_key = first[keep], weight[keep], node_key[keep]
    return np.concatenate(out) if out else np.zeros((0, 4), np.int64)


def _nearest_greater(d):
    """for every gap: index of the nearest gap to the left / right with a larger d (-1 / len(d) where there is none)"""
    n = d.size
    left = np.full(n, -1, np.int64)
    right = np.full(n, n, np.int64)
    for b in np.unique(d)[::-1]:
        above = np.flatnonzero(d > b)
        here = np.flatnonzero(d == b)
        if above.size:
            p = np.searchsorted(above, here)
            left[here] = np.where(p > 0, above[np.maximum(p - 1, 0)], -1)
            right[here] = np.where(p < above.size, above[np.minimum(p, above.size - 1)], n)
    return left, right


def build_tree(keys, check=True):
    """sorted distinct keys -> dict of int64 arrays over the gaps: d, lo, hi, w1, w2, left, right; `order` (gaps in coding order) and
    `bucket` [65] (the gaps of split bit d are order[bucket[63 - d] : bucket[64 - d]])"""
    keys = np.asarray(keys, np.uint64)
    n = keys.size
    g = max(n - 1, 0)
    idx = np.arange(g, dtype=np.int64)
    d = msb(keys[1:] ^ keys[:-1]) if g else np.zeros(0, np.int64)
    gl, gr = _nearest_greater(d)
    lo, hi = gl + 1, gr
    # children: every gap hangs under whichever of its two nearest greater gaps has the smaller d; every leaf under the lower of the two gaps
    # beside it
    left = np.full(g, np.iinfo(np.int64).min, np.int64)
    right = left.copy()
    if g:
        dl = np.where(gl >= 0, d[np.maximum(gl, 0)], 99)
        dr = np.where(gr < g, d[np.minimum(gr, g - 1)], 99)
        root = (gl < 0) & (gr >= g)
        under_left = ~root & (dl < dr)                          # the parent lies to the left: this gap is its right child
        right[gl[under_left]] = idx[under_left]
        under_right = ~root & ~under_left
        left[gr[under_right]] = idx[under_right]
        leaf = np.arange(n, dtype=np.int64)
        dl = np.where(leaf > 0, d[np.maximum(leaf - 1, 0)], 99)
        dr = np.where(leaf < g, d[np.minimum(leaf, g - 1)], 99)
        ul = dl < dr
        right[leaf[ul] - 1] = ~leaf[ul]
        left[leaf[~ul]] = ~leaf[~ul]
        assert (left != np.iinfo(np.int64).min).all() and (right != np.iinfo(np.int64).min).all()
    order = np.argsort(63 - d, kind='stable')
    bucket = np.concatenate([[0], np.cumsum(np.bincount(63 - d, minlength=64))]).astype(np.int64)
    tree = dict(n=n, d=d, lo=lo, hi=hi, w1=idx - lo + 1, w2=hi - idx, left=left, right=right, order=order, bucket=bucket)
    if check:
        naive = naive_merges(keys)
        mine = np.stack([d, idx, tree['w1'], tree['w2']], 1)[np.lexsort((idx, d))]
        assert np.array_equal(naive, mine), 'the gap formulation and the bit-by-bit merge disagree'
    return tree


# ---------------------------------------------------------------------------------------------------------------- lifting
def forward(tree, values):
    """leaf values int [N,3] in sorted order -> (H int64 [N-1,3], DC int64 [3])"""
    val = np.asarray(values).astype(np.int64).copy()
    H = np.zeros((max(tree['n'] - 1, 0), 3), np.int64)
    d, lo, w1, w2 = tree['d'], tree['lo'], tree['w1'], tree['w2']
    for b in np.unique(d):
        g = np.flatnonzero(d == b)
        a1, a2 = val[lo[g]], val[g + 1]
        h = a2 - a1
        H[g] = h
        val[lo[g]] = a1 + (w2[g, None] * h) // (w1[g] + w2[g])[:, None]
    return H, val[0].copy()


def inverse(tree, Hhat, dc):
    """-> leaf values int64 [N,3] in sorted order (node values are int32 in the format: 64-bit products, 32-bit stores)"""
    n = tree['n']
    val = np.zeros((n, 3), np.int64)
    val[0] = dc
    Hhat = np.asarray(Hhat).astype(np.int64)
    d, lo, w1, w2 = tree['d'], tree['lo'], tree['w1'], tree['w2']
    for b in np.unique(d)[::-1]:
        g = np.flatnonzero(d == b)
        a1 = val[lo[g]] - (w2[g, None] * Hhat[g]) // (w1[g] + w2[g])[:, None]
        a1 = a1.astype(np.int32).astype(np.int64)
        val[lo[g]] = a1
        val[g + 1] = (a1 + Hhat[g]).astype(np.int32).astype(np.int64)
    return val


# ---------------------------------------------------------------------------------------------------------------- quantiser
def isqrt(v):
    """floor(sqrt(v)) of int64 v in [0, 2^62), exact"""
    v = np.asarray(v, np.int64)
    r = np.sqrt(v.astype(np.float64)).astype(np.int64)
    for _ in range(2):
        r = np.where(r * r > v, r - 1, r)
        r = np.where((r + 1) * (r + 1) <= v, r + 1, r)
    assert ((r * r <= v) & ((r + 1) * (r + 1) > v)).all()
    return r


def delta16(Q, w1, w2):
    """the step of a node of weights (w1, w2) in sixteenths"""
    w1, w2 = np.asarray(w1, np.int64), np.asarray(w2, np.int64)
    if Q == 0:
        return np.full(w1.shape, 16, np.int64)
    return np.maximum(16, isqrt((256 * int(Q) * int(Q) * (w1 + w2)) // (w1 * w2)))


def delta16_exact(Q, w1, w2):
    """the same in Python integers (math.isqrt), one node"""
    return 16 if Q == 0 else max(16, math.isqrt((256 * Q * Q * (w1 + w2)) // (w1 * w2)))


def quantize(H, D16):
    H = np.asarray(H, np.int64)
    return np.sign(H) * ((32 * np.abs(H) + D16) // (2 * D16))


def dequantize(k, D16):
    k = np.asarray(k, np.int64)
    return np.sign(k) * ((np.abs(k) * D16 + 8) // 16)


def steps(tree, q_luma, q_chroma):
    """D16 [N-1,3]"""
    dl = delta16(q_luma, tree['w1'], tree['w2'])
    dc = delta16(q_chroma, tree['w1'], tree['w2'])
    return np.stack([dl, dc, dc], 1)


# ---------------------------------------------------------------------------------------------------------------- tokens
def tokens(tree, k):
    """levels k [N-1,3] per gap -> (token int16 [3(N-1)], ctx uint16 [3(N-1)], escapes uint16 [E], histogram int64 [48,64]), coding order"""
    order = tree['order']
    k = np.asarray(k, np.int64)[order]
    z = np.where(k >= 0, 2 * k, -2 * k - 1)
    tok = np.minimum(z, ESCAPE)
    ctx = 16 * np.arange(3)[None, :] + np.minimum(tree['d'][order] // 3, 15)[:, None]
    tok, ctx, z = tok.reshape(-1), ctx.reshape(-1), z.reshape(-1)
    esc = (z[tok == ESCAPE] - ESCAPE)
    assert esc.size == 0 or esc.max() < 1 << ESCAPE_BITS
    hist = np.zeros((CONTEXTS, 64), np.int64)
    np.add.at(hist, (ctx, tok), 1)
    return tok.astype(np.int16), ctx.astype(np.uint16), esc.astype(np.uint16), hist


def levels(tree, tok, esc):
    """the inverse of `tokens` -> k [N-1,3] per gap"""
    tok = np.asarray(tok).astype(np.int64)
    z = tok.copy()
    at = np.flatnonzero(tok == ESCAPE)
    if at.size != np.asarray(esc).size:
        raise ValueError(f'{at.size} escape tokens but {np.asarray(esc).size} escapes')
    z[at] += np.asarray(esc).astype(np.int64)
    k = np.where(z & 1, -(z + 1) // 2, z // 2).reshape(-1, 3)
    out = np.zeros_like(k)
    out[tree['order']] = k
    return out


# ---------------------------------------------------------------------------------------------------------------- tables
def frequencies(counts):
    """counts int [64] (total > 0) -> int64 [64] summing to 65536, 0 exactly where the count is 0 — except the escape token 63, which is
    counted at least once: a row is stored as 16-bit cumulative entries 1 .. 63 (and handed to the range coder as such), and entry 63 could
    not say 65536, which is what it would have to say in every row whose escape token never occurs."""
    counts = np.asarray(counts, np.int64).copy()
    counts[ESCAPE] = max(int(counts[ESCAPE]), 1)
    total = int(counts.sum())
    f = np.where(counts > 0, np.maximum(1, (counts * 65536) // total), 0)
    f[int(np.argmax(counts))] += 65536 - int(f.sum())
    return f


def cdf_table(hist):
    """histogram [48,64] -> (rows: the contexts that occur, uint16 table [48,65] in rc_encode_ctx's convention: entry 0 is 0, entry 64
    stands for 0x10000)"""
    table = np.zeros((CONTEXTS, 65), np.uint16)
    rows = [c for c in range(CONTEXTS) if hist[c].sum() > 0]
    for c in rows:
        table[c, 1:] = (np.cumsum(frequencies(hist[c])) & 0xFFFF).astype(np.uint16)
    return rows, table


# ---------------------------------------------------------------------------------------------------------------- container
def pack_escapes(esc):
    bits = ((np.asarray(esc, np.uint16)[:, None] >> np.arange(ESCAPE_BITS, dtype=np.uint16)) & 1).astype(np.uint8).reshape(-1)
    return np.packbits(bits, bitorder='little').tobytes()


def unpack_escapes(data, count):
    bits = np.unpackbits(np.frombuffer(data, np.uint8), bitorder='little')[:count * ESCAPE_BITS].reshape(count, ESCAPE_BITS)
    return (bits.astype(np.uint16) << np.arange(ESCAPE_BITS, dtype=np.uint16)).sum(1).astype(np.uint16)


def pack_stream(n, q_luma, q_chroma, dc, rows, table, n_tokens, payload, esc, crc32):
    blob = HEAD.pack(MAGIC, VERSION, n, q_luma, q_chroma, int(dc[0]), int(dc[1]), int(dc[2]), len(rows))
    for c in rows:
        blob += struct.pack('<H', c) + table[c, 1:64].astype('<u2').tobytes()
    blob += SIZES.pack(n_tokens, len(payload), len(esc)) + payload + pack_escapes(esc)
    return blob + struct.pack('<I', crc32(blob))


def encode(xyz, rgb, q_luma, q_chroma, rc_encode_ctx, crc32):
    """the bytes of `_A.bin` for rows (x, y, z) with colours rgb, and the colours a decoder gets back, in the caller's row order"""
    keys, perm = sort_cloud(xyz)
    tree = build_tree(keys)
    H, dc = forward(tree, ycocg_forward(np.asarray(rgb)[perm]))
    D16 = steps(tree, q_luma, q_chroma)
    k = quantize(H, D16)
    tok, ctx, esc, hist = tokens(tree, k)
    rows, table = cdf_table(hist)
    payload = rc_encode_ctx(table, ctx, tok) if tok.size else b''
    blob = pack_stream(keys.size, q_luma, q_chroma, dc, rows, table, tok.size, payload, esc, crc32)
    out = np.zeros((keys.size, 3), np.uint8)
    out[perm] = ycocg_inverse(inverse(tree, dequantize(k, D16), dc))
    return blob, out


def decode(xyz, blob, rc_decode_ctx, crc32):
    """-> uint8 [N,3] in the row order of xyz (the checks a decoder owes a damaged file are attributes.py's; this reads a sound one)"""
    keys, perm = sort_cloud(xyz)
    tree = build_tree(keys, check=False)
    assert struct.unpack('<I', blob[-4:])[0] == crc32(blob[:-4])
    magic, version, n, ql, qc, y, co, cg, R = HEAD.unpack_from(blob, 0)
    assert (magic, version, n) == (MAGIC, VERSION, keys.size)
    table = np.zeros((CONTEXTS, 65), np.uint16)
    pos = HEAD.size
    for _ in range(R):
        c = struct.unpack_from('<H', blob, pos)[0]
        table[c, 1:64] = np.frombuffer(blob, '<u2', 63, pos + 2)
        pos += 128
    n_tok, n_pay, n_esc = SIZES.unpack_from(blob, pos)
    pos += SIZES.size
    order = tree['order']
    ctx = (16 * np.arange(3)[None, :] + np.minimum(tree['d'][order] // 3, 15)[:, None]).reshape(-1).astype(np.uint16)
    tok = rc_decode_ctx(table, ctx, blob[pos:pos + n_pay]) if n_tok else np.zeros(0, np.int16)
    esc = unpack_escapes(blob[pos + n_pay:-4], n_esc)
    k = levels(tree, tok, esc)
    out = np.zeros((keys.size, 3), np.uint8)
    out[perm] = ycocg_inverse(inverse(tree, dequantize(k, steps(tree, ql, qc)), (y, co, cg)))
    return out


# ---------------------------------------------------------------------------------------------------------------- yardstick
def orthonormal_luma_mse(tree, luma, Q):
    """the textbook orthonormal RAHT in fp64 with a uniform step Q on every AC coefficient (DC exact) -> (MSE of the reconstruction,
    first-order entropy of the levels in bit per coefficient)"""
    d, lo, w1, w2 = tree['d'], tree['lo'], tree['w1'].astype(np.float64), tree['w2'].astype(np.float64)
    val = np.asarray(luma, np.float64).copy()
    n = val.size
    coef = np.zeros(n - 1)
    bits = np.unique(d)
    a, b = np.sqrt(w1 / (w1 + w2)), np.sqrt(w2 / (w1 + w2))
    for bit in bits:
        g = np.flatnonzero(d == bit)
        x1, x2 = val[lo[g]], val[g + 1]
        val[lo[g]] = a[g] * x1 + b[g] * x2
        coef[g] = -b[g] * x1 + a[g] * x2
    k = np.round(coef / Q)
    rec = np.zeros(n)
    rec[0] = val[0]
    for bit in bits[::-1]:
        g = np.flatnonzero(d == bit)
        low, high = rec[lo[g]], k[g] * Q
        rec[lo[g]] = a[g] * low - b[g] * high
        rec[g + 1] = b[g] * low + a[g] * high
    return float(np.mean((rec - np.asarray(luma, np.float64)) ** 2)), entropy(k)


def entropy(symbols):
    _, c = np.unique(np.asarray(symbols), return_counts=True)
    p = c / c.sum()
    return float(-(p * np.log2(p)).sum())


def lifting_luma_mse(tree, luma, Q):
    """the format's own luma path on the same tree -> (MSE, first-order entropy of the levels)"""
    v = np.stack([np.asarray(luma, np.int64)] * 3, 1)
    H, dc = forward(tree, v)
    D16 = steps(tree, Q, Q)
    k = quantize(H, D16)
    rec = inverse(tree, dequantize(k, D16), dc)[:, 0]
    return float(np.mean((rec - np.asarray(luma, np.float64)) ** 2)), entropy(k[:, 0])
