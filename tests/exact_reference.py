"""Brute-force definitions of the select, coordinate and entropy-front-end operations of PCGCv2, for tests (a helper module, like
fp64_reference.py).  numpy (and torch on the CPU where the reference itself uses it); no oracle, no product import.

Every result here is an integer or a boolean, so everything is compared for EQUALITY: there is no tolerance.  Each function is the
plainest statement of the operation, written from the reference's call sites (data_utils.py:55-118, autoencoder.py:155-161,237-249,
entropy_model.py:103-110,151-196) and DESIGN.md §3-§4:

    topk_mask             the k rows that come first when the rows are ordered by (value descending, row ascending) — istopk
    dedup                 one row per distinct coordinate, the first (or last) that holds it, input order kept — ME.SparseTensor
    quantize / pyramid    coarse cell floor(c / 2s) 2s of a k2 s2 conv, cells in first-occurrence order, parent_of and the 8-slot down map
    children              row 8 i + j = parent i + (s / 2) d(j) — the generative transpose
    k3_map / down_map     a dictionary {(batch, x, y, z): row} asked once per kernel offset
    prune_map             a map restricted to surviving rows and renumbered
    sort_zyx / sort_bzyx  np.lexsort with z (batch) as the most significant field — array2vector's order
    scale                 (C * factor).round().int() with torch on the CPU, as data_utils.py:113 does it
    round_minmax, symbolize, desymbolize      np.rint (half to even), `+ 0` (no -0 in a header)
    mix64, coord_key, home_slot, occupied_slots   the coordinate hash restated in uint64 numpy (csrc/pcgc_common.h), so that the host can
                          predict which slots a linear-probing table holds: that SET does not depend on the insertion order

The input generators below each ASSERT their own precondition (digit, bin, population, wrap, lane position), so that a case cannot
silently stop exercising what it is named for."""
import numpy as np

LIM = 1 << 20                                   # coordinates are 20-bit, the batch index 4-bit


# ================================================================================================ select
def _clamp_k(k, n):
    return int(min(max(int(k), 0), n))


def topk_mask(v, k, tie='low'):
    """istopk for one item (data_utils.py:77-89): rows ordered by value descending; among equal values the lower row first ('low') or
    the higher row first ('high'); -0 == +0.  NaN has no place in that order: callers keep NaN out."""
    v = np.asarray(v, np.float32).ravel() + np.float32(0)
    n = len(v)
    rows = np.arange(n)
    order = np.lexsort((rows if tie == 'low' else -rows, -v.astype(np.float64)))
    mask = np.zeros(n, bool)
    mask[order[:_clamp_k(k, n)]] = True
    return mask


def topk_mask_segments(v, seg_rows, seg_k, tie='low'):
    """istopk over a collated batch: item b = the next seg_rows[b] rows with its own budget (clamped to [0, rows])"""
    v = np.asarray(v, np.float32).ravel()
    assert sum(seg_rows) == len(v)
    out, off = np.zeros(len(v), bool), 0
    for r, k in zip(seg_rows, seg_k):
        out[off:off + r] = topk_mask(v[off:off + r], k, tie)
        off += r
    return out


def select_outputs(mask, coords):
    """what the one-sweep prune writes for a survivor mask: (bitmap bytes, bit m of word m // 64 = row m survives, whole 64-bit words;
    wprefix = survivors before every 64th row; orig = the surviving rows; their coordinates)"""
    mask = np.asarray(mask, bool)
    n = len(mask)
    words = (n + 63) // 64
    padded = np.zeros(words * 64, np.uint8)
    padded[:n] = mask
    bits = np.packbits(padded, bitorder='little')
    excl = np.concatenate([[0], np.cumsum(mask)])[:-1] if n else np.zeros(0, np.int64)
    return bits, excl[::64].astype(np.int32), np.nonzero(mask)[0].astype(np.int32), np.asarray(coords)[mask]


def order_key(v):
    """csrc/select.hip's order-preserving uint32 image of an fp32 value (restated for the generators' own assertions)"""
    b = (np.asarray(v, np.float32) + np.float32(0)).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def key_to_float(key):
    """the fp32 value whose order_key is `key` (key 0x7FFFFFFF would be -0, which order_key never yields: callers re-derive the keys)"""
    key = np.asarray(key, np.uint32)
    b = np.where(key & np.uint32(0x80000000), key & np.uint32(0x7FFFFFFF), ~key).astype(np.uint32)
    return b.view(np.float32)


RADIX_SHIFT, RADIX_BITS = (21, 10, 0), (11, 11, 10)             # three passes of 11 / 11 / 10 bits, most significant first
RADIX_PER = (8, 8, 4)                                           # bins per thread of the 256-thread pick
RADIX_BIN_KINDS = ('range_first', 'range_last', 'g0_last', 'g255_first', 'mid_group_first', 'mid_group_last')


def radix_bin(pass_, bin_kind, sign):
    """the digit a bin kind names, or None where no finite fp32 value has it.  Pass 0's digit holds the sign and the exponent: bins 0-3 and
    2044-2047 hold only NaN / inf, negative values have bins < 1024 — 'range_first' / 'range_last' are there the first / last bin with
    finite values of that sign (1023 and 1024 are the denormal bins on either side of zero)."""
    nb, per = 1 << RADIX_BITS[pass_], RADIX_PER[pass_]
    if pass_ == 0:
        table = {'range_first': (4, 1024), 'range_last': (1023, 2043), 'g0_last': (7, None), 'g255_first': (None, 2040),
                 'mid_group_first': (480, 1520), 'mid_group_last': (487, 1527)}
        return table[bin_kind][0 if sign == 'neg' else 1]
    return {'range_first': 0, 'range_last': nb - 1, 'g0_last': per - 1, 'g255_first': nb - per, 'mid_group_first': 100 * per,
            'mid_group_last': 100 * per + per - 1}[bin_kind]


def radix_case(pass_, bin_kind, sign, n, dup, seed=0):
    """fp32 values built from bit patterns so that every key shares the digits above pass `pass_`, the k-th largest key has digit
    radix_bin(...) in that pass, at least `dup` rows equal it and fewer than all of them are needed.  k follows from the population (with
    the last bin of the last pass no key can be larger than the threshold), so it is returned: -> (values, k)."""
    rng = np.random.default_rng([seed, pass_, RADIX_BIN_KINDS.index(bin_kind), sign == 'neg'])
    bin_ = radix_bin(pass_, bin_kind, sign)
    assert bin_ is not None, 'no finite value has this digit'
    shift, bits = RADIX_SHIFT[pass_], RADIX_BITS[pass_]
    nb, per = 1 << bits, RADIX_PER[pass_]
    base = int(order_key(np.float32(-1.5 if sign == 'neg' else 1.5)))
    above = (0xFFFFFFFF << (shift + bits)) & 0xFFFFFFFF
    prefix = base & above
    lo_bin, hi_bin = (0, nb - 1) if pass_ else ((4, 1023) if sign == 'neg' else (1024, 2043))
    low_mask = (1 << shift) - 1
    T = prefix | (bin_ << shift) | (int(rng.integers(1, low_mask)) if shift else 0)
    m = dup + 3                                                   # rows equal to the threshold
    digits = rng.integers(lo_bin, hi_bin + 1, size=n - m, dtype=np.int64)
    digits[: (n - m) // 4] = bin_                                 # a populated bin: the later passes have work too
    lows = rng.integers(0, low_mask + 1, size=n - m, dtype=np.int64) if shift else np.zeros(n - m, np.int64)
    keys = (prefix | (digits << shift) | lows).astype(np.uint32)
    keys = keys[(keys != np.uint32(T)) & (keys != np.uint32(0x7FFFFFFF))]
    keys = np.concatenate([keys, np.full(m, T, np.uint32)])
    keys = keys[rng.permutation(len(keys))]
    v = key_to_float(keys)
    assert np.isfinite(v).all()
    # ---- the preconditions, from the keys the kernel will see
    got = order_key(v)
    assert np.array_equal(got, keys)
    assert ((got & np.uint32(above)) == np.uint32(prefix)).all(), 'a key leaves the shared digits'
    need = max(1, m // 2)
    k = int((got > np.uint32(T)).sum()) + need
    kth = np.sort(got)[::-1][k - 1]
    assert int(kth) == T and (int(kth) >> shift) & (nb - 1) == bin_
    count_eq = int((got == kth).sum())
    assert count_eq >= dup and 0 < need < count_eq, 'the threshold is not a populated, partly needed tie'
    if pass_ < 2:
        in_bin = ((got >> np.uint32(shift)) & np.uint32(nb - 1)) == bin_
        assert in_bin.sum() > count_eq + 8, 'the bin of the threshold is not populated beyond the tie'
    group, slot = divmod(bin_, per)
    assert {'range_first': pass_ == 0 or bin_ == 0, 'range_last': pass_ == 0 or bin_ == nb - 1, 'g0_last': group == 0 and slot == per - 1,
            'g255_first': group == 255 and slot == 0, 'mid_group_first': 0 < group < 255 and slot == 0,
            'mid_group_last': 0 < group < 255 and slot == per - 1}[bin_kind]
    assert (v < 0).all() if sign == 'neg' else (v >= 0).all()
    return v, k


def radix_cases(n=6000, dup=5):
    """every (pass, bin kind, sign) that exists -> [(name, values, k)]"""
    out = []
    for p in range(3):
        for kind in RADIX_BIN_KINDS:
            for sign in ('pos', 'neg'):
                if radix_bin(p, kind, sign) is not None:
                    out.append((f'pass{p}-{kind}-{sign}',) + radix_case(p, kind, sign, n, dup))
    return out


F32 = np.float32
SPECIALS = [('zero', F32(0)), ('min_denormal', F32(1.401298464324817e-45)), ('max_denormal', np.uint32(0x007FFFFF).view(F32)),
            ('flt_min', F32(1.1754943508222875e-38)), ('flt_max', F32(3.4028234663852886e38)), ('inf', F32(np.inf))]


def special_values(seed=0):
    """+-0, the smallest and largest denormals of both signs, +-FLT_MIN, +-FLT_MAX, +-inf (three rows each) mixed into ordinary values,
    with the threshold placed on each of them in turn -> [(name, values, k)]; 2 of the 3 (zero: 2 of the 6 rows +0 / -0) are needed."""
    rng = np.random.default_rng(seed)
    spec = []
    for _, s in SPECIALS:
        spec += [s, -s] * 3
    base = np.concatenate([rng.standard_normal(700).astype(F32) * F32(3), np.array(spec, F32)])
    v = base[rng.permutation(len(base))]
    v[np.nonzero(v == 0)[0]] = np.array([-0.0, 0.0] * 3, F32)         # the first zero row is -0: needed, and never ranked below a +0
    assert (np.signbit(v) & (v == 0)).sum() == 3 and (v == 0).sum() == 6
    out = []
    for name, s in SPECIALS:
        for t in ((s,) if name == 'zero' else (s, -s)):
            k = int((v > t).sum()) + 2
            kth = np.sort(v)[::-1][k - 1]
            assert kth == t and (v == t).sum() in (3, 6) and k < len(v)
            out.append((f'{name}{"-" if np.signbit(t) else "+"}', v, k))
    return out


# ================================================================================================ coordinates
def _rows(coords):
    return [tuple(int(a) for a in r) for r in np.asarray(coords)]


def dedup(coords, keep='first'):
    """-> (rows kept, in input order; for every row the kept row that holds its coordinate)"""
    where = {}
    for i, r in enumerate(_rows(coords)):
        if keep == 'last' or r not in where:
            where[r] = i
    holder = np.array([where[r] for r in _rows(coords)], np.int64).reshape(-1)
    return np.nonzero(holder == np.arange(len(holder)))[0], holder


def quantize(coords, stride):
    """floor(c / stride) stride on x, y, z (the cell of a conv whose output stride is `stride`)"""
    c = np.asarray(coords, np.int64).copy()
    c[:, 1:] = np.floor_divide(c[:, 1:], stride) * stride
    return c


def slot_of(coords, stride, order='xyz'):
    """which of the 8 offsets of a k2 kernel reaches each fine row from its coarse cell (the kernel offset index, by offset order)"""
    c = np.asarray(coords, np.int64)
    j = [(c[:, a] // stride) & 1 for a in (1, 2, 3)]
    return j[0] + 2 * j[1] + 4 * j[2] if order == 'xyz' else j[2] + 2 * j[1] + 4 * j[0]


def pyramid(coords, stride, levels, order='xyz'):
    """`levels` strided levels below `coords` (tensor stride `stride`) -> [(coarse rows in first-occurrence order, parent_of, down [8, nc])]"""
    out, cur, s = [], np.asarray(coords, np.int64), stride
    for _ in range(levels):
        q = quantize(cur, 2 * s)
        kept, holder = dedup(q)
        coarse = q[kept]
        number = np.full(len(q), -1, np.int64)
        number[kept] = np.arange(len(kept))
        parent_of = number[holder]
        down = np.full((8, len(coarse)), -1, np.int64)
        down[slot_of(cur, s, order), parent_of] = np.arange(len(cur))
        out.append((coarse, parent_of, down))
        cur, s = coarse, 2 * s
    return out


def offsets(n, order='xyz'):
    """[n^3, 3] kernel offsets (n = 3: {-1, 0, 1}^3, n = 2: {0, 1}^3), 'xyz': x fastest, 'zyx': z fastest"""
    lo = -1 if n == 3 else 0
    cube = [(a + lo, b + lo, c + lo) for c in range(n) for b in range(n) for a in range(n)]        # a fastest
    return np.array(cube if order == 'xyz' else [(c, b, a) for a, b, c in cube], np.int64)


def children(coords, stride, order='xyz'):
    """generative transpose k2 s2 on a level of tensor stride `stride`: row 8 i + j = coords[i] + (stride / 2) d(j)"""
    c = np.asarray(coords, np.int64)
    out = np.repeat(c, 8, axis=0)
    out[:, 1:] += np.tile(offsets(2, order) * (stride // 2), (len(c), 1))
    return out


def in_range(coords):
    """rows the 4 + 20 + 20 + 20-bit key can hold (batch 15 at the far corner is the key that means 'empty': excluded)"""
    c = np.asarray(coords, np.int64)
    ok = ((c[:, 1:] >= 0) & (c[:, 1:] < LIM)).all(1) & (c[:, 0] >= 0) & (c[:, 0] < 16)
    return ok & ~((c[:, 0] == 15) & (c[:, 1:] == LIM - 1).all(1))


def _identity(r):
    return r


def neighbour_map(coords_out, coords_in, deltas, key=_identity):
    """[K, n_out]: row of coords_in at coords_out + deltas[k], -1 = none.  `key` maps a row tuple to what the dictionary is keyed by
    (tests mutate it)."""
    table = {}
    for i, r in enumerate(_rows(coords_in)):
        table.setdefault(key(r), i)
    out = np.full((len(deltas), len(coords_out)), -1, np.int64)
    rows = _rows(coords_out)
    for k, d in enumerate(np.asarray(deltas).tolist()):
        out[k] = [table.get(key((b, x + d[0], y + d[1], z + d[2])), -1) for b, x, y, z in rows]
    return out


def k3_map(coords, stride, order='xyz', key=_identity):
    return neighbour_map(coords, coords, offsets(3, order) * stride, key)


def down_map(fine, coarse, stride_fine, order='xyz', key=_identity):
    return neighbour_map(coarse, fine, offsets(2, order) * stride_fine, key)


def prune_map(nbr, mask):
    """the map of the level that keeps the rows of `mask`: surviving columns, surviving neighbours renumbered, the others -1"""
    mask = np.asarray(mask, bool)
    number = np.where(mask, np.cumsum(mask) - 1, -1)
    nbr = np.asarray(nbr)
    return np.where(nbr >= 0, number[np.maximum(nbr, 0)], -1)[:, mask]


def sort_zyx(coords):
    """stable argsort by (z, y, x, batch), z most significant: array2vector(C, C.max() + 1) (data_utils.py:55-61, 91-95)"""
    c = np.asarray(coords, np.int64)
    return np.lexsort((c[:, 0], c[:, 1], c[:, 2], c[:, 3]))


def sort_bzyx(coords):
    """stable argsort by (batch, z, y, x): every item of a collated batch in the order it has when coded alone"""
    c = np.asarray(coords, np.int64)
    return np.lexsort((c[:, 1], c[:, 2], c[:, 3], c[:, 0]))


def scale(coords, factor):
    """scale_sparse_tensor (data_utils.py:113): (x.C[:, 1:] * factor).round().int(), with torch on the CPU"""
    import torch
    c = np.asarray(coords, np.int32).copy()
    c[:, 1:] = (torch.from_numpy(c[:, 1:].copy()) * factor).round().int().numpy()
    return c


# ================================================================================================ entropy front end
def round_minmax(x):
    """entropy_model.py:155-157: min and max of round(x) (half to even), as fp32, never -0"""
    r = np.rint(np.asarray(x, np.float32)) + np.float32(0)
    return np.float32(r.min()), np.float32(r.max())


def symbolize(x, min_v):
    """entropy_model.py:161-163: (round(x) - min_v).to(int16)"""
    d = np.rint(np.asarray(x, np.float32)) - np.float32(min_v)
    assert (d >= 0).all() and (d < 32768).all(), 'not an int16 alphabet'
    return d.astype(np.int16)


def desymbolize(sym, min_v):
    """entropy_model.py:193-194: values.float() + min_v"""
    return np.asarray(sym).astype(np.float32) + np.float32(min_v)


# ================================================================================================ the coordinate hash
def mix64(v):
    v = np.asarray(v, np.uint64).copy()
    with np.errstate(over='ignore'):
        v ^= v >> np.uint64(33); v *= np.uint64(0xff51afd7ed558ccd); v ^= v >> np.uint64(33); v *= np.uint64(0xc4ceb9fe1a85ec53); v ^= v >> np.uint64(33)
    return v


def coord_key(coords):
    """4-bit batch | 20-bit z | 20-bit y | 20-bit x"""
    c = np.asarray(coords, np.int64)
    assert in_range(c).all()
    c = c.astype(np.uint64)
    return (c[:, 0] << np.uint64(60)) | (c[:, 3] << np.uint64(40)) | (c[:, 2] << np.uint64(20)) | c[:, 1]


def home_slot(key, cap):
    assert cap & (cap - 1) == 0
    return (mix64(key) & np.uint64(cap - 1)).astype(np.int64)


def hash_capacity(n):
    """the table size the product gives n rows: the smallest power of two >= max(1024, 2 n) — an empty slot always exists"""
    cap = 1024
    while cap < 2 * n:
        cap *= 2
    return cap


def occupied_slots(keys, cap):
    """{slot: key} of a linear-probing table after inserting `keys` one by one.  Each key lands on the first free slot from its home on;
    which KEY sits in which slot depends on the order, the SET of occupied slots does not (every order fills the same runs)."""
    table = {}
    for key, h in zip(np.asarray(keys, np.uint64).tolist(), home_slot(keys, cap).tolist()):
        while h in table and table[h] != key:
            h = (h + 1) & (cap - 1)
        table[h] = key
    return table


# ================================================================================================ coordinate generators
_POOL = {}


def _pool():
    """4 M random legal coordinates and their mixed keys (built once): ~3900 per slot at capacity 1024, ~950 at 4096"""
    if not _POOL:
        rng = np.random.default_rng(2024)
        c = np.empty((1 << 22, 4), np.int32)
        c[:, 0] = rng.integers(0, 16, len(c))
        c[:, 1:] = rng.integers(0, LIM, (len(c), 3))
        c = c[in_range(c)]
        _POOL['c'], _POOL['mix'] = c, mix64(coord_key(c))
    return _POOL['c'], _POOL['mix']


def collision_case(cap, home, length, n=None, seed=0):
    """n (default: `length`) distinct legal rows for a table of capacity `cap`, `length` of which have home slot `home`: a probe chain of
    that length, which wraps from slot cap - 1 to 0 when home + length > cap; plus rows that are NOT in the table although their home
    lies inside the chain (a lookup must walk to the chain's end to say so).  -> (rows, shuffled; absent rows)"""
    n = length if n is None else n
    assert hash_capacity(n) == cap and n >= length
    c, mix = _pool()
    rng = np.random.default_rng([seed, cap, home, length])
    slot = (mix & np.uint64(cap - 1)).astype(np.int64)
    chain_rows = np.nonzero(slot == home)[0]
    assert len(chain_rows) >= length + 4, 'pool too small for this chain'
    inside = np.nonzero(((slot - home) % cap > 0) & ((slot - home) % cap < length))[0]
    others = np.nonzero((slot - home) % cap >= length + 64)[0]       # (filler rows start well clear of the chain)
    rows = np.concatenate([c[chain_rows[:length]], c[rng.choice(others, n - length, replace=False)]])
    rows = np.unique(rows, axis=0)
    assert len(rows) == n, 'the pool drew a coordinate twice'
    rows = rows[rng.permutation(n)]
    absent = np.concatenate([c[chain_rows[length:length + 4]], c[inside[:8]]])
    # ---- preconditions
    occ = occupied_slots(coord_key(rows), cap)
    assert all((home + i) % cap in occ for i in range(length)), 'the chain does not fill its run of slots'
    if home + length > cap:
        assert 0 in occ and cap - 1 in occ, 'the chain does not wrap'
    assert (home_slot(coord_key(rows), cap) == home).sum() == length
    present = set(_rows(rows))
    assert not any(r in present for r in _rows(absent))
    assert all(0 <= (h - home) % cap < length for h in home_slot(coord_key(absent), cap))
    return rows.astype(np.int32), absent.astype(np.int32)


def lane_duplicates(n=6000, seed=0):
    """distinct random rows, then runs of 1..9 equal rows placed so that runs start at lanes 0, 62 and 63 of a 64-lane wave and straddle rows
    63|64 (two waves), 255|256 and 511|512 (two 256-thread blocks), plus coordinates repeated far apart -> (rows, [(start, length)])"""
    assert n >= 4096
    rng = np.random.default_rng(seed)
    c = np.empty((n, 4), np.int32)
    c[:, 0] = rng.integers(0, 16, n)
    c[:, 1:] = rng.integers(0, LIM - 1, (n, 3))                     # (x < 2^20 - 1: never the excluded key)
    assert len(np.unique(c, axis=0)) == n
    runs = [(60, 8), (250, 9), (509, 6)]
    for L in range(1, 10):
        for i, lane in enumerate((0, 62, 63)):
            runs.append((1024 + 128 * (3 * (L - 1) + i) + lane, L))
    for start, L in runs:
        c[start:start + L] = c[start]
    far = [(5, n - 1), (5, n - 100), (60, 3000), (runs[7][0], 3500)]      # (source row, a far row that repeats it)
    for src, dst in far:
        c[dst] = c[src]
    # ---- preconditions
    assert {s % 64 for s, _ in runs[3:]} == {0, 62, 63} and {L for _, L in runs[3:]} == set(range(1, 10))
    assert any(s <= 63 < 64 < s + L for s, L in runs) and any(s <= 255 < 256 < s + L for s, L in runs) and any(s <= 511 < 512 < s + L for s, L in runs)
    assert any(s % 64 == 63 and L >= 2 for s, L in runs), 'no run crosses lane 63 -> 64'
    ends = sorted((s, s + L) for s, L in runs)
    assert all(a[1] <= b[0] for a, b in zip(ends, ends[1:])), 'runs overlap'
    for s, L in runs:
        assert (c[s:s + L] == c[s]).all() and (s == 0 or (c[s - 1] != c[s]).any()) and (c[s + L] != c[s]).any()
    assert in_range(c).all()
    return c, runs


def _cluster(n):
    return np.array([(x, y, z) for z in range(n) for y in range(n) for x in range(n)], np.int64)


def border_cloud(stride=1):
    """points at 0, 1, 2^20 - 2, 2^20 - 1 (times `stride` from either end) on every axis, and full 2x2x2 and 3x3x3 clusters in each corner of
    the cube; batch 0, distinct rows on the lattice of `stride`"""
    s = stride
    top = (LIM // s - 1) * s                                         # the last lattice point
    ends = [0, s, top - s, top]
    pts = [np.array([(x, y, z) for z in ends for y in ends for x in ends], np.int64)]
    for cx in (0, 1):
        for cy in (0, 1):
            for cz in (0, 1):
                for n in (2, 3):
                    cl = _cluster(n) * s
                    origin = np.array([cx * (top - (n - 1) * s), cy * (top - (n - 1) * s), cz * (top - (n - 1) * s)])
                    pts.append(cl + origin)
    p = np.concatenate(pts)
    _, first = np.unique(p, axis=0, return_index=True)
    p = p[np.sort(first)]
    c = np.concatenate([np.zeros((len(p), 1), np.int64), p], 1)
    assert in_range(c).all() and (c[:, 1:] % s == 0).all()
    for v in ends:
        assert all((c[:, a] == v).any() for a in (1, 2, 3))
    assert c[:, 1:].max() == top and c[:, 1:].min() == 0
    return c.astype(np.int32)


def shell_cloud(radius, seed, centre=None):
    """a voxelised sphere shell (distinct rows [n, 3]): a small smooth surface like the codec's inputs"""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((40 * radius * radius, 3))
    p = np.rint(d / np.linalg.norm(d, axis=1, keepdims=True) * radius).astype(np.int64) + (radius + 2 if centre is None else centre)
    _, first = np.unique(p, axis=0, return_index=True)
    return p[np.sort(first)]


def batch_cloud(items=(0, 7, 15), shuffle=False, seed=0):
    """the SAME points under each batch index of `items` (item-contiguous rows): 3x3x3 clusters at the origin, in the far corner and
    mid-cube, the cube's eight corners and a small shell.  The one excluded key (batch 15 at the far corner) is left out."""
    parts = [_cluster(3), _cluster(3) + (LIM - 3), _cluster(3) + 5000, shell_cloud(9, 3, centre=700),
             np.array([(x, y, z) for z in (0, LIM - 1) for y in (0, LIM - 1) for x in (0, LIM - 1)], np.int64)]
    p = np.concatenate(parts)
    _, first = np.unique(p, axis=0, return_index=True)
    p = p[np.sort(first)]
    if shuffle:
        p = p[np.random.default_rng(seed).permutation(len(p))]
    c = np.concatenate([np.concatenate([np.full((len(p), 1), b, np.int64), p], 1) for b in items])
    n_before = len(c)
    c = c[in_range(c)]
    assert len(c) == n_before - (15 in items), 'exactly the excluded key is dropped'
    for b in items:
        assert (c[:, 0] == b).sum() >= len(p) - 1
    assert len(np.unique(c, axis=0)) == len(c) and (np.diff(c[:, 0]) >= 0).all()
    assert len(np.unique(c[:, 1:], axis=0)) == len(p), 'the items do not share their points'
    return c.astype(np.int32)


def collated_cloud():
    """three different small clouds collated as items 0, 1, 2 (ME.utils.sparse_collate: the item index in column 0)"""
    clouds = [shell_cloud(11, 1), shell_cloud(7, 2, centre=40), shell_cloud(14, 3, centre=100)]
    c = np.concatenate([np.concatenate([np.full((len(p), 1), b, np.int64), p], 1) for b, p in enumerate(clouds)])
    assert len({len(p) for p in clouds}) == 3 and in_range(c).all()
    return c.astype(np.int32)


ILLEGAL_ROWS = {'batch 15 at the far corner': (15, LIM - 1, LIM - 1, LIM - 1), 'x = -1': (0, -1, 5, 5), 'z = -1': (3, 5, 5, -1),
                'y = 2^20': (0, 5, LIM, 5), 'batch 16': (16, 1, 2, 3), 'batch -1': (-1, 1, 2, 3)}
for _name, _row in ILLEGAL_ROWS.items():
    assert not in_range(np.array([_row]))[0], _name


# ================================================================================================ latent generators
def entropy_cases(seed=0):
    """[N, 8] fp32 latents for the entropy front end -> [(name, x)]: every half from -3.5 to 3.5 (and -0.2, which rounds to -0 and must be
    coded as +0), large magnitudes with small alphabets, min == max, row counts around the 4-wide loads and the 1024-thread stride, and
    alphabets of 1, 2 and 32767 symbols (the int16 limit).  Each case asserts what it is named for."""
    rng = np.random.default_rng(seed)

    def fill(values, rows):
        v = np.asarray(values, F32)
        x = v[rng.integers(0, len(v), rows * 8)]
        x[:len(v)] = v[:rows * 8]                                   # every value at least once
        return x.reshape(rows, 8)

    halves = np.concatenate([np.arange(-7, 8, dtype=F32) / F32(2), np.array([-0.2, 0.2, -0.0], F32)])
    out = [('halves', fill(halves, 40))]
    assert {-3.5, -2.5, -0.5, 0.5, 2.5, 3.5} <= set(out[0][1].ravel().tolist())
    out.append(('all_round_to_zero', fill([-0.2, -0.4, -0.0, 0.3, -0.5, 0.5], 16)))
    assert round_minmax(out[-1][1]) == (0, 0) and not np.signbit(round_minmax(out[-1][1])[0])
    big = [('near_-2^24-2', F32(-16777218.0) + F32(2) * np.arange(4, dtype=F32)),
           ('near_2^23-0.5', F32(8388607.5) - F32(0.5) * np.arange(9, dtype=F32)),
           ('near_2^23', F32(8388608.0) + np.arange(6, dtype=F32))]
    for name, vals in big:
        assert len(np.unique(vals)) == len(vals) and (np.abs(vals) >= 2 ** 22).all()
        out.append((name, fill(vals, 24)))
        lo, hi = round_minmax(out[-1][1])
        assert 1 < hi - lo + 1 <= 8
    assert (out[-2][1] % 1 == 0.5).any(), 'no half at large magnitude'
    out.append(('constant', np.full((33, 8), 7.0, F32)))
    for rows in (1, 3, 4, 5, 1023, 1025):
        out.append((f'rows{rows}', (rng.standard_normal((rows, 8)) * 4).astype(F32)))
    out.append(('alphabet1', np.full((5, 8), -3.0, F32) + rng.uniform(-0.4, 0.4, (5, 8)).astype(F32)))
    out.append(('alphabet2', fill([0.0, 1.0, 0.4, 0.6], 9)))
    wide = np.rint(rng.uniform(0, 32766, (64, 8))).astype(F32)
    wide[0, 0], wide[-1, -1] = 0, 32766
    out.append(('alphabet32767', wide - F32(20000)))
    for name, want in (('alphabet1', 1), ('alphabet2', 2), ('alphabet32767', 32767), ('constant', 1)):
        lo, hi = round_minmax(dict(out)[name])
        assert hi - lo + 1 == want, name
    return out


def device_minmax(x):
    """min and max of round(x) + 0 in the order the device reduces in (csrc/entropy.hip f2ord: the fp32 bit pattern as a signed integer, the
    negative half reversed): finite values and infinities in float order, +NaN above +inf, -NaN below -inf — so a value that is not finite
    always reaches one end of the range"""
    r = (np.rint(np.asarray(x, F32)) + F32(0)).ravel()
    b = r.view(np.int32)
    o = np.where(b >= 0, b, b ^ np.int32(0x7fffffff))
    return r[o.argmin()], r[o.argmax()]


def unsupported_latents():
    """[N, 8] latents that int16 symbols cannot code -> [(name, x)]: an alphabet of 32768, and a NaN / infinite value"""
    base = np.zeros((40, 8), F32)
    out = []
    for name, v in (('alphabet32768', 32767.0), ('alphabet_huge', 3e9), ('nan', np.nan), ('-nan', -np.nan), ('+inf', np.inf), ('-inf', -np.inf)):
        x = base.copy()
        x[17, 3] = v
        out.append((name, x))
    lo, hi = round_minmax(out[0][1])
    assert hi - lo + 1 == 32768
    return out
