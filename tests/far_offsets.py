"""Levels whose gathered rows lie past byte offset 2^31 and up to the 32-bit offset limits of the LDS-DMA kernels (a helper module, like
fp64_reference.py): the generator (index arithmetic on the host, the level itself built on the device) and a numpy emulation of the
gather under wrong offset arithmetic.

A level of `n` feature rows of `row_bytes` bytes holds
  * a clump: one solid 14^3 block of voxels (all 27 offsets present inside it) whose fp64 definition and oracle answer are computed on
    the clump alone; its rows are dealt round-robin into three windows of the level — rows [0, w), the w rows straddling byte offset 2^31
    and the last w rows before the guard rows — so that almost every clump row gathers neighbours from the other two windows.  (When the
    level ends less than w rows after 2^31 the middle window is moved down to end where the last one begins: the two together straddle.)
  * fillers: every other row is an isolated voxel with zero features (only the centre entry of the map present): its output is one
    constant row whatever the family;
  * guard rows: the last 8 rows, and the rows the two absent-neighbour sentinels 0xF0000000 / 0xFFFFFFF0 name where the level reaches
    them, are isolated fillers with NaN features: their own outputs are excluded, any other non-finite output is a stray read.
Kinds: 'plain' (a level with its own [27][n] map), 'children' (rows 8 p + j belong to parent p; the map is the parents' [27][n / 8]: whole
parents are dealt, guarded and excluded), 'down' (the k2 s2 conv: [8][n] map from n coarse rows onto the n fine rows; every filler fine row
is the only child of the coarse row of the same index).

Every far operand is a view into one allocation [2 GiB lead pad | n rows | 64 tail rows], NaN-filled first: a sign-extended offset lands
in the pad, a wrapped one in the payload, an overrun in the tail — a wrong offset is a wrong number, never a stray access."""
import numpy as np

import fp64_reference as R

ROW_BYTES, LD = 256, 64
SIGN = 1 << 31                       # the first byte offset with the top bit set
LIMIT = 0xF0000000                   # rows / packed / children kernels: the tensor ends below it (their absent-neighbour offset)
GATHER_LIMIT = 0xFFFFFFF0            # gather MFMA / row-split kernels and the fused VALU InceptionResNet
GUARD, SIDE = 8, 14
PAD_BYTES, TAIL_ROWS = 1 << 31, 64
ROWS_SIGN = SIGN // ROW_BYTES                     # 8 388 608
ROWS_LIMIT = LIMIT // ROW_BYTES                   # 15 728 640: the first refused row count
ROWS_GATHER = GATHER_LIMIT // ROW_BYTES + 1       # 16 777 216: 2^32 bytes; one row fewer is the last accepted
W = -(-SIDE ** 3 // 3)                            # rows per window of a plain level (915)
W_PARENTS = -(-(SIDE // 2) ** 3 // 3)             # parents per window of a children level (115)
RULES = ('wrap32', 'signed31', 'records_signed', 'sentinel_in_range')

# the cases of the device tests: name -> (kind, rows n of the gathered input, row bytes)
CASES = {
    'sign bit': ('plain', ROWS_SIGN + W + GUARD, ROW_BYTES),
    'sign bit down': ('down', ROWS_SIGN + W + GUARD, ROW_BYTES),
    'sign bit children': ('children', 8 * (ROWS_SIGN // 8 + W_PARENTS + 1), ROW_BYTES),
    'below LIMIT': ('plain', ROWS_LIMIT - 1, ROW_BYTES),
    'below LIMIT down': ('down', ROWS_LIMIT - 1, ROW_BYTES),
    'below LIMIT children': ('children', 8 * (ROWS_LIMIT // 8 - 1), ROW_BYTES),
    'at LIMIT': ('plain', ROWS_LIMIT, ROW_BYTES),
    'at LIMIT down': ('down', ROWS_LIMIT, ROW_BYTES),
    'at LIMIT children': ('children', ROWS_LIMIT, ROW_BYTES),
    'below GATHER_LIMIT': ('plain', ROWS_GATHER - 1, ROW_BYTES),
    'past 4 GiB': ('plain', ROWS_GATHER + W + GUARD, ROW_BYTES),
    'map gate below': ('plain', 39768215, 64),
    'map gate above': ('plain', 39768216, 64),
}


def _block(side, step):
    g = np.arange(side) * step
    c = np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3) + 64
    return np.concatenate([np.zeros((len(c), 1), np.int64), c.astype(np.int64)], 1)


class Level:
    """kind, n (feature rows), row_bytes; coords (clump voxels, [m, 4]); rows [m]: level row of clump voxel i; nbr [K][m_out]: the clump's
    map in CLUMP indices; out_rows [m_out]: level row of clump output i; n_out; map_rows / map_cols: the level's map is [map_rows][map_cols];
    excluded: sorted level rows whose features are NaN (guards, sentinel rows); windows: ((first row, rows), ...) in feature rows"""


def make_level(n, kind='plain', row_bytes=ROW_BYTES):
    """index arithmetic only: nothing of size n is allocated"""
    L = Level()
    L.kind, L.n, L.row_bytes = kind, int(n), int(row_bytes)
    unit = 8 if kind == 'children' else 1                      # feature rows per dealt item
    assert n % unit == 0
    items = n // unit
    if kind == 'children':
        L.parents = _block(SIDE // 2, 2)                                      # stride-2 parents; their children are the 14^3 block
        L.coords = R.children_coords(L.parents, 2)
        L.parent_nbr = R.neighbour_map(L.parents, L.parents, R.offsets(3) * 2)
        m = len(L.parents)
    else:
        L.coords = _block(SIDE, 1)
        m = len(L.coords)
    w = -(-m // 3)
    guard = GUARD // unit
    last = items - guard - w
    mid = min(SIGN // (row_bytes * unit) - w // 2, last - w)
    assert w <= mid, 'the level is too small for three windows'
    starts = np.array([0, mid, last], np.int64)
    i = np.arange(m)
    item_rows = starts[i % 3] + i // 3
    L.w, L.windows = w * unit, tuple((int(s) * unit, w * unit) for s in starts)
    if kind == 'children':
        L.parent_rows = item_rows
        L.rows = (8 * item_rows[:, None] + np.arange(8)[None]).reshape(-1)      # child j of clump parent i is clump row 8 i + j
        L.map_rows, L.map_cols = 27, items
    else:
        L.rows = item_rows
        L.map_rows, L.map_cols = (27, n) if kind == 'plain' else (8, n)
    L.nbr = R.neighbour_map(L.coords, L.coords, R.offsets(3))
    L.out_rows, L.n_out = L.rows, n
    if kind == 'down':
        L.coarse = R.down_coords(L.coords, 1)
        L.down_nbr = R.neighbour_map(L.coarse, L.coords, R.offsets(2))
        L.out_rows = L.rows[:len(L.coarse)]                                     # clump coarse row i sits at the level row of clump voxel i
    excl = set(range(n - GUARD, n))
    inside = lambda r: any(s <= r < s + c for s, c in L.windows)
    for sentinel in (LIMIT, GATHER_LIMIT):
        r = sentinel // row_bytes // unit * unit
        if r + unit <= n - GUARD and not inside(r):
            excl.update(range(r, r + unit))
    L.excluded = np.array(sorted(excl), np.int64)
    return L


def gather_map(L):
    """(map in clump indices [K][m_out], level row of every clump INPUT row) of the gather the kernels of this kind perform"""
    return (L.down_nbr if L.kind == 'down' else L.nbr), L.rows


def applicable(rule, L, sentinel=LIMIT):
    extent = L.n * L.row_bytes
    if rule == 'wrap32':
        return extent > (1 << 32)
    if rule in ('signed31', 'records_signed'):
        return extent > SIGN
    if rule == 'sentinel_in_range':
        return sentinel + 16 <= extent
    return rule == 'exact'


def emulate(L, x, Wk, b, rule='exact', sentinel=LIMIT):
    """the clump outputs of the gather conv out[o] = b + sum_k W[k]^T x[map[k][o]] in float64, with the byte offset of every gathered row
    computed under `rule`:
        exact               offset = row x row bytes; absent reads zero
        wrap32              offset mod 2^32
        signed31            offsets >= 2^31 sign-extended (they land in the lead pad)
        records_signed      num_records taken as a signed int: every offset >= 2^31 is out of range and reads zero
        sentinel_in_range   the absent offset `sentinel` is not outside the tensor: it reads the row it names
    Features are a function of the row index (clump value, zero for a filler, NaN for a guard, the pad and the tail)."""
    nbr, in_rows = gather_map(L)
    x = np.asarray(x, np.float64)
    Wk = np.asarray(Wk, np.float64)
    rb, extent = L.row_bytes, L.n * L.row_bytes
    order = np.argsort(in_rows)
    sorted_rows = in_rows[order]

    def features(row):
        """row: int64 array of level rows; -1 reads zero, -2 reads NaN"""
        f = np.zeros((len(row), x.shape[1]))
        pos = np.minimum(np.searchsorted(sorted_rows, row), len(sorted_rows) - 1)
        hit = sorted_rows[pos] == row
        f[hit] = x[order[pos[hit]]]
        f[(row == -2) | (row >= L.n) | np.isin(row, L.excluded)] = np.nan
        return f

    y = np.zeros((nbr.shape[1], Wk.shape[2])) + np.asarray(b, np.float64).reshape(1, -1)
    for k in range(nbr.shape[0]):
        present = nbr[k] >= 0
        off = np.where(present, in_rows[np.maximum(nbr[k], 0)] * rb, -1)
        row = np.where(present, off // rb, -1)
        if rule == 'wrap32':
            row = np.where(present, (off % (1 << 32)) // rb, -1)
        elif rule == 'signed31':
            row = np.where(present & (off >= SIGN), -2, row)
        elif rule == 'records_signed':
            row = np.where(present & (off >= SIGN), -1, row)
        elif rule == 'sentinel_in_range':
            if sentinel + 16 <= extent:
                row = np.where(present, row, sentinel // rb)
        else:
            assert rule == 'exact', rule
        with np.errstate(invalid='ignore'):
            y += features(row) @ Wk[k]
    return y


# ------------------------------------------------------------------------------------------------ the level on the device
def far_buffer(n, row_bytes, device, pad_bytes=PAD_BYTES):
    """-> (allocation, [n, row_bytes / 4] view of its payload): [2 GiB lead pad | n rows | 64 tail rows], all NaN"""
    import torch
    ld = row_bytes // 4
    buf = torch.full(((pad_bytes + (n + TAIL_ROWS) * row_bytes) // 4,), float('nan'), device=device)
    return buf, buf[pad_bytes // 4:pad_bytes // 4 + n * ld].view(n, ld)


def far_features(L, x, device, rows=None, pad_bytes=PAD_BYTES):
    """x [m, C] (clump values) -> (allocation, [n, C] view): fillers zero, guards and every other column NaN.  rows: level rows of x
    (default: the clump's input rows)"""
    import torch
    buf, view = far_buffer(L.n, L.row_bytes, device, pad_bytes)
    C = x.shape[1]
    f = view[:, :C]
    f.zero_()
    f[torch.as_tensor(L.rows if rows is None else rows, device=device)] = torch.as_tensor(np.ascontiguousarray(x, np.float32), device=device)
    f[torch.as_tensor(L.excluded, device=device)] = float('nan')
    return buf, f


def far_map(L, device):
    """the level's map on the device, int32 [map_rows][map_cols]: -1 everywhere but the centre row of the fillers (down: offset 0) and the
    clump's own entries re-indexed to its scattered rows"""
    import torch
    nbr = torch.full((L.map_rows, L.map_cols), -1, dtype=torch.int32, device=device)
    nbr[13 if L.map_rows == 27 else 0] = torch.arange(L.map_cols, dtype=torch.int32, device=device)
    if L.kind == 'children':
        clump, src, cols = L.parent_nbr, L.parent_rows, L.parent_rows
    elif L.kind == 'down':
        clump, src, cols = L.down_nbr, L.rows, L.out_rows
        nbr[:, torch.as_tensor(L.rows, device=device)] = -1                    # (coarse rows at clump positions past the clump's own: empty)
    else:
        clump, src, cols = L.nbr, L.rows, L.rows
    scattered = np.where(clump >= 0, src[np.maximum(clump, 0)], -1).astype(np.int32)
    nbr[:, torch.as_tensor(cols, device=device)] = torch.as_tensor(scattered, device=device)
    return nbr


def check_fillers(L, got, constant):
    """every output row that belongs neither to the clump nor to an excluded row equals `constant` ([1, C]; children: [8, C], one row per
    child of an isolated parent) — ONE comparison on the device -> number of rows that differ"""
    import torch
    n, C = got.shape
    const = torch.as_tensor(np.ascontiguousarray(constant, np.float32), device=got.device)
    if const.shape[0] == 1:
        bad = (got != const).any(1)
    else:
        bad = (got.view(n // 8, 8, C) != const[None]).any(2).view(n)
    bad[torch.as_tensor(L.out_rows, device=got.device)] = False
    excl = L.excluded[L.excluded < n]
    bad[torch.as_tensor(excl, device=got.device)] = False
    return int(bad.sum().item())
