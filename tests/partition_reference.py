"""The definition of the kd-tree block partition: numpy, integers only.  Every output of ops.partition (csrc/partition.hip)
is held to equality with this file.

    cell = coord // align             align a power of two in 8 .. 1024: no stride-`align` cell is ever shared by two blocks
    rounds                            one block holds all rows; in a round every block with more than max_num rows and a cell extent above 0
                                      on some axis is split, all of them at once; the round that splits nothing is the end
    axis                              the largest cell extent cmax - cmin, ties to x before y before z
    plane                             for k in cmin + 1 .. cmax, L(k) = rows with cell below k; the k with the smallest |2 L(k) - n|, ties to
                                      the smaller k; rows with cell below k are the left child
    order                             the children take the parent's place as (left, right): blocks are numbered in the in-order of the tree;
                                      rows keep their input order inside a block

A block of more than max_num rows that lie in one cell stays as it is and is counted in `oversize`.  More than MAX_BLOCKS blocks is an error."""
from collections import namedtuple

import numpy as np

MAX_BLOCKS = 1024
MAX_ROWS = 1 << 27
COORD_LIMIT = 1 << 20
Partition = namedtuple('Partition', 'block_of perm table rounds oversize')


def check(coords, max_num, align=8):
    """the preconditions; every violation is a ValueError that names a count -> xyz int64 [N,3]"""
    if isinstance(max_num, bool) or not isinstance(max_num, (int, np.integer)) or max_num < 1:
        raise ValueError(f'partition: max_num {max_num!r}: an integer of at least 1')
    if isinstance(align, bool) or not isinstance(align, (int, np.integer)) or align not in (8, 16, 32, 64, 128, 256, 512, 1024):
        raise ValueError(f'partition: align {align!r}: a power of two in 8 .. 1024')
    if getattr(coords, 'ndim', 0) != 2 or coords.shape[1] not in (3, 4) or coords.dtype != np.int32:
        raise ValueError(f'partition: coords must be int32 [N,3] or [N,4], got {getattr(coords, "dtype", None)} {getattr(coords, "shape", None)}')
    n = coords.shape[0]
    if n > MAX_ROWS:
        raise ValueError(f'partition: {n} rows; at most 2^27')
    c = np.asarray(coords)
    if c.shape[1] == 4:
        other = int((c[:, 0] != 0).sum())
        if other:
            raise ValueError(f'partition: {other} of {n} rows have a batch index other than 0')
    xyz = c[:, -3:].astype(np.int64)
    outside = int(((xyz < 0) | (xyz >= COORD_LIMIT)).any(1).sum())
    if outside:
        raise ValueError(f'partition: {outside} of {n} rows are outside 0 .. 2^20 - 1')
    return xyz


def choose_axis(cells):
    """cells int64 [n,3] of one block -> (axis, cmin, cmax) of the largest extent, ties to the smaller axis"""
    lo, hi = cells.min(0), cells.max(0)
    axis = int(np.argmax(hi - lo))                                       # (argmax takes the first of equal values)
    return axis, int(lo[axis]), int(hi[axis])


def choose_plane(v, cmin, cmax):
    """v int64 [n]: the block's cells along the axis, cmin < cmax -> (k, L(k)).  L is read off the sorted values at the planes that follow an
    occupied cell: a plane inside an empty run has the L of the run's first plane and a larger k, so it never wins"""
    n = len(v)
    occupied, counts = np.unique(v, return_counts=True)
    k = occupied[:-1] + 1                                                # every first plane of a run of equal L, ascending; cmax is no start
    L = np.cumsum(counts)[:-1]
    best = int(np.argmin(np.abs(2 * L - n)))                             # (the first of equal values: the smaller k)
    assert cmin + 1 <= k[best] <= cmax
    return int(k[best]), int(L[best])


def partition(coords, max_num, align=8):
    """-> Partition(block_of int32 [N], perm int32 [N], table int32 [B,8] = (first_row, rows, lo_x, lo_y, lo_z, hi_x, hi_y, hi_z), rounds,
    oversize).  ValueError naming the count for every violated precondition and for more than MAX_BLOCKS blocks."""
    xyz = check(coords, max_num, align)
    n = len(xyz)
    cells = xyz // align
    blocks = [np.arange(n)] if n else []
    rounds = 0
    while True:
        nxt, split = [], 0
        for rows in blocks:
            if len(rows) > max_num:
                axis, cmin, cmax = choose_axis(cells[rows])
                if cmax > cmin:
                    v = cells[rows, axis]
                    k, L = choose_plane(v, cmin, cmax)
                    left = v < k
                    assert left.sum() == L and 0 < L < len(rows)
                    nxt += [rows[left], rows[~left]]                     # (boolean selection keeps the input order)
                    split += 1
                    continue
            nxt.append(rows)
        if not split:
            break
        if len(nxt) > MAX_BLOCKS:
            raise ValueError(f'partition: {len(nxt)} blocks; at most {MAX_BLOCKS} (a larger max_num gives fewer)')
        blocks, rounds = nxt, rounds + 1
    block_of = np.zeros(n, np.int32)
    table = np.zeros((len(blocks), 8), np.int32)
    first = 0
    for b, rows in enumerate(blocks):
        block_of[rows] = b
        table[b] = [first, len(rows), *xyz[rows].min(0), *xyz[rows].max(0)]
        first += len(rows)
    perm = np.argsort(block_of, kind='stable').astype(np.int32)
    oversize = int((table[:, 1] > max_num).sum())
    return Partition(block_of, perm, table, rounds, oversize)
