"""The kd-tree block partition, the parts that need no GPU: the definition (tests/partition_reference.py) against an independent brute force
that counts every candidate plane directly, the figures pinned for the project's own clouds, hand-made cases, every refusal with its count,
`_P.bin` written, read back and refused, CLI parsing, and the C-ABI entries' refusals before anything is touched."""
import struct
import zlib

import numpy as np
import pytest

import partition_reference as R
from pcgcv2_amd import _lib, coder, partition, synthetic
from pcgcv2_amd._lib import PcgcError


def _named(name, order='raster'):
    return synthetic.cloud(name, order=order, seed=3).numpy().astype(np.int32)


# ---- the definition against brute force -----------------------------------------------------------------------------------------------------
def _brute_blocks(xyz, rows, max_num, align, depth=0):
    """recursive, every plane k in cmin + 1 .. cmax counted by itself -> ([row arrays in the in-order of the tree], depth of the tree)"""
    cells = xyz[rows] // align
    if len(rows) <= max_num:
        return [rows], depth
    extent = cells.max(0) - cells.min(0)
    axis = [a for a in range(3) if extent[a] == extent.max()][0]
    if extent[axis] == 0:
        return [rows], depth
    v = cells[:, axis]
    best = None
    for k in range(int(v.min()) + 1, int(v.max()) + 1):
        cost = abs(2 * int((v < k).sum()) - len(rows))
        if best is None or cost < best[0]:
            best = (cost, k)
    left, ldepth = _brute_blocks(xyz, rows[v < best[1]], max_num, align, depth + 1)
    right, rdepth = _brute_blocks(xyz, rows[v >= best[1]], max_num, align, depth + 1)
    return left + right, max(ldepth, rdepth)


def _check_against_brute(c, max_num, align=8):
    xyz = c[:, -3:].astype(np.int64)
    got = R.partition(c, max_num, align)
    blocks, depth = _brute_blocks(xyz, np.arange(len(c)), max_num, align)
    assert len(got.table) == len(blocks) and got.rounds == depth
    first = 0
    for b, rows in enumerate(blocks):
        assert np.array_equal(np.flatnonzero(got.block_of == b), rows)
        assert np.array_equal(got.perm[first:first + len(rows)], rows)                 # block-major, the input order inside a block
        assert got.table[b].tolist() == [first, len(rows), *xyz[rows].min(0), *xyz[rows].max(0)]
        first += len(rows)
    assert got.oversize == sum(len(r) > max_num for r in blocks)
    assert got.block_of.dtype == got.perm.dtype == got.table.dtype == np.int32 and got.table.shape == (len(blocks), 8)
    return got


@pytest.mark.parametrize('n,max_num,seed', [(50, 1, 0), (50, 7, 1), (120, 3, 2), (200, 20, 3), (400, 100, 4), (400, 1, 5), (333, 50, 6), (77, 76, 7)])
def test_definition_against_brute_force(n, max_num, seed):
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 64, (n, 3)).astype(np.int32)
    _check_against_brute(c, max_num)
    c4 = np.concatenate([np.zeros((n, 1), np.int32), c], 1)
    a, b = R.partition(c, max_num), R.partition(c4, max_num)
    assert all(np.array_equal(u, v) for u, v in zip(a[:3], b[:3])) and a[3:] == b[3:]


# ---- pinned figures -------------------------------------------------------------------------------------------------------------------------
PINS = {                                                                               # blocks at max_num = N, N - 1, 4000, 1000, 300
    'shell7': (12132, [1, 2, 4, 16, 52]),
    'multi_s': (15733, [1, 2, 5, 23, 76]),
    'noisy_s': (11086, [1, 2, 4, 16, 50]),
    'solid_cube_s': (13824, [1, 2, 6, 27, 27]),
    # (a block of N rows is above max_num = N - 1 and spans more than one cell: the definition splits it)
    'sparse_s': (7571, [1, 2, 2, 8, 37]),
}


@pytest.mark.parametrize('name', sorted(PINS))
def test_pinned_figures(name):
    c = _named(name)
    n, blocks = PINS[name]
    assert len(c) == n
    got = [R.partition(c, m) for m in (n, n - 1, 4000, 1000, 300)]
    assert [len(p.table) for p in got] == blocks
    for p in got:
        assert p.table[:, 1].sum() == n and np.array_equal(np.sort(p.perm), np.arange(n))
    if name == 'shell7':
        assert [p.rounds for p in got] == [0, 1, 2, 4, 6] and [int(p.table[:, 1].max()) for p in got] == [12132, 6066, 3044, 785, 297]
    if name == 'multi_s':
        assert [p.rounds for p in got] == [0, 1, 3, 5, 8]
    if name == 'solid_cube_s':                                                         # 27 full 8^3 cells of 512 rows
        assert got[4].oversize == 27 and (got[4].table[:, 1] == 512).all() and got[3].oversize == 0
    assert all(p.oversize == 0 for p in got[:4])


# ---- properties and hand-made cases ---------------------------------------------------------------------------------------------------------
def test_shuffled_rows_give_the_same_blocks_as_sets():
    c = _named('sparse_s')
    a = R.partition(c, 300)
    order = np.random.default_rng(5).permutation(len(c))
    b = R.partition(c[order], 300)
    assert np.array_equal(a.table[:, 1:], b.table[:, 1:]) and (a.rounds, a.oversize) == (b.rounds, b.oversize)
    assert np.array_equal(b.block_of, a.block_of[order])                               # the same voxel, the same block
    for blk in range(len(b.table)):
        mine = b.perm[b.table[blk, 0]:b.table[blk, 0] + b.table[blk, 1]]
        assert (np.diff(mine) > 0).all() and (b.block_of[mine] == blk).all()           # perm follows the input order


def test_duplicate_rows_share_a_block():
    rng = np.random.default_rng(11)
    c = rng.integers(0, 40, (150, 3)).astype(np.int32)
    c = np.concatenate([c, c[:60], c[:20]])[rng.permutation(230)]
    got = _check_against_brute(c, 9)
    _, inverse = np.unique(c, axis=0, return_inverse=True)
    for voxel in range(inverse.max() + 1):
        assert len(set(got.block_of[inverse.reshape(-1) == voxel].tolist())) == 1


def test_align_16():
    c = np.random.default_rng(2).integers(0, 128, (300, 3)).astype(np.int32)
    got = _check_against_brute(c, 10, align=16)
    owner = {}
    for cell, b in zip(map(tuple, (c // 16).tolist()), got.block_of.tolist()):       # no stride-16 cell is shared by two blocks
        assert owner.setdefault(cell, b) == b


def test_balance_tie_goes_to_the_smaller_plane():
    x = np.array([0] * 3 + [8] * 2 + [16] * 3, np.int32)                               # cell counts (3, 2, 3): L(1) = 3 and L(2) = 5 are as far from 4
    c = np.stack([x, np.zeros(8, np.int32), np.zeros(8, np.int32)], 1)
    got = R.partition(c, 7)
    assert got.table[:, 1].tolist() == [3, 5] and got.table[0, 5] == 0 and got.table[1, 2] == 8
    assert R.choose_plane(x.astype(np.int64) // 8, 0, 2) == (1, 3)


def test_extent_tie_goes_to_x():
    g = np.arange(0, 32, 8, dtype=np.int32)
    c = np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3)               # a cube of 4^3 cells, one row each
    got = R.partition(c, 63)
    assert len(got.table) == 2 and got.table[0, 2:].tolist() == [0, 0, 0, 8, 24, 24] and got.table[1, 2:].tolist() == [16, 0, 0, 24, 24, 24]
    flat = c.copy()
    flat[:, 0] = 0                                                                     # x has no extent: y before z
    got = R.partition(flat, 63)
    assert got.table[0, 2:].tolist() == [0, 0, 0, 0, 8, 24]


def test_one_cell_is_oversize_and_empty_is_nothing():
    g = np.arange(8, dtype=np.int32)
    c = np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3) + 40
    got = R.partition(c, 100)
    assert (len(got.table), got.rounds, got.oversize) == (1, 0, 1) and got.table[0].tolist() == [0, 512, 40, 40, 40, 47, 47, 47]
    none = R.partition(np.zeros((0, 3), np.int32), 5)
    assert none.table.shape == (0, 8) and none.block_of.shape == (0,) and none.perm.shape == (0,) and (none.rounds, none.oversize) == (0, 0)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_count():
    ok = np.array([[0, 0, 0], [8, 0, 0], [16, 0, 0], [24, 0, 0]], np.int32)
    far = ok.copy()
    far[1, 0], far[2, 2], far[3, 1] = 1 << 20, -1, (1 << 20) - 1                       # the last one is inside
    with pytest.raises(ValueError, match='2 of 4 rows are outside'):
        R.partition(far, 2)
    batch = np.concatenate([np.array([[0], [1], [0], [-1]], np.int32), ok], 1)
    with pytest.raises(ValueError, match='2 of 4 rows have a batch index other than 0'):
        R.partition(batch, 2)
    for bad in (0, -3, True, 2.0):
        with pytest.raises(ValueError, match='max_num'):
            R.partition(ok, bad)
    for bad in (4, 12, 2048, 0, True):
        with pytest.raises(ValueError, match='align'):
            R.partition(ok, 2, align=bad)
    with pytest.raises(ValueError, match='int32'):
        R.partition(ok.astype(np.int64), 2)
    with pytest.raises(ValueError, match='int32'):
        R.partition(np.zeros((4, 5), np.int32), 2)
    line = np.zeros((1025, 3), np.int32)
    line[:, 0] = 8 * np.arange(1025)
    with pytest.raises(ValueError, match='1025 blocks'):
        R.partition(line, 1)
    assert len(R.partition(line[:1024], 1).table) == 1024 and R.partition(line[:1024], 1).rounds == 10

    class Big:                                                                         # 2^27 + 1 rows without the memory
        ndim, shape, dtype = 2, ((1 << 27) + 1, 3), np.dtype(np.int32)
    with pytest.raises(ValueError, match='134217729 rows'):
        R.check(Big(), 5)


# ---- _P.bin ---------------------------------------------------------------------------------------------------------------------------------
def _table():
    return R.partition(_named('sparse_s'), 1000).table


def _refit(blob):
    return blob[:-4] + struct.pack('<I', zlib.crc32(blob[:-4]))


def test_blocks_file_round_trip():
    t = _table()
    blob = partition.pack_blocks(t, 8, 1000, 0)
    assert len(blob) == 28 + 28 * len(t) + 4 and blob[:4] == b'PCGP'
    got = partition.unpack_blocks(blob)
    assert (got.align, got.max_num, got.mode) == (8, 1000, 0)
    assert np.array_equal(got.rows, t[:, 1]) and np.array_equal(got.lo, t[:, 2:5]) and np.array_equal(got.hi, t[:, 5:8])
    big = partition.unpack_blocks(partition.pack_blocks(t[:, 1:], 1024, (1 << 64) - 1, 1))
    assert (big.align, big.max_num, big.mode) == (1024, (1 << 64) - 1, 1)
    empty = partition.unpack_blocks(partition.pack_blocks(np.zeros((0, 8), np.int32), 8, 1, 0))
    assert len(empty.rows) == 0
    assert partition.blocks_meeting(got, (0, 0, 0, (1 << 20) - 1, (1 << 20) - 1, (1 << 20) - 1)) == list(range(len(t)))
    lo, hi = t[3, 2:5], t[3, 5:8]
    assert 3 in partition.blocks_meeting(got, (*hi, *hi)) and 3 in partition.blocks_meeting(got, (*lo, *lo))
    assert partition.blocks_meeting(got, (1 << 19, 1 << 19, 1 << 19, 1 << 19, 1 << 19, 1 << 19)) == []
    assert partition.block_postfix('_r1', 7) == '_r1_b0007'


# (offset, format, damaged value, what the reader says when the CRC has been made to fit)
DAMAGE = [(0, '<4s', b'PCGQ', 'magic'), (4, '<I', 2, 'version'), (8, '<I', 12, 'align'), (12, '<Q', 0, 'max_num'), (20, '<I', 2, 'mode'),
          (24, '<I', 1025, 'blocks'), (24, '<I', 3, 'bytes'), (28, '<I', 0, 'no row'), (28, '<I', 1 << 31, 'more rows than'),
          (32, '<I', 1 << 20, '2\\^20'), (52, '<I', 1 << 20, '2\\^20'), (36, '<I', (1 << 20) - 1, 'lo above hi')]


@pytest.mark.parametrize('offset,fmt,value,says', DAMAGE)
def test_blocks_file_damage_is_refused(offset, fmt, value, says):
    blob = partition.pack_blocks(_table(), 8, 1000, 0)
    size = struct.calcsize(fmt)
    bad = blob[:offset] + struct.pack(fmt, value) + blob[offset + size:]
    assert bad != blob
    with pytest.raises(PcgcError):                                                     # the CRC no longer fits (or an earlier check speaks)
        partition.unpack_blocks(bad)
    with pytest.raises(PcgcError, match=says):                                         # and with a CRC made to fit the field itself is refused
        partition.unpack_blocks(_refit(bad))


def test_blocks_file_length_and_crc():
    blob = partition.pack_blocks(_table(), 8, 1000, 0)
    for bad in (blob[:-1], blob + b'\0', blob[:20], b''):
        with pytest.raises(PcgcError, match='bytes'):
            partition.unpack_blocks(bad)
    with pytest.raises(PcgcError, match='CRC'):
        partition.unpack_blocks(blob[:-1] + bytes([blob[-1] ^ 1]))
    with pytest.raises(PcgcError, match='CRC'):
        partition.unpack_blocks(blob[:33] + bytes([blob[33] ^ 4]) + blob[34:])
    for kw in (dict(align=12), dict(max_num=0), dict(mode=2)):
        with pytest.raises(ValueError):
            partition.pack_blocks(_table(), **{**dict(align=8, max_num=1000, mode=0), **kw})
    with pytest.raises(ValueError):
        partition.pack_blocks(np.zeros((1025, 8), np.int32), 8, 1000, 0)


# ---- CLI ------------------------------------------------------------------------------------------------------------------------------------
def test_cli_parsing(capsys):
    args = partition.parse_args(['--filedir', 'vox.ply', '--max_num', '4000'])
    assert (args.max_num, args.align, args.ckptdir, args.lossless, args.roi, args.block_batch, args.outdir) == (4000, 8, None, False, None, 16, './output')
    args = partition.parse_args(['--filedir', 'vox.ply', '--max_num', '300', '--align', '16', '--ckptdir', 'm.pth', '--lossless', '--roi', '0,1,2,30,40,50',
                                 '--outdir', 'o', '--block_batch', '5'])
    assert (args.align, args.ckptdir, args.lossless, args.roi, args.outdir, args.block_batch) == (16, 'm.pth', True, (0, 1, 2, 30, 40, 50), 'o', 5)
    for bad in (['--max_num', '0'], ['--max_num', '9', '--align', '12'], ['--max_num', '9', '--lossless'], ['--max_num', '9', '--roi', '0,0,0,1,1,1'],
                ['--max_num', '9', '--ckptdir', 'm', '--roi', '0,0,0,1,1'], ['--max_num', '9', '--ckptdir', 'm', '--roi', '5,0,0,1,1,1'],
                ['--max_num', '9', '--ckptdir', 'm', '--block_batch', '17'], ['--max_num', '9', '--ckptdir', 'm', '--lossless', '--rho', '0.5'], []):
        with pytest.raises(SystemExit):
            partition.parse_args(['--filedir', 'vox.ply'] + bad)
    args = coder._parse_cli(['--filedir', 'vox.ply', '--max_num', '4000', '--block_batch', '4', '--roi', '0,0,0,63,63,63', '--recolour'])
    assert (args.max_num, args.block_batch, args.roi, args.recolour) == (4000, 4, (0, 0, 0, 63, 63, 63), True)
    args = coder._parse_cli(['--filedir', 'vox.ply'])                                  # without the flag nothing moves
    assert (args.max_num, args.block_batch, args.roi, args.res, args.rho) == (None, 16, None, 1024, 1.0)
    for bad in (['--max_num', '0'], ['--roi', '0,0,0,1,1,1'], ['--block_batch', '4'], ['--block_batch', '16'], ['--max_num', '9', '--block_batch', '0'],
                ['--max_num', '9', '--roi', 'a,b'], ['--max_num', '9', '--lossless']):
        with pytest.raises(SystemExit):
            coder._parse_cli(['--filedir', 'vox.ply'] + bad)
    assert 'pcgcv2_amd.partition --lossless' in capsys.readouterr().err


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------------
EXPORTS = ('pcgc_partition_workspace_bytes', 'pcgc_partition', 'pcgc_partition_gather')


def test_exports_and_refusals_before_anything_is_touched():
    import ctypes
    L = _lib.lib()
    for name in EXPORTS:
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    err = lambda: L.pcgc_last_error().decode()
    p = 4096                                                                           # a pointer that is not null and must never be followed
    info = (ctypes.c_int64 * 8)(*([7] * 8))
    n = 1000
    need = int(L.pcgc_partition_workspace_bytes(n))
    fixed = int(L.pcgc_partition_workspace_bytes(0))
    assert fixed >= 1024 * (2 * 1024 + 128) * 4 and need >= 1024 * (2 * 1024 + 128) * 4 + 3 * 4 * n        # the histograms, three words a row
    assert int(L.pcgc_partition_workspace_bytes(1 << 20)) - fixed <= 64 * (1 << 20)    # O(n): no term in any block's extent

    def call(n=n, cols=3, max_num=10, align=8, ws=need, hole=None, ws_at=p):
        a = [None if j == hole else p for j in range(5)]
        return L.pcgc_partition(a[0], n, cols, max_num, align, a[1], a[2], a[3], None if hole == 4 else info, None, None if hole == 5 else ws_at, ws, None)
    assert call(n=-1) == -2 and 'row count' in err()
    assert call(n=(1 << 27) + 1, ws=1 << 40) == -2 and 'row count' in err()
    assert call(cols=5) == -2 and call(cols=2) == -2 and 'columns' in err()
    assert call(max_num=0) == -2 and 'max_num' in err()
    for bad in (4, 12, 2048, 0, -8):
        assert call(align=bad) == -2 and 'align' in err(), bad
    assert call(ws=need - 1) == -2 and 'too small' in err()
    for hole in range(6):
        assert call(hole=hole) == -2 and 'null' in err(), hole
    assert call(ws_at=p + 8) == -2 and 'misaligned' in err()
    assert list(info) == [7] * 8                                                       # nothing was written

    def gather(n=n, cols=4, first_row=0, rows=10, first_block=0, hole=None, out=p):
        a = [None if j == hole else p for j in range(3)]
        return L.pcgc_partition_gather(a[0], n, cols, a[1], a[2], first_row, rows, first_block, None if hole == 3 else out, None)
    assert gather(n=-1) == -2 and gather(n=(1 << 27) + 1) == -2 and gather(cols=5) == -2
    assert gather(first_row=-1) == -2 and gather(rows=-1) == -2 and gather(first_row=995, rows=6) == -2 and 'outside the rows' in err()
    assert gather(first_block=-1) == -2 and gather(first_block=1024) == -2
    for hole in range(4):
        assert gather(hole=hole) == -2 and 'null' in err(), hole
    assert gather(out=p + 4) == -2 and 'misaligned' in err()
