"""The kd-tree block partition on the GPU (csrc/partition.hip, pcgcv2_amd/partition.py): block_of, perm, the table, rounds and oversize EQUAL
to the numpy definition (tests/partition_reference.py), no tolerance, at the smallest shapes at which the kernels can go wrong: no row, one
and two rows, an empty run of 2^17 - 2 cells, one full cell, 1 024 and 1 025 blocks, a chain 12 deep, bins of more than one cell with the
occupied cell before the crossing three bins back, row counts around the multiples of a wave and a workgroup with two blocks interleaved;
then the codec in blocks against coding every block alone, the region of interest, the lossless mode and the three command lines."""
import ctypes
import os

import numpy as np
import pytest
import torch

import partition_reference as R
import scratch_arena as SA
from pcgcv2_amd import coder, ops, partition, synthetic
from pcgcv2_amd._lib import lib
from pcgcv2_amd.coder import Coder, STREAMS
from pcgcv2_amd.data_utils import read_ply_ascii_geo, write_ply_ascii_geo
from pcgcv2_amd.lossless import same_voxels
from pcgcv2_amd.pcc_model import PCCModel
from pcgcv2_amd.sparse import SparseTensor

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
MAX_NUMS = lambda n: (n, n - 1, 4000, 1000, 300)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same(got, want):
    assert got.block_of.dtype == got.perm.dtype == got.table.dtype == torch.int32 and tuple(got.table.shape) == want.table.shape
    assert np.array_equal(got.table.cpu().numpy(), want.table)
    assert np.array_equal(got.block_of.cpu().numpy(), want.block_of)
    assert np.array_equal(got.perm.cpu().numpy(), want.perm)
    assert (got.rounds, got.oversize) == (want.rounds, want.oversize)


def _check(c, max_num, align=8):
    c = np.asarray(c, np.int32)
    want = R.partition(c, max_num, align)
    got = ops.partition(_dev(c), max_num, align=align)
    _same(got, want)
    return want


_NAMED = {}


def _named(name, order='raster'):
    if (name, order) not in _NAMED:
        _NAMED[name, order] = synthetic.cloud(name, order=order, seed=3).numpy().astype(np.int32)
    return _NAMED[name, order]


def _line(cells, axis=0):
    c = np.zeros((len(cells), 3), np.int32)
    c[:, axis] = 8 * np.asarray(cells)
    return c


# ---- the smallest clouds ----------------------------------------------------------------------------------------------------------------------
def test_no_row_and_one_row():
    for cols in (3, 4):
        got = ops.partition(torch.zeros((0, cols), dtype=torch.int32, device=DEV), 5)
        assert tuple(got.table.shape) == (0, 8) and len(got.block_of) == len(got.perm) == 0 and (got.rounds, got.oversize) == (0, 0)
    assert _check([[5, 6, 7]], 1).table.tolist() == [[0, 1, 5, 6, 7, 5, 6, 7]]
    assert _check([[0, (1 << 20) - 1, 9, 3]], 1).table.tolist() == [[0, 1, (1 << 20) - 1, 9, 3, (1 << 20) - 1, 9, 3]]


def test_two_rows():
    one_cell = _check([[8, 8, 8], [15, 15, 15]], 1)
    assert (len(one_cell.table), one_cell.rounds, one_cell.oversize) == (1, 0, 1)
    adjacent = _check([[8, 0, 0], [7, 0, 0]], 1)                                      # the second row is the left child
    assert adjacent.block_of.tolist() == [1, 0] and adjacent.perm.tolist() == [1, 0] and adjacent.rounds == 1
    _check([[8, 0, 0], [7, 0, 0]], 2)
    for axis in range(3):                                                             # an empty run of 2^17 - 2 cells: the plane is 1
        c = np.zeros((2, 3), np.int32)
        c[1, axis] = (1 << 20) - 1
        far = _check(c, 1)
        assert far.table[:, 1].tolist() == [1, 1] and far.table[1, 2 + axis] == (1 << 20) - 1
        _check(c[::-1], 1)


def test_one_full_cell_is_oversize():
    g = np.arange(8, dtype=np.int32)
    c = np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3) + 1016
    want = _check(c, 100)
    assert (len(want.table), want.rounds, want.oversize) == (1, 0, 1)


def test_1024_blocks_and_the_refusal_of_1025():
    want = _check(_line(np.arange(1024)), 1)
    assert (len(want.table), want.rounds) == (1024, 10)
    _check(_line(np.arange(1024))[np.random.default_rng(0).permutation(1024)], 1, align=8)
    c = _dev(_line(np.arange(1025), axis=1))
    with pytest.raises(ValueError, match='1025 blocks'):
        ops.partition(c, 1)
    # nothing of the caller's has been written when the entry refuses
    n = 1025
    outs = [torch.full((n,), 77, dtype=torch.int32, device=DEV), torch.full((n,), 77, dtype=torch.int32, device=DEV),
            torch.full((1024, 8), 77, dtype=torch.int32, device=DEV)]
    need = int(lib().pcgc_partition_workspace_bytes(n))
    ws = torch.empty((need + 7) // 8, dtype=torch.int64, device=DEV)
    info = (ctypes.c_int64 * 8)()
    rc = lib().pcgc_partition(c.data_ptr(), n, 3, 1, 8, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), info, None, ws.data_ptr(), need, None)
    torch.cuda.synchronize()
    assert rc == -4 and info[5] == 1025 and all(bool((o == 77).all()) for o in outs)
    rc = lib().pcgc_partition(c.data_ptr(), n, 3, 1, 8, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), info, None, ws.data_ptr(), need - 1, None)
    torch.cuda.synchronize()
    assert rc == -2 and all(bool((o == 77).all()) for o in outs)


def test_refusals_name_the_count():
    ok = np.array([[0, 0, 0], [8, 0, 0], [16, 0, 0], [24, 0, 0]], np.int32)
    far = ok.copy()
    far[1, 0], far[2, 2], far[3, 1] = 1 << 20, -1, (1 << 20) - 1
    with pytest.raises(ValueError, match='2 of 4 rows are outside'):
        ops.partition(_dev(far), 2)
    batch = np.concatenate([np.array([[0], [1], [0], [-1]], np.int32), ok], 1)
    with pytest.raises(ValueError, match='2 of 4 rows have a batch index other than 0'):
        ops.partition(_dev(batch), 2)
    for kw in (dict(max_num=0), dict(max_num=True), dict(max_num=2, align=12), dict(max_num=2, align=4)):
        with pytest.raises(ValueError):
            ops.partition(_dev(ok), **kw)
    with pytest.raises(ValueError, match='int32'):
        ops.partition(_dev(ok).long(), 2)
    with pytest.raises(Exception, match='device'):
        ops.partition(torch.from_numpy(ok), 2)


def test_a_chain_12_deep():
    rows = []
    for j in range(13):                                                               # cell j holds 2^(12 - j) rows (voxels of the cell, repeated)
        i = np.arange(1 << (12 - j))
        rows.append(np.stack([8 * j + i % 8, i // 8 % 8, i // 64 % 8], 1))
    c = np.concatenate(rows).astype(np.int32)
    want = _check(c, 1)
    assert (len(want.table), want.rounds, want.oversize) == (13, 12, 12) and want.table[:, 1].tolist() == [1 << (12 - j) for j in range(13)]
    _check(c[np.random.default_rng(1).permutation(len(c))], 1)


def test_bins_of_16_cells_and_the_occupied_cell_three_bins_back():
    # 4 097 occupied cells over an extent of 16 384: w = 16.  Row 2 049 of the sorted cells, the crossing, is cell 2085 in bin 130; the
    # occupied cell before it is 2047 in bin 127; planes 2048 (L = 2048) and 2086 (L = 2049) are as good: the smaller one
    cells = np.concatenate([np.arange(2048), [2085], np.arange(2086, 2086 + 2047), [16383]])
    assert len(cells) == 4097
    for axis in range(3):
        want = _check(_line(cells, axis), 4096)
        assert want.table[:, 1].tolist() == [2048, 2049] and want.table[1, 2 + axis] == 8 * 2085
    _check(_line(cells), 100)                                                         # and on down, bins of 16, 3 and 2 cells and of one
    _check(_line(cells)[np.random.default_rng(2).permutation(4097)], 100)
    shifted = cells.copy()
    shifted[2048] = 2086 + 2047 + 40                                                  # the crossing moves to 2086: the plane before it is 2048, three bins back
    _check(_line(shifted, 2), 4096)


@pytest.mark.parametrize('n', [63, 64, 65, 255, 256, 257, 1023, 1024, 1025])
def test_row_counts_around_waves_and_workgroups_with_two_blocks_interleaved(n):
    rng = np.random.default_rng(n)
    c = rng.integers(0, 40, (n, 3)).astype(np.int32)
    c[1::2, 0] += 4000                                                                # odd rows far away: every wave holds rows of both blocks
    for max_num in ((n + 1) // 2, max(1, n // 8), 1):
        _check(c, max_num)
    _check(c, 5, align=16)


# ---- the project's clouds ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('order', ['raster', 'shuffled'])
@pytest.mark.parametrize('name', ['shell7', 'multi_s', 'noisy_s', 'solid_cube_s', 'sparse_s'])
def test_synthetic_clouds(name, order):
    c = _named(name, order)
    d = _dev(c)
    for max_num in MAX_NUMS(len(c)):
        _same(ops.partition(d, max_num), R.partition(c, max_num))


def test_strided_input_and_the_batch_column():
    c = _named('sparse_s', 'shuffled')
    want = R.partition(c, 300)
    wide = torch.zeros((len(c), 7), dtype=torch.int32, device=DEV)
    wide[:, 2:5] = _dev(c)
    _same(ops.partition(wide[:, 2:5], 300), want)                                    # rows 28 bytes apart
    _same(ops.partition(wide[:, 1:5], 300), want)                                    # with a batch column of zeros
    twice = torch.stack([_dev(c), _dev(c) + 1], 1).reshape(-1, 3)
    _same(ops.partition(twice[::2], 300), want)                                      # every other row
    x = SparseTensor(torch.ones((len(c), 1)), coordinates=torch.cat([torch.zeros((len(c), 1), dtype=torch.int32), torch.from_numpy(c)], 1),
                     tensor_stride=1, device=DEV)
    _same(partition.partition(x, 300), want)                                         # a sparse tensor's coordinates


def test_two_runs_byte_for_byte():
    d = _dev(_named('multi_s', 'shuffled'))
    a, b = ops.partition(d, 300), ops.partition(d, 300)
    assert torch.equal(a.block_of, b.block_of) and torch.equal(a.perm, b.perm) and torch.equal(a.table, b.table) and a[3:] == b[3:]
    times = {}
    t = ops.partition(d, 300, times=times)                                           # the measurement hook changes nothing
    assert torch.equal(a.block_of, t.block_of) and torch.equal(a.perm, t.perm) and torch.equal(a.table, t.table)
    assert set(times) == set(ops.PARTITION_PHASES) and all(v >= 0 for v in times.values())


def test_recycled_scratch_and_guard_bands():
    """one run on fresh memory, one on the blocks an other cloud's run left behind: the same bytes, every guard intact"""
    a, b = _named('noisy_s', 'shuffled'), _named('solid_cube_s', 'shuffled')
    a = np.concatenate([a, a[:len(b) - len(a)] + np.array([1, 0, 0], np.int32)])     # as many rows as b
    assert len(a) == len(b)
    run = lambda c: ops.partition(_dev(c), 300)
    want = R.partition(b, 300)
    run(a)
    fresh, rec = SA.Arena(), SA.Arena()
    outs = []
    for arena, cloud in ((fresh, b), (rec, a)):
        with SA.installed(arena):
            outs.append(run(cloud))
        torch.cuda.synchronize()
        arena.finish()
        arena.check()
    stale = rec.replay()
    with SA.installed(stale):
        got = run(b)
    torch.cuda.synchronize()
    stale.finish()
    for arena in (fresh, rec, stale):
        arena.check()
    _same(got, want)
    _same(outs[0], want)
    allocs, replayed, _ = stale.stats()
    assert allocs >= 4 and replayed == allocs and not stale.served_fresh


def test_gather_of_a_run_of_blocks():
    c = _named('sparse_s', 'shuffled')
    want = R.partition(c, 300)
    d = _dev(c)
    part = ops.partition(d, 300)
    for first, blocks in ((0, 16), (16, 16), (32, 5), (36, 1), (0, 1)):
        rows = want.perm[want.table[first, 0]:want.table[first + blocks - 1, 0] + want.table[first + blocks - 1, 1]]
        expect = np.concatenate([(want.block_of[rows] - first)[:, None], c[rows]], 1)
        assert np.array_equal(ops.partition_gather(d, part, first, blocks).cpu().numpy(), expect)
    with pytest.raises(ValueError):
        ops.partition_gather(d, part, 30, 8)


# ---- the codec in blocks ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def model():
    m = PCCModel().to(DEV)
    m.load_state_dict(synthetic.synthetic_state_dict())
    return m


def _tensor(xyz):
    c4 = np.concatenate([np.zeros((len(xyz), 1), np.int32), np.asarray(xyz, np.int32)], 1)
    return SparseTensor(torch.ones((len(c4), 1)), coordinates=torch.from_numpy(c4), tensor_stride=1, device=DEV)


FILES = STREAMS + ('_F.idx',)


def _files(stem):
    return {s: open(stem + s, 'rb').read() if os.path.exists(stem + s) else None for s in FILES}


@pytest.fixture(scope='module')
def shell7_alone(model, tmp_path_factory):
    """shell7's blocks at max_num = 4000 and 300, each coded ALONE by Coder.encode, on demand and once: (cloud, {max_num: definition},
    files(max_num, i), decoded(max_num, i, rho))"""
    d = tmp_path_factory.mktemp('alone')
    c = _named('shell7')
    wants = {m: R.partition(c, m) for m in (4000, 300)}
    alone = Coder(model, str(d / 'a'))
    done = {}

    def files(max_num, i):
        if (max_num, i) not in done:
            alone.encode(_tensor(c[wants[max_num].block_of == i]), postfix=f'_{max_num}_{i}')
            done[max_num, i] = _files(str(d / 'a') + f'_{max_num}_{i}')
        return done[max_num, i]

    def decoded(max_num, i, rho):
        files(max_num, i)
        return alone.decode(rho=rho, postfix=f'_{max_num}_{i}').C
    return c, wants, files, decoded


def test_four_blocks_in_one_batch(model, shell7_alone, tmp_path):
    c, wants, files, decoded = shell7_alone
    want = wants[4000]
    bc = partition.BlockCoder(model, str(tmp_path / 'b'), 4000)
    part = bc.encode(_tensor(c))
    _same(part, want)
    assert len(want.table) == 4
    blocks = partition.read_blocks(str(tmp_path / 'b'))
    assert (blocks.align, blocks.max_num, blocks.mode) == (8, 4000, 0) and np.array_equal(blocks.rows, want.table[:, 1])
    assert np.array_equal(blocks.lo, want.table[:, 2:5]) and np.array_equal(blocks.hi, want.table[:, 5:8])
    for i in range(4):
        assert _files(str(tmp_path / 'b') + f'_b{i:04d}') == files(4000, i), i
    for rho in (1, 0.7):
        merged = bc.decode(rho=rho)
        assert torch.equal(merged.C, torch.cat([decoded(4000, i, rho) for i in range(4)], 0)), rho
        assert bool((merged.C[:, 0] == 0).all())
    bits = sum(8 * len(v) for i in range(4) for s, v in files(4000, i).items() if s in STREAMS) + 8 * os.path.getsize(str(tmp_path / 'b_P.bin'))
    assert bc.block_bits() == partition.block_bits(str(tmp_path / 'b')) == bits


def test_52_blocks_in_batches_of_16_and_of_5(model, shell7_alone, tmp_path):
    c, wants, files, decoded = shell7_alone
    want = wants[300]
    assert len(want.table) == 52
    b16, b5 = partition.BlockCoder(model, str(tmp_path / 'p'), 300), partition.BlockCoder(model, str(tmp_path / 'q'), 300, batch_items=5)
    _same(b16.encode(_tensor(c)), want)
    _same(b5.encode(_tensor(c), postfix='_r'), want)
    edges = (0, 15, 16, 31, 32, 47, 48, 51)                                           # the first and last block of each batch of 16
    for i in edges:
        assert _files(str(tmp_path / 'p') + f'_b{i:04d}') == files(300, i), i
    for i in range(52):
        assert _files(str(tmp_path / 'p') + f'_b{i:04d}') == _files(str(tmp_path / 'q') + f'_r_b{i:04d}'), i
    assert open(str(tmp_path / 'p_P.bin'), 'rb').read() == open(str(tmp_path / 'q_r_P.bin'), 'rb').read()
    for rho in (1, 0.7):
        merged = b16.decode(rho=rho)
        assert torch.equal(merged.C, b5.decode(rho=rho, postfix='_r').C)
        # the decoded voxels of a block lie in the block's own stride-8 cells, which no other block shares: that tells whose each row is
        cell_block = {tuple(v): b for v, b in zip((c // 8).tolist(), want.block_of.tolist())}
        owner = np.array([cell_block[tuple(v)] for v in (merged.C[:, 1:].cpu().numpy() // 8).tolist()])
        assert (np.diff(owner) >= 0).all()                                            # block order
        for i in edges:
            rows = np.flatnonzero(owner == i)
            assert len(rows) and torch.equal(merged.C[rows[0]:rows[-1] + 1], decoded(300, i, rho)), (rho, i)


def test_one_block_is_the_plain_coder(model, tmp_path):
    c = _named('shell7')
    bc = partition.BlockCoder(model, str(tmp_path / 'b'), len(c))
    part = bc.encode(_tensor(c))
    assert len(part.table) == 1 and part.rounds == 0
    plain = Coder(model, str(tmp_path / 'plain'))
    plain.encode(_tensor(c))
    assert _files(str(tmp_path / 'b_b0000')) == _files(str(tmp_path / 'plain'))
    assert torch.equal(bc.decode().C, plain.decode().C)


def test_region_of_interest(model, shell7_alone, tmp_path):
    c, wants, files, decoded = shell7_alone
    table = wants[4000].table
    stem = str(tmp_path / 'b')
    bc = partition.BlockCoder(model, stem, 4000)
    bc.encode(_tensor(c))
    roi = (60, 40, 32, 70, 50, 95)
    met = [i for i in range(4) if (table[i, 2:5] <= np.array(roi[3:])).all() and (table[i, 5:8] >= np.array(roi[:3])).all()]
    assert len(met) == 2
    want = torch.cat([decoded(4000, i, 1) for i in met], 0)
    assert torch.equal(bc.decode(roi=roi).C, want)
    for i in range(4):                                                                # no file of any other block is opened: they are gone
        if i not in met:
            for s in FILES:
                if os.path.exists(stem + f'_b{i:04d}' + s):
                    os.remove(stem + f'_b{i:04d}' + s)
    assert torch.equal(bc.decode(roi=roi).C, want)
    one = tuple(int(v) for v in table[met[1], 2:5]) * 2                               # a single voxel: a corner of the second block's box
    assert torch.equal(bc.decode(roi=one).C, decoded(4000, met[1], 1))
    nothing = bc.decode(roi=(1 << 19, 1 << 19, 1 << 19, (1 << 19) + 5, (1 << 19) + 5, (1 << 19) + 5))
    assert tuple(nothing.C.shape) == (0, 4) and len(nothing) == 0
    with pytest.raises(ValueError, match='roi'):
        bc.decode(roi=(5, 0, 0, 1, 1, 1))
    with pytest.raises(Exception):                                                    # the whole cloud does need them
        bc.decode()


def test_lossless_blocks(model, tmp_path):
    c = _named('multi_s')
    x = _tensor(c)
    bc = partition.BlockCoder(model, str(tmp_path / 'l'), 1000, lossless=True)
    part = bc.encode(x)
    assert len(part.table) == 23
    merged = bc.decode()
    assert same_voxels(merged.C, x.C)
    blocks = partition.read_blocks(str(tmp_path / 'l'))
    assert blocks.mode == 1 and all(os.path.exists(str(tmp_path / 'l') + f'_b{i:04d}_O.bin') for i in range(23))
    assert len(partition.block_stream_bits(str(tmp_path / 'l'))) == 6
    with pytest.raises(Exception, match='mode'):
        partition.BlockCoder(model, str(tmp_path / 'l'), 1000).decode()


# ---- the three command lines --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def sparse_ply(tmp_path_factory):
    d = tmp_path_factory.mktemp('partition')
    c = _named('sparse_s', 'shuffled')
    path = str(d / 'sparse.ply')
    write_ply_ascii_geo(path, c)
    ckpt = str(d / 'synthetic.pth')
    torch.save({'model': synthetic.synthetic_state_dict()}, ckpt)
    return d, path, ckpt, c


def test_partition_cli_prints_the_table(sparse_ply, capsys):
    d, path, _, c = sparse_ply
    want = R.partition(c, 1000)
    assert partition.main(['--filedir', path, '--max_num', '1000']) == 0
    text = capsys.readouterr().out
    assert f'{len(c)} rows, 8 blocks, {want.rounds} rounds, 0 oversize, largest {want.table[:, 1].max()}, smallest {want.table[:, 1].min()}' in text
    for i, row in enumerate(want.table):
        assert f'{i}\t {row[0]}\t {row[1]}\t {tuple(int(v) for v in row[2:5])}' in text


def test_partition_cli_codes_and_checks(sparse_ply, capsys):
    d, path, ckpt, c = sparse_ply
    want = R.partition(c, 4000)
    lo = tuple(int(v) for v in want.table[1, 2:5])
    outdir = str(d / 'lossy')
    assert partition.main(['--filedir', path, '--max_num', '4000', '--ckptdir', ckpt, '--outdir', outdir, '--roi', ','.join(str(v) for v in lo * 2)]) == 0
    text = capsys.readouterr().out
    assert '2 blocks' in text and 'round trip OK' in text and 'blocks [1]' in text
    assert os.path.exists(os.path.join(outdir, 'sparse_P.bin')) and len(read_ply_ascii_geo(os.path.join(outdir, 'sparse_dec.ply'))) > 0
    outdir = str(d / 'lossless')
    assert partition.main(['--filedir', path, '--max_num', '4000', '--ckptdir', ckpt, '--outdir', outdir, '--lossless']) == 0
    assert "the voxel set is the input's" in capsys.readouterr().out
    decoded = read_ply_ascii_geo(os.path.join(outdir, 'sparse_dec.ply')).astype(np.int64)
    key = lambda v: np.sort((v[:, 2] << 40) | (v[:, 1] << 20) | v[:, 0])
    assert np.array_equal(key(decoded), key(c.astype(np.int64)))


def test_coder_cli_with_max_num(sparse_ply, capsys):
    d, path, ckpt, c = sparse_ply
    want = R.partition(c, 4000)
    outdir = str(d / 'coder')
    coder.main(['--ckptdir', ckpt, '--filedir', path, '--outdir', outdir, '--max_num', '4000', '--block_batch', '1'])
    text = capsys.readouterr().out
    assert f'Blocks:\t {len(c)} rows, 2 blocks, {want.rounds} rounds, 0 oversize' in text and 'D1 PSNR' in text
    stem = os.path.join(outdir, 'sparse')
    blocks = partition.read_blocks(stem)
    assert np.array_equal(blocks.rows, want.table[:, 1]) and all(os.path.exists(stem + f'_b{i:04d}' + s) for i in range(2) for s in STREAMS)
    assert not os.path.exists(stem + '_F.bin')                                        # the whole cloud was not coded beside its blocks
    assert str(partition.block_bits(stem)) in text                                    # the total counts _P.bin
    assert len(read_ply_ascii_geo(stem + '_dec.ply')) > 0
