"""AttributeCoder.encode_batch / decode_batch on the GPU: every file of a batch EQUAL, byte for byte, to the definition of
that frame alone (tests/raht_reference.py for version 1, tests/attr_rans_reference.py for version 2) and to the frame-by-frame encode of this
repository; every decoded colour equal to the frame-by-frame decode; both forms of the transform, both coders, at the smallest shapes at
which a batch can go wrong: frames without tokens, the same voxels in several frames, sixteen frames and the largest key, frame boundaries
around tile boundaries, a frame without escapes between two that have some, per-frame quantisers, every edge of the chunking."""
import os
import struct

import numpy as np
import pytest
import torch

import attr_rans_reference as ar
import raht_reference as R
import scratch_arena as SA
import test_attributes_device as AT
from pcgcv2_amd import attributes as at, ops
from pcgcv2_amd._lib import PcgcError
from pcgcv2_amd.data_utils import read_ply_ascii_with_colours, write_ply_ascii_geo_rgb

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
T = AT.T
TOP = AT.TOP
CODERS = [('host', 4096), ('device', 16)]                       # (attribute_coder, chunk_steps)


def _np(t):
    return t.cpu().numpy()


def _read(prefix):
    with open(prefix + at.SUFFIX, 'rb') as fh:
        return fh.read()


def _collate(frames, order=None):
    """frames: [(pts [n,3], rgb [n,3])] -> (coords int32 [N,4] device rows (b, x, y, z), rgb device, rows of every frame); order: a
    permutation of all rows (default: the frames one after the other)"""
    c = np.concatenate([np.concatenate([np.full((len(p), 1), b), p], 1) for b, (p, _) in enumerate(frames)]).astype(np.int32)
    rgb = np.concatenate([r for _, r in frames]).astype(np.uint8)
    idx = np.arange(len(c)) if order is None else order
    at_row, edges = np.argsort(idx), np.concatenate([[0], np.cumsum([len(p) for p, _ in frames])])
    rows = [at_row[edges[b]:edges[b + 1]] for b in range(len(frames))]              # where frame b's rows stand, in the frame's own order
    return torch.from_numpy(c[idx]).to(DEV), torch.from_numpy(rgb[idx]).to(DEV), rows


_DEFINITION = {}


def _definition(pts, rgb, ql, qc, coder, S):
    """(bytes, decoded colours) of one frame alone, computed once per input"""
    key = (pts.tobytes(), rgb.tobytes(), ql, qc, coder, S if coder == 'device' else None)
    if key not in _DEFINITION:
        _DEFINITION[key] = R.encode(pts, rgb, ql, qc, ops.rc_encode_ctx, ops.crc32) if coder == 'host' else \
            ar.encode_v2(pts, rgb, ql, qc, S, ops.crc32)
    return _DEFINITION[key]


def _q(q, b):
    return int(q[b]) if hasattr(q, '__len__') else int(q)


def _check(tmp_path, frames, ql=4, qc=None, coders=CODERS, forms=tuple(ops.RAHT_FORMS), order=None, tag='b'):
    """the whole contract for one batch -> {coder: [bytes per frame]}"""
    B = len(frames)
    qc = ql if qc is None else qc
    coords, rgb, rows = _collate(frames, order)
    postfixes = [f'_{b}' for b in range(B)]
    out = {}
    for coder_name, S in coders:
        want, want_rgb = [], []
        for b, (pts, col) in enumerate(frames):
            blob, rec = _definition(np.asarray(pts, np.int64), col, _q(ql, b), _q(qc, b), coder_name, S)
            single = at.AttributeCoder(str(tmp_path / f'{tag}_single_{coder_name}'), attribute_coder=coder_name, chunk_steps=S)
            single.encode(AT._coords(pts), torch.from_numpy(col).to(DEV), _q(ql, b), _q(qc, b), postfix=postfixes[b])
            assert _read(str(tmp_path / f'{tag}_single_{coder_name}') + postfixes[b]) == blob           # (frame by frame is the definition)
            dec = _np(single.decode(AT._coords(pts), postfix=postfixes[b]))
            assert np.array_equal(dec, rec)
            want.append(blob)
            want_rgb.append(dec)
        for form in forms:
            prefix = str(tmp_path / f'{tag}_{coder_name}_{form}')
            coder = at.AttributeCoder(prefix, form=form, attribute_coder=coder_name, chunk_steps=S)
            records = coder.encode_batch(coords, rgb, ql, None if qc is ql else qc, postfixes=postfixes)
            assert len(records) == B
            for b in range(B):
                got = _read(prefix + postfixes[b])
                assert got == want[b], (coder_name, form, b, len(got), len(want[b]))
                n_tok = 3 * (len(frames[b][0]) - 1)
                assert records[b]['bits_A'] == 8 * len(got) and records[b]['tokens'] == n_tok and 'tree' not in records[b]
                assert set(records[b]) == {'bits_A', 'tokens', 'escapes', 'payload_bytes'}
            dec = _np(coder.decode_batch(coords, postfixes=postfixes))
            assert dec.shape == (len(coords), 3) and dec.dtype == np.uint8
            for b in range(B):
                assert np.array_equal(dec[rows[b]], want_rgb[b]), (coder_name, form, b)
        out[coder_name] = want
    return out


def _frame(pts, kind='random', seed=0):
    pts = np.asarray(pts, np.int64)
    return pts, AT._colours(kind, pts, seed)


def _small(n, seed, grid=16):
    return AT._random_cloud(n, grid, seed)


# ---- the shapes of a batch ---------------------------------------------------------------------------------------------------------------------
def test_one_frame_is_encode(tmp_path):
    _check(tmp_path, [_frame(_small(40, 1), seed=1)])
    _check(tmp_path, [_frame([[7, 8, 9]])], tag='one')


def test_no_token_anywhere(tmp_path, monkeypatch):
    out = _check(tmp_path, [_frame([[7, 8, 9]]), _frame([[7, 8, 9]], seed=2)])
    for blobs in out.values():
        for blob in blobs:
            assert len(blob) == R.HEAD.size + R.SIZES.size + 4                   # DC only, an empty payload
    # neither coder entry is reached
    coords, rgb, _ = _collate([_frame([[1, 2, 3]]), _frame([[1, 2, 3]])])
    tree = ops.raht_tree_batch(coords, 2)
    H, dc = ops.raht_forward_batch(tree, rgb)
    tokens, ctx, esc, hist = ops.raht_quantize_batch(tree, H, [1, 1], [1, 1])
    assert tokens.numel() == 0 and not _np(hist).any()
    monkeypatch.setattr(ops, 'lib', lambda: (_ for _ in ()).throw(AssertionError('a launch without tokens')))
    assert ops.attr_rans_encode_batch(np.zeros((2, 48, 65), np.uint16), ctx, tokens, tree.tok, 16) == [b'', b'']
    got, n_escape = ops.attr_rans_decode_batch(np.zeros((2, 48, 65), np.uint16), tree, [b'', b''])
    assert got.numel() == 0 and not n_escape.any()


def test_a_frame_without_tokens_between_two_others(tmp_path):
    _check(tmp_path, [_frame([[7, 8, 9], [1, 2, 3]], seed=1), _frame([[5, 5, 5]], seed=2), _frame([[7, 8, 9], [1, 2, 3], [1, 2, 2]], seed=3)])


def test_the_same_voxels_in_every_frame_are_no_duplicates(tmp_path):
    pts = np.array([[7, 8, 9], [1, 2, 3], [1, 2, 2]])
    frames = [_frame(pts, seed=1), _frame(pts[:2], seed=2), _frame(pts[:1], seed=3)]
    _check(tmp_path, frames)
    coords, rgb, _ = _collate(frames)
    dup = torch.cat([coords, coords[3:4]])                                        # frame 1's first voxel once more, inside frame 1 only
    assert int(dup[-1, 0]) == 1
    for coder_name, S in CODERS:
        coder = at.AttributeCoder(str(tmp_path / 'dup'), attribute_coder=coder_name, chunk_steps=S)
        with pytest.raises(ValueError, match='frame 1 .*duplicate'):
            coder.encode_batch(dup, torch.cat([rgb, rgb[3:4]]), 4, postfixes=['a', 'b', 'c'])
        with pytest.raises(ValueError, match='frame 1 .*duplicate'):
            coder.decode_batch(dup, postfixes=['a', 'b', 'c'])
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith('dup')]


def test_refusals_that_need_the_device(tmp_path):
    frames = [_frame(_small(20, 1), seed=1), _frame(_small(30, 2), seed=2)]
    coords, rgb, _ = _collate(frames)
    coder = at.AttributeCoder(str(tmp_path / 'r'))
    with pytest.raises(ValueError, match='frame 2 has no rows'):                   # a frame index without rows
        coder.encode_batch(coords, rgb, 4, postfixes=['a', 'b', 'c'])
    with pytest.raises(ValueError, match='frame index outside'):                   # one outside 0 .. B - 1
        coder.encode_batch(coords, rgb, 4, postfixes=['a'])
    gap = coords.clone()
    gap[gap[:, 0] == 1, 0] = 2
    with pytest.raises(ValueError, match='frame 1 has no rows'):
        coder.decode_batch(gap, postfixes=['a', 'b', 'c'])
    negative = coords.clone()
    negative[0, 0] = -1
    with pytest.raises(ValueError, match='frame index outside'):
        coder.encode_batch(negative, rgb, 4, postfixes=['a', 'b'])
    for bad in (-1, 1 << 20):
        far = coords.clone()
        far[25, 2] = bad
        with pytest.raises(ValueError, match='outside \\[0, 2\\^20\\)'):
            coder.encode_batch(far, rgb, 4, postfixes=['a', 'b'])
    with pytest.raises(ValueError):
        coder.encode_batch(coords, rgb[:-1], 4, postfixes=['a', 'b'])
    with pytest.raises(PcgcError, match='device tensor'):
        coder.encode_batch(coords.cpu(), rgb, 4, postfixes=['a', 'b'])
    assert not os.listdir(str(tmp_path))
    coder.encode_batch(coords, rgb, 4, postfixes=['a', 'b'])
    with pytest.raises(PcgcError, match='rb' + at.SUFFIX + '.*points'):           # another geometry: the item is named
        coder.decode_batch(coords[:-1], postfixes=['a', 'b'])


def test_sixteen_frames_and_the_largest_key(tmp_path):
    frames = [_frame(_small(1 + b % 3, 30 + b, grid=1 << 20), seed=b) for b in range(15)]
    frames.append(_frame([[TOP, TOP, TOP], [0, 0, 0], [TOP, TOP, TOP - 1]], seed=15))
    _check(tmp_path, frames)
    coords, _, _ = _collate(frames)
    tree = ops.raht_tree_batch(coords, 16)
    keys = _np(tree.keys).view(np.uint64)
    assert keys[-1] == np.uint64(0xFFFFFFFFFFFFFFFF) and (np.diff(keys.astype(object)) > 0).all()       # unsigned order, bit 63 set from frame 8
    assert (keys >> np.uint64(60)).tolist() == sorted(_np(coords[:, 0]).tolist())


@pytest.mark.parametrize('sizes', [(T - 1, 2), (T, T), (T + 1, T - 1), (3, 2 * T + 1, 5)], ids=str)
@pytest.mark.parametrize('kind', ['equal', 'alternating', 'random'])
def test_frame_boundaries_around_tile_boundaries(tmp_path, sizes, kind):
    frames = [_frame(AT._line(n, x0=b), kind, seed=b) for b, n in enumerate(sizes)]
    _check(tmp_path, frames, ql=0 if kind == 'alternating' else 4, qc=0 if kind == 'alternating' else 9)
    coords, _, _ = _collate(frames)
    tree = ops.raht_tree_batch(coords, len(sizes))
    assert tree.starts.tolist() == np.concatenate([[0], np.cumsum(sizes)]).tolist()
    lo, hi, d = _np(tree.lo), _np(tree.hi), _np(tree.d)
    edge = tree.starts[1:-1] - 1                                                  # the gaps that are frame boundaries
    assert (d[edge] >= 60).all() and (lo[edge] == -1).all() and (hi[edge] == -1).all() and (np.delete(d, edge) < 60).all()
    assert np.array_equal(np.sort(_np(tree.order)[len(d) - len(edge):]), edge)   # behind the coding order


def test_subtrees_that_straddle_every_tile_boundary_in_the_middle_frame(tmp_path):
    frames = [_frame(AT._line(5), seed=1), _frame(AT._two_lines(2 * T + 1), seed=2), _frame(AT._line(T + 3, 3), seed=3)]
    _check(tmp_path, frames, ql=2, qc=5)
    coords, _, _ = _collate(frames)
    tree = ops.raht_tree_batch(coords, 3)
    lo, hi = _np(tree.lo).astype(np.int64), _np(tree.hi).astype(np.int64)
    crossing = (lo >= 0) & (lo // T != hi // T)
    assert tree.cross[-1] == crossing.sum() > 2                                   # one workgroup gets the crossing gaps of all frames
    assert set(_np(tree.cross_order)[:crossing.sum()].tolist()) == set(np.flatnonzero(crossing).tolist())
    inside = crossing & (np.arange(len(lo)) % T != T - 1)
    assert inside.any()


def test_every_frame_has_its_own_escapes(tmp_path):
    """quantiser 0 on alternating 0 / 255 escapes; the frame in the middle has none"""
    frames = [_frame(_small(60, 1), 'alternating'), _frame(_small(50, 2), 'equal'), _frame(_small(70, 3), 'alternating')]
    _check(tmp_path, frames, ql=0, qc=0)
    coords, rgb, _ = _collate(frames)
    records = at.AttributeCoder(str(tmp_path / 'e')).encode_batch(coords, rgb, 0, postfixes=['0', '1', '2'])
    assert records[0]['escapes'] > 0 and records[1]['escapes'] == 0 and records[2]['escapes'] > 0


def test_quantisers_per_frame(tmp_path):
    frames = [_frame(_small(300, 4, 32), seed=4), _frame(_small(200, 5, 32), seed=5), _frame(_small(257, 6, 32), seed=6)]
    out = _check(tmp_path, frames, ql=(0, 16, 255), qc=(4, 0, 3))
    for blobs in out.values():
        assert [struct.unpack_from('<HH', blob, 12) for blob in blobs] == [(0, 4), (16, 0), (255, 3)]


@pytest.mark.parametrize('chunk_steps', [1, 3, 0])
def test_chunks_never_straddle_frames(tmp_path, chunk_steps):
    sizes = (22, 23, 65, 66)                                                      # 63, 66, 192 and 195 tokens
    frames = [_frame(_small(n, 40 + n, 32), seed=n) for n in sizes]
    out = _check(tmp_path, frames, ql=1, qc=2, coders=[('device', chunk_steps)])
    for blob, n in zip(out['device'], sizes):
        n_tok = 3 * (n - 1)
        rows = struct.unpack_from('<H', blob, 22)[0]
        S, K = struct.unpack_from('<II', blob, R.HEAD.size + 128 * rows + 24)
        assert (S, K) == ((chunk_steps, ar.chunks_of(n_tok, chunk_steps)) if chunk_steps else (-(-n_tok // 64), 1))


def test_rows_in_any_order_and_repeatability(tmp_path):
    frames = [_frame(_small(90, 7, 32), seed=7), _frame(_small(120, 8, 32), seed=8), _frame(_small(60, 9, 32), seed=9)]
    first = _check(tmp_path, frames, ql=3, qc=6, tag='o0')
    n = sum(len(p) for p, _ in frames)
    for seed in (1, 2):                                                           # rows of all frames shuffled together
        again = _check(tmp_path, frames, ql=3, qc=6, order=np.random.default_rng(seed).permutation(n), tag=f'o{seed}')
        assert again == first
    assert _check(tmp_path, frames, ql=3, qc=6, tag='o3') == first                # two runs, the same bytes


# ---- a single frame is the batch of one --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 2, 3, T - 1, T, T + 1, 2 * T + 1])
def test_single_entries_are_the_batch_of_one(n):
    """every array the single entries give against the batch entries' at B = 1, below the level of a whole file"""
    pts = AT._random_cloud(n, 64, n)
    coords, rgb = AT._coords(pts), torch.from_numpy(AT._colours('random', pts, n)).to(DEV)      # (random colours: Q = 0 escapes)
    one, bat = ops.raht_tree(coords), ops.raht_tree_batch(coords, 1)
    assert one.n == bat.n == n and bat.frames == 1 and bat.starts.tolist() == [0, n]
    for field in ('keys', 'perm', 'd', 'lo', 'hi', 'left', 'right', 'order', 'cross_order'):
        assert np.array_equal(_np(getattr(one, field)), _np(getattr(bat, field))), field
    assert one.offsets.numel() == 130 and np.array_equal(_np(one.offsets), _np(bat.offsets))
    assert np.array_equal(one.bucket, bat.bucket[0]) and np.array_equal(one.cross, bat.cross)
    n_tok = 3 * (n - 1)
    for ql, qc in ((0, 0), (4, 9)):
        for form in ops.RAHT_FORMS:
            H, dc = ops.raht_forward(one, rgb, form=form)
            H_b, dc_b = ops.raht_forward_batch(bat, rgb, form=form)
            assert np.array_equal(_np(H), _np(H_b)) and np.array_equal(_np(dc), _np(dc_b)[0]), (form, 'forward')
        tok, ctx, esc, hist = ops.raht_quantize(one, H, ql, qc)
        tok_b, ctx_b, esc_b, hist_b = ops.raht_quantize_batch(bat, H_b, [ql], [qc])
        E = int(_np(hist)[:, ops.RAHT_ESCAPE].sum())
        assert esc.numel() == E and (E > 0 or ql > 0 or n < T)                       # (quantiser 0 on random colours escapes)
        assert np.array_equal(_np(tok), _np(tok_b)) and np.array_equal(_np(ctx), _np(ctx_b)) and tok.numel() == n_tok
        assert np.array_equal(_np(esc), _np(esc_b)[:E]) and np.array_equal(_np(hist), _np(hist_b)[0]) and tuple(hist_b.shape) == (1, 48, 64)
        Hh = ops.raht_dequantize(one, tok, esc, ql, qc)
        Hh_b = ops.raht_dequantize_batch(bat, tok_b, esc_b[:E], [E], [ql], [qc])
        assert np.array_equal(_np(Hh), _np(Hh_b))
        for form in ops.RAHT_FORMS:
            got = ops.raht_inverse(one, Hh, dc.tolist(), form=form)
            got_b = ops.raht_inverse_batch(bat, Hh_b, _np(dc_b), form=form)
            assert np.array_equal(_np(got), _np(got_b)), (form, 'inverse')
        if ql == 0:
            assert np.array_equal(_np(got), _np(rgb))
        _, table = at.frequency_rows(_np(hist))
        for chunk_steps in (1, 3, 0):
            payload = ops.attr_rans_encode(table, ctx, tok, chunk_steps or max(1, ops.attr_rans_chunks(n_tok, 1)))
            assert ops.attr_rans_encode_batch(table[None], ctx_b, tok_b, bat.tok, chunk_steps) == [payload], chunk_steps
            dec, n_escape = ops.attr_rans_decode(table, one, payload, n_tok)
            dec_b, n_escape_b = ops.attr_rans_decode_batch(table[None], bat, [payload])
            assert np.array_equal(_np(dec), _np(dec_b)) and np.array_equal(_np(dec), _np(tok)) and [n_escape] == n_escape_b.tolist() == [E]


@pytest.mark.parametrize('rows, first', [(3, 0), (3, 3), (257, 0), (257, 3)])
def test_a_batch_index_in_a_single_frame_touches_nothing_else(rows, first):
    """rows whose batch column is 1, 5, 15 or -1 are refused by the single entry, and neither its two-int status nor any other guarded
    allocation is written outside its bounds: such a row must not enter the key's frame bits, which index the duplicate counters"""
    coords = AT._coords(AT._random_cloud(rows, 32, rows))
    coords[:, 0] = torch.from_numpy(np.roll(np.resize(np.array([1, 5, 15, -1], np.int32), rows + 4), -first)[:rows]).to(DEV)
    assert set(_np(coords[:, 0]).tolist()) >= ({1, 5, 15} if first == 0 and rows == 3 else {-1, 1, 5})
    arena = SA.Arena()
    with SA.installed(arena):
        with pytest.raises(ValueError, match='one frame'):
            ops.raht_tree(coords)
    torch.cuda.synchronize()
    assert len(arena.blocks) > 0
    arena.finish()
    arena.check()


# ---- files cross over ------------------------------------------------------------------------------------------------------------------------
def test_files_of_encode_and_encode_batch_are_read_by_either(tmp_path):
    frames = [_frame(_small(80, 11, 32), seed=11), _frame(_small(100, 12, 32), seed=12), _frame(_small(1, 13, 32), seed=13),
              _frame(_small(70, 14, 32), 'alternating')]
    coords, rgb, rows = _collate(frames, np.random.default_rng(3).permutation(251))
    postfixes = ['_a', '_b', '_c', '_d']
    prefix = str(tmp_path / 'x')
    want = []
    for b, (pts, col) in enumerate(frames):                                       # written by encode, a mix of version 1 and version 2
        single = at.AttributeCoder(prefix, attribute_coder='device' if b % 2 else 'host', chunk_steps=1)
        single.encode(AT._coords(pts), torch.from_numpy(col).to(DEV), 1, 3, postfix=postfixes[b])
        want.append(_np(single.decode(AT._coords(pts), postfix=postfixes[b])))
    assert [struct.unpack_from('<I', _read(prefix + p), 4)[0] for p in postfixes] == [1, 2, 1, 2]
    for form in ops.RAHT_FORMS:
        dec = _np(at.AttributeCoder(prefix, form=form).decode_batch(coords, postfixes=postfixes))
        for b in range(4):
            assert np.array_equal(dec[rows[b]], want[b]), (form, b)
    for coder_name, S in CODERS:                                                  # written by encode_batch, read by decode
        batch = at.AttributeCoder(str(tmp_path / coder_name), attribute_coder=coder_name, chunk_steps=S)
        batch.encode_batch(coords, rgb, 1, 3, postfixes=postfixes)
        for b, (pts, col) in enumerate(frames):
            got = _np(at.AttributeCoder(str(tmp_path / coder_name)).decode(AT._coords(pts), postfix=postfixes[b]))
            assert np.array_equal(got, want[b]), (coder_name, b)


# ---- damage ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('coder_name, S', CODERS)
def test_a_damaged_item_is_named(tmp_path, coder_name, S):
    frames = [_frame(_small(150, 21, 32), 'alternating'), _frame(_small(200, 22, 32), 'alternating'), _frame(_small(100, 23, 32), 'alternating')]
    coords, rgb, rows = _collate(frames)
    postfixes = ['_0', '_1', '_2']
    prefix = str(tmp_path / 'd')
    coder = at.AttributeCoder(prefix, attribute_coder=coder_name, chunk_steps=S)
    record = coder.encode_batch(coords, rgb, 0, postfixes=postfixes)[1]
    tree = ops.raht_tree_batch(coords, 3)
    want = _np(coder.decode_batch(coords, postfixes=postfixes, tree=tree))
    good = _read(prefix + '_1')
    table_rows = struct.unpack_from('<H', good, 22)[0]
    sizes_at = R.HEAD.size + 128 * table_rows
    n_tok, n_pay, n_esc = R.SIZES.unpack_from(good, sizes_at)
    assert n_pay == record['payload_bytes'] > 64 and n_esc > 0

    def refused(blob, match):
        with open(prefix + '_1' + at.SUFFIX, 'wb') as fh:
            fh.write(blob)
        with pytest.raises(PcgcError, match=match) as e:
            coder.decode_batch(coords, postfixes=postfixes, tree=tree)
        assert (prefix + '_1' + at.SUFFIX) in str(e.value)                         # the item is named

    for i in (9, R.HEAD.size + 5, sizes_at + 24 + n_pay // 2, len(good) - 2):      # header, table, payload, CRC
        refused(good[:i] + bytes([good[i] ^ 0x10]) + good[i + 1:], 'CRC')
    refused(good[:len(good) // 2], None)                                           # cut
    refused(_read(prefix + '_0'), None)                                            # a sound file of another frame
    if coder_name == 'device':                                                     # behind a CRC made to fit: the chunk check on the device
        word = sizes_at + 24 + n_pay - 6
        bad = good[:word] + bytes([good[word] ^ 0x40]) + good[word + 1:]
        refused(bad[:-4] + struct.pack('<I', ops.crc32(bad[:-4])), 'unsound|escape')
    with open(prefix + '_1' + at.SUFFIX, 'wb') as fh:
        fh.write(good)
    assert np.array_equal(_np(coder.decode_batch(coords, postfixes=postfixes, tree=tree)), want)
    assert np.array_equal(want, _np(rgb))                                          # quantiser 0


def test_an_undersized_workspace_is_refused_before_any_launch():
    L, n, B = ops.lib(), 100, 3
    one = torch.zeros(8, dtype=torch.int64, device=DEV)
    p = one.data_ptr()
    q = np.zeros(B, np.int32)
    assert L.pcgc_raht_keys_batch(p, n, B, p, p, p, p, int(L.pcgc_raht_keys_batch_workspace_bytes(n)) - 1, None) == -2
    assert L.pcgc_raht_tree_batch(p, n, B, p, p, p, p, p, p, p, p, p, int(L.pcgc_raht_tree_batch_workspace_bytes(n)) - 1, None) == -2
    assert L.pcgc_raht_quantize_batch(p, n, B, p, p, p, p, p, q.ctypes.data, q.ctypes.data, p, p, p, p, p, p,
                                      int(L.pcgc_raht_quantize_batch_workspace_bytes(n, B)) - 1, None) == -2
    assert L.pcgc_raht_dequantize_batch(p, p, 0, n, B, p, p, p, p, q.ctypes.data, q.ctypes.data, p, p, p,
                                        int(L.pcgc_raht_dequantize_batch_workspace_bytes(n, B)) - 1, None) == -2
    lay = ops.attr_rans_batch_layout([96, 99, 96], 1)
    tok, steps, pay = lay['tok'], lay['steps'], lay['pay']
    size = (lay['room']).astype(np.int64)
    host = np.zeros(2 * B, np.int64)
    short = int(L.pcgc_attr_rans_batch_workspace_bytes(int(tok[-1]), int(lay['first_chunk'][-1]))) - 1
    assert L.pcgc_attr_rans_encode_batch(p, p, p, B, tok.ctypes.data, steps.ctypes.data, p, pay.ctypes.data, host.ctypes.data, p, short, None) == -2
    assert L.pcgc_attr_rans_decode_batch(p, p, B, tok.ctypes.data, steps.ctypes.data, p, pay.ctypes.data, size.ctypes.data, p, host.ctypes.data,
                                         p, short, None) == -2
    torch.cuda.synchronize()
    assert not _np(one).any()                                                      # nothing was written


# ---- scratch state ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('coder_name, S', CODERS)
def test_encode_batch_and_decode_batch_on_recycled_scratch(tmp_path, coder_name, S):
    """fresh memory, then the memory a sibling batch left behind (the same shapes, other colours, another split of the rows among the
    frames): guards intact, bytes and colours unchanged"""
    pts = _small(300, 50, 32)

    def make(seed, split):
        rng = np.random.default_rng(seed)
        edges = np.concatenate([[0], np.cumsum(split)])
        frames = [(pts[edges[b]:edges[b + 1]] + 64 * rng.integers(1, 40, 3), AT._colours('random', pts[edges[b]:edges[b + 1]], seed + b))
                  for b in range(len(split))]
        coords, rgb, _ = _collate(frames, rng.permutation(len(pts)))
        return coords, rgb

    def fn(inp):
        coords, rgb = inp
        coder = at.AttributeCoder(str(tmp_path / 'arena'), attribute_coder=coder_name, chunk_steps=S)
        coder.encode_batch(coords, rgb, (4, 2, 0), (9, 1, 3), postfixes=['_0', '_1', '_2'])
        blobs = b''.join(_read(str(tmp_path / 'arena') + p) for p in ('_0', '_1', '_2'))
        return np.frombuffer(blobs, np.uint8).copy(), _np(coder.decode_batch(coords, postfixes=['_0', '_1', '_2']))

    def run(arena, inp):
        with SA.installed(arena):
            out = fn(inp)
        torch.cuda.synchronize()
        arena.finish()
        arena.check()
        return out

    A, B = make(80, (90, 130, 80)), make(81, (130, 80, 90))
    fn(A)
    fresh, rec = SA.Arena(), SA.Arena()
    want = run(fresh, B)
    run(rec, A)
    stale = rec.replay()
    got = run(stale, B)
    for a in (fresh, rec, stale):
        a.check()
    allocs, replayed, _ = stale.stats()
    assert allocs > 0 and replayed == allocs and not stale.served_fresh
    assert got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1])


# ---- command line ----------------------------------------------------------------------------------------------------------------------------
def test_attributes_cli_on_several_files(tmp_path, capsys):
    files, clouds = [], []
    for b, n in enumerate((120, 80, 150)):
        pts, rgb = _frame(_small(n, 60 + b, 32), seed=b)
        files.append(str(tmp_path / f'cloud{b}.ply'))
        write_ply_ascii_geo_rgb(files[-1], pts, rgb)
        clouds.append((pts, rgb))
    for coder_name in ('host', 'device'):
        out_dir = str(tmp_path / coder_name)
        at.main(['--filedir', *files, '--qstep', '0', '--outdir', out_dir, '--attribute_coder', coder_name, '--chunk_steps', '2'])
        out = capsys.readouterr().out
        lines = [l for l in out.splitlines() if l.startswith(at.SUFFIX)]
        assert len(lines) == 3 and len(AT._printed(out, 'Colour PSNR (Y)')) == 3
        for b, (pts, rgb) in enumerate(clouds):
            blob = _read(os.path.join(out_dir, f'cloud{b}'))
            assert int(lines[b].split('\t')[1].split()[0]) == 8 * len(blob) == 8 * os.path.getsize(os.path.join(out_dir, f'cloud{b}') + at.SUFFIX)
            assert struct.unpack_from('<I', blob, 4)[0] == at.CODERS[coder_name]
            xyz, got = read_ply_ascii_with_colours(os.path.join(out_dir, f'cloud{b}_dec.ply'))
            assert np.array_equal(xyz.astype(np.int64), pts) and np.array_equal(got, rgb)      # quantiser 0
        assert AT._printed(out, 'Colour PSNR (Y)') == ['inf'] * 3
