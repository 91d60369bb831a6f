"""GPU tests of the batched lossless mode.  The definition of a batch is the definition applied to each frame alone:
pcgc_occ_symbols_segments against lossless_reference.occ_symbols of every frame, pcgc_occ_rans_encode_batch / _decode_batch against
rans_reference.encode of every frame (byte equality), and LosslessCoder.encode_batch / decode_batch / estimate_batch against encode / decode /
estimate of every item alone (byte equality of all files, key-by-key equality of the records, set equality of the decoded voxels).
Synthetic weights throughout: the rate they give says nothing about trained models."""
import os
import re
import shutil
import struct

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import lossless_reference as lr
import rans_reference as rr
import scratch_arena as SA
from pcgcv2_amd import lossless, ops, synthetic
from pcgcv2_amd.coder import STREAMS, INDEX_SUFFIX
from pcgcv2_amd.pcc_model import PCCModel
from pcgcv2_amd.sparse import SparseTensor, sparse_collate
from scratch_arena import Arena

DEV = torch.device('cuda:0')
HEAD = struct.Struct('<4sII6Q')
FILES = STREAMS + (INDEX_SUFFIX, lossless.SUFFIX)


@pytest.fixture(autouse=True)
def _restore_path_config():
    """(as tests/test_gpu_parity.py: a test that replaces the dispatch record gets the previous one back)"""
    keep = ops.PATH
    yield
    ops.configure(keep)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- pcgc_occ_symbols_segments ----------------------------------------------------------------------------------------------------------------
SYMBOL_SPLITS = [(1,), (8, 8, 8), (1023, 1, 1025), (1024, 1024), (8,) * 16, (0, 5, 0, 2051, 0)]


def _layouts(z):
    """(name, device view) of the same logits: dense and aligned (the vector path), rows of a wider buffer ([n, 1], ld = 3) and a dense view
    at an odd element offset (the scalar path)"""
    n = len(z)
    t = _t(z)
    off = torch.zeros(n + 1, dtype=torch.float32, device=DEV)
    off[1:] = t
    wide = torch.full((n, 3), 7.0, dtype=torch.float32, device=DEV)
    wide[:, 1] = t
    return (('dense', t), ('dense [n, 1]', t.view(n, 1)), ('ld = 3', wide[:, 1:2]), ('offset by one element', off[1:]))


@pytest.mark.parametrize('split', SYMBOL_SPLITS, ids=[f'{len(s)}x{max(s)}' for s in SYMBOL_SPLITS])
def test_occ_symbols_segments_equal_the_definition_of_every_frame(split):
    n = sum(split)
    z, truth = lr.random_logits(n, seed=n + len(split))
    want_words, _, _ = lr.occ_symbols(z, truth)
    edge = np.concatenate([[0], np.cumsum(split)])
    want_sums = [lr.occ_symbols(z[edge[f]:edge[f + 1]], truth[edge[f]:edge[f + 1]])[1:] for f in range(len(split))]
    truth_d = _t(truth)
    for name, view in _layouts(z):
        packed, sums = ops.occ_symbols_segments(view, split, truth_d)
        assert sums.shape == (len(split), 2) and sums.dtype == torch.int64
        words, occupied, cost = ops.occ_words_host_segments(packed, sums)
        assert np.array_equal(words, want_words), name
        assert [(int(o), int(c)) for o, c in zip(occupied, cost)] == want_sums, name
        single, _ = ops.occ_symbols(view, truth_d)
        assert torch.equal(packed, single), name
        packed, sums = ops.occ_symbols_segments(view, split)                        # truth = NULL: contexts only
        assert sums is None and np.array_equal(packed.cpu().numpy().view(np.uint16), lr.occ_symbols(z)[0]), name


def test_occ_symbols_segments_special_logits_in_small_frames():
    z, q = lr.special_logits()
    split = [8] * (len(z) // 8) + [len(z) % 8]
    split = [sum(split[:-15])] + split[-15:]                                        # sixteen frames, the last fifteen of 8 rows or fewer
    truth = (np.arange(len(z)) % 3 == 0).astype(np.uint8) * 5                       # any non-zero byte is "occupied"
    packed, sums = ops.occ_symbols_segments(_t(z), split, _t(truth))
    words, occupied, cost = ops.occ_words_host_segments(packed, sums)
    assert np.array_equal(words >> 1, q + lr.QMAX) and np.array_equal(words & 1, truth != 0)
    edge = np.concatenate([[0], np.cumsum(split)])
    for f in range(16):
        assert (int(occupied[f]), int(cost[f])) == lr.occ_symbols(z[edge[f]:edge[f + 1]], truth[edge[f]:edge[f + 1]])[1:]
    with pytest.raises(ops.PcgcError):
        ops.occ_symbols_segments(torch.zeros(5, device=DEV), [2, 2])


# ---- pcgc_occ_rans_encode_batch / _decode_batch -------------------------------------------------------------------------------------------------
def _packed(ctx, bit=None):
    """what occ_symbols hands on: int16 [n] on the device, ctx << 1 | bit (bit 0 on the decoder's side)"""
    w = np.asarray(ctx, dtype=np.int64) << 1
    if bit is not None:
        w = w | np.asarray(bit, dtype=np.int64)
    return torch.from_numpy(w.astype(np.int16)).to(DEV) if len(w) else torch.empty(0, dtype=torch.int16, device=DEV)


def _steps_of(n, chunk_steps):
    return chunk_steps or max(1, rr.chunks_of(n, 1))


def _frames_equal_the_definition(frames, chunk_steps, what=''):
    """frames: [(ctx, bit)] -> the definition's payloads, after every equality in both directions"""
    split = [len(c) for c, _ in frames]
    ctx, bit = np.concatenate([c for c, _ in frames]), np.concatenate([b for _, b in frames])
    want = [rr.encode(c, b, _steps_of(len(c), chunk_steps)) for c, b in frames]
    got = ops.occ_rans_encode_batch(_packed(ctx, bit), split, chunk_steps)
    for f in range(len(frames)):
        assert got[f] == want[f], f'{what}: split {split}, S = {chunk_steps}: frame {f}: {len(got[f])} bytes, the definition has {len(want[f])}'
    mask, occupied = ops.occ_rans_decode_batch(_packed(ctx), split, want)            # the kernel decodes the definition's payloads
    assert mask.dtype == torch.uint8 and mask.device.type == 'cuda'
    assert np.array_equal(mask.cpu().numpy(), bit), f'{what}: split {split}, S = {chunk_steps}'
    assert occupied.tolist() == [int(b.sum()) for _, b in frames]
    return want


def _model_drawn(split, seed):
    return [rr.model_drawn(n, seed=seed + 31 * f + n) for f, n in enumerate(split)]


@pytest.mark.parametrize('S', [1, 3, 0])
def test_rans_batch_bytes_and_bits_equal_the_definition(S):
    s = S or 2
    for split in ((1,), (63, 65), (64, 0, 64), (64 * s, 64 * s + 1, 1), (3, 2 * 64 * s + 1, 5), tuple((37 * i) % 130 + 1 for i in range(16))):
        _frames_equal_the_definition(_model_drawn(split, seed=S), S, 'model-drawn')
        _frames_equal_the_definition([rr.cyclic(n, seed=n + S) for n in split], S, 'cyclic')


@pytest.mark.parametrize('S', [1, 3, 0])
def test_rans_batch_extreme_contexts_in_the_middle_frame(S):
    mid = 3 * 64 * (S or 2) + 17
    for what, middle in (('improbable bit at every row', rr.extreme(mid, True)), ('only lane 63 improbable', rr.extreme(mid, False, lanes=(63,))),
                         ('probable bit at every row', rr.extreme(mid, False))):
        _frames_equal_the_definition([rr.extreme(65, False), middle, rr.extreme(63, False)], S, what)


def test_rans_batch_one_long_chunk_between_two_small_frames_refills_the_word_ring():
    """cyclic contexts with random bits cost about 4.5 bits a row: 9 000 rows in ONE chunk (chunk_steps = 0) are 1 125 words"""
    frames = [rr.cyclic(65, seed=1), rr.cyclic(9000, seed=2), rr.cyclic(7, seed=3)]
    want = _frames_equal_the_definition(frames, 0, 'one chunk')
    assert np.frombuffer(want[1], '<u4', 1, 8 + 512)[0] > 1024 and struct.unpack_from('<II', want[1]) == (141, 1)


@pytest.mark.parametrize('S', [1, 3])
def test_rans_batch_of_one_equals_the_single_entries(S):
    for n in (1, 63, 64, 65, 64 * S + 1):
        ctx, bit = rr.model_drawn(n, seed=n + S)
        single = ops.occ_rans_encode(_packed(ctx, bit), S)
        assert ops.occ_rans_encode_batch(_packed(ctx, bit), [n], S) == [single]
        mask, occupied = ops.occ_rans_decode_batch(_packed(ctx), [n], [single])
        want_mask, want_occupied = ops.occ_rans_decode(_packed(ctx), single, n)
        assert torch.equal(mask, want_mask) and occupied.tolist() == [want_occupied]


def test_rans_batch_carries_the_sums_of_occ_symbols_segments():
    split = (1023, 1, 1025)
    z, truth = lr.random_logits(sum(split), seed=4)
    packed, sums = ops.occ_symbols_segments(_t(z), split, _t(truth))
    edge = np.concatenate([[0], np.cumsum(split)])
    for fetch in (True, False):
        coded, occupied, cost = ops.occ_rans_encode_batch(packed, split, 3, sums, fetch=fetch)
        payloads = coded if fetch else ops.occ_rans_payloads([coded])[0]
        for f in range(3):
            words, want_occupied, want_cost = lr.occ_symbols(z[edge[f]:edge[f + 1]], truth[edge[f]:edge[f + 1]])
            assert payloads[f] == rr.encode(words >> 1, words & 1, 3)
            assert (int(occupied[f]), int(cost[f])) == (want_occupied, want_cost)


def _refusal_frames():
    ctx, bit, S = rr.three_chunks()
    return [rr.cyclic(65, seed=8), (ctx, bit), rr.cyclic(130, seed=9)], S


def test_rans_batch_refuses_an_unsound_frame_by_name_and_decodes_the_sound_one_afterwards():
    frames, S = _refusal_frames()
    split = [len(c) for c, _ in frames]
    good = [rr.encode(c, b, S) for c, b in frames]
    contexts, bits = _packed(np.concatenate([c for c, _ in frames])), np.concatenate([b for _, b in frames])
    mask = torch.empty(sum(split), dtype=torch.uint8, device=DEV)
    for what, payload in rr.damaged(good[1]).items():
        with pytest.raises(ops.PcgcError, match='frame 1'):
            ops.occ_rans_decode_batch(contexts, split, [good[0], payload, good[2]], mask=mask)
            pytest.fail(f'{what}: decoded')
        with pytest.raises(ops.PcgcError, match='the middle one'):
            ops.occ_rans_decode_batch(contexts, split, [good[0], payload, good[2]], mask=mask, names=['a', 'the middle one', 'c'])
    for what, payload in {'wrong K': struct.pack('<II', S, 4) + good[1][8:], 'S = 0': struct.pack('<II', 0, 3) + good[1][8:], 'another frame\'s': good[0]}.items():
        with pytest.raises(ops.PcgcError, match='frame 1'):
            ops.occ_rans_decode_batch(contexts, split, [good[0], payload, good[2]], mask=mask)
            pytest.fail(f'{what}: decoded')
    got, occupied = ops.occ_rans_decode_batch(contexts, split, good, mask=mask)     # the same buffers, the sound payloads
    assert got is mask and np.array_equal(mask.cpu().numpy(), bits) and occupied.tolist() == [int(b.sum()) for _, b in frames]


def test_rans_batch_leaves_the_mask_of_a_frame_that_is_not_decoded_here_alone():
    frames, S = _refusal_frames()
    split = [len(c) for c, _ in frames]
    good = [rr.encode(c, b, S) for c, b in frames]
    contexts = _packed(np.concatenate([c for c, _ in frames]))
    edge = np.concatenate([[0], np.cumsum(split)])
    for absent in ((1,), (0, 2), (0, 1, 2)):
        mask = torch.full((sum(split),), 7, dtype=torch.uint8, device=DEV)
        _, occupied = ops.occ_rans_decode_batch(contexts, split, [None if f in absent else good[f] for f in range(3)], mask=mask)
        host = mask.cpu().numpy()
        for f, (_, bit) in enumerate(frames):
            assert np.array_equal(host[edge[f]:edge[f + 1]], np.full(split[f], 7) if f in absent else bit), (absent, f)
            assert occupied[f] == (0 if f in absent else int(bit.sum()))


def _last_error():
    return ops.lib().pcgc_last_error().decode()


def _frozen(out):
    payloads, mask, occupied = out
    return payloads, mask.cpu().numpy().copy(), occupied.tolist()


def test_rans_batch_on_recycled_scratch_and_refusals_under_guard_bands(monkeypatch):
    """two splits of the same 128 rows with the same chunks (3 at S = 1) and payload room: every request of the second run is served from the
    first run's blocks, stale; then the refusals, with every guard intact and nothing of the refused call's own allocations written"""
    S = 1
    A, B = _model_drawn((1, 127), seed=1), _model_drawn((63, 65), seed=2)

    def both(frames):
        split = [len(c) for c, _ in frames]
        ctx, bit = np.concatenate([c for c, _ in frames]), np.concatenate([b for _, b in frames])
        payloads = ops.occ_rans_encode_batch(_packed(ctx, bit), split, S)
        mask, occupied = ops.occ_rans_decode_batch(_packed(ctx), split, payloads)
        return payloads, mask, occupied

    def run(arena, frames):
        with SA.installed(arena):
            out = both(frames)
        torch.cuda.synchronize()
        frozen = _frozen(out)
        arena.finish()
        arena.check()
        return frozen

    both(A)
    torch.cuda.synchronize()
    fresh, rec = Arena(), Arena()
    want = run(fresh, B)
    run(rec, A)
    stale = rec.replay()
    got = run(stale, B)
    assert got[0] == want[0] == [rr.encode(c, b, S) for c, b in B] and np.array_equal(got[1], want[1]) and got[2] == want[2]
    allocs, replayed, _ = stale.stats()
    assert allocs >= 4 and replayed == allocs and not stale.served_fresh

    # undersized workspace (the sizing call answers one byte less; the wrapper passes on what it was told): refused before any launch
    split = [63, 65]
    ctx, bit = np.concatenate([c for c, _ in B]), np.concatenate([b for _, b in B])
    true = ops.lib().pcgc_occ_rans_batch_workspace_bytes
    monkeypatch.setattr(ops.lib(), 'pcgc_occ_rans_batch_workspace_bytes', lambda *a: int(true(*a)) - 1)
    arena = Arena()
    with SA.installed(arena):
        with pytest.raises(ops.PcgcError, match='too small'):
            ops.occ_rans_encode_batch(_packed(ctx, bit), split, S)
    arena.check()
    assert arena.blocks and all(not b.payload().any() for b in arena.blocks if b.caller in ('occ_rans_encode_batch', '_rans_batch_ws'))
    monkeypatch.undo()

    # the native entries themselves, on guard-banded buffers: a short workspace, a misaligned payload, a misaligned payload offset
    L = ops.lib()
    lay = ops.occ_rans_batch_layout(split, S)
    arena = Arena()
    with SA.installed(arena):
        out = ops.torch.empty(int(lay['pay'][-1]) + 8, dtype=torch.uint8, device=DEV)
        ws_bytes = int(true(128, 3))
        ws = ops.torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
        mask = ops.torch.empty(128, dtype=torch.uint8, device=DEV)
    packed, contexts = _packed(ctx, bit), _packed(ctx)
    host = np.zeros(6, np.int64)
    row, steps, pay = lay['row'], lay['steps'], lay['pay']
    stream = torch.cuda.current_stream(DEV).cuda_stream
    enc = lambda payload, pay_, ws_bytes_: L.pcgc_occ_rans_encode_batch(packed.data_ptr(), 2, row.ctypes.data, steps.ctypes.data, None, payload,
                                                                         pay_.ctypes.data, host.ctypes.data, ws.data_ptr(), ws_bytes_, stream)
    assert enc(out.data_ptr(), pay, ws_bytes - 1) == -2 and 'too small' in _last_error()
    assert enc(out.data_ptr() + 4, pay, ws_bytes) == -2 and 'misaligned' in _last_error()
    assert enc(out.data_ptr(), pay + np.array([0, 4, 4]), ws_bytes) == -2
    assert enc(out.data_ptr(), pay - np.array([0, 8, 8]), ws_bytes) == -2 and 'too small' in _last_error()      # frame 0's room
    up = torch.frombuffer(bytearray(want[0][0] + bytes(-len(want[0][0]) % 8) + want[0][1]), dtype=torch.uint8).to(DEV)
    size = np.array([len(p) for p in want[0]], np.int64)
    at = np.array([0, (len(want[0][0]) + 7) // 8 * 8], np.int64)
    dec = lambda payload, at_, ws_bytes_: L.pcgc_occ_rans_decode_batch(contexts.data_ptr(), 2, row.ctypes.data, steps.ctypes.data, payload, at_.ctypes.data,
                                                                       size.ctypes.data, mask.data_ptr(), host.ctypes.data, ws.data_ptr(), ws_bytes_, stream)
    assert dec(up.data_ptr(), at, 3 * 16 * 8 + 16 - 1) == -2 and 'too small' in _last_error()
    assert dec(up.data_ptr() + 4, at, ws_bytes) == -2 and 'misaligned' in _last_error()
    assert dec(up.data_ptr(), at + np.array([0, 4]), ws_bytes) == -2
    arena.check()
    assert not any(b.payload().any() for b in arena.blocks), 'a refused call wrote to its buffers'
    assert dec(up.data_ptr(), at, 3 * 16 * 8 + 16) == 0 and np.array_equal(mask.cpu().numpy(), bit)              # (the decoder accepts as little)
    arena.check()


# ---- LosslessCoder.encode_batch / decode_batch / estimate_batch -----------------------------------------------------------------------------------
CLOUDS = dict(lr.clouds())
_rng = np.random.default_rng(16)
for _i in range(16):                                       # sixteen small clouds: 1 to 40 distinct voxels somewhere in a 32^3 cube
    _pts = np.unique(_rng.integers(0, 12, size=(1 + 3 * _i % 40, 3)) + _rng.integers(0, 20, size=3), axis=0)
    CLOUDS[f'small {_i}'] = _pts[_rng.permutation(len(_pts))].astype(np.int32)
BATCHES = {
    'three': ('single voxel', 'one voxel per stride-8 cell', 'sphere shell'),
    'two solids': ('filled ball', 'two components'),
    'shell twice': ('sphere shell', 'shuffled shell'),
    'one': ('two components',),
    'sixteen': tuple(f'small {i}' for i in range(16)),
}
CODER_CASES = [(c, s) for c in ('host', 'device') for s in (1, 3, None, 0)]


@pytest.fixture(scope='module')
def model():
    m = PCCModel().to(DEV)
    m.load_state_dict(synthetic.synthetic_state_dict())
    return m


def _tensor(*clouds, **kw):
    coords, feats = sparse_collate([torch.from_numpy(np.ascontiguousarray(p, dtype=np.int32)) for p in clouds], [torch.ones((len(p), 1)) for p in clouds])
    return SparseTensor(feats, coordinates=coords, tensor_stride=1, device=DEV, **kw)


def _rows(c):
    c = np.asarray(c.cpu().numpy() if torch.is_tensor(c) else c)
    return c[np.lexsort(c.T[::-1])]


def _set_of(pts):
    return _rows(np.concatenate([np.zeros((len(pts), 1), np.int32), np.asarray(pts, np.int32)], 1))


def _files(stem):
    return {s: open(stem + s, 'rb').read() for s in FILES}


_SINGLES = {}


@pytest.fixture(scope='module')
def singles(model, tmp_path_factory):
    """(cloud, coder, chunk_steps) -> (files, record, estimate) of LosslessCoder.encode of the cloud alone: computed once, shared, never changed"""
    root = tmp_path_factory.mktemp('singles')

    def get(name, coder_name, steps):
        key = (name, coder_name, steps if coder_name == 'device' else None)
        if key not in _SINGLES:
            stem = str(root / f'{len(_SINGLES)}')
            coder = lossless.LosslessCoder(model, stem, occupancy_coder=coder_name, chunk_steps=steps)
            x = _tensor(CLOUDS[name])
            record = coder.encode(x)
            _SINGLES[key] = (_files(stem), record, coder.estimate(x), stem)
        return _SINGLES[key]
    return get


@pytest.mark.parametrize('coder_name, steps', CODER_CASES, ids=[f'{c}-S{s}' for c, s in CODER_CASES])
@pytest.mark.parametrize('batch', list(BATCHES), ids=[b.replace(' ', '_') for b in BATCHES])
def test_a_batch_writes_the_files_of_every_item_alone_and_decodes_every_item(batch, coder_name, steps, model, singles, tmp_path):
    names = BATCHES[batch]
    postfixes = [f'_{i}' for i in range(len(names))]
    coder = lossless.LosslessCoder(model, str(tmp_path / 'b'), occupancy_coder=coder_name, chunk_steps=steps)
    x = _tensor(*[CLOUDS[n] for n in names])
    records = coder.encode_batch(x, postfixes)
    assert len(records) == len(names)
    for name, postfix, record in zip(names, postfixes, records):
        want_files, want_record, _, _ = singles(name, coder_name, steps)
        got_files = _files(str(tmp_path / 'b') + postfix)
        for s in FILES:
            assert got_files[s] == want_files[s], f'{name}: {s} of the batch differs from the file of the item coded alone'
        assert set(record) == set(want_record)
        for key in want_record:
            assert record[key] == want_record[key], f'{name}: record[{key!r}]'
    if batch == 'shell twice':
        assert _files(str(tmp_path / 'b') + '_0')[lossless.SUFFIX] == _files(str(tmp_path / 'b') + '_1')[lossless.SUFFIX]
    outs = coder.decode_batch(postfixes)
    assert len(outs) == len(names)
    for name, out in zip(names, outs):
        assert out.cmap.stride == 1 and np.array_equal(_rows(out.C), _set_of(CLOUDS[name])), f'{name}: the decoded voxel set is not the input set'
    assert coder.estimate_batch(x) == [singles(name, coder_name, steps)[2] for name in names]


def test_files_cross_between_the_single_and_the_batch_calls_with_versions_mixed(model, singles, tmp_path):
    names = BATCHES['three']
    stem = str(tmp_path / 'x')
    # written one by one, in alternating versions and chunk sizes, read as one batch by a coder of either kind
    for i, name in enumerate(names):
        src = singles(name, ('device', 'host', 'device')[i], (3, None, None)[i])[3]
        for s in FILES:
            shutil.copyfile(src + s, stem + f'_{i}' + s)
    assert [HEAD.unpack_from(open(stem + f'_{i}' + lossless.SUFFIX, 'rb').read(), 0)[1] for i in range(3)] == [2, 1, 2]
    for coder_name in ('host', 'device'):
        outs = lossless.LosslessCoder(model, stem, occupancy_coder=coder_name).decode_batch(['_0', '_1', '_2'])
        for name, out in zip(names, outs):
            assert np.array_equal(_rows(out.C), _set_of(CLOUDS[name])), (coder_name, name)
    # written as one batch, read one by one
    for coder_name in ('host', 'device'):
        coder = lossless.LosslessCoder(model, str(tmp_path / coder_name), occupancy_coder=coder_name, chunk_steps=3)
        coder.encode_batch(_tensor(*[CLOUDS[n] for n in names]), ['_0', '_1', '_2'])
        reader = lossless.LosslessCoder(model, str(tmp_path / coder_name))
        for i, name in enumerate(names):
            assert np.array_equal(_rows(reader.decode(postfix=f'_{i}').C), _set_of(CLOUDS[name])), (coder_name, name)


def test_bytes_do_not_depend_on_the_kernel_family_a_level_size_selects(model, singles, tmp_path):
    """the row gates moved so that on every decoder level a gate lies strictly between one frame's rows and the batch's rows: the frames coded
    alone and the batch take different kernel families at that level, and `_O.bin` is the same to the byte"""
    names = BATCHES['shell twice']
    want_files, want_record, _, _ = singles(names[0], 'device', None)
    r = want_record['rows']                                                         # candidate rows of one frame at the three decoder levels
    gate = [n + n // 2 for n in r]
    changes = dict(ROWS_IRN64_MIN=gate[0], PACKED_CONV64_MIN=gate[0], ROWS_IRN32_MIN=gate[1], ROWS_CONV_MIN=gate[1], ROWS_Q4_MIN=gate[1],
                   CHILD_Q4_MIN_PARENTS=gate[2] // 8)
    for l, gates in enumerate((('ROWS_IRN64_MIN', 'PACKED_CONV64_MIN'), ('ROWS_IRN32_MIN', 'ROWS_CONV_MIN', 'ROWS_Q4_MIN'), ('CHILD_Q4_MIN_PARENTS',))):
        for g in gates:
            at = changes[g] * (8 if g == 'CHILD_Q4_MIN_PARENTS' else 1)
            assert r[l] < at < 2 * r[l], f'level {l}: gate {g} = {at} does not separate {r[l]} rows from {2 * r[l]}'
    with ops.path(**changes):
        from pcgcv2_amd import dispatch
        assert dispatch.select('irn', (64,), r[0]).family != dispatch.select('irn', (64,), 2 * r[0]).family
        assert dispatch.select('irn', (32,), r[1]).family != dispatch.select('irn', (32,), 2 * r[1]).family
        alone = lossless.LosslessCoder(model, str(tmp_path / 'alone'), occupancy_coder='device')
        alone.encode(_tensor(CLOUDS[names[0]]))
        coder = lossless.LosslessCoder(model, str(tmp_path / 'b'), occupancy_coder='device')
        records = coder.encode_batch(_tensor(*[CLOUDS[n] for n in names]), ['_0', '_1'])
        assert [rec['rows'] for rec in records] == [r, r]
        outs = coder.decode_batch(['_0', '_1'])
    assert _files(str(tmp_path / 'alone')) == want_files                            # (the frame alone, on the other side of every gate)
    for i in range(2):
        assert _files(str(tmp_path / 'b') + f'_{i}') == want_files
        assert np.array_equal(_rows(outs[i].C), _set_of(CLOUDS[names[0]]))
    assert ops.PATH.ROWS_IRN64_MIN != gate[0]                                       # (the record is the default one again)


class _Contexts:
    """records the contexts of every level of a decode_batch (what ops.occ_symbols_segments hands on)"""

    def __init__(self, monkeypatch):
        self.levels = []
        inner = ops.occ_symbols_segments

        def spy(logits, seg_rows, truth=None):
            packed, sums = inner(logits, seg_rows, truth)
            edge = np.concatenate([[0], np.cumsum(seg_rows)])
            words = packed.cpu().numpy().view(np.uint16)
            self.levels.append([words[edge[f]:edge[f + 1]].astype(np.int64) >> 1 for f in range(len(seg_rows))])
            return packed, sums
        monkeypatch.setattr(ops, 'occ_symbols_segments', spy)


@pytest.mark.parametrize('coder_name', ['host', 'device'])
def test_damaged_files_of_one_item_are_refused_by_name_and_the_sound_batch_decodes_afterwards(coder_name, model, tmp_path, monkeypatch):
    names = ('filled ball', 'sphere shell', 'two components')
    postfixes = ['_0', '_1', '_2']
    coder = lossless.LosslessCoder(model, str(tmp_path / 'd'), occupancy_coder=coder_name, chunk_steps=1)
    coder.encode_batch(_tensor(*[CLOUDS[n] for n in names]), postfixes)
    spy = _Contexts(monkeypatch)
    coder.decode_batch(postfixes)
    ctx0 = spy.levels[0][1]                                                         # item 1's contexts at the first level: no payload decides them
    monkeypatch.undo()
    path = str(tmp_path / 'd') + '_1' + lossless.SUFFIX
    good = open(path, 'rb').read()
    magic, version, crc, *sizes = HEAD.unpack_from(good, 0)
    assert sizes[0] == len(ctx0)
    first = good[HEAD.size:HEAD.size + sizes[1]]
    word_at = HEAD.size + (8 + 516 * struct.unpack_from('<II', first)[1] + 4 if version == 2 else sizes[1] // 2)
    flip = lambda at, bit=0x01: good[:at] + bytes([good[at] ^ bit]) + good[at + 1:]
    damaged = {'magic': flip(0, 0x20), 'version': flip(4, 0x04), 'table CRC': flip(8), 'rows of level 1': flip(12 + 16, 0x08), 'rows of level 0': flip(12, 0x08),
               'cut by one byte': good[:-1], 'cut by one word': good[:-4], 'extended': good + b'\0\0\0\0',
               'another item\'s file': open(str(tmp_path / 'd') + '_0' + lossless.SUFFIX, 'rb').read()}
    if version == 2:
        damaged['S of the first payload'] = flip(HEAD.size, 0x02)
    refused_always = set(damaged)
    damaged['a payload word'] = flip(word_at, 0x10)
    for what, blob in damaged.items():
        open(path, 'wb').write(blob)
        must = what in refused_always or version == 1
        if not must:                                                                # version 2: refused wherever the definition refuses
            try:
                rr.decode(ctx0, blob[HEAD.size:HEAD.size + sizes[1]])
            except rr.Unsound:
                must = True
        try:
            outs = coder.decode_batch(postfixes)
        except ops.PcgcError as e:
            assert re.search(re.escape(path), str(e)), f'{what}: the refusal does not name the file: {e}'
            continue
        assert not must, f'{what}: decoded'
        assert not np.array_equal(_rows(outs[1].C), _set_of(CLOUDS[names[1]]))
    open(path, 'wb').write(good)
    for name, out in zip(names, coder.decode_batch(postfixes)):
        assert np.array_equal(_rows(out.C), _set_of(CLOUDS[name]))


def test_arguments_and_inputs_that_are_no_batch_are_refused(model, tmp_path):
    coder = lossless.LosslessCoder(model, str(tmp_path / 'r'), occupancy_coder='device')
    a, b = CLOUDS['one voxel per stride-8 cell'], CLOUDS['filled ball']
    two = _tensor(a, b)
    with pytest.raises(ValueError, match='postfixes'):                              # postfix count against items
        coder.encode_batch(two, ['_0', '_1', '_2'])
    with pytest.raises(ops.PcgcError, match='17 items'):
        coder.encode_batch(two, [f'_{i}' for i in range(17)])
    with pytest.raises(ops.PcgcError, match='17 items'):
        coder.decode_batch([f'_{i}' for i in range(17)])
    with pytest.raises(ops.PcgcError):
        coder.estimate_batch(_tensor(*[CLOUDS['single voxel']] * 17))
    for single_call in (coder.encode, coder.estimate):                              # one frame per call, as before
        with pytest.raises(ValueError, match='one frame'):
            single_call(two)
    # the same voxel twice, in item 1 alone: not a set
    twice = np.concatenate([b, b[:1]])
    with pytest.raises(ops.PcgcError, match='item 1'):
        coder.encode_batch(_tensor(a, twice, assume_unique=True), ['_0', '_1'])
    # a missing file names itself
    coder.encode_batch(two, ['_0', '_1'])
    os.remove(str(tmp_path / 'r') + '_1' + lossless.SUFFIX)
    with pytest.raises((ops.PcgcError, OSError), match='_1'):
        coder.decode_batch(['_0', '_1'])


def test_the_command_line_codes_several_files_as_one_batch(model, tmp_path, capsys):
    from pcgcv2_amd.data_utils import read_ply_ascii_geo, write_ply_ascii_geo
    ckpt = str(tmp_path / 'ckpt.pth')
    torch.save({'model': synthetic.synthetic_state_dict()}, ckpt)
    names = ('single voxel', 'one voxel per stride-8 cell', 'small 7')
    plys = []
    for i, name in enumerate(names):
        plys.append(str(tmp_path / f'cloud{i}.ply'))
        write_ply_ascii_geo(plys[-1], CLOUDS[name])
    out = str(tmp_path / 'out')
    lossless.main(['--ckptdir', ckpt, '--outdir', out, '--occupancy_coder', 'device', '--filedir'] + plys)
    text = capsys.readouterr().out
    assert text.count('lossless:\t exact') == 3 and text.count('\n' + lossless.SUFFIX + ':') == 3
    for i, name in enumerate(names):
        assert os.path.getsize(os.path.join(out, f'cloud{i}') + lossless.SUFFIX) > 0
        dec = np.asarray(read_ply_ascii_geo(os.path.join(out, f'cloud{i}_dec.ply')), dtype=np.int32)
        assert np.array_equal(_rows(np.concatenate([np.zeros((len(dec), 1), np.int32), dec], 1)), _set_of(CLOUDS[name]))
    lossless.main(['--ckptdir', ckpt, '--outdir', out + '1', '--filedir', plys[1]])          # one file behaves as before
    assert 'lossless:\t exact' in capsys.readouterr().out
    assert open(os.path.join(out + '1', 'cloud1_C.bin'), 'rb').read() == open(os.path.join(out, 'cloud1_C.bin'), 'rb').read()
