"""The batched lossless mode (LosslessCoder.encode_batch / decode_batch) as far as it goes without a GPU: the new C-ABI entries
are exported and declared, the host's cut of a batch's level into per-frame chunks and payloads agrees with the definition of one frame
(tests/rans_reference.py), and every argument a batch can be refused for before the device is looked at is refused."""
import os
import re

import numpy as np
import pytest
import torch

import rans_reference as rr
from pcgcv2_amd import lossless, ops
from pcgcv2_amd.pcc_model import PCCModel

ENTRIES = ['pcgc_occ_symbols_segments', 'pcgc_occ_rans_batch_workspace_bytes', 'pcgc_occ_rans_encode_batch', 'pcgc_occ_rans_decode_batch']
ROWS = [0, 1, 63, 64, 65, 192, 193]


def test_entries_are_exported_and_declared():
    header = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'pcgc_hip.h')).read()
    for name in ENTRIES:
        assert getattr(ops.lib(), name) is not None, name
        assert re.search(r'\b(int|size_t|int64_t) ' + name + r'\(', header), name


@pytest.mark.parametrize('chunk_steps', [1, 3, 0])
def test_layout_agrees_with_the_definition_of_one_frame(chunk_steps):
    lay = ops.occ_rans_batch_layout(ROWS, chunk_steps)
    assert lay['row'].tolist() == np.concatenate([[0], np.cumsum(ROWS)]).tolist()
    assert lay['first_chunk'].tolist() == np.concatenate([[0], np.cumsum(lay['chunks'])]).tolist()
    for f, n in enumerate(ROWS):
        S = chunk_steps or max(1, rr.chunks_of(n, 1))              # one chunk with the frame's own S, as LosslessCoder.encode does it
        assert lay['steps'][f] == S and lay['chunks'][f] == rr.chunks_of(n, S) == ops.occ_rans_chunks(n, S)
        if chunk_steps == 0:
            assert lay['chunks'][f] == (1 if n else 0)
        # a payload of the definition for these n rows parses under the frame's (S, K), and fits the room the batch gives it
        ctx, bit = rr.model_drawn(n, seed=n)
        payload = rr.encode(ctx, bit, S)
        got_S, chunks = rr.parse(payload, n)
        assert got_S == lay['steps'][f] and len(chunks) == lay['chunks'][f]
        assert ops.occ_rans_layout(payload, n) == (lay['steps'][f], lay['chunks'][f])
        assert len(payload) <= lay['room'][f] == 8 + 516 * len(chunks) + 4 * n
        assert lay['pay'][f] % 8 == 0 and lay['pay'][f + 1] - lay['pay'][f] >= lay['room'][f]
    assert lay['room'][0] == 8 == len(rr.encode([], [], int(lay['steps'][0])))      # a frame without rows: the head S | 0
    mixed = ops.occ_rans_batch_layout(ROWS, [5, 1, 3, 0, 2, 1, 0])                  # steps per frame
    assert mixed['steps'].tolist() == [5, 1, 3, 1, 2, 1, 4] and mixed['chunks'].tolist() == [0, 1, 1, 1, 1, 3, 1]


def test_layout_refusals():
    for rows, steps in (([], 1), ([8] * 17, 1), ([8, -8], 1), ([8, 8], -1), ([8, 8], (1 << 24) + 1), ([8, 8], [1, 2, 3]), ([1 << 30, 1 << 30], 1)):
        with pytest.raises(ValueError):
            ops.occ_rans_batch_layout(rows, steps)
    assert ops.occ_rans_batch_layout([8] * 16, 1 << 24)['chunks'].tolist() == [1] * 16


def test_arguments_are_refused_before_the_device(tmp_path):
    coder = lossless.LosslessCoder(PCCModel(), str(tmp_path / 'x'))
    many = [str(i) for i in range(17)]
    for postfixes in ([], many):
        with pytest.raises(ops.PcgcError, match='items'):
            coder.encode_batch(None, postfixes)
        with pytest.raises(ops.PcgcError, match='items'):
            coder.decode_batch(postfixes)
    with pytest.raises(ValueError, match='differ'):
        coder.encode_batch(None, ['a', 'b', 'a'])
    with pytest.raises(ValueError, match='differ'):
        coder.decode_batch(['a', 'a'])
    with pytest.raises(TypeError):
        coder.encode_batch(np.zeros((4, 4)), ['a', 'b'])
    with pytest.raises(TypeError):
        coder.estimate_batch(None)
    assert not os.listdir(str(tmp_path))
    meta = torch.empty(16, dtype=torch.int16, device='meta')
    with pytest.raises(ValueError, match='payloads'):                               # payload count against frames
        ops.occ_rans_decode_batch(meta, [8, 8], [b''])
    for rows in ([], [1] * 17, [8, -8]):
        with pytest.raises(ValueError):
            ops.occ_rans_decode_batch(meta, rows, [None] * len(rows))
        with pytest.raises(ValueError):
            ops.occ_rans_encode_batch(meta, rows, 1)
        with pytest.raises(ValueError):
            ops.occ_symbols_segments(torch.empty(16, dtype=torch.float32, device='meta'), rows)
    with pytest.raises(ValueError):
        ops.occ_rans_encode_batch(meta, [8, 8], (1 << 24) + 1)


def test_native_entries_refuse_before_anything_is_touched():
    L = ops.lib()
    row, steps, pay = np.array([0, 8, 16], np.int64), np.array([1, 1], np.int32), np.array([0, 1024, 2048], np.int64)
    one = np.ones(1, np.int64)                                                      # (a non-null pointer the entry never follows)
    bad = [(np.array([0, 8, 4], np.int64), steps, pay),                             # a negative row count
           (np.array([8, 8, 16], np.int64), steps, pay),                            # rows not from 0
           (np.array([0, 8, 1 << 31], np.int64), steps, pay),                       # 2^31 rows
           (row, np.array([1, -1], np.int32), pay),
           (row, np.array([1, (1 << 24) + 1], np.int32), pay),
           (row, steps, np.array([0, 1020, 2048], np.int64))]                       # a payload offset off the 8-byte grid
    for r, s, p in bad:
        assert L.pcgc_occ_rans_encode_batch(None, 2, r.ctypes.data, s.ctypes.data, None, None, p.ctypes.data, None, None, 0, None) == -2
        assert L.pcgc_occ_rans_decode_batch(None, 2, r.ctypes.data, s.ctypes.data, None, p.ctypes.data, one.ctypes.data, None, None, None, 0, None) == -2
    assert L.pcgc_occ_rans_encode_batch(None, 2, row.ctypes.data, np.array([1, 0], np.int32).ctypes.data, None, None, pay.ctypes.data, None, None, 0,
                                        None) == -2                                 # the encoder codes every frame
    for frames in (0, 17, -1):
        assert L.pcgc_occ_rans_encode_batch(None, frames, row.ctypes.data, steps.ctypes.data, None, None, pay.ctypes.data, None, None, 0, None) == -2
        assert L.pcgc_occ_rans_decode_batch(None, frames, row.ctypes.data, steps.ctypes.data, None, pay.ctypes.data, one.ctypes.data, None, None, None, 0,
                                            None) == -2
        assert L.pcgc_occ_symbols_segments(None, 1, frames, one.ctypes.data, None, None, None, None) == -2
    assert L.pcgc_occ_symbols_segments(None, 1, 2, np.array([8, -8], np.int64).ctypes.data, None, None, None, None) == -2
    assert L.pcgc_occ_symbols_segments(None, 0, 1, one.ctypes.data, None, None, None, None) == -2
    assert L.pcgc_occ_rans_batch_workspace_bytes(128, 3) == 3 * 16 * 8 + 16 + 4 * 128 + 64


@pytest.mark.parametrize('kind', ['occ', 'attr'])
def test_the_single_sizing_entry_is_the_batch_entry_at_the_frame_s_own_chunks(kind):
    """the single entries run on the batch's slot layout (csrc/rans_core.h): one workspace layout per coder"""
    L = ops.lib()
    single, batch = getattr(L, f'pcgc_{kind}_rans_workspace_bytes'), getattr(L, f'pcgc_{kind}_rans_batch_workspace_bytes')
    for n in (0, 1, 64, 65, 193):
        for S in (1, 3):
            assert int(single(n, S)) == int(batch(n, -(-n // (64 * S)))), (kind, n, S)
