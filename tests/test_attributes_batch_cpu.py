"""The batched colour codec (AttributeCoder.encode_batch / decode_batch) as far as it goes without a GPU: the new C-ABI
entries are exported and declared, the host's cut of a batch into per-frame chunks and payloads agrees with the definition of one frame
(tests/attr_rans_reference.py), and every argument a batch can be refused for before the device is looked at is refused."""
import os
import re

import numpy as np
import pytest
import torch

import attr_rans_reference as ar
from pcgcv2_amd import attributes as at, ops

ENTRIES = ['pcgc_raht_keys_batch_workspace_bytes', 'pcgc_raht_keys_batch', 'pcgc_raht_tree_batch_workspace_bytes', 'pcgc_raht_tree_batch',
           'pcgc_raht_forward_batch', 'pcgc_raht_inverse_batch', 'pcgc_raht_quantize_batch_workspace_bytes', 'pcgc_raht_quantize_batch',
           'pcgc_raht_dequantize_batch_workspace_bytes', 'pcgc_raht_dequantize_batch', 'pcgc_attr_rans_batch_workspace_bytes',
           'pcgc_attr_rans_encode_batch', 'pcgc_attr_rans_decode_batch']
TOKENS = [0, 63, 66, 192, 195]                                  # frames of 1, 22, 23, 65 and 66 points


def test_entries_are_exported_and_declared():
    header = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'pcgc_hip.h')).read()
    for name in ENTRIES:
        assert getattr(ops.lib(), name) is not None, name
        assert re.search(r'\b(int|size_t|int64_t) ' + name + r'\(', header), name


@pytest.mark.parametrize('chunk_steps', [1, 3, 0])
def test_layout_agrees_with_the_definition_of_one_frame(chunk_steps):
    lay = ops.attr_rans_batch_layout(TOKENS, chunk_steps)
    assert lay['tok'].tolist() == np.concatenate([[0], np.cumsum(TOKENS)]).tolist()
    assert lay['first_chunk'].tolist() == np.concatenate([[0], np.cumsum(lay['chunks'])]).tolist()
    for b, n in enumerate(TOKENS):
        S = chunk_steps or max(1, ar.chunks_of(n, 1))            # one chunk with the frame's own S, as encode does it
        if n == 0:
            assert lay['steps'][b] == 0 and lay['chunks'][b] == 0 and lay['room'][b] == 0
            continue
        assert lay['steps'][b] == S and lay['chunks'][b] == ar.chunks_of(n, S)
        if chunk_steps == 0:
            assert lay['chunks'][b] == 1
        # a payload of the definition for these n tokens parses under the frame's (S, K), and fits the room the batch gives it
        table, bucket, ctx, tokens = ar.model_drawn(n, seed=n)
        payload = ar.encode(table, ctx, tokens, S)
        got_S, chunks = ar.parse(payload, n)
        assert got_S == lay['steps'][b] and len(chunks) == lay['chunks'][b]
        assert ops.attr_rans_layout(payload, n) == (lay['steps'][b], lay['chunks'][b])
        assert len(payload) <= lay['room'][b] == 8 + 516 * len(chunks) + 4 * n
        assert lay['pay'][b] % 8 == 0 and lay['pay'][b + 1] - lay['pay'][b] >= lay['room'][b]
    mixed = ops.attr_rans_batch_layout(TOKENS, [5, 1, 3, 0, 2])  # steps per frame
    assert mixed['steps'].tolist() == [0, 1, 3, 3, 2] and mixed['chunks'].tolist() == [0, 1, 1, 1, 2]
    with pytest.raises(ValueError):
        ops.attr_rans_batch_layout(TOKENS, -1)
    with pytest.raises(ValueError):
        ops.attr_rans_batch_layout([3, -3], 1)


def _meta(n, cols=4):
    return torch.empty((n, cols), dtype=torch.int32, device='meta')


def test_arguments_are_refused_before_the_device(tmp_path):
    coder = at.AttributeCoder(str(tmp_path / 'x'))
    coords, rgb = _meta(10), torch.empty((10, 3), dtype=torch.uint8, device='meta')
    many = [str(i) for i in range(17)]
    for postfixes in ([], many, ['a', 'a'], ['a', 'b', 'a'], 'ab', None, ['a', 1]):
        with pytest.raises(ValueError, match='frames|postfixes'):
            coder.encode_batch(coords, rgb, 4, postfixes=postfixes)
        with pytest.raises(ValueError, match='frames|postfixes'):
            coder.decode_batch(coords, postfixes=postfixes)
    two = ['a', 'b']
    for q in ([4], [4, 5, 6], [4, 256], [-1, 4], 256, -1, [4, 2.5], None, [True, 4]):
        with pytest.raises(ValueError, match='qstep'):
            coder.encode_batch(coords, rgb, q, postfixes=two)
        with pytest.raises(ValueError, match='qstep_chroma'):
            coder.encode_batch(coords, rgb, 4, q if q is not None else [1], postfixes=two)
    with pytest.raises(ValueError, match='2\\^24'):
        coder.encode_batch(_meta((1 << 24) + 1), rgb, 4, postfixes=two)
    with pytest.raises(ValueError, match='2\\^24'):
        coder.decode_batch(_meta((1 << 24) + 1), postfixes=two)
    with pytest.raises(ValueError, match=r'\[N,4\]'):
        coder.encode_batch(_meta(10, 3), rgb, 4, postfixes=two)
    assert not os.listdir(str(tmp_path))
    # the native entries refuse the same before anything is touched
    L = ops.lib()
    assert L.pcgc_raht_keys_batch(None, (1 << 24) + 1, 2, None, None, None, None, 0, None) == -2
    assert L.pcgc_raht_keys_batch(None, 10, 0, None, None, None, None, 0, None) == -2
    assert L.pcgc_raht_keys_batch(None, 10, 17, None, None, None, None, 0, None) == -2
    assert L.pcgc_raht_tree_batch(None, (1 << 24) + 1, 2, None, None, None, None, None, None, None, None, None, 0, None) == -2
    assert L.pcgc_raht_tree_batch(None, 10, 17, None, None, None, None, None, None, None, None, None, 0, None) == -2
    assert L.pcgc_raht_quantize_batch(None, 1, 2, None, None, None, None, None, None, None, None, None, None, None, None, None, 0, None) == -2
    assert L.pcgc_raht_dequantize_batch(None, None, 0, 1, 2, None, None, None, None, None, None, None, None, None, 0, None) == -2
    tok, steps, pay = np.array([0, 3, 6], np.int64), np.array([1, 1], np.int32), np.array([0, 1024, 2048], np.int64)
    for bad_tok, bad_steps, bad_pay in ((np.array([0, 4, 6], np.int64), steps, pay), (np.array([3, 3, 6], np.int64), steps, pay),
                                       (tok, np.array([1, 0], np.int32), pay), (tok, steps, np.array([0, 1020, 2048], np.int64))):
        assert L.pcgc_attr_rans_encode_batch(None, None, None, 2, bad_tok.ctypes.data, bad_steps.ctypes.data, None, bad_pay.ctypes.data, None,
                                             None, 0, None) == -2
    assert L.pcgc_attr_rans_encode_batch(None, None, None, 17, tok.ctypes.data, steps.ctypes.data, None, pay.ctypes.data, None, None, 0, None) == -2
