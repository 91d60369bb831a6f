"""GPU tests of the lossless mode: pcgc_occ_symbols (csrc/occupancy.hip) against the numpy definition of tests/lossless_reference.py, and
LosslessCoder (pcgcv2_amd/lossless.py) end to end — exact reconstruction, the lossy files untouched, length accounting, damaged streams.
Synthetic weights throughout: the rate they give says nothing about trained models."""
import os
import struct

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import lossless_reference as lr
from pcgcv2_amd import lossless, occupancy_model as om, ops, synthetic
from pcgcv2_amd.coder import Coder, STREAMS, INDEX_SUFFIX
from pcgcv2_amd.pcc_model import PCCModel
from pcgcv2_amd.sparse import SparseTensor, sparse_collate

DEV = torch.device('cuda:0')
BLOCK_ROWS = 1024                                  # rows one workgroup of k_occ_symbols covers (256 threads x 4 rows)
# 320 008 rows are 313 workgroups: the one-block final stage adds slots t, t + 256, ... and takes a second trip
SIZES = (8, 264, BLOCK_ROWS - 1, BLOCK_ROWS, BLOCK_ROWS + 1, 320008)
HEAD = struct.Struct('<4sII6Q')


# ---- pcgc_occ_symbols -----------------------------------------------------------------------------------------------------------------------
def _layouts(z):
    """(name, device view [n, 1] or [n]) of the same logits: dense and aligned, dense at an odd element offset, rows of a wider buffer"""
    n = len(z)
    t = torch.from_numpy(z).to(DEV)
    off = torch.zeros(n + 1, dtype=torch.float32, device=DEV)
    off[1:] = t
    wide = torch.full((n, 3), 7.0, dtype=torch.float32, device=DEV)
    wide[:, 1] = t
    return (('dense', t), ('dense [n, 1]', t.view(n, 1)), ('offset by one element', off[1:]), ('ld = 3', wide[:, 1:2]))


@pytest.mark.parametrize('n', SIZES)
def test_occ_symbols_equal_the_definition(n):
    z, truth = lr.random_logits(n, seed=n)
    want_words, want_occupied, want_cost = lr.occ_symbols(z, truth)
    want_ctx_only, _, _ = lr.occ_symbols(z)
    truth_d = torch.from_numpy(truth).to(DEV)
    for name, view in _layouts(z):
        packed, sums = ops.occ_symbols(view, truth_d)
        words, occupied, cost = ops.occ_words_host(packed, sums)
        assert np.array_equal(words, want_words), name
        assert (occupied, cost) == (want_occupied, want_cost), name
        packed, sums = ops.occ_symbols(view)                       # truth = NULL: contexts only
        assert sums is None
        assert np.array_equal(ops.occ_words_host(packed)[0], want_ctx_only), name


def test_occ_symbols_special_logits_and_empty():
    z, q = lr.special_logits()
    both = np.concatenate([z, z])
    truth = np.concatenate([np.zeros(len(z), np.uint8), np.full(len(z), 3, np.uint8)])     # any non-zero byte is "occupied"
    packed, sums = ops.occ_symbols(torch.from_numpy(both).to(DEV), torch.from_numpy(truth).to(DEV))
    words, occupied, cost = ops.occ_words_host(packed, sums)
    ctx = np.concatenate([q, q]) + lr.QMAX
    assert np.array_equal(words >> 1, ctx) and np.array_equal(words & 1, truth != 0)
    assert occupied == len(z) and cost == int(om.cost()[ctx, (truth != 0).astype(int)].astype(np.int64).sum())
    packed, sums = ops.occ_symbols(torch.empty(0, dtype=torch.float32, device=DEV), torch.empty(0, dtype=torch.uint8, device=DEV))
    assert packed.numel() == 0 and sums.tolist() == [0, 0]
    with pytest.raises(ops.PcgcError):
        ops.occ_symbols(torch.zeros(5, device=DEV), torch.zeros(4, dtype=torch.uint8, device=DEV))


# ---- LosslessCoder ----------------------------------------------------------------------------------------------------------------------------
def _model():
    model = PCCModel().to(DEV)
    model.load_state_dict(synthetic.synthetic_state_dict())
    return model


@pytest.fixture(scope='module')
def model():
    return _model()


def _tensor(pts):
    coords, feats = sparse_collate([torch.from_numpy(np.ascontiguousarray(pts, dtype=np.int32))], [torch.ones((len(pts), 1))])
    return SparseTensor(feats, coordinates=coords, tensor_stride=1, device=DEV)


def _rows(t):
    """the coordinate rows of a tensor, sorted: equal arrays = equal sets (rows are distinct)"""
    c = t.cpu().numpy()
    return c[np.lexsort(c.T[::-1])]


def _files(prefix, names):
    return {s: open(prefix + s, 'rb').read() for s in names}


CLOUDS = lr.clouds()


@pytest.mark.parametrize('name', list(CLOUDS))
def test_round_trip_is_exact_and_leaves_the_lossy_files_alone(name, model, tmp_path):
    pts = CLOUDS[name]
    lossy_names = STREAMS + (INDEX_SUFFIX,)
    plain = Coder(model, str(tmp_path / 'plain'))
    plain.encode(_tensor(pts))
    plain_dec = _rows(plain.decode().C)
    coder = lossless.LosslessCoder(model, str(tmp_path / 'exact'))
    x = _tensor(pts)
    record = coder.encode(x)
    out = coder.decode()
    assert np.array_equal(_rows(out.C), _rows(x.C)), 'the decoded voxel set is not the input set'
    assert out.cmap.stride == 1 and len(out) == len(pts)
    assert _files(str(tmp_path / 'exact'), lossy_names) == _files(str(tmp_path / 'plain'), lossy_names)
    assert np.array_equal(_rows(Coder(model, str(tmp_path / 'exact')).decode().C), plain_dec), 'Coder.decode of the lossy files changed'
    assert record['bits_O'] == 8 * os.path.getsize(str(tmp_path / 'exact') + lossless.SUFFIX)
    assert record['rows'][1] % 8 == 0 and record['rows'][2] == 8 * (record['rows'][2] // 8)
    assert lossless.same_voxels(out.C, x.C)


def _cls_layers(m):
    return [getattr(m.decoder, f'conv{l}_cls') for l in range(3)]


def test_saturated_logits_still_round_trip(tmp_path):
    """cls kernels x 1e3 (in-place under no_grad: the version counter moves, derived.py rebuilds the tables): contexts pile up at 0 and 352,
    many confident predictions are wrong and cost 16 bits each — the round trip is exact all the same"""
    m = _model()
    with torch.no_grad():
        for layer in _cls_layers(m):
            layer.kernel.mul_(1e3)
    seen = []
    coder = lossless.LosslessCoder(m, str(tmp_path / 'sat'))
    x = _tensor(CLOUDS['sphere shell'])
    words_host = ops.occ_words_host
    try:
        ops.occ_words_host = lambda packed, sums=None: seen.append(words_host(packed, sums)) or seen[-1]
        coder.encode(x)
    finally:
        ops.occ_words_host = words_host
    ctx = np.concatenate([w[0] >> 1 for w in seen])
    extreme = np.isin(ctx, (0, 2 * lr.QMAX)).mean()
    print(f'saturated: {extreme:.3f} of {len(ctx)} contexts at 0 or 352')
    assert extreme > 0.5
    assert np.array_equal(_rows(coder.decode().C), _rows(x.C))


def test_nan_logits_cost_one_bit_per_candidate(tmp_path):
    m = _model()
    with torch.no_grad():
        for layer in _cls_layers(m):
            layer.bias.fill_(float('nan'))
    coder = lossless.LosslessCoder(m, str(tmp_path / 'nan'))
    x = _tensor(CLOUDS['sphere shell'])
    record = coder.encode(x)
    candidates = sum(record['rows'])
    assert record['est_units_O'] == candidates * om.COST_UNIT               # every context is 176: exactly one bit each
    assert 8 * sum(record['payload_bytes']) <= lr.length_bound(candidates, candidates, payloads=3)
    assert np.array_equal(_rows(coder.decode().C), _rows(x.C))


def test_length_accounting(model, tmp_path, monkeypatch):
    seen = []
    words_host = ops.occ_words_host
    monkeypatch.setattr(ops, 'occ_words_host', lambda packed, sums=None: seen.append(words_host(packed, sums)) or seen[-1])
    coder = lossless.LosslessCoder(model, str(tmp_path / 'len'))
    x = _tensor(CLOUDS['sphere shell'])
    record = coder.encode(x)
    assert len(seen) == 3
    cost = om.cost().astype(np.int64)
    host_units = sum(int(cost[w >> 1, w & 1].sum()) for w, _, _ in seen)
    assert record['est_units_O'] == host_units == sum(c for _, _, c in seen)
    assert record['est_bits_O'] == host_units / om.COST_UNIT
    assert [len(w) for w, _, _ in seen] == record['rows']
    assert coder.estimate(x) == record['est_bits_O']
    assert coder.estimate(_tensor(CLOUDS['shuffled shell'])) == record['est_bits_O']       # (the row order of the input changes nothing)
    realised = 8 * sum(record['payload_bytes'])
    print(f"ideal {record['est_bits_O']:.1f} bits, payloads {realised} bits, rows {record['rows']}")
    assert realised <= lr.length_bound(record['est_bits_O'], sum(record['rows']), payloads=3)
    assert record['bits_O'] == realised + 8 * HEAD.size


def test_a_batch_is_refused(model, tmp_path):
    a, b = CLOUDS['single voxel'], CLOUDS['one voxel per stride-8 cell']
    coords, feats = sparse_collate([torch.from_numpy(a), torch.from_numpy(b)], [torch.ones((len(a), 1)), torch.ones((len(b), 1))])
    batch = SparseTensor(feats, coordinates=coords, tensor_stride=1, device=DEV)
    coder = lossless.LosslessCoder(model, str(tmp_path / 'batch'))
    with pytest.raises(ValueError):
        coder.encode(batch)
    with pytest.raises(ValueError):
        coder.estimate(batch)


def test_damaged_streams_are_refused(model, tmp_path):
    coder = lossless.LosslessCoder(model, str(tmp_path / 'dmg'))
    x = _tensor(CLOUDS['sphere shell'])
    coder.encode(x)
    path = str(tmp_path / 'dmg') + lossless.SUFFIX
    good = open(path, 'rb').read()
    magic, version, crc, *sizes = HEAD.unpack_from(good, 0)
    body = good[HEAD.size:]

    def rewritten(sizes_, body_):
        return HEAD.pack(magic, version, crc, *sizes_) + body_

    assert rewritten(sizes, body) == good
    cut = list(sizes)
    cut[5] -= 1                                                      # the last payload loses its last byte, the header agrees
    rows_off = list(sizes)
    rows_off[2] += 8
    damaged = {
        'flipped magic': bytes([good[0] ^ 0x20]) + good[1:],
        'wrong table CRC': good[:8] + struct.pack('<I', crc ^ 0x1) + good[12:],
        'file cut by one byte': good[:-1],
        'payload cut by one byte': rewritten(cut, body[:-1]),
        'first payload cut by one byte': rewritten([sizes[0], sizes[1] - 1] + sizes[2:], body[:sizes[1] - 1] + body[sizes[1]:]),
        'declared rows off by 8': rewritten(rows_off, body),
    }
    for what, blob in damaged.items():
        open(path, 'wb').write(blob)
        with pytest.raises(ops.PcgcError):
            coder.decode()
            pytest.fail(f'{what}: decoded')
    # one payload bit flipped in the middle: refused, or another set — never the input's, never a fault
    at = HEAD.size + sizes[1] + sizes[3] + sizes[5] // 2
    open(path, 'wb').write(good[:at] + bytes([good[at] ^ 0x04]) + good[at + 1:])
    try:
        out = coder.decode()
    except ops.PcgcError:
        out = None
    assert out is None or not np.array_equal(_rows(out.C), _rows(x.C))
    open(path, 'wb').write(good)
    assert np.array_equal(_rows(coder.decode().C), _rows(x.C))
