"""GPU tests of the occupancy stream's device coder (csrc/occupancy_rans.hip, `_O.bin` version 2): byte and bit equality with the plain-integer
definition of tests/rans_reference.py in both directions, the refusals the definition gives (test_occ_rans_cpu.py shows that it gives them),
and LosslessCoder(occupancy_coder='device') end to end.  Synthetic weights throughout: the rate they give says nothing about trained models."""
import os
import struct

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import lossless_reference as lr
import rans_reference as rr
import scratch_arena as SA
from pcgcv2_amd import lossless, ops, synthetic
from pcgcv2_amd.coder import STREAMS
from pcgcv2_amd.pcc_model import PCCModel
from pcgcv2_amd.sparse import SparseTensor, sparse_collate
from scratch_arena import Arena

DEV = torch.device('cuda:0')
HEAD = struct.Struct('<4sII6Q')


def _packed(ctx, bit=None):
    """what occ_symbols hands on: int16 [n] on the device, ctx << 1 | bit (bit 0 on the decoder's side)"""
    w = np.asarray(ctx, dtype=np.int64) << 1
    if bit is not None:
        w = w | np.asarray(bit, dtype=np.int64)
    return torch.from_numpy(w.astype(np.int16)).to(DEV)


def _both_directions(ctx, bit, S, what=''):
    n = len(ctx)
    want = rr.encode(ctx, bit, S)
    got = ops.occ_rans_encode(_packed(ctx, bit), S)
    assert got == want, f'{what}: n = {n}, S = {S}: the kernel\'s payload ({len(got)} bytes) is not the definition\'s ({len(want)})'
    mask, occupied = ops.occ_rans_decode(_packed(ctx), want, n)               # the kernel decodes the definition's payload
    assert mask.dtype == torch.uint8 and mask.device.type == 'cuda'
    assert np.array_equal(mask.cpu().numpy(), bit) and occupied == int(np.sum(bit)), f'{what}: n = {n}, S = {S}'
    assert np.array_equal(rr.decode(ctx, got), bit)                           # the definition decodes the kernel's payload


@pytest.mark.parametrize('S', [1, 4, 16])
def test_bytes_and_bits_equal_the_definition_at_chunk_edges(S):
    for n in (0, 1, 63, 64, 65, 64 * S - 1, 64 * S, 64 * S + 1, 3 * 64 * S + 17):
        ctx, bit = rr.cyclic(n, seed=n + S)
        _both_directions(ctx, bit, S, 'cyclic')
        ctx, bit = rr.model_drawn(n, seed=n + S)
        _both_directions(ctx, bit, S, 'model-drawn')


def test_default_steps_just_past_one_chunk():
    n = 64 * lossless.CHUNK_STEPS + 77
    ctx, bit = rr.model_drawn(n, seed=3)
    _both_directions(ctx, bit, lossless.CHUNK_STEPS, 'default S')


def test_one_chunk_of_many_steps_refills_the_word_ring():
    """cyclic contexts with random bits cost about 4.5 bits a row: 20 000 rows are some 2 800 words, several refills of 512"""
    ctx, bit = rr.cyclic(20000, seed=11)
    _both_directions(ctx, bit, 512, 'one chunk')


@pytest.mark.parametrize('S', [4, 16])
def test_extreme_contexts(S):
    n = 3 * 64 * S + 17
    for what, (ctx, bit) in {
        'improbable bit at every row': rr.extreme(n, True),                   # the capacity bound: 16 bits a row
        'probable bit at every row': rr.extreme(n, False),                    # no lane ever emits: W_k = 0
        'only lane 0 improbable': rr.extreme(n, False, lanes=(0,)),
        'only lane 63 improbable': rr.extreme(n, False, lanes=(63,)),
        'alternating lanes improbable': rr.extreme(n, False, lanes=range(0, 64, 2)),
    }.items():
        _both_directions(ctx, bit, S, what)
    counts = np.frombuffer(ops.occ_rans_encode(_packed(*rr.extreme(n, False)), S), '<u4', 4, 8 + 512 * 4)
    assert not counts.any()


def test_special_logits_through_occ_symbols():
    z, q = lr.special_logits()
    z = np.concatenate([z, z])
    truth = (np.arange(len(z)) % 3 == 0).astype(np.uint8)
    packed, sums = ops.occ_symbols(torch.from_numpy(z).to(DEV), torch.from_numpy(truth).to(DEV))
    ctx = np.concatenate([q, q]) + lr.QMAX
    for S in (1, 4):
        payload, occupied, cost = ops.occ_rans_encode(packed, S, sums)
        assert payload == rr.encode(ctx, truth, S)
        assert occupied == int(truth.sum()) and cost == round(rr.ideal_bits(ctx, truth) * 65536)
        contexts, _ = ops.occ_symbols(torch.from_numpy(z).to(DEV))
        mask, kept = ops.occ_rans_decode(contexts, payload, len(z))
        assert np.array_equal(mask.cpu().numpy(), truth) and kept == occupied


def test_unsound_payloads_are_refused_and_the_sound_one_still_decodes():
    ctx, bit, S = rr.three_chunks()
    good = rr.encode(ctx, bit, S)
    contexts = _packed(ctx)
    for what, payload in rr.damaged(good).items():
        with pytest.raises(ops.PcgcError):
            ops.occ_rans_decode(contexts, payload, len(ctx))
            pytest.fail(f'{what}: decoded')
    for what, payload in {'wrong K': struct.pack('<II', S, 4) + good[8:], 'S = 0': struct.pack('<II', 0, 3) + good[8:],
                          'another n': good}.items():
        with pytest.raises(ops.PcgcError):
            ops.occ_rans_decode(_packed(ctx[:64]) if what == 'another n' else contexts, payload, 64 if what == 'another n' else len(ctx))
            pytest.fail(f'{what}: decoded')
    mask, occupied = ops.occ_rans_decode(contexts, good, len(ctx))
    assert np.array_equal(mask.cpu().numpy(), bit) and occupied == int(bit.sum())


# ---- the single entries on the batch's slot layout (csrc/rans_core.h) ---------------------------------------------------------------------------
def test_single_decoder_takes_exactly_the_batch_slot_and_refuses_one_byte_less():
    """pcgc_occ_rans_decode at n = 65, S = 1 (two chunks) needs 384 + 8 ceil(K / 2) bytes: a byte less is refused before any launch (the mask
    and the workspace under guard bands stay unwritten), exactly as much decodes what the definition says"""
    n, S = 65, 1
    ctx, bit = rr.model_drawn(n, seed=5)
    payload = rr.encode(ctx, bit, S)
    need = 384 + 8 * ((rr.chunks_of(n, S) + 1) // 2)
    assert rr.chunks_of(n, S) == 2 and need == 392
    arena = Arena()
    with SA.installed(arena):
        ws = ops.torch.empty(need, dtype=torch.uint8, device=DEV)
        mask = ops.torch.empty(n, dtype=torch.uint8, device=DEV)
    contexts = _packed(ctx)
    up = torch.frombuffer(bytearray(payload + bytes(-len(payload) % 8)), dtype=torch.uint8).to(DEV)
    host = np.zeros(2, np.int64)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    dec = lambda ws_bytes: ops.lib().pcgc_occ_rans_decode(contexts.data_ptr(), n, up.data_ptr(), len(payload), S, mask.data_ptr(), host.ctypes.data,
                                                          ws.data_ptr(), ws_bytes, stream)
    assert dec(need - 1) == -2 and 'too small' in ops.lib().pcgc_last_error().decode()
    arena.check()
    assert not any(b.payload().any() for b in arena.blocks), 'a refused call wrote to its buffers'
    assert dec(need) == 0 and host.tolist() == [int(bit.sum()), 0]
    assert np.array_equal(mask.cpu().numpy(), rr.decode(ctx, payload)) and np.array_equal(mask.cpu().numpy(), bit)
    arena.check()


def test_encoder_zeroes_its_slot_on_a_workspace_full_of_ones():
    """frames of (64, 0, 64) rows on recycled scratch whose workspace block arrives as 0xff bytes: the payloads are the definition's"""
    S, split = 1, (64, 0, 64)
    frames = [rr.model_drawn(n, seed=7 + f) for f, n in enumerate(split)]
    ctx, bit = np.concatenate([c for c, _ in frames]), np.concatenate([b for _, b in frames])
    want = [rr.encode(c, b, S) for c, b in frames]

    def run(arena):
        with SA.installed(arena):
            out = ops.occ_rans_encode_batch(_packed(ctx, bit), split, S)
        arena.finish()
        arena.check()
        return out

    rec = Arena()
    assert run(rec) == want
    workspace = [b for b in rec.blocks if b.caller == '_rans_batch_ws']
    assert len(workspace) == 1
    workspace[0].payload().view(torch.uint8).fill_(0xff)
    stale = rec.replay()
    assert run(stale) == want
    allocs, replayed, _ = stale.stats()
    assert replayed == allocs and not stale.served_fresh


# ---- LosslessCoder(occupancy_coder='device') ------------------------------------------------------------------------------------------------
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
    c = t.cpu().numpy()
    return c[np.lexsort(c.T[::-1])]


CLOUDS = lr.clouds()
LOSSY = STREAMS                                     # _C, _F, _H, _num_points


@pytest.mark.parametrize('name', list(CLOUDS))
def test_device_mode_round_trips_and_both_objects_read_both_versions(name, model, tmp_path):
    x = _tensor(CLOUDS[name])
    want = _rows(x.C)
    host = lossless.LosslessCoder(model, str(tmp_path / 'host'))
    device = lossless.LosslessCoder(model, str(tmp_path / 'device'), occupancy_coder='device', chunk_steps=16)
    host_record = host.encode(x)
    record = device.encode(x)
    out = device.decode()
    assert np.array_equal(_rows(out.C), want), 'the decoded voxel set is not the input set'
    assert out.cmap.stride == 1
    for s in LOSSY:
        assert open(str(tmp_path / 'device') + s, 'rb').read() == open(str(tmp_path / 'host') + s, 'rb').read(), s
    head = HEAD.unpack_from(open(str(tmp_path / 'device') + lossless.SUFFIX, 'rb').read(), 0)
    assert head[1] == 2 and HEAD.unpack_from(open(str(tmp_path / 'host') + lossless.SUFFIX, 'rb').read(), 0)[1] == 1
    # either object reads either form
    assert np.array_equal(_rows(lossless.LosslessCoder(model, str(tmp_path / 'device')).decode().C), want)
    assert np.array_equal(_rows(lossless.LosslessCoder(model, str(tmp_path / 'host'), occupancy_coder='device').decode().C), want)
    # the record keeps its keys and adds chunks; the length stays inside the bound
    assert set(host_record) | {'chunks'} == set(record) and 'chunks' not in host_record
    assert record['rows'] == host_record['rows'] and record['est_units_O'] == host_record['est_units_O']
    assert record['chunks'] == [rr.chunks_of(r, 16) for r in record['rows']]
    assert record['bits_O'] == 8 * os.path.getsize(str(tmp_path / 'device') + lossless.SUFFIX) == 8 * (HEAD.size + sum(record['payload_bytes']))
    # (the ideal of all levels together: length_bound is linear in it, so the sum over levels is the bound of the sums)
    bound = 8 * HEAD.size + rr.length_bound(record['est_bits_O'], sum(record['rows']), sum(record['chunks'])) + 64 * (lossless.LEVELS - 1)
    print(f"{name}: bits_O {record['bits_O']} (host coder {host_record['bits_O']}), ideal {record['est_bits_O']:.1f}, bound {bound:.1f}, "
          f"chunks {record['chunks']}")
    assert record['bits_O'] <= bound


def test_default_chunk_steps_and_one_chunk_per_level(model, tmp_path):
    x = _tensor(CLOUDS['sphere shell'])
    for steps, chunks in ((None, None), (0, [1, 1, 1])):
        coder = lossless.LosslessCoder(model, str(tmp_path / 'c'), occupancy_coder='device', chunk_steps=steps)
        record = coder.encode(x)
        assert record['chunks'] == (chunks or [rr.chunks_of(r, lossless.CHUNK_STEPS) for r in record['rows']])
        assert np.array_equal(_rows(coder.decode().C), _rows(x.C))


def test_saturated_logits_round_trip_in_device_mode(tmp_path, monkeypatch):
    """cls kernels x 1e3: contexts pile up at 0 and 352 and many confident predictions are wrong, 16 bits each"""
    seen, encode = [], ops.occ_rans_encode
    monkeypatch.setattr(ops, 'occ_rans_encode', lambda packed, steps, sums=None: seen.append(packed.cpu().numpy().view(np.uint16) >> 1) or
                        encode(packed, steps, sums))
    m = _model()
    with torch.no_grad():
        for l in range(3):
            getattr(m.decoder, f'conv{l}_cls').kernel.mul_(1e3)
    coder = lossless.LosslessCoder(m, str(tmp_path / 'sat'), occupancy_coder='device', chunk_steps=16)
    x = _tensor(CLOUDS['sphere shell'])
    record = coder.encode(x)
    ctx = np.concatenate(seen)
    assert len(ctx) == sum(record['rows']) and np.isin(ctx, (0, 2 * lr.QMAX)).mean() > 0.5
    assert np.array_equal(_rows(coder.decode().C), _rows(x.C))


def test_a_damaged_device_stream_is_refused(model, tmp_path):
    coder = lossless.LosslessCoder(model, str(tmp_path / 'dmg'), occupancy_coder='device', chunk_steps=16)
    x = _tensor(CLOUDS['sphere shell'])
    record = coder.encode(x)
    path = str(tmp_path / 'dmg') + lossless.SUFFIX
    good = open(path, 'rb').read()
    sizes = HEAD.unpack_from(good, 0)[3:]
    state_at = HEAD.size + sizes[1] + sizes[3] + 8 + 8 * 3                    # lane 3 of the last level's first chunk
    rows_off = list(sizes)
    rows_off[4] += 8
    for what, blob in {'a state below 2^31': good[:state_at] + struct.pack('<Q', 12345) + good[state_at + 8:],
                       'file cut by one word': good[:-4],
                       'declared rows off by 8': good[:12] + struct.pack('<6Q', *rows_off) + good[HEAD.size:],
                       'version 3': good[:4] + struct.pack('<I', 3) + good[8:]}.items():
        open(path, 'wb').write(blob)
        with pytest.raises(ops.PcgcError):
            coder.decode()
            pytest.fail(f'{what}: decoded')
    open(path, 'wb').write(good)
    assert np.array_equal(_rows(coder.decode().C), _rows(x.C)) and record['chunks'][2] > 1


def test_a_batch_is_still_refused_and_the_arguments_are_checked(model, tmp_path):
    a, b = CLOUDS['single voxel'], CLOUDS['one voxel per stride-8 cell']
    coords, feats = sparse_collate([torch.from_numpy(a), torch.from_numpy(b)], [torch.ones((len(a), 1)), torch.ones((len(b), 1))])
    batch = SparseTensor(feats, coordinates=coords, tensor_stride=1, device=DEV)
    coder = lossless.LosslessCoder(model, str(tmp_path / 'batch'), occupancy_coder='device')
    with pytest.raises(ValueError):
        coder.encode(batch)
    with pytest.raises(ValueError):
        lossless.LosslessCoder(model, str(tmp_path / 'x'), occupancy_coder='gpu')
    with pytest.raises(ValueError):
        lossless.LosslessCoder(model, str(tmp_path / 'x'), occupancy_coder='device', chunk_steps=-1)
