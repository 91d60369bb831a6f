"""The colour stream's device coder on the GPU (csrc/attribute_rans.hip, ops.attr_rans_*, AttributeCoder(attribute_coder='device')): the
payload bytes EQUAL to the definition (tests/attr_rans_reference.py) and the decoded tokens equal to the input at every edge of the
chunking; the f = 65536 and f = 1 rows; a chunk that refills the decoder's word ring four times; every damaged payload refused; `_A.bin`
version 2 equal to the definition's bytes and decoding to what version 1 decodes; recycled scratch; the command lines."""
import functools
import os
import struct
import types

import numpy as np
import pytest
import torch

import attr_rans_reference as ar
import raht_reference as R
import scratch_arena as SA
import test_attributes_device as AT            # (its geometries and colour kinds)
from pcgcv2_amd import attributes as at, ops, synthetic
from pcgcv2_amd._lib import PcgcError
from pcgcv2_amd.data_utils import read_ply_ascii_with_colours, write_ply_ascii_geo_rgb

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
RING_FILL = 512                                 # words the decoder stages at a time (AR_FILL in csrc/attribute_rans.hip)


def _np(t):
    return t.cpu().numpy()


def _dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16).copy()).to(DEV)


def _tree(bucket):
    """what ops.attr_rans_decode reads of a RahtTree: its 130 offsets on the device, the 65 bucket offsets first"""
    off = np.zeros(130, np.int32)
    off[:65] = bucket
    return types.SimpleNamespace(offsets=torch.from_numpy(off).to(DEV))


@functools.lru_cache(maxsize=None)
def _case(kind, n, S, seed=0):
    """(table, bucket, ctx, tokens, the definition's payload), computed once"""
    table, bucket, ctx, tokens = ar.improbable(n) if kind == 'improbable' else ar.model_drawn(n, seed)
    return table, bucket, ctx, tokens, ar.encode(table, ctx, tokens, S)


def _check(table, bucket, ctx, tokens, want, S):
    n = len(tokens)
    got = ops.attr_rans_encode(table, _dev16(ctx), _dev16(tokens), S)
    assert got == want, f'{n} tokens, S = {S}: {len(got)} bytes against the definition\'s {len(want)}'
    dec, n63 = ops.attr_rans_decode(table, _tree(bucket), got, n)
    assert dec.dtype == torch.int16 and np.array_equal(_np(dec), tokens), (n, S)
    assert n63 == int(np.count_nonzero(tokens == 63))


# ---- op level --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S', ar.STEPS)
def test_payload_equals_the_definition_at_every_edge_of_the_chunking(S):
    for n in ar.sizes(S):
        _check(*_case('drawn', n, S, seed=n), S)


def test_every_context_and_the_extreme_rows():
    table, bucket, ctx, tokens, want = _case('drawn', 20000, 16, seed=1)       # 20 chunks; rows with f = 65536, 65535 and 1 among the 48
    assert set(ctx.tolist()) == set(range(48))
    _check(table, bucket, ctx, tokens, want, 16)
    # split bit 0 alone: contexts 0, 16, 32; channel 0 is the row that token 63 owns, the others send their most frequent token
    freq = ar.mixed_table()[1]
    low = ar.spread_bucket(300, bits=[0])
    ctx0 = ar.bucket_contexts(low, 300)
    tok0 = np.where(ctx0 == 0, 63, np.argmax(freq, 1)[ctx0]).astype(np.int16)
    _check(table, low, ctx0, tok0, ar.encode(table, ctx0, tok0, 4), 4)


def test_a_chunk_that_refills_the_word_ring_more_than_once():
    n, S = 4096, 64                                                            # one chunk; f = 1 tokens cost 16 bits: about n / 2 words
    table, bucket, ctx, tokens, want = _case('improbable', n, S)
    words = struct.unpack_from('<I', want, 8 + 512)[0]
    assert struct.unpack_from('<II', want, 0) == (S, 1) and words > 3 * RING_FILL
    _check(table, bucket, ctx, tokens, want, S)
    _check(*_case('improbable', 2 * n + 77, S), S)                             # the same over three chunks


def test_no_token_is_an_empty_payload_without_a_launch():
    table, _ = ar.mixed_table()
    empty = torch.empty(0, dtype=torch.int16, device=DEV)
    assert ops.attr_rans_encode(table, empty, empty, 4096) == b''
    dec, n63 = ops.attr_rans_decode(table, _tree(np.zeros(65, np.int32)), b'', 0)
    assert dec.numel() == 0 and n63 == 0


def test_a_token_that_cannot_be_coded_is_reported():
    table, bucket, ctx, tokens, want = _case('drawn', 300, 4, seed=2)
    for c, a in ((0, 5), (1, 5), (2, 64), (48, 0), (2, -1)):                   # frequency 0 twice, then a token and a context outside their ranges
        bad_c, bad_t = ctx.copy(), tokens.copy()
        bad_c[150], bad_t[150] = c, a
        with pytest.raises(PcgcError, match='cannot be coded'):
            ops.attr_rans_encode(table, _dev16(bad_c), _dev16(bad_t), 4)
    assert ops.attr_rans_encode(table, _dev16(ctx), _dev16(tokens), 4) == want
    with pytest.raises(PcgcError):
        ops.attr_rans_encode(table, _dev16(ctx), _dev16(tokens), 0)
    with pytest.raises(PcgcError):
        ops.attr_rans_encode(table[:, :64], _dev16(ctx), _dev16(tokens), 4)


def test_undersized_scratch_is_refused_before_any_launch(monkeypatch):
    """the sizing call answers one byte less, the wrapper passes on what it was told: both entries refuse, nothing they were given is written"""
    table, bucket, ctx, tokens, want = _case('drawn', 300, 4, seed=2)
    true = ops.lib().pcgc_attr_rans_workspace_bytes
    assert int(true(300, 4)) >= 32 + 8 + 4 * 300
    monkeypatch.setattr(ops.lib(), 'pcgc_attr_rans_workspace_bytes', lambda *a: int(true(*a)) - 1)
    for call in (lambda: ops.attr_rans_encode(table, _dev16(ctx), _dev16(tokens), 4), lambda: ops.attr_rans_decode(table, _tree(bucket), want, 300)):
        arena = SA.Arena()
        with SA.installed(arena):
            with pytest.raises(PcgcError, match='too small'):
                call()
        arena.check()
        assert arena.blocks and not any(bool(b.payload().any()) for b in arena.blocks)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def test_every_damaged_payload_is_refused_and_the_sound_one_decodes_afterwards():
    table, bucket, ctx, tokens, S = ar.three_chunks()
    good = ar.encode(table, ctx, tokens, S)
    tree, n = _tree(bucket), len(tokens)
    assert ops.attr_rans_encode(table, _dev16(ctx), _dev16(tokens), S) == good
    damaged = ar.damaged(good)
    assert len(damaged) == 5
    for what, payload in damaged.items():
        with pytest.raises(PcgcError):
            ops.attr_rans_decode(table, tree, payload, n)
            pytest.fail(f'{what}: decoded')
    with pytest.raises(PcgcError, match='words in all'):                       # (a length that does not add up never reaches the device)
        ops.attr_rans_decode(table, tree, damaged['the last word dropped'], n)
    for what in ('one flipped bit in a middle word', 'W_1 plus one, a word inserted', 'W_1 minus one, its last word removed', 'a state replaced by L - 1'):
        with pytest.raises(PcgcError, match='unsound'):                        # (these pass the host's checks: the kernel's verdict)
            ops.attr_rans_decode(table, tree, damaged[what], n)
    dec, n63 = ops.attr_rans_decode(table, tree, good, n)
    assert np.array_equal(_np(dec), tokens) and n63 == int(np.count_nonzero(tokens == 63))


# ---- file level ------------------------------------------------------------------------------------------------------------------------------
QSTEPS = [(0, 0), (16, 4), (255, 16), (0, 255)]
FILE_GEOMETRY = {'one': 4096, 'two': 4096, 'chain': 1, f'line{AT.T + 1}': 16, 'random': 16}          # name -> chunk_steps


def _cloud(name):
    pts = np.asarray(AT.GEOMETRY[name](), np.int64)
    return pts[np.random.default_rng(len(pts)).permutation(len(pts))]


def _read(prefix):
    with open(prefix + at.SUFFIX, 'rb') as fh:
        return fh.read()


@pytest.mark.parametrize('name', sorted(FILE_GEOMETRY))
def test_file_equals_the_definition_and_decodes_to_what_version_1_decodes(name, tmp_path):
    pts, S = _cloud(name), FILE_GEOMETRY[name]
    coords = AT._coords(pts)
    for kind, (ql, qc) in (('random', QSTEPS[0]), ('random', QSTEPS[1]), ('alternating', QSTEPS[2]), ('random', QSTEPS[3])):
        rgb = AT._colours(kind, pts, 9)
        rgb_d = torch.from_numpy(rgb).to(DEV)
        blob, rec = ar.encode_v2(pts, rgb, ql, qc, S, ops.crc32)
        host = at.AttributeCoder(str(tmp_path / 'v1'))
        host.encode(coords, rgb_d, ql, qc)
        assert struct.unpack_from('<I', _read(str(tmp_path / 'v1')), 4)[0] == 1
        v1 = _np(host.decode(coords))
        assert np.array_equal(v1, rec)
        if (ql, qc) == (0, 0):
            assert np.array_equal(rec, rgb)                                    # Q = 0 returns the colours exactly
        for form in ops.RAHT_FORMS:
            prefix = str(tmp_path / f'{name}_{form}')
            coder = at.AttributeCoder(prefix, form=form, attribute_coder='device', chunk_steps=S)
            record = coder.encode(coords, rgb_d, ql, qc)
            assert _read(prefix) == blob, (kind, ql, qc, form)
            assert record['bits_A'] == 8 * len(blob)
            assert np.array_equal(_np(coder.decode(coords)), v1), (kind, ql, qc, form)
            assert np.array_equal(_np(at.AttributeCoder(prefix, form=form).decode(coords)), v1)                   # a host-mode object reads version 2
        assert np.array_equal(_np(at.AttributeCoder(str(tmp_path / 'v1'), attribute_coder='device').decode(coords)), v1)     # and the other way round
    if name == 'one':
        assert len(blob) == R.HEAD.size + R.SIZES.size + 4 and struct.unpack_from('<I', blob, 4)[0] == 2          # DC only, no payload


def test_chunk_steps(tmp_path):
    pts = _cloud('random')
    coords, rgb = AT._coords(pts), AT._colours('random', pts, 3)
    rgb_d = torch.from_numpy(rgb).to(DEV)
    n_tok = 3 * (len(pts) - 1)
    want = None
    for S in (4096, 0, 7):                                                     # the default, one chunk whatever the size, and 21 chunks
        prefix = str(tmp_path / f's{S}')
        coder = at.AttributeCoder(prefix, attribute_coder='device', chunk_steps=S) if S != 4096 else at.AttributeCoder(prefix, attribute_coder='device')
        coder.encode(coords, rgb_d, 8, 3)
        blob, rec = ar.encode_v2(pts, rgb, 8, 3, S, ops.crc32)
        assert _read(prefix) == blob
        rows = struct.unpack_from('<H', blob, 22)[0]
        assert struct.unpack_from('<II', blob, R.HEAD.size + 128 * rows + 24) == ((S, ar.chunks_of(n_tok, S)) if S else (-(-n_tok // 64), 1))
        dec = _np(coder.decode(coords))
        assert np.array_equal(dec, rec) and (want is None or np.array_equal(dec, want))
        want = dec
    for bad in (-1, (1 << 24) + 1, 2.5, None, True):
        with pytest.raises(ValueError, match='chunk_steps'):
            at.AttributeCoder(str(tmp_path / 'bad'), attribute_coder='device', chunk_steps=bad)
    with pytest.raises(ValueError, match='attribute_coder'):
        at.AttributeCoder(str(tmp_path / 'bad'), attribute_coder='gpu')


def test_row_order_and_repeatability(tmp_path):
    pts = _cloud('random')
    rgb = AT._colours('random', pts, 21)
    a = at.AttributeCoder(str(tmp_path / 'a'), attribute_coder='device', chunk_steps=16)
    a.encode(AT._coords(pts), torch.from_numpy(rgb).to(DEV), 4, 7)
    first = _read(str(tmp_path / 'a'))
    a.encode(AT._coords(pts), torch.from_numpy(rgb).to(DEV), 4, 7)
    assert _read(str(tmp_path / 'a')) == first                                 # two runs, the same bytes
    shuffle = np.random.default_rng(22).permutation(len(pts))
    b = at.AttributeCoder(str(tmp_path / 'b'), attribute_coder='device', chunk_steps=16)
    b.encode(AT._coords(pts[shuffle]), torch.from_numpy(rgb[shuffle]).to(DEV), 4, 7)
    assert _read(str(tmp_path / 'b')) == first                                 # shuffled rows, the same bytes
    dec = _np(a.decode(AT._coords(pts)))
    assert np.array_equal(_np(a.decode(AT._coords(pts[shuffle]))), dec[shuffle])


def test_a_flipped_byte_anywhere_is_refused_by_the_crc(tmp_path):
    pts = _cloud('chain')
    coords, rgb = AT._coords(pts), torch.from_numpy(AT._colours('random', pts, 5)).to(DEV)
    prefix = str(tmp_path / 'c')
    coder = at.AttributeCoder(prefix, attribute_coder='device', chunk_steps=1)
    tree = coder.encode(coords, rgb, 2, 5)['tree']
    good = _read(prefix)
    want = _np(coder.decode(coords, tree=tree))
    for i in range(len(good)):
        with open(prefix + at.SUFFIX, 'wb') as fh:
            fh.write(good[:i] + bytes([good[i] ^ 0x01]) + good[i + 1:])
        with pytest.raises(PcgcError, match=None if i < 8 else 'CRC'):         # (magic and version are looked at before the CRC)
            coder.decode(coords, tree=tree)
            pytest.fail(f'byte {i} flipped: decoded')
    with open(prefix + at.SUFFIX, 'wb') as fh:
        fh.write(good)
    assert np.array_equal(_np(coder.decode(coords, tree=tree)), want)


def test_damage_behind_a_fitting_crc_is_refused_before_the_dequantiser(tmp_path):
    """a file whose CRC was made to fit: a payload word, an escape count and a CDF row each meet their own check"""
    pts = _cloud('random')
    coords, rgb = AT._coords(pts), torch.from_numpy(AT._colours('alternating', pts, 5)).to(DEV)
    prefix = str(tmp_path / 'd')
    coder = at.AttributeCoder(prefix, attribute_coder='device', chunk_steps=16)
    record = coder.encode(coords, rgb, 0, 0)
    good = _read(prefix)
    rows = struct.unpack_from('<H', good, 22)[0]
    sizes_at = R.HEAD.size + 128 * rows
    n_tok, n_pay, n_esc = R.SIZES.unpack_from(good, sizes_at)
    assert n_esc > 0 and n_pay == record['payload_bytes']

    def refused(blob, match):
        with open(prefix + at.SUFFIX, 'wb') as fh:
            fh.write(blob[:-4] + struct.pack('<I', ops.crc32(blob[:-4])))
        with pytest.raises(PcgcError, match=match):
            coder.decode(coords, tree=record['tree'])

    word = sizes_at + 24 + n_pay - 6
    refused(good[:word] + bytes([good[word] ^ 0x40]) + good[word + 1:], 'unsound|escape')
    refused(good[:sizes_at + 24] + struct.pack('<I', 0) + good[sizes_at + 28:], 'steps per chunk')
    cdfs = [np.frombuffer(good, '<u2', 63, R.HEAD.size + 128 * r + 2).astype(np.int64) for r in range(rows)]
    r = next(r for r in range(rows) if (np.diff(cdfs[r]) > 0).any())             # (a row that one token owns has no step to undo)
    cdf = cdfs[r]
    j = int(np.flatnonzero(np.diff(cdf) > 0)[0])
    at_j = R.HEAD.size + 128 * r + 2 + 2 * j
    refused(good[:at_j] + struct.pack('<H', int(cdf[j + 1]) + 1) + good[at_j + 2:], 'monotone')
    # one escape less, the list cut to fit: the count disagrees with the escape tokens the kernel counted
    fewer = good[:sizes_at + 16] + struct.pack('<Q', n_esc - 1) + good[sizes_at + 24:sizes_at + 24 + n_pay] + at._pack_escapes(np.zeros(n_esc - 1, np.uint16)) + good[-4:]
    refused(fewer, 'escape')
    with open(prefix + at.SUFFIX, 'wb') as fh:
        fh.write(good)
    assert np.array_equal(_np(coder.decode(coords)), _np(rgb))


# ---- scratch state ---------------------------------------------------------------------------------------------------------------------------
def test_encode_and_decode_on_recycled_scratch(tmp_path):
    """fresh memory, then the memory a sibling input of the same shape left behind: guards intact, bytes and colours unchanged"""
    pts = _cloud('random')

    def make(seed):
        rng = np.random.default_rng(seed)
        moved = pts + 64 * rng.integers(1, 40, 3)
        return AT._coords(moved[rng.permutation(len(moved))]), torch.from_numpy(AT._colours('random', pts, seed)).to(DEV)

    def fn(inp):
        coords, rgb = inp
        coder = at.AttributeCoder(str(tmp_path / 'arena'), attribute_coder='device', chunk_steps=16)
        coder.encode(coords, rgb, 4, 9)
        return np.frombuffer(_read(str(tmp_path / 'arena')), np.uint8).copy(), _np(coder.decode(coords))

    def run(arena, inp):
        with SA.installed(arena):
            out = fn(inp)
        torch.cuda.synchronize()
        arena.finish()
        arena.check()
        return out

    A, B = make(80), make(81)
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
    assert struct.unpack_from('<I', want[0].tobytes(), 4)[0] == 2


# ---- command lines ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def coloured_cloud(tmp_path_factory):
    d = tmp_path_factory.mktemp('attr_rans_e2e')
    pts = synthetic.shell('shell7').numpy()
    t = np.asarray(pts, np.float64) / 128
    rgb = np.clip(np.rint(np.stack([255 * t[:, 0], 127.5 * (1 + np.sin(5 * t[:, 1])), 255 * t[:, 2] * t[:, 0]], 1)), 0, 255).astype(np.uint8)
    ply = d / 'shell7c.ply'
    write_ply_ascii_geo_rgb(str(ply), pts, rgb)
    ckpt = d / 'r.pth'
    torch.save({'model': synthetic.synthetic_state_dict(gain=50.0)}, str(ckpt))
    return d, str(ply), pts, rgb, str(ckpt)


def test_attributes_cli(coloured_cloud, capsys):
    d, ply, pts, rgb, ckpt = coloured_cloud
    at.main(['--filedir', ply, '--qstep', '8', '--outdir', str(d / 'host')])
    capsys.readouterr()
    at.main(['--filedir', ply, '--qstep', '8', '--outdir', str(d / 'dev'), '--attribute_coder', 'device', '--chunk_steps', '64'])
    out = capsys.readouterr().out
    line, = [l for l in out.splitlines() if l.startswith(at.SUFFIX)]
    blob = _read(str(d / 'dev' / 'shell7c'))
    assert int(line.split('\t')[1].split()[0]) == 8 * len(blob) and struct.unpack_from('<I', blob, 4)[0] == 2
    rows = struct.unpack_from('<H', blob, 22)[0]
    assert struct.unpack_from('<I', blob, R.HEAD.size + 128 * rows + 24)[0] == 64
    xyz, got = read_ply_ascii_with_colours(str(d / 'dev' / 'shell7c_dec.ply'))
    _, host = read_ply_ascii_with_colours(str(d / 'host' / 'shell7c_dec.ply'))
    assert got is not None and np.array_equal(got, host)                       # the colours version 1 decodes
    again = at.AttributeCoder(str(d / 'dev' / 'shell7c')).decode(AT._coords(xyz.astype(np.int64)))
    assert np.array_equal(_np(again), got)


def test_coder_attributes_cli(coloured_cloud, capsys):
    from pcgcv2_amd import coder
    d, ply, pts, rgb, ckpt = coloured_cloud
    coder.main(['--ckptdir', ckpt, '--filedir', ply, '--outdir', str(d / 'lossy'), '--res', '128', '--attributes', '8', '--attribute_coder', 'device'])
    out = capsys.readouterr().out
    bits = AT._printed(out, 'bits _A.bin')
    blob = _read(str(d / 'lossy' / 'shell7c'))
    assert len(bits) == 1 and int(bits[0]) == 8 * len(blob) and struct.unpack_from('<I', blob, 4)[0] == 2
    psnr = AT._printed(out, 'Colour PSNR (Y)')
    assert len(psnr) == 1 and np.isfinite(float(psnr[0]))
    xyz, got = read_ply_ascii_with_colours(str(d / 'lossy' / 'shell7c_dec.ply'))
    assert got is not None and got.shape == (len(xyz), 3)
    again = at.AttributeCoder(str(d / 'lossy' / 'shell7c')).decode(AT._coords(xyz.astype(np.int64)))
    assert np.array_equal(_np(again), got)


def test_lossless_attributes_zero_with_the_device_coder_returns_the_colours(coloured_cloud, capsys):
    from pcgcv2_amd import coder
    d, ply, pts, rgb, ckpt = coloured_cloud
    coder.main(['--ckptdir', ckpt, '--filedir', ply, '--outdir', str(d / 'exact'), '--lossless', '--attributes', '0', '--attribute_coder', 'device'])
    out = capsys.readouterr().out
    assert AT._printed(out, 'Colour PSNR (Y)') == ['inf']
    assert struct.unpack_from('<I', _read(str(d / 'exact' / 'shell7c')), 4)[0] == 2
    xyz, got = read_ply_ascii_with_colours(str(d / 'exact' / 'shell7c_dec.ply'))
    a = np.concatenate([xyz.astype(np.int64), got], 1)
    b = np.concatenate([np.asarray(pts, np.int64), rgb], 1)
    assert np.array_equal(a[np.lexsort(a.T[::-1])], b[np.lexsort(b.T[::-1])])
