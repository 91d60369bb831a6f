"""CPU tests of the lossless mode's format constants (pcgcv2_amd/occupancy_model.py), its context definition (tests/lossless_reference.py)
and its host coder (pcgc_rc_encode_ctx / pcgc_rc_decode_ctx of csrc/hostcodec.cpp)."""
import os
import sys

import numpy as np
import pytest

import lossless_reference as lr
from pcgcv2_amd import occupancy_model as om, ops

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))

R, LP = om.CONTEXTS, 3
CDF = om.cdf_rows()
CYCLIC_N = (0, 1, 7, 65537)


# ---- tables ---------------------------------------------------------------------------------------------------------------------------------
def test_committed_tables_are_the_generators():
    import make_occupancy_tables as gen
    p1, cost = gen.tables()
    assert list(om.P1) == p1
    assert om.cost().tolist() == cost
    assert om.TABLE_CRC == gen.table_crc(p1, cost) == om.table_crc()


def test_library_tables_are_the_committed_ones():
    p1, cost = ops.occ_tables()
    assert np.array_equal(p1, om.p1()) and np.array_equal(cost, om.cost())


def test_p1_symmetric_bounded_monotone():
    p = om.p1().astype(np.int64)
    assert len(p) == R == 353
    assert p.min() >= 1 and p.max() <= 65535
    assert np.array_equal(p + p[::-1], np.full(R, 65536))       # P1[-q] = 65536 - P1[q], exactly
    assert p[lr.QMAX] == 32768
    assert np.all(np.diff(p) >= 0) and np.all(np.diff(p)[100:253] > 0)


def test_cost_is_minus_log2_to_the_stated_rounding():
    import mpmath
    mpmath.mp.dps = 50
    p, cost = om.p1().astype(np.int64), om.cost()
    for ctx in range(R):
        for bit, v in ((0, 65536 - p[ctx]), (1, p[ctx])):
            exact = 65536 * -mpmath.log(mpmath.mpf(int(v)) / 65536, 2)
            assert abs(int(cost[ctx, bit]) - exact) <= 0.5
    assert cost.min() >= 1 and cost.max() == 16 * 65536


def test_cdf_rows_follow_the_coder_convention():
    assert CDF.dtype == np.uint16 and CDF.shape == (R, LP)
    assert np.all(CDF[:, 0] == 0) and np.all(CDF[:, 2] == 0)
    assert np.array_equal(CDF[:, 1].astype(np.int64), 65536 - om.p1().astype(np.int64))


# ---- context definition ---------------------------------------------------------------------------------------------------------------------
def test_context_of_special_logits():
    z, q = lr.special_logits()
    assert np.array_equal(lr.context(z).astype(np.int64), q + lr.QMAX)


def test_context_is_monotone_and_covers_every_row():
    z = np.linspace(-12, 12, 200001).astype(np.float32)
    ctx = lr.context(z).astype(np.int64)
    assert np.all(np.diff(ctx) >= 0) and set(ctx.tolist()) == set(range(R))


# ---- host coder -----------------------------------------------------------------------------------------------------------------------------
def _ideal_bits(ctx, sym):
    return float(om.cost()[np.asarray(ctx, np.int64), np.asarray(sym, np.int64)].astype(np.int64).sum()) / om.COST_UNIT


def _cyclic(n):
    return (np.arange(n) % R).astype(np.uint16), np.random.default_rng(0).integers(0, 2, n).astype(np.int16)


@pytest.mark.parametrize('n', CYCLIC_N)
def test_cyclic_contexts_give_the_channel_coders_bytes(n):
    ctx, sym = _cyclic(n)
    stream = ops.rc_encode_ctx(CDF, ctx, sym)
    assert stream == ops.rc_encode(CDF, sym)
    assert np.array_equal(ops.rc_decode_ctx(CDF, ctx, stream), sym)
    if n:
        assert np.array_equal(ops.rc_decode(CDF, stream, n), sym)


def test_cyclic_excess_is_the_recorded_one():
    """the yardstick of lr.length_bound: the parent coder's excess over the ideal, per symbol, on the cyclic-context input"""
    n = 65537
    ctx, sym = _cyclic(n)
    excess = (8 * len(ops.rc_encode(CDF, sym)) - _ideal_bits(ctx, sym)) / n
    print(f'pcgc_rc_encode, cyclic contexts, n = {n}: {excess * n:.3f} bits over the ideal, {excess:.3e} per symbol')
    assert 0 <= excess <= lr.MEASURED_EXCESS_PER_SYMBOL


def _model_symbols(ctx, rng):
    return (rng.random(len(ctx)) < om.p1()[ctx] / 65536.0).astype(np.int16)


@pytest.mark.parametrize('name', ['random contexts', 'extreme contexts, improbable bit', 'single context', 'random contexts, random bits'])
def test_round_trip_and_length(name):
    rng = np.random.default_rng(11)
    n = 200003
    if name == 'random contexts':
        ctx = rng.integers(0, R, n).astype(np.uint16)
        sym = _model_symbols(ctx, rng)
    elif name == 'extreme contexts, improbable bit':
        n = 5000
        ctx = np.where(rng.random(n) < 0.5, 0, R - 1).astype(np.uint16)
        sym = (ctx == 0).astype(np.int16)                        # occupied under P1 = 1 / 65536, empty under 65535 / 65536: 16 bits each
    elif name == 'single context':
        ctx = np.full(n, 200, dtype=np.uint16)
        sym = _model_symbols(ctx, rng)
    else:
        ctx = rng.integers(0, R, n).astype(np.uint16)
        sym = rng.integers(0, 2, n).astype(np.int16)
    stream = ops.rc_encode_ctx(CDF, ctx, sym)
    assert np.array_equal(ops.rc_decode_ctx(CDF, ctx, stream), sym)
    ideal = _ideal_bits(ctx, sym)
    print(f'{name}: n = {n}, ideal {ideal:.1f} bits, stream {8 * len(stream)} bits')
    assert 8 * len(stream) <= lr.length_bound(ideal, n)
    assert 8 * len(stream) >= ideal - 1e-4 * n - 8             # (nor can a sound stream be shorter than the ideal: COST's own rounding aside)


def test_every_truncation_and_a_trailing_byte_are_refused():
    rng = np.random.default_rng(5)
    n = 300
    ctx = rng.integers(120, 233, n).astype(np.uint16)
    sym = _model_symbols(ctx, rng)
    stream = ops.rc_encode_ctx(CDF, ctx, sym)
    assert len(stream) > 8
    assert np.array_equal(ops.rc_decode_ctx(CDF, ctx, stream), sym)
    for k in range(len(stream)):
        with pytest.raises(ops.PcgcError):
            ops.rc_decode_ctx(CDF, ctx, stream[:k])
    for tail in (b'\x00', b'\xff', b'\x00\x00\x00\x00\x00\x00\x00\x00\x00'):
        with pytest.raises(ops.PcgcError):
            ops.rc_decode_ctx(CDF, ctx, stream + tail)


def test_a_flipped_bit_is_refused_or_decodes_other_symbols():
    rng = np.random.default_rng(6)
    n = 2000
    ctx = rng.integers(0, R, n).astype(np.uint16)
    sym = _model_symbols(ctx, rng)
    stream = bytearray(ops.rc_encode_ctx(CDF, ctx, sym))
    for at in (0, len(stream) // 2, len(stream) - 1):
        bad = bytearray(stream)
        bad[at] ^= 0x10
        try:
            got = ops.rc_decode_ctx(CDF, ctx, bytes(bad))
        except ops.PcgcError:
            continue
        assert not np.array_equal(got, sym)


def test_bad_arguments_are_refused():
    with pytest.raises(ops.PcgcError):
        ops.rc_encode_ctx(CDF, np.array([R], np.uint16), np.array([0], np.int16))          # context outside the table
    with pytest.raises(ops.PcgcError):
        ops.rc_encode_ctx(CDF, np.array([0], np.uint16), np.array([2], np.int16))          # symbol outside the row
    with pytest.raises(ops.PcgcError):
        ops.rc_encode_ctx(CDF, np.array([0, 1], np.uint16), np.array([0], np.int16))
    with pytest.raises(ops.PcgcError):
        ops.rc_decode_ctx(CDF, np.array([R], np.uint16), b'\x40')
    assert ops.rc_decode_ctx(CDF, np.zeros(0, np.uint16), ops.rc_encode_ctx(CDF, np.zeros(0, np.uint16), np.zeros(0, np.int16))).size == 0
    with pytest.raises(ops.PcgcError):
        ops.rc_decode_ctx(CDF, np.zeros(0, np.uint16), b'')                                # even no symbols have a (one-byte) stream


# ---- the stream header (no GPU needed: the reader refuses before anything is decoded) --------------------------------------------------------
def test_occupancy_stream_header_checks(tmp_path):
    import struct
    from pcgcv2_amd import lossless
    lc = lossless.LosslessCoder.__new__(lossless.LosslessCoder)
    lc.filename = str(tmp_path / 'f')
    good = struct.pack('<4sII', b'PCGL', 1, om.table_crc()) + struct.pack('<6Q', 8, 1, 16, 1, 24, 2) + b'\x40\x40\x40\x40'
    (tmp_path / 'f_O.bin').write_bytes(good)
    rows, payloads = lc._read_stream('')
    assert rows == (8, 16, 24) and [len(p) for p in payloads] == [1, 1, 2]
    for bad in (b'PCGX' + good[4:], good[:4] + struct.pack('<I', 2) + good[8:], good[:8] + struct.pack('<I', om.table_crc() ^ 1) + good[12:],
                good[:-1], good + b'\x00', good[:20]):
        (tmp_path / 'f_O.bin').write_bytes(bad)
        with pytest.raises(ops.PcgcError):
            lc._read_stream('')
