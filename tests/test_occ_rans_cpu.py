"""The device coder of the occupancy stream (`_O.bin` version 2) as tests/rans_reference.py defines it, in plain Python integers: it round-trips,
every lane ends at L, its length stays inside the recorded bound, its parser refuses inconsistent payloads, and it refuses every damaged
payload the device test (test_occ_rans_device.py) hands to the kernel — so that test asks the kernel only for the definition's verdict."""
import struct

import numpy as np
import pytest

import rans_reference as rr
from pcgcv2_amd import occupancy_model as om

CASES = {
    'cyclic, one lane': (rr.cyclic(1), 4),
    'cyclic, 63 rows': (rr.cyclic(63), 1),
    'cyclic, three chunks and a tail': (rr.cyclic(3 * 64 * 4 + 17), 4),
    'cyclic, S = 1': (rr.cyclic(200), 1),
    'model-drawn': (rr.model_drawn(5003, seed=1), 16),
    'improbable everywhere': (rr.extreme(64 * 4 + 5, True), 4),
    'probable everywhere': (rr.extreme(64 * 4 + 5, False), 4),
    'only lane 0 improbable': (rr.extreme(64 * 16, False, lanes=(0,)), 16),
    'only lane 63 improbable': (rr.extreme(64 * 16, False, lanes=(63,)), 16),
    'alternating lanes improbable': (rr.extreme(64 * 16, False, lanes=range(0, 64, 2)), 16),
}


@pytest.mark.parametrize('name', list(CASES))
def test_definition_round_trips_and_every_lane_ends_at_L(name):
    (ctx, bit), S = CASES[name]
    payload = rr.encode(ctx, bit, S)
    assert np.array_equal(rr.decode(ctx, payload), bit)       # (decode raises unless every lane ends at L and W_k words were consumed)
    got_S, chunks = rr.parse(payload, len(ctx))
    assert got_S == S and len(chunks) == rr.chunks_of(len(ctx), S)
    assert 8 * len(payload) <= rr.length_bound(rr.ideal_bits(ctx, bit), len(ctx), len(chunks))


def test_empty_input_is_a_head_alone():
    payload = rr.encode([], [], 7)
    assert payload == struct.pack('<II', 7, 0)
    assert len(rr.decode([], payload)) == 0


def test_no_lane_emits_under_probable_bits_and_every_lane_under_improbable_ones():
    ctx, bit = rr.extreme(64 * 8, False)
    assert [len(w) for _, w in rr.encode_chunks(ctx, bit, 8)] == [0]
    ctx, bit = rr.extreme(64 * 8, True)                        # 16 bits a row: a lane emits at every second row
    (states, words), = rr.encode_chunks(ctx, bit, 8)
    assert len(words) == 64 * 8 // 2 and all(v >> 31 == 1 for v in states)


def test_recorded_excess_is_reproduced():
    ctx, bit = rr.cyclic(65537, seed=0)
    payload = rr.encode(ctx, bit, 4096)
    chunks = rr.chunks_of(65537, 4096)
    excess = 8 * len(payload) - rr.ideal_bits(ctx, bit) - chunks * (64 * 64 + 32) - 64
    print(f'excess beyond the states, counts and head: {excess:.4f} bits over 65 537 symbols in {chunks} chunk')
    assert abs(excess - rr.MEASURED_EXCESS_BITS) < 1e-3
    assert rr.EPS == (2 * rr.MEASURED_EXCESS_BITS / 65537 if rr.MEASURED_EXCESS_BITS > 0 else 1e-6)


@pytest.mark.parametrize('make, S', [(lambda: rr.cyclic(65537, seed=0), 4096), (lambda: rr.cyclic(65537, seed=0), 64),
                                     (lambda: rr.model_drawn(200003, seed=2), 4096), (lambda: rr.extreme(5000, True), 16)],
                         ids=['cyclic', 'cyclic in 16 chunks', 'model-drawn', 'all improbable'])
def test_length_bound_holds(make, S):
    ctx, bit = make()
    payload = rr.encode(ctx, bit, S)
    ideal, chunks = rr.ideal_bits(ctx, bit), rr.chunks_of(len(ctx), S)
    print(f'{8 * len(payload)} bits against an ideal of {ideal:.1f} in {chunks} chunks; bound {rr.length_bound(ideal, len(ctx), chunks):.1f}')
    assert 8 * len(payload) <= rr.length_bound(ideal, len(ctx), chunks)
    assert 8 * len(payload) >= ideal                          # (the states alone carry at least 31 bits each)


def _sound():
    ctx, bit, S = rr.three_chunks()
    return ctx, bit, S, rr.encode(ctx, bit, S)


def test_parser_refuses_inconsistent_payloads():
    ctx, bit, S, good = _sound()
    n, K = len(ctx), 3
    rr.parse(good, n)
    states_at, counts_at = 8, 8 + 512 * K
    bad = {
        'wrong K': struct.pack('<II', S, K + 1) + good[8:],
        'S = 0': struct.pack('<II', 0, K) + good[8:],
        'sum(W_k) against the byte length': good[:counts_at] + struct.pack('<I', struct.unpack_from('<I', good, counts_at)[0] + 1) + good[counts_at + 4:],
        'a state below 2^31': good[:states_at + 8 * 5] + struct.pack('<Q', (1 << 31) - 1) + good[states_at + 8 * 6:],
        'a state at 2^63': good[:states_at + 8 * 5] + struct.pack('<Q', 1 << 63) + good[states_at + 8 * 6:],
    }
    for what, payload in bad.items():
        assert len(payload) == len(good), what
        with pytest.raises(rr.Unsound):
            rr.parse(payload, n)
            pytest.fail(f'{what}: parsed')


def test_definition_refuses_the_damaged_payloads_of_the_device_test():
    ctx, bit, S, good = _sound()
    assert np.array_equal(rr.decode(ctx, good), bit)
    damaged = rr.damaged(good)
    assert len(damaged) == 5
    for what, payload in damaged.items():
        with pytest.raises(rr.Unsound):
            rr.decode(ctx, payload)
            pytest.fail(f'{what}: decoded')
    assert np.array_equal(rr.decode(ctx, good), bit)


def test_tables_are_the_format_s():
    assert rr._P1 == [int(v) for v in om.p1()] and min(rr._P1) == 1 and max(rr._P1) == 65535
