"""The colour stream's device coder as a definition (tests/attr_rans_reference.py): plain Python integers, no GPU.  What is shown here is
what the device test then demands of the kernels byte for byte: the arithmetic round-trips at every edge of the chunking, a token that owns
its row (f = 65536) and one at f = 1 are coded, a token of frequency 0 is refused, the states stay in [2^31, 2^63), the length stays within
its bound, and every damaged payload is refused.  Also the host's own layout checks (ops.attr_rans_layout), which run before any launch."""
import struct

import numpy as np
import pytest

import attr_rans_reference as ar
import raht_reference as R
from pcgcv2_amd import ops
from pcgcv2_amd._lib import PcgcError


@pytest.mark.parametrize('S', ar.STEPS)
def test_definition_round_trips_at_every_edge_of_the_chunking(S):
    for n in ar.sizes(S):
        table, bucket, ctx, tokens = ar.model_drawn(n, seed=n)
        payload = ar.encode(table, ctx, tokens, S)
        _, chunks = ar.parse(payload, n)
        assert len(chunks) == ar.chunks_of(n, S)
        for states, _ in chunks:
            assert all(ar.L <= v < ar.STATE_END for v in states)
        assert np.array_equal(ar.decode(table, ctx, payload), tokens), (S, n)


def test_every_context_and_both_extreme_rows_are_coded():
    table, bucket, ctx, tokens = ar.model_drawn(20000, seed=1)
    assert set(ctx.tolist()) == set(range(ar.CONTEXTS))
    cdf = ar.cdf_rows(table)
    freq = {cdf[int(c)][int(a) + 1] - cdf[int(c)][int(a)] for c, a in zip(ctx, tokens)}
    assert {65536, 65535}.issubset(freq) and min(freq) >= 1
    payload = ar.encode(table, ctx, tokens, 16)
    assert np.array_equal(ar.decode(table, ctx, payload), tokens)
    # f = 1 next to f = 65535 (sixteen bits a token: a lane emits at every second one), then a row owned by one token (nothing emitted)
    table, bucket, ctx, tokens = ar.improbable(64 * 8)
    (states, words), = ar.encode_chunks(table, ctx, tokens, 8)
    assert all(ar.L <= v < ar.STATE_END for v in states) and 64 * 8 * 3 // 8 <= len(words) <= 64 * 8 // 2
    assert np.array_equal(ar.decode(table, ctx, ar.pack(8, [(states, words)])), tokens)
    owned = np.full(64 * 8, 63, np.int16)
    (states, words), = ar.encode_chunks(table, np.zeros(64 * 8, np.uint16), owned, 8)
    assert words == [] and states == [ar.L] * 64
    assert np.array_equal(ar.decode(table, np.zeros(64 * 8, np.uint16), ar.pack(8, [(states, words)])), owned)


def test_no_token_is_an_empty_payload():
    table, _ = ar.mixed_table()
    assert ar.encode(table, np.zeros(0, np.uint16), np.zeros(0, np.int16), 4096) == b''
    assert ar.decode(table, np.zeros(0, np.uint16), b'').size == 0
    with pytest.raises(ar.Unsound):
        ar.decode(table, np.zeros(0, np.uint16), b'\0' * 8)


def test_a_token_without_frequency_is_refused_by_the_encoder():
    table, bucket, ctx, tokens = ar.model_drawn(300, seed=2)
    ar.encode(table, ctx, tokens, 4)
    for c, a in ((0, 5), (1, 5), (2, 64), (48, 0), (2, -1)):          # frequency 0 twice, then a token and a context outside their ranges
        bad_c, bad_t = ctx.copy(), tokens.copy()
        bad_c[150], bad_t[150] = c, a
        with pytest.raises(ValueError, match='no frequency'):
            ar.encode(table, bad_c, bad_t, 4)


def test_recorded_excess_is_reproduced():
    table, bucket, ctx, tokens = ar.model_drawn(65537, seed=0)
    payload = ar.encode(table, ctx, tokens, 4096)
    chunks = ar.chunks_of(65537, 4096)
    excess = 8 * len(payload) - ar.ideal_bits(table, ctx, tokens) - chunks * (64 * 64 + 32) - 64
    print(f'excess beyond the states, counts and head: {excess:.4f} bits over 65 537 tokens in {chunks} chunk')
    assert abs(excess - ar.MEASURED_EXCESS_BITS) < 1e-3
    assert ar.EPS == (2 * ar.MEASURED_EXCESS_BITS / 65537 if ar.MEASURED_EXCESS_BITS > 0 else 1e-6)


@pytest.mark.parametrize('make, S', [(lambda: ar.model_drawn(65537, seed=0), 4096), (lambda: ar.model_drawn(65537, seed=0), 64),
                                     (lambda: ar.model_drawn(20000, seed=3), 128), (lambda: ar.improbable(5000), 16)],
                         ids=['one chunk', '16 chunks', 'three chunks, the last partial', 'all improbable'])
def test_length_bound_holds(make, S):
    table, bucket, ctx, tokens = make()
    payload = ar.encode(table, ctx, tokens, S)
    ideal, chunks = ar.ideal_bits(table, ctx, tokens), ar.chunks_of(len(ctx), S)
    print(f'{8 * len(payload)} bits against an ideal of {ideal:.1f} in {chunks} chunks; bound {ar.length_bound(ideal, len(ctx), chunks):.1f}')
    assert 8 * len(payload) <= ar.length_bound(ideal, len(ctx), chunks)
    assert 8 * len(payload) >= ideal                          # (the states alone carry at least 31 bits each)


def _sound():
    table, bucket, ctx, tokens, S = ar.three_chunks()
    return table, ctx, tokens, S, ar.encode(table, ctx, tokens, S)


def _inconsistent(good, S, K):
    states_at, counts_at = 8, 8 + 512 * K
    return {
        'S = 0': struct.pack('<II', 0, K) + good[8:],
        'wrong K': struct.pack('<II', S, K + 1) + good[8:],
        'cut inside the tables': good[:counts_at + 4],
        'sum(W_k) against the byte length': good[:counts_at] + struct.pack('<I', struct.unpack_from('<I', good, counts_at)[0] + 1) + good[counts_at + 4:],
        'a state below 2^31': good[:states_at + 8 * 5] + struct.pack('<Q', (1 << 31) - 1) + good[states_at + 8 * 6:],
        'a state at 2^63': good[:states_at + 8 * 5] + struct.pack('<Q', 1 << 63) + good[states_at + 8 * 6:],
    }


def test_parser_refuses_inconsistent_payloads():
    table, ctx, tokens, S, good = _sound()
    ar.parse(good, len(ctx))
    for what, payload in _inconsistent(good, S, 3).items():
        with pytest.raises(ar.Unsound):
            ar.parse(payload, len(ctx))
            pytest.fail(f'{what}: parsed')
    for what, payload in ar.damaged(good).items():
        if len(payload) != len(good) or what.startswith('a state'):          # (the others are the decoder's to refuse)
            continue
        ar.parse(payload, len(ctx))


def test_definition_refuses_the_damaged_payloads_of_the_device_test():
    table, ctx, tokens, S, good = _sound()
    assert np.array_equal(ar.decode(table, ctx, good), tokens)
    damaged = ar.damaged(good)
    assert len(damaged) == 5
    for what, payload in damaged.items():
        with pytest.raises(ar.Unsound):
            ar.decode(table, ctx, payload)
            pytest.fail(f'{what}: decoded')
    assert np.array_equal(ar.decode(table, ctx, good), tokens)


def test_layout_checks_of_the_host_refuse_before_any_launch():
    """ops.attr_rans_layout reads bytes only: S = 0, a wrong K, a cut inside the tables, word counts that do not add up"""
    table, ctx, tokens, S, good = _sound()
    n = len(ctx)
    assert ops.attr_rans_layout(good, n) == (S, 3) and ops.attr_rans_chunks(n, S) == 3
    bad = _inconsistent(good, S, 3)
    for what, match in (('S = 0', 'steps per chunk'), ('wrong K', 'chunks declared'), ('cut inside the tables', 'cut inside'),
                        ('sum(W_k) against the byte length', 'words in all')):
        with pytest.raises(PcgcError, match=match):
            ops.attr_rans_layout(bad[what], n)
    with pytest.raises(PcgcError, match='words in all'):
        ops.attr_rans_layout(good[:-4], n)
    with pytest.raises(PcgcError, match='steps per chunk'):
        ops.attr_rans_layout(struct.pack('<II', (1 << 24) + 1, 1) + good[8:], n)
    with pytest.raises(PcgcError, match='shorter'):
        ops.attr_rans_layout(good[:7], n)
    assert ops.attr_rans_layout(b'', 0) == (0, 0)
    with pytest.raises(PcgcError, match='without tokens'):
        ops.attr_rans_layout(good, 0)


def test_bucket_contexts_are_the_tree_s():
    """the inputs' contexts are what a tree with these bucket offsets gives (raht_reference.tokens' ctx), cut to n tokens"""
    pts = np.unique(np.random.default_rng(0).integers(0, 32, (400, 3)), axis=0)
    keys, _ = R.sort_cloud(pts)
    tree = R.build_tree(keys)
    _, ctx, _, _ = R.tokens(tree, np.zeros((len(keys) - 1, 3), np.int64))
    assert np.array_equal(ar.bucket_contexts(tree['bucket'], ctx.size), ctx) and np.array_equal(ar.bucket_contexts(tree['bucket'], 100), ctx[:100])
    for n in (1, 63, 64, 200):
        b = ar.spread_bucket(n)
        assert b[0] == 0 and b[-1] == -(-n // 3) and (np.diff(b) >= 0).all() and ar.bucket_contexts(b, n).size == n


def test_whole_file_round_trips_and_differs_from_version_1_in_version_and_payload_alone():
    rng = np.random.default_rng(7)
    pts = np.unique(rng.integers(0, 24, (300, 3)), axis=0)
    rgb = rng.integers(0, 256, (len(pts), 3)).astype(np.uint8)
    for ql, qc, S in ((0, 0, 4096), (16, 4, 2), (255, 16, 0)):
        blob, rec = ar.encode_v2(pts, rgb, ql, qc, S, ops.crc32)
        assert np.array_equal(ar.decode_v2(pts, blob, ops.crc32), rec)
        if ql == 0:
            assert np.array_equal(rec, rgb)
        v1, rec1 = R.encode(pts, rgb, ql, qc, lambda table, ctx, tok: b'', ops.crc32)          # version 1 around an empty payload
        assert np.array_equal(rec1, rec)
        rows = struct.unpack_from('<H', blob, 22)[0]
        sizes_at = R.HEAD.size + 128 * rows
        assert blob[:4] == v1[:4] and struct.unpack_from('<I', blob, 4)[0] == 2 and blob[8:sizes_at + 8] == v1[8:sizes_at + 8]
        n_tok, n_pay, n_esc = R.SIZES.unpack_from(blob, sizes_at)
        assert blob[sizes_at + 24 + n_pay:-4] == v1[sizes_at + 24:-4]                          # the escapes
        steps, chunks = ops.attr_rans_layout(blob[sizes_at + 24:sizes_at + 24 + n_pay], n_tok)
        assert (steps, chunks) == ((S, ar.chunks_of(n_tok, S)) if S else (-(-n_tok // 64), 1))
    blob, rec = ar.encode_v2(pts[:1], rgb[:1], 4, 4, 4096, ops.crc32)
    assert len(blob) == R.HEAD.size + R.SIZES.size + 4 and np.array_equal(ar.decode_v2(pts[:1], blob, ops.crc32), rec)
