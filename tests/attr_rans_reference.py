"""The colour stream's device coder (`_A.bin` version 2; csrc/attribute_rans.hip) in plain Python integers: interleaved rANS over 64-ary
tokens, 64 lanes per chunk sharing one stream of 32-bit words.  Also the inputs both test files share, the damaged payloads, the length
bound and the whole-file form on top of raht_reference.  The kernels, include/pcgc_hip.h and DESIGN.md 8k follow THIS file.

Payload, little endian:  u32 S | u32 K = ceil(tokens / (64 S)) | K x 64 x u64 initial decoder states | K x u32 W_k | the chunks' words.
Chunk k covers tokens [64 S k, min(tokens, 64 S (k + 1))) in coding order; lane j codes tokens base + 64 t + j, t = 0 .. S - 1.  64-bit
state, 32-bit words, L = 2^31.  Tables are uint16 [48, 65] in rc_encode_ctx's convention: cdf[ctx][0] = 0 and cdf[ctx][64] = 65536 whatever
entries 0 and 64 say; token a under ctx has c = cdf[ctx][a] and f = cdf[ctx][a + 1] - c.  f = 65536 (a token that owns its row) is legal:
the update is the identity and the token never emits.  f <= 0 cannot be coded: the encoder refuses it."""
import math
import struct

import numpy as np

import raht_reference as ref

LANES = 64
TOKENS = 64
CONTEXTS = ref.CONTEXTS
L = 1 << 31
STATE_END = 1 << 63
VERSION = 2

# Realised against ideal length.  Every lane stores a 64-bit state that carries between 31 and 63 bits of the message, so a chunk costs at
# most 64 x 64 bits beyond its ideal, plus its u32 word count; the payload's head is 64 bits.  What is left is the arithmetic's own loss.
# Measured by test_attr_rans_cpu.py::test_recorded_excess_is_reproduced (which fails if the figure moves): `model_drawn(65537, seed 0)`
# (all 48 contexts in the order a tree gives them, tokens drawn from each context's own row), S = 4096 (one chunk): the payload exceeds
# ideal + chunks * (4096 + 32) + 64  by MEASURED_EXCESS_BITS in all.  It is negative (the final states hold more than 32 bits each), so the
# per-symbol allowance is the floor.
MEASURED_EXCESS_BITS = -948.9307
EPS_FLOOR = 1e-6                                          # bit per symbol
EPS = 2 * MEASURED_EXCESS_BITS / 65537 if MEASURED_EXCESS_BITS > 0 else EPS_FLOOR


class Unsound(ValueError):
    """a payload that is not what the encoder writes for the tokens it decodes to"""


def chunks_of(n, S):
    return -(-n // (LANES * S))


def length_bound(ideal_bits, symbols, chunks):
    """largest sound payload length in bits for `symbols` tokens of ideal length `ideal_bits` in `chunks` chunks"""
    return ideal_bits + chunks * (LANES * 64 + 32) + 64 + EPS * symbols


def cdf_rows(table):
    """uint16 [48, 65] -> 48 lists of 65 Python integers with entry 0 = 0 and entry 64 = 65536"""
    return [[0] + [int(v) for v in row[1:TOKENS]] + [65536] for row in np.asarray(table).reshape(CONTEXTS, TOKENS + 1)]


def ideal_bits(table, ctx, tokens):
    cdf = cdf_rows(table)
    return sum(-math.log2((cdf[int(c)][int(a) + 1] - cdf[int(c)][int(a)]) / 65536) for c, a in zip(ctx, tokens))


def encode_chunks(table, ctx, tokens, S):
    """-> [(final states of the 64 lanes, words in decoder order)] per chunk; ValueError on a token outside 0 .. 63, a context outside
    0 .. 47 or a token whose frequency is not positive"""
    cdf = cdf_rows(table)
    ctx, tokens = [int(v) for v in ctx], [int(v) for v in tokens]
    n = len(tokens)
    for r in range(n):
        if not (0 <= ctx[r] < CONTEXTS and 0 <= tokens[r] < TOKENS) or cdf[ctx[r]][tokens[r] + 1] <= cdf[ctx[r]][tokens[r]]:
            raise ValueError(f'token {tokens[r]} under context {ctx[r]} at {r} has no frequency')
    out = []
    for k in range(chunks_of(n, S)):
        base = LANES * S * k
        x = [L] * LANES
        emitted = []
        for t in range(S - 1, -1, -1):
            for j in range(LANES - 1, -1, -1):
                r = base + LANES * t + j
                if r >= n:
                    continue
                c = cdf[ctx[r]][tokens[r]]
                f = cdf[ctx[r]][tokens[r] + 1] - c
                v = x[j]
                if v >= f << 47:
                    emitted.append(v & 0xffffffff)
                    v >>= 32
                x[j] = ((v // f) << 16) + v % f + c
        out.append((x, emitted[::-1]))
    return out


def pack(S, chunks):
    states = [v for x, _ in chunks for v in x]
    counts = [len(w) for _, w in chunks]
    words = [v for _, w in chunks for v in w]
    return struct.pack('<II', S, len(chunks)) + np.array(states, dtype='<u8').tobytes() + np.array(counts, dtype='<u4').tobytes() + \
        np.array(words, dtype='<u4').tobytes()


def encode(table, ctx, tokens, S):
    """-> payload bytes (empty when there is no token)"""
    return pack(S, encode_chunks(table, ctx, tokens, S)) if len(tokens) else b''


def parse(payload, n):
    """-> (S, [(states, words)] per chunk); Unsound on a payload whose S / K / lengths disagree with n and its own size, or on a state
    outside [2^31, 2^63)"""
    if len(payload) < 8:
        raise Unsound(f'{len(payload)} bytes, shorter than the head')
    S, K = struct.unpack_from('<II', payload, 0)
    if S < 1:
        raise Unsound('S = 0')
    if K != chunks_of(n, S):
        raise Unsound(f'K = {K} for {n} tokens in chunks of 64 x {S}')
    if len(payload) < 8 + 516 * K:
        raise Unsound('cut inside the tables')
    states = np.frombuffer(payload, '<u8', LANES * K, 8).tolist()
    counts = np.frombuffer(payload, '<u4', K, 8 + 512 * K).tolist()
    if 8 + 516 * K + 4 * sum(counts) != len(payload):
        raise Unsound(f'{len(payload)} bytes, but the word counts sum to {sum(counts)}')
    words = np.frombuffer(payload, '<u4', sum(counts), 8 + 516 * K).tolist()
    for v in states:
        if not L <= v < STATE_END:
            raise Unsound(f'state {v:#x} outside [2^31, 2^63)')
    chunks, at = [], 0
    for k in range(K):
        chunks.append((states[LANES * k:LANES * (k + 1)], words[at:at + counts[k]]))
        at += counts[k]
    return S, chunks


def decode(table, ctx, payload):
    """-> tokens (int16 ndarray [len(ctx)]); Unsound on an unsound stream.  The table's rows are monotone (attributes.read_stream refuses
    any other before it decodes)."""
    cdf = cdf_rows(table)
    ctx = [int(v) for v in ctx]
    n = len(ctx)
    out = np.zeros(n, dtype=np.int16)
    if n == 0:
        if len(payload):
            raise Unsound('a payload without tokens')
        return out
    S, chunks = parse(payload, n)
    for k, (states, words) in enumerate(chunks):
        base = LANES * S * k
        x = list(states)
        pos, past = 0, False
        for t in range(S):
            for j in range(LANES):
                r = base + LANES * t + j
                if r >= n:
                    break
                row = cdf[ctx[r]]
                s = x[j] & 0xffff
                a = sum(1 for i in range(1, TOKENS) if row[i] <= s)          # the token with cdf[a] <= s < cdf[a + 1]
                c = row[a]
                f = row[a + 1] - c
                v = f * (x[j] >> 16) + s - c
                if v < L:
                    if pos >= len(words):
                        past = True
                    v = (v << 32) | (words[pos] if pos < len(words) else 0)
                    pos += 1
                x[j] = v & (STATE_END * 2 - 1)
                out[r] = a
        if past or pos != len(words) or any(v != L for v in x):
            raise Unsound(f'chunk {k}: {pos} of {len(words)} words consumed, {sum(v != L for v in x)} lanes not at L')
    return out


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
# The decoder derives its contexts from the tree's 65 bucket offsets, so the inputs are shaped as a tree shapes them: position p of the
# coding order carries tokens 3 p, 3 p + 1, 3 p + 2 under contexts level, 16 + level, 32 + level, and the level never rises along p.
def bucket_contexts(bucket, n):
    """the contexts of the first n tokens under the 65 bucket offsets `bucket` (attributes.contexts, cut to n) -> uint16 [n]"""
    d = np.repeat(63 - np.arange(64), np.diff(np.asarray(bucket, np.int64)))
    return (16 * np.arange(3)[None, :] + np.minimum(d // 3, 15)[:, None]).reshape(-1)[:n].astype(np.uint16)


def spread_bucket(n, bits=range(59, -1, -1)):
    """bucket offsets [65] that spread the ceil(n / 3) positions of n tokens evenly over the split bits `bits` (descending): every level,
    so with 60 positions or more every one of the 48 contexts, occurs"""
    gaps, bits = -(-n // 3), list(bits)
    count = np.zeros(64, np.int64)
    count[63 - np.array(bits)] = [gaps * (i + 1) // len(bits) - gaps * i // len(bits) for i in range(len(bits))]
    return np.concatenate([[0], np.cumsum(count)]).astype(np.int32)


def table_of(freq):
    """frequencies int [48, 64], every row summing to 65536 -> uint16 [48, 65].  Entries 1 .. 63 are 16 bits wide and cannot say 65536, so
    token 63 has a frequency of 1 at least in every row (raht_reference.frequencies sees to that in the tables of a stream)."""
    freq = np.asarray(freq, np.int64)
    assert freq.shape == (CONTEXTS, TOKENS) and (freq.sum(1) == 65536).all() and (freq >= 0).all() and (freq[:, 63] >= 1).all()
    table = np.zeros((CONTEXTS, TOKENS + 1), np.uint16)
    table[:, 1:] = (np.cumsum(freq, 1) & 0xFFFF).astype(np.uint16)
    return table


def mixed_table(seed=3):
    """48 rows: row 0 belongs to token 63 alone (f = 65536); rows 1, 17 and 33 (level 1 of the three channels) have token 6 at f = 65535
    next to token 63 at f = 1; row 2 is uniform (f = 1024); the others are random, about a third of their tokens at frequency 0"""
    rng = np.random.default_rng(seed)
    freq = np.zeros((CONTEXTS, TOKENS), np.int64)
    for c in range(CONTEXTS):
        w = rng.integers(1, 1000, TOKENS) ** 2 * (rng.random(TOKENS) > 0.33)
        w[63] += 1
        f = np.where(w > 0, np.maximum(1, (w * 65536) // w.sum()), 0)
        f[int(np.argmax(w))] += 65536 - f.sum()
        freq[c] = f
    freq[0] = 0
    freq[0, 63] = 65536
    for c in (1, 17, 33):
        freq[c] = 0
        freq[c, 6], freq[c, 63] = 65535, 1
    freq[2] = 1024
    return table_of(freq), freq


def model_drawn(n, seed=0, bucket=None):
    """-> (table, bucket, ctx, tokens) of mixed_table: the contexts of `bucket` (default: spread_bucket(n)), every token drawn with the
    probability its context gives it (so frequency-0 tokens never occur, and rows 0 and 1 show the f = 65536, 1 and 65535 cases)"""
    table, freq = mixed_table()
    rng = np.random.default_rng(seed)
    bucket = spread_bucket(n) if bucket is None else bucket
    ctx = bucket_contexts(bucket, n)
    cum = np.cumsum(freq, 1)
    tokens = np.array([np.searchsorted(cum[c], s, side='right') for c, s in zip(ctx, rng.integers(0, 65536, n))], np.int64)
    return table, bucket, ctx, tokens.astype(np.int16)


def improbable(n):
    """-> (table, bucket, ctx, tokens): level 1 only (contexts 1, 17, 33), the f = 1 token at every position (16 bits each) except every
    7th, which is the f = 65535 token"""
    table, _ = mixed_table()
    bucket = spread_bucket(n, bits=[4])
    tokens = np.where(np.arange(n) % 7 == 6, 6, 63).astype(np.int16)
    return table, bucket, bucket_contexts(bucket, n), tokens


def sizes(S):
    return [1, 63, 64, 65, 64 * S - 1, 64 * S, 64 * S + 1, 2 * 64 * S + 3 * 64 + 17]


STEPS = (1, 4, 16)


# ---- damaged payloads (of a payload with at least three chunks and words in its middle chunk) ------------------------------------------------
def damaged(payload):
    """{what: bytes}: the refusals of the device test; the CPU test shows that the definition refuses every one"""
    S, K = struct.unpack_from('<II', payload, 0)
    assert K >= 3
    counts = np.frombuffer(payload, '<u4', K, 8 + 512 * K).astype(np.int64)
    words_at = 8 + 516 * K
    assert counts[1] >= 2 and counts[2] >= 1
    mid = words_at + 4 * int(counts[0] + counts[1] // 2)                      # a word in the middle of chunk 1
    end1 = words_at + 4 * int(counts[0] + counts[1])                          # first byte after chunk 1's words
    w1 = 8 + 512 * K + 4

    def with_w1(delta, body):
        return body[:w1] + struct.pack('<I', int(counts[1]) + delta) + body[w1 + 4:]

    return {
        'one flipped bit in a middle word': payload[:mid + 1] + bytes([payload[mid + 1] ^ 0x10]) + payload[mid + 2:],
        'W_1 plus one, a word inserted': with_w1(+1, payload[:end1] + b'\0\0\0\0' + payload[end1:]),
        'W_1 minus one, its last word removed': with_w1(-1, payload[:end1 - 4] + payload[end1:]),
        'a state replaced by L - 1': payload[:8 + 8 * 70] + struct.pack('<Q', L - 1) + payload[8 + 8 * 71:],
        'the last word dropped': payload[:-4],
    }


def three_chunks(S=16, seed=5):
    """(table, bucket, ctx, tokens, S) of the refusal tests: three chunks, the last one partial; split bits 59 .. 9 (levels 15 .. 3) cost
    several bits a token, so every chunk holds words"""
    n = 2 * LANES * S + 11 * LANES + 17                                       # (about 45 bits per lane in the last chunk: it holds words too)
    return model_drawn(n, seed, spread_bucket(n, bits=range(59, 8, -1))) + (S,)


# ---- the whole file ------------------------------------------------------------------------------------------------------------------------
def pack_stream_v2(n, q_luma, q_chroma, dc, rows, table, n_tokens, payload, esc, crc32):
    """version 1's container (raht_reference.pack_stream) with version = 2 and this file's payload"""
    blob = ref.HEAD.pack(ref.MAGIC, VERSION, n, q_luma, q_chroma, int(dc[0]), int(dc[1]), int(dc[2]), len(rows))
    for c in rows:
        blob += struct.pack('<H', c) + table[c, 1:64].astype('<u2').tobytes()
    blob += ref.SIZES.pack(n_tokens, len(payload), len(esc)) + payload + ref.pack_escapes(esc)
    return blob + struct.pack('<I', crc32(blob))


def _tree_ctx(tree):
    return (16 * np.arange(3)[None, :] + np.minimum(tree['d'][tree['order']] // 3, 15)[:, None]).reshape(-1).astype(np.uint16)


def encode_v2(xyz, rgb, q_luma, q_chroma, S, crc32):
    """the bytes of `_A.bin` version 2 for rows (x, y, z) with colours rgb in chunks of 64 S tokens (S = 0: one chunk), and the colours a
    decoder gets back, in the caller's row order"""
    keys, perm = ref.sort_cloud(xyz)
    tree = ref.build_tree(keys)
    H, dc = ref.forward(tree, ref.ycocg_forward(np.asarray(rgb)[perm]))
    D16 = ref.steps(tree, q_luma, q_chroma)
    k = ref.quantize(H, D16)
    tok, ctx, esc, hist = ref.tokens(tree, k)
    rows, table = ref.cdf_table(hist)
    payload = encode(table, ctx, tok, S if S else max(1, chunks_of(tok.size, 1)))
    blob = pack_stream_v2(keys.size, q_luma, q_chroma, dc, rows, table, tok.size, payload, esc, crc32)
    out = np.zeros((keys.size, 3), np.uint8)
    out[perm] = ref.ycocg_inverse(ref.inverse(tree, ref.dequantize(k, D16), dc))
    return blob, out


def decode_v2(xyz, blob, crc32):
    """-> uint8 [N,3] in the row order of xyz (the checks a decoder owes a damaged file are attributes.py's; this reads a sound one)"""
    keys, perm = ref.sort_cloud(xyz)
    tree = ref.build_tree(keys, check=False)
    assert struct.unpack('<I', blob[-4:])[0] == crc32(blob[:-4])
    magic, version, n, ql, qc, y, co, cg, R = ref.HEAD.unpack_from(blob, 0)
    assert (magic, version, n) == (ref.MAGIC, VERSION, keys.size)
    table = np.zeros((CONTEXTS, 65), np.uint16)
    pos = ref.HEAD.size
    for _ in range(R):
        c = struct.unpack_from('<H', blob, pos)[0]
        table[c, 1:64] = np.frombuffer(blob, '<u2', 63, pos + 2)
        pos += 128
    n_tok, n_pay, n_esc = ref.SIZES.unpack_from(blob, pos)
    pos += ref.SIZES.size
    tok = decode(table, _tree_ctx(tree)[:n_tok], blob[pos:pos + n_pay])
    esc = ref.unpack_escapes(blob[pos + n_pay:-4], n_esc)
    k = ref.levels(tree, tok, esc)
    out = np.zeros((keys.size, 3), np.uint8)
    out[perm] = ref.ycocg_inverse(ref.inverse(tree, ref.dequantize(k, ref.steps(tree, ql, qc)), (y, co, cg)))
    return out
