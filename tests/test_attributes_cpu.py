"""CPU tests of the colour format (tests/raht_reference.py is its definition) and of the host side of pcgcv2_amd/attributes.py: the
transform's exactness at quantiser 0, the two formulations of the tree, the quantiser's limits, the frequency rule, the lifting form against
the orthonormal fp64 RAHT, the container's round trip through the host range coder and every refusal a decoder owes a bad file."""
import math
import struct

import numpy as np
import pytest

import raht_reference as R
from pcgcv2_amd import attributes as at, ops, synthetic
from pcgcv2_amd._lib import PcgcError


# ---- fixtures -------------------------------------------------------------------------------------------------------------------------------
def _random_cloud(n, grid, seed):
    rng = np.random.default_rng(seed)
    pts = np.unique(rng.integers(0, grid, size=(3 * n, 3)), axis=0)
    return pts[rng.permutation(len(pts))[:n]].astype(np.int64)


def _chain():
    """x = 0, 1, 2, 4, ..., 2^19: every merge is (k, 1)"""
    x = np.array([0] + [1 << i for i in range(20)], np.int64)
    return np.stack([x, np.zeros_like(x), np.zeros_like(x)], 1)


def _block():
    return np.array([[x, y, z] for z in range(2) for y in range(2) for x in range(2)], np.int64) + 5


def _alternating(keys_perm, n):
    """0 / 255 alternating along Morton order in every channel, blue against red and green: Co swings between 255 and -255"""
    _, perm = keys_perm
    rgb = np.zeros((n, 3), np.uint8)
    i = np.arange(n)
    rgb[perm] = np.stack([255 * (i & 1), 255 * (i & 1), 255 * ((i + 1) & 1)], 1).astype(np.uint8)
    return rgb


@pytest.fixture(scope='module')
def shell8():
    """shell8 with a smooth colour field plus integer-hash noise of +-12 (no random generator: the figures below must not move)"""
    pts = synthetic.cloud('shell8').numpy().astype(np.int64)
    t = pts / float(pts.max() + 1)
    noise = np.stack([((pts[:, 0] * 73856093) ^ (pts[:, 1] * 19349663) ^ (pts[:, 2] * 83492791) ^ (c * 2654435761)) % 25 - 12 for c in range(3)], 1)
    rgb = np.stack([255 * t[:, 0], 127.5 * (1 + np.sin(40 * t[:, 1])), 255 * t[:, 2] * t[:, 0]], 1)
    rgb = np.clip(np.rint(rgb) + noise, 0, 255).astype(np.uint8)
    keys, perm = R.sort_cloud(pts)
    return pts, rgb, keys, perm, R.build_tree(keys)


def _reconstruct(pts, rgb, ql, qc):
    return R.encode(pts, rgb, ql, qc, ops.rc_encode_ctx, ops.crc32)


# ---- colour space, tree ----------------------------------------------------------------------------------------------------------------------
def test_ycocg_is_reversible_on_every_extreme():
    v = np.array([0, 1, 2, 127, 128, 254, 255])
    rgb = np.stack(np.meshgrid(v, v, v, indexing='ij'), -1).reshape(-1, 3).astype(np.uint8)
    ycc = R.ycocg_forward(rgb)
    assert np.array_equal(R.ycocg_inverse(ycc), rgb)
    assert ycc[:, 0].min() >= 0 and ycc[:, 0].max() <= 255 and np.abs(ycc[:, 1:]).max() <= 255


def test_morton_bit_layout():
    k = R.morton_keys(np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1 << 19, 0, 0], [0, 0, 1 << 19], [(1 << 20) - 1] * 3]))
    assert k.tolist() == [1, 2, 4, 1 << 57, 1 << 59, (1 << 60) - 1]
    with pytest.raises(ValueError):
        R.morton_keys(np.array([[1 << 20, 0, 0]]))
    with pytest.raises(ValueError):
        R.sort_cloud(np.array([[1, 2, 3], [1, 2, 3]]))


@pytest.mark.parametrize('cloud', ['random', 'chain', 'block', 'pair59', 'pair0', 'one'])
def test_the_two_tree_formulations_agree(cloud):
    pts = {'random': _random_cloud(3000, 64, 1), 'chain': _chain(), 'block': _block(), 'pair59': np.array([[3, 4, 0], [3, 4, 1 << 19]]),
           'pair0': np.array([[6, 4, 9], [7, 4, 9]]), 'one': np.array([[9, 9, 9]])}[cloud]
    keys, _ = R.sort_cloud(pts)
    tree = R.build_tree(keys, check=True)                      # (asserts the agreement of merges, weights and order)
    n = len(pts)
    assert tree['bucket'][-1] == n - 1 and sorted(tree['order'].tolist()) == list(range(n - 1))
    if cloud == 'pair59':
        assert tree['d'].tolist() == [59]
    if cloud == 'pair0':
        assert tree['d'].tolist() == [0]
    if cloud == 'chain':
        assert tree['w2'].tolist() == [1] * 20 and tree['w1'].tolist() == list(range(1, 21))
    # every node's children tile its range: sizes add up, and each gap and leaf is the child of exactly one node
    if n > 1:
        kids = np.concatenate([tree['left'], tree['right']])
        assert sorted(kids[kids >= 0].tolist()) == sorted(set(range(n - 1)) - {int(np.argmax(tree['d']))})
        assert sorted((~kids[kids < 0]).tolist()) == list(range(n))


# ---- exactness -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cloud', ['random', 'chain', 'block', 'one'])
@pytest.mark.parametrize('colours', ['random', 'equal', 'alternating'])
def test_quantiser_zero_is_exact(cloud, colours):
    pts = {'random': _random_cloud(2500, 40, 2), 'chain': _chain(), 'block': _block(), 'one': np.array([[9, 9, 9]])}[cloud]
    n = len(pts)
    rgb = {'random': np.random.default_rng(3).integers(0, 256, (n, 3)).astype(np.uint8), 'equal': np.full((n, 3), 200, np.uint8),
           'alternating': _alternating(R.sort_cloud(pts), n)}[colours]
    blob, rec = _reconstruct(pts, rgb, 0, 0)
    assert np.array_equal(rec, rgb)
    assert np.array_equal(R.decode(pts, blob, ops.rc_decode_ctx, ops.crc32), rgb)
    keys, perm = R.sort_cloud(pts)
    tree = R.build_tree(keys)
    H, _ = R.forward(tree, R.ycocg_forward(rgb[perm]))
    assert np.abs(H).max(initial=0) <= 510
    if colours == 'equal':
        assert not H.any()
    if colours == 'alternating' and n > 2:
        assert np.abs(H).max() == 510                          # the escape path
        assert R.tokens(tree, R.quantize(H, R.steps(tree, 0, 0)))[2].size > 0


def test_quantiser_zero_is_exact_on_a_shell(shell8):
    pts, rgb, *_ = shell8
    _, rec = _reconstruct(pts, rgb, 0, 0)
    assert np.array_equal(rec, rgb)


def test_low_pass_stays_between_its_children(shell8):
    _, rgb, _, perm, tree = shell8
    val = R.ycocg_forward(rgb[perm])
    for b in np.unique(tree['d'])[:6]:
        g = np.flatnonzero(tree['d'] == b)
        a1, a2 = val[tree['lo'][g]], val[g + 1]
        L = a1 + (tree['w2'][g, None] * (a2 - a1)) // (tree['w1'][g] + tree['w2'][g])[:, None]
        assert ((L >= np.minimum(a1, a2)) & (L <= np.maximum(a1, a2))).all()
        val[tree['lo'][g]] = L


# ---- quantiser -------------------------------------------------------------------------------------------------------------------------------
def test_isqrt_and_step_at_their_limits():
    v = np.array([0, 1, 2, 3, 4, 15, 16, 17, (1 << 49) - 1, 1 << 49, (1 << 25) ** 2 - 1, (1 << 25) ** 2, 3037000499 ** 2 - 1], np.int64)
    assert R.isqrt(v).tolist() == [math.isqrt(int(x)) for x in v]
    top = (1 << 24) - 1
    for Q in (0, 1, 4, 16, 64, 255):
        for w1, w2 in ((1, 1), (1, top), (top, 1), (1 << 23, 1 << 23), (3, 5)):
            assert int(R.delta16(Q, np.array([w1]), np.array([w2]))[0]) == R.delta16_exact(Q, w1, w2)
    assert R.delta16_exact(0, 1, 1) == 16
    assert R.delta16_exact(255, 1, 1) == math.isqrt(256 * 255 * 255 * 2) == 5769       # 255 sqrt(2) in sixteenths
    assert R.delta16_exact(255, 1, top) == math.isqrt((256 * 255 * 255 * (1 << 24)) // top) == 4080
    assert R.delta16_exact(1, 1 << 23, 1 << 23) == 16                                   # heavy nodes hit the floor: coded exactly
    assert 256 * 255 * 255 * (1 << 24) < 1 << 49


def test_levels_round_trip_and_the_step_floor():
    H = np.arange(-510, 511)
    for D in (16, 17, 23, 64, 4080, 5769):
        k = R.quantize(H, D)
        Hh = R.dequantize(k, D)
        assert np.abs(16 * Hh - 16 * H).max() <= D // 2 + 8    # half a step, plus the rounding of the reconstruction to an integer
        assert np.array_equal(np.sign(k) * np.sign(H), np.abs(np.sign(k)))
    assert np.array_equal(R.dequantize(R.quantize(H, 16), 16), H)
    z = np.where(R.quantize(H, 16) >= 0, 2 * R.quantize(H, 16), -2 * R.quantize(H, 16) - 1)
    assert z.max() == 1020 and z.max() - R.ESCAPE < 1 << R.ESCAPE_BITS


# ---- tables ----------------------------------------------------------------------------------------------------------------------------------
def _check_row(counts):
    counts = np.asarray(counts, np.int64)
    f = R.frequencies(counts)
    assert int(f.sum()) == 65536
    assert (f[counts > 0] >= 1).all()
    assert not f[:R.ESCAPE][counts[:R.ESCAPE] == 0].any()
    assert f[R.ESCAPE] >= 1                                     # (the one exception: see raht_reference.frequencies)
    hist = np.zeros((R.CONTEXTS, 64), np.int64)
    hist[7] = counts
    rows, table = at.frequency_rows(hist)
    rows_r, table_r = R.cdf_table(hist)
    assert rows == rows_r == [7] and np.array_equal(table, table_r)
    assert table[7, 0] == 0 and table[7, 64] == 0 and (np.diff(table[7, :64].astype(np.int64)) >= 0).all()
    assert np.array_equal(np.diff(np.append(table[7, :64].astype(np.int64), 65536)), f)
    return f


def test_frequency_rule():
    once = np.ones(64, np.int64)
    once[5] += 10 ** 6
    f = _check_row(once)
    assert f[5] == 65536 - 63 and (np.delete(f, 5) == 1).all()
    for t in (0, 17, 62, 63):
        single = np.zeros(64, np.int64)
        single[t] = 12345
        f = _check_row(single)
        assert f[t] + (f[63] if t != 63 else 0) == 65536 and f[t] >= 65500 and np.count_nonzero(f) == (1 if t == 63 else 2)
    tie = np.zeros(64, np.int64)
    tie[[3, 9]] = 5
    f = _check_row(tie)
    assert f[3] > f[9]                                          # the remainder goes to the lowest index of a tie
    rng = np.random.default_rng(5)
    for _ in range(50):
        c = rng.integers(0, 3, 64) * rng.integers(1, 10 ** int(rng.integers(1, 7)), 64)
        if c.sum():
            _check_row(c)


# ---- the lifting form against the orthonormal transform ----------------------------------------------------------------------------------------
# luma MSE of the lifting form over that of the orthonormal fp64 RAHT with a uniform step Q, on the shell8 fixture above (48 636 voxels), as
# this computation gives them; the remaining gap is the integer step granularity
MSE_RATIO = {4: 1.6666, 16: 1.1420, 64: 1.0794}           # lifting / orthonormal: 2.2461 / 1.3477, 21.5511 / 18.8721, 104.1174 / 96.4544


@pytest.mark.parametrize('Q', [4, 16, 64])
def test_lifting_against_orthonormal_luma_mse(shell8, Q):
    _, rgb, _, perm, tree = shell8
    luma = R.ycocg_forward(rgb[perm])[:, 0]
    lift, _ = R.lifting_luma_mse(tree, luma, Q)
    orth, _ = R.orthonormal_luma_mse(tree, luma, Q)
    print(f'Q = {Q}: luma MSE lifting {lift:.4f} orthonormal {orth:.4f} ratio {lift / orth:.4f}')
    assert abs(lift / orth - MSE_RATIO[Q]) <= 0.01 * MSE_RATIO[Q]


def test_psnr_and_stream_length_fall_with_the_quantiser(shell8):
    pts, rgb, *_ = shell8
    sizes, mses = [], []
    for Q in (0, 1, 4, 16, 64, 255):
        blob, rec = _reconstruct(pts, rgb, Q, Q)
        sizes.append(len(blob))
        mses.append(float(np.mean((rec.astype(np.float64) - rgb) ** 2)))
    assert mses[0] == 0.0
    assert all(a >= b for a, b in zip(sizes, sizes[1:])) and all(a <= b for a, b in zip(mses, mses[1:]))


# ---- the container ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def stream(tmp_path_factory):
    """a small cloud with escapes, coded by the definition -> (path, pts, rgb, blob, reconstruction, tree)"""
    pts = _random_cloud(700, 24, 11)
    keys, perm = R.sort_cloud(pts)
    rgb = np.random.default_rng(12).integers(0, 256, (len(pts), 3)).astype(np.uint8)
    rgb[perm[:40]] = _alternating((keys, perm), len(pts))[perm[:40]]
    blob, rec = _reconstruct(pts, rgb, 1, 3)
    path = str(tmp_path_factory.mktemp('attr') / 'cloud')
    with open(path + at.SUFFIX, 'wb') as fh:
        fh.write(blob)
    return path, pts, rgb, blob, rec, R.build_tree(keys)


def test_file_round_trip_through_the_host_coder(stream):
    path, pts, rgb, blob, rec, tree = stream
    assert np.array_equal(R.decode(pts, blob, ops.rc_decode_ctx, ops.crc32), rec)
    ql, qc, dc, tokens, esc = at.read_stream(path + at.SUFFIX, len(pts), tree['bucket'])
    H, dc_r = R.forward(tree, R.ycocg_forward(rgb[R.sort_cloud(pts)[1]]))
    tok_r, ctx_r, esc_r, hist = R.tokens(tree, R.quantize(H, R.steps(tree, 1, 3)))
    assert (ql, qc) == (1, 3) and list(dc) == dc_r.tolist()
    assert np.array_equal(tokens, tok_r) and np.array_equal(esc, esc_r) and esc.size > 0
    assert np.array_equal(at.contexts(tree['bucket']), ctx_r)
    assert blob[:4] == b'PCGA' and struct.unpack_from('<I', blob, 4)[0] == 1
    assert struct.unpack('<I', blob[-4:])[0] == ops.crc32(blob[:-4])


def test_tokens_that_own_their_row_round_trip():
    """few points: most contexts see token 63 only, which then owns its whole row (width 0x10000), between rows of power-of-two widths that
    bring the coder's span back to 2^32"""
    table = np.zeros((R.CONTEXTS, 65), np.uint16)
    table[15, 13:39], table[15, 39:64] = 16384, 32768
    table[47, 33:56], table[47, 56:64] = 16384, 32768
    tok = np.array([63, 63, 63, 38, 63, 55, 63, 63, 63, 12, 63, 32, 63, 63, 63], np.int16)
    ctx = np.array([15, 31, 47, 15, 31, 47, 15, 31, 47, 15, 31, 47, 0, 16, 32], np.uint16)
    payload = ops.rc_encode_ctx(table, ctx, tok)
    assert len(payload) == 2                                    # 12 bits of information
    assert np.array_equal(ops.rc_decode_ctx(table, ctx, payload), tok)
    top = (1 << 20) - 1
    pts = np.array([[top, top, top], [top - 1, top, top], [0, 0, 0], [top, 0, top], [0, top, 0], [top, top, 0]])
    rgb = np.random.default_rng(9).integers(0, 256, (6, 3)).astype(np.uint8)
    for q in (0, 1, 40):
        blob, rec = _reconstruct(pts, rgb, q, q)
        assert np.array_equal(R.decode(pts, blob, ops.rc_decode_ctx, ops.crc32), rec)


def test_one_point_has_a_dc_and_no_payload(tmp_path):
    pts, rgb = np.array([[5, 6, 7]]), np.array([[10, 200, 30]], np.uint8)
    blob, rec = _reconstruct(pts, rgb, 9, 9)
    assert np.array_equal(rec, rgb) and len(blob) == R.HEAD.size + R.SIZES.size + 4
    path = str(tmp_path / 'one')
    open(path + at.SUFFIX, 'wb').write(blob)
    ql, qc, dc, tokens, esc = at.read_stream(path + at.SUFFIX, 1, np.zeros(65, np.int64))
    assert tokens.size == 0 and esc.size == 0 and list(dc) == R.ycocg_forward(rgb)[0].tolist()


def _resealed(blob):
    return blob[:-4] + struct.pack('<I', ops.crc32(blob[:-4]))


def _patched(blob, offset, fmt, value, reseal=True):
    b = bytearray(blob)
    struct.pack_into(fmt, b, offset, value)
    return _resealed(bytes(b)) if reseal else bytes(b)


def _refused(tmp_path, blob, n, bucket, match=None):
    path = str(tmp_path / 'bad') + at.SUFFIX
    with open(path, 'wb') as fh:
        fh.write(blob)
    with pytest.raises(PcgcError, match=match):
        at.read_stream(path, n, bucket)


def test_every_refusal(stream, tmp_path):
    _, pts, _, blob, _, tree = stream
    n, bucket = len(pts), tree['bucket']
    R_rows = struct.unpack_from('<H', blob, 22)[0]
    sizes_at = R.HEAD.size + 128 * R_rows
    n_tok, n_pay, n_esc = R.SIZES.unpack_from(blob, sizes_at)
    # the CRC sees every damaged field; a file whose CRC was made to fit is still refused by the field's own check
    for reseal in (False, True):
        _refused(tmp_path, _patched(blob, 0, '<4s', b'PCGX', reseal), n, bucket, 'magic')
        _refused(tmp_path, _patched(blob, 4, '<I', 2, reseal), n, bucket, 'version')
        _refused(tmp_path, _patched(blob, 8, '<I', n + 1, reseal), n, bucket, None if not reseal else 'points')
        _refused(tmp_path, _patched(blob, 12, '<H', 256, reseal), n, bucket, None if not reseal else 'quantiser')
        _refused(tmp_path, _patched(blob, 14, '<H', 300, reseal), n, bucket, None if not reseal else 'quantiser')
        _refused(tmp_path, _patched(blob, 22, '<H', R_rows - 1, reseal), n, bucket)
        _refused(tmp_path, _patched(blob, 22, '<H', R_rows + 1, reseal), n, bucket)
        _refused(tmp_path, _patched(blob, sizes_at, '<Q', n_tok + 3, reseal), n, bucket, None if not reseal else 'tokens')
        _refused(tmp_path, _patched(blob, sizes_at + 8, '<Q', n_pay - 1, reseal), n, bucket, None if not reseal else 'declares')
        _refused(tmp_path, _patched(blob, sizes_at + 16, '<Q', n_esc + 1, reseal), n, bucket, None if not reseal else 'declares')
    _refused(tmp_path, blob, n + 1, bucket, 'points')                                    # N != len(coords)
    _refused(tmp_path, blob[:-1], n, bucket)                                             # cut by one byte
    _refused(tmp_path, blob + b'\0', n, bucket)                                          # extended by one byte
    _refused(tmp_path, _resealed(blob[:-5] + blob[-4:]), n, bucket)                      # cut, CRC made to fit
    _refused(tmp_path, _resealed(blob[:-4] + b'\0' + blob[-4:]), n, bucket)              # extended, CRC made to fit
    _refused(tmp_path, blob[:10], n, bucket, 'shorter')
    # the DC is data: any value is a stream, but not the same one
    assert at.read_stream(_write(tmp_path, _patched(blob, 16, '<h', -7)), n, bucket)[2][0] == -7
    _refused(tmp_path, _patched(blob, 16, '<h', -7, reseal=False), n, bucket, 'CRC')
    # a non-monotone CDF row, a context without a row, rows out of order
    row0 = R.HEAD.size
    cdf = np.frombuffer(blob, '<u2', 63, row0 + 2).astype(np.int64)
    j = int(np.flatnonzero(np.diff(cdf) > 0)[0])
    _refused(tmp_path, _patched(blob, row0 + 2 + 2 * j, '<H', int(cdf[j + 1]) + 1), n, bucket, 'monotone')
    dropped = _patched(blob[:row0] + blob[row0 + 128:], 22, '<H', R_rows - 1)
    _refused(tmp_path, dropped, n, bucket, 'no table row')
    assert R_rows >= 2
    _refused(tmp_path, _patched(blob, row0, '<H', 47), n, bucket, 'ascending')
    _refused(tmp_path, _patched(blob, row0, '<H', 48), n, bucket, 'ascending')
    # a damaged payload byte, CRC made to fit: the range decoder codes what it decoded again and compares
    at_pay = sizes_at + R.SIZES.size + n_pay // 2
    _refused(tmp_path, _patched(blob, at_pay, '<B', blob[at_pay] ^ 0x10), n, bucket)
    # an escape count that disagrees with the tokens: one escape fewer, the file's length made to fit
    esc = R.unpack_escapes(blob[sizes_at + R.SIZES.size + n_pay:-4], n_esc)
    fewer = blob[:sizes_at] + R.SIZES.pack(n_tok, n_pay, n_esc - 1) + blob[sizes_at + R.SIZES.size:sizes_at + R.SIZES.size + n_pay] + \
        R.pack_escapes(esc[:-1]) + b'\0\0\0\0'
    _refused(tmp_path, _resealed(fewer), n, bucket, 'escape')
    # another geometry with the same point count: contexts or payload disagree
    other = R.build_tree(R.sort_cloud(_random_cloud(n, 200, 99))[0])
    _refused(tmp_path, blob, n, other['bucket'])


def _write(tmp_path, blob):
    path = str(tmp_path / 'ok') + at.SUFFIX
    with open(path, 'wb') as fh:
        fh.write(blob)
    return path


def test_quantiser_steps_outside_0_255_are_value_errors():
    for q in ((-1, None), (256, None), (4, 256), (4, -1)):
        with pytest.raises(ValueError):
            at._qsteps(*q)
    assert at._qsteps(7, None) == (7, 7) and at._qsteps(0, 9) == (0, 9)
