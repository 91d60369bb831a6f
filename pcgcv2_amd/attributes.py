"""Colour codec: `_A.bin`, the colours of one frame on a geometry both sides hold, by an integer lifting form of the region-adaptive
hierarchical transform (RAHT, the attribute transform of G-PCC) on YCoCg-R (the definition is tests/raht_reference.py).

The transform is exactly invertible, so quantiser 0 returns the colours bit for bit, and it is integer arithmetic throughout, so the
device kernels (csrc/raht.hip) are held to equality with a numpy definition.  The tree is the binary radix tree of the voxels' Morton
keys: a function of the geometry alone, built the same way by encoder and decoder.

`_A.bin`, little endian:
    4s magic "PCGA" | u32 version (1 or 2) | u32 N | u16 Q_luma | u16 Q_chroma | 3 x i16 DC (Y, Co, Cg) | u16 R
    R x (u16 ctx, 63 x u16 cdf[1 .. 63])          the contexts that occur, ascending; cdf[0] = 0 and cdf[64] = 0x10000 are implied
    u64 tokens = 3 (N - 1) | u64 payload bytes | u64 escapes
    payload                                        the tokens in coding order (empty when there is no token)
                                                   version 1: ops.rc_encode_ctx, coded on the host (attribute_coder='host', the default)
                                                   version 2: ops.attr_rans_encode, interleaved rANS coded on the device
                                                   (attribute_coder='device'):  u32 S | u32 K = ceil(tokens / (64 S)) | K x 64 x u64 initial
                                                   decoder states | K x u32 W_k | the chunks' 32-bit words (include/pcgc_hip.h; DESIGN.md 8k;
                                                   the definition is tests/attr_rans_reference.py)
    escapes                                        10 bits each, packed LSB first, zero-padded to a byte
    u32 CRC-32 of all that precedes (ops.crc32)
The tables are semi-static, per stream: frequencies out of 65536 from the stream's own histogram.  The two versions differ in the version
field and the payload alone; a decoder reads either, whatever coder it was made with.  In version 2 the tokens and their contexts never
cross the bus: the encoder copies down the histogram, the DC and the escapes, the decoder copies up the tables, the payload and the escapes.

AttributeCoder.encode_batch / decode_batch code up to 16 frames in one pass over the device: the same files, the same colours.

    python -m pcgcv2_amd.attributes --filedir CLOUD.ply [MORE.ply ...] --qstep Q [--qstep_chroma Qc] [--outdir DIR]
                                    [--attribute_coder device [--chunk_steps S]]        (several files: one batch)
                                    [--voxelize B [--merge mean|first] [--devoxelize]]  (raw clouds: voxelised to B bits first, voxelize.py)
                                    [--clean K,M [--clean_r2 R] [--keep_largest n]]     (outliers and fragments removed first, clean.py)
"""
import os
import struct

import numpy as np
import torch

from . import ops
from ._lib import PcgcError
from .coder import _dump, _slurp

SUFFIX = '_A.bin'
MAGIC, VERSION = b'PCGA', 1
VERSION_DEVICE = 2                                # payload coded by ops.attr_rans_encode
CODERS = {'host': VERSION, 'device': VERSION_DEVICE}
CHUNK_STEPS = 4096                                # steps per chunk of the device coder; 0: one chunk
CONTEXTS, TOKENS, ESCAPE, ESCAPE_BITS = ops.RAHT_CONTEXTS, 64, ops.RAHT_ESCAPE, 10
_HEAD = struct.Struct('<4sIIHH3hH')
_ROW = 2 + 2 * (TOKENS - 1)
_SIZES = struct.Struct('<3Q')


def frequency_rows(hist):
    """histogram int [48,64] -> (contexts that occur, uint16 [48,65] table in rc_encode_ctx's convention: entry 0 is 0, entry 64 stands
    for 0x10000).  Per row: 0 where the count is 0, else max(1, floor(count 65536 / total)); the difference to 65536 goes to the most
    frequent token (lowest index on a tie).  Token 63 is counted at least once, so that entry 63 never has to say 0x10000."""
    hist = np.asarray(hist, np.int64)
    rows = np.flatnonzero(hist.sum(1) > 0)
    table = np.zeros((CONTEXTS, TOKENS + 1), np.uint16)
    if rows.size:
        c = hist[rows].copy()
        c[:, ESCAPE] = np.maximum(c[:, ESCAPE], 1)
        f = np.where(c > 0, np.maximum(1, (c * 65536) // c.sum(1, keepdims=True)), 0)
        f[np.arange(rows.size), np.argmax(c, 1)] += 65536 - f.sum(1)
        table[rows, 1:] = (np.cumsum(f, 1) & 0xFFFF).astype(np.uint16)
    return [int(r) for r in rows], table


def contexts(bucket):
    """the context of every token in coding order, from the 65 bucket offsets of the tree alone (the gaps of split bit d are positions
    bucket[63 - d] .. bucket[64 - d]) -> uint16 [3 (N - 1)]"""
    d = np.repeat(63 - np.arange(64), np.diff(np.asarray(bucket, np.int64)))
    return (16 * np.arange(3)[None, :] + np.minimum(d // 3, 15)[:, None]).reshape(-1).astype(np.uint16)


def _pack_escapes(esc):
    bits = ((np.asarray(esc, np.uint16)[:, None] >> np.arange(ESCAPE_BITS, dtype=np.uint16)) & 1).astype(np.uint8).reshape(-1)
    return np.packbits(bits, bitorder='little').tobytes()


def _container(version, n, ql, qc, dc, rows, table, n_tok, payload, esc):
    """the bytes of one `_A.bin`: head, the table rows of the contexts that occur, sizes, payload, escapes, CRC"""
    blob = _HEAD.pack(MAGIC, version, n, ql, qc, dc[0], dc[1], dc[2], len(rows))
    blob += b''.join(struct.pack('<H', c) + table[c, 1:TOKENS].astype('<u2').tobytes() for c in rows)
    blob += _SIZES.pack(n_tok, len(payload), esc.size) + payload + _pack_escapes(esc)
    return blob + struct.pack('<I', ops.crc32(blob))


def _unpack_escapes(data, count):
    bits = np.unpackbits(np.frombuffer(data, np.uint8), bitorder='little')
    if bits[count * ESCAPE_BITS:].any():
        raise PcgcError('non-zero padding behind the escapes')
    bits = bits[:count * ESCAPE_BITS].reshape(count, ESCAPE_BITS)
    return (bits.astype(np.uint16) << np.arange(ESCAPE_BITS, dtype=np.uint16)).sum(1).astype(np.uint16)


def _qsteps(qstep, qstep_chroma):
    ql = int(qstep)
    qc = ql if qstep_chroma is None else int(qstep_chroma)
    if not (0 <= ql <= 255 and 0 <= qc <= 255):
        raise ValueError(f'quantiser steps ({qstep}, {qstep_chroma}): integers in 0 .. 255')
    return ql, qc


def read_container(path, n, bucket, versions=(VERSION, VERSION_DEVICE)):
    """Every check of `_A.bin` that needs neither the decoded tokens nor the device, for a geometry of n points whose tree has the bucket
    offsets `bucket` -> (version, q_luma, q_chroma, dc, table uint16 [48,65], payload bytes, escapes uint16 [E]).  PcgcError on bad magic,
    a version not in `versions`, a bad CRC, a length that disagrees with the header, another point count, a non-monotone CDF row and a
    context that occurs without a row."""
    blob = _slurp(path)
    if len(blob) < _HEAD.size + _SIZES.size + 4:
        raise PcgcError(f'{path}: {len(blob)} bytes, shorter than its header')
    magic, version, n_file, ql, qc, y, co, cg, R = _HEAD.unpack_from(blob, 0)
    if magic != MAGIC:
        raise PcgcError(f'{path}: not a colour stream (magic {magic!r})')
    if version not in versions:
        raise PcgcError(f'{path}: version {version}; this decoder reads version {" and ".join(str(v) for v in versions)}')
    if struct.unpack_from('<I', blob, len(blob) - 4)[0] != ops.crc32(blob[:-4]):
        raise PcgcError(f'{path}: CRC-32 mismatch (cut, extended or damaged)')
    if n_file != n:
        raise PcgcError(f'{path}: coded for {n_file} points; the geometry has {n}')
    if ql > 255 or qc > 255:
        raise PcgcError(f'{path}: quantiser steps ({ql}, {qc}) outside 0 .. 255')
    pos = _HEAD.size + R * _ROW
    if R > CONTEXTS or len(blob) < pos + _SIZES.size + 4:
        raise PcgcError(f'{path}: {R} table rows do not fit the file')
    n_tok, n_pay, n_esc = _SIZES.unpack_from(blob, pos)
    pos += _SIZES.size
    if n_tok != 3 * (n - 1):
        raise PcgcError(f'{path}: {n_tok} tokens declared; {n} points have {3 * (n - 1)}')
    if n_esc > n_tok or len(blob) != pos + n_pay + (n_esc * ESCAPE_BITS + 7) // 8 + 4:
        raise PcgcError(f'{path}: {len(blob)} bytes, but the header declares a payload of {n_pay} bytes and {n_esc} escapes')
    if n_tok == 0 and (n_pay or R):
        raise PcgcError(f'{path}: a payload or tables without tokens')
    table = np.zeros((CONTEXTS, TOKENS + 1), np.uint16)
    rows, last = [], -1
    for r in range(R):
        at = _HEAD.size + r * _ROW
        c = struct.unpack_from('<H', blob, at)[0]
        if c >= CONTEXTS or c <= last:
            raise PcgcError(f'{path}: table row {r} names context {c} (rows are ascending, below {CONTEXTS})')
        cdf = np.frombuffer(blob, '<u2', TOKENS - 1, at + 2)
        if (np.diff(cdf.astype(np.int64), prepend=0) < 0).any():
            raise PcgcError(f'{path}: the CDF of context {c} is not monotone')
        table[c, 1:TOKENS] = cdf
        rows.append(c)
        last = c
    try:
        esc = _unpack_escapes(blob[pos + n_pay:-4], n_esc)
    except PcgcError as e:
        raise PcgcError(f'{path}: {e}') from None
    levels = np.minimum((63 - np.flatnonzero(np.diff(np.asarray(bucket, np.int64)) > 0)) // 3, 15)
    missing = sorted({int(16 * ch + lv) for ch in range(3) for lv in levels} - set(rows))
    if missing:
        raise PcgcError(f'{path}: contexts {missing} occur on this geometry but have no table row')
    return version, ql, qc, (y, co, cg), table, blob[pos:pos + n_pay], esc


def read_stream(path, n, bucket):
    """The host side of decoding a version-1 file: read_container's checks, then the payload decoded by ops.rc_decode_ctx ->
    (q_luma, q_chroma, dc, tokens int16 [3 (n - 1)], escapes uint16 [E]).  PcgcError also on an escape count that disagrees with the
    tokens, and on whatever ops.rc_decode_ctx refuses."""
    _, ql, qc, dc, table, payload, esc = read_container(path, n, bucket, versions=(VERSION,))
    return ql, qc, dc, _host_tokens(path, table, bucket, payload, esc), esc


def _host_tokens(path, table, bucket, payload, esc):
    """the tokens of a version-1 payload that read_container has passed -> int16 [3 (n - 1)]"""
    ctx = contexts(bucket)
    try:
        tokens = ops.rc_decode_ctx(table, ctx, payload) if ctx.size else np.zeros(0, np.int16)
    except PcgcError as e:
        raise PcgcError(f'{path}: {e}') from None
    if int(np.count_nonzero(tokens == ESCAPE)) != esc.size:
        raise PcgcError(f'{path}: {int(np.count_nonzero(tokens == ESCAPE))} escape tokens but {esc.size} escapes')
    return tokens


class AttributeCoder():
    """AttributeCoder(filename): encode writes `filename + postfix + '_A.bin'`, decode reads it.  One frame per call: coordinates are
    int32 [N,4] device rows (0, x, y, z) of distinct voxels (or [N,3] rows (x, y, z)); a batch, duplicates or coordinates outside
    [0, 2^20) are a ValueError.  form: ops.RAHT_FORMS (None: ops.RAHT_FORM); the bytes and colours do not depend on it.
    attribute_coder: 'host' writes version 1, 'device' version 2 in chunks of 64 x chunk_steps tokens (0: one chunk); decode reads either
    version whatever these two say.  encode_batch / decode_batch take rows (b, x, y, z) of up to 16 frames through the device once and
    write / read every frame's own file: the bytes and colours of encode / decode on that frame alone."""

    def __init__(self, filename, form=None, attribute_coder='host', chunk_steps=CHUNK_STEPS):
        if attribute_coder not in CODERS:
            raise ValueError(f'attribute_coder {attribute_coder!r}: one of {sorted(CODERS)}')
        if isinstance(chunk_steps, bool) or not isinstance(chunk_steps, (int, np.integer)) or not 0 <= chunk_steps <= ops.RANS_MAX_STEPS:
            raise ValueError(f'chunk_steps {chunk_steps!r}: an integer in 0 .. 2^24 (0: one chunk)')
        self.filename = filename
        self.form = form
        self.attribute_coder = attribute_coder
        self.chunk_steps = int(chunk_steps)
        self.times = None                         # measurement hook (tools/attributes_time.py): a dict -> seconds per phase, synchronised

    def _tick(self, phase, t0, dev=None):
        return ops.tick_phase(self.times, phase, t0, dev)

    @staticmethod
    def _coords(coords):
        if not torch.is_tensor(coords) or not coords.is_cuda:
            raise PcgcError('AttributeCoder: coordinates must be a ROCm device tensor (no CPU fallback exists)')
        if coords.dim() != 2 or coords.shape[1] not in (3, 4):
            raise ValueError(f'AttributeCoder: coordinates must be [N,4] (batch, x, y, z) or [N,3], got {tuple(coords.shape)}')
        coords = coords.to(torch.int32)
        if coords.shape[1] == 3:
            coords = torch.cat([torch.zeros((coords.shape[0], 1), dtype=torch.int32, device=coords.device), coords], 1)
        return coords.contiguous()

    def _tree(self, coords, tree):
        if tree is None:
            tree = ops.raht_tree(coords, times=self.times)
        elif tree.n != coords.shape[0]:
            raise ValueError(f'AttributeCoder: a tree of {tree.n} leaves for {coords.shape[0]} rows')
        return tree

    @torch.no_grad()
    def encode(self, coords, rgb, qstep, qstep_chroma=None, postfix='', tree=None):
        """colours rgb uint8 [N,3] (device) of the rows of coords -> writes `_A.bin`; -> {bits_A, tokens, escapes, payload_bytes, tree}.
        tree: ops.raht_tree(coords) when the caller holds it already."""
        ql, qc = _qsteps(qstep, qstep_chroma)
        coords = self._coords(coords)
        dev = coords.device
        with torch.cuda.device(dev):
            tree = self._tree(coords, tree)
            t = self._tick(None, 0.0, dev)
            H, dc = ops.raht_forward(tree, rgb, form=self.form)
            t = self._tick('forward', t, dev)
            tokens, ctx, esc, hist = ops.raht_quantize(tree, H, ql, qc)
            t = self._tick('quantise', t, dev)
            device = self.attribute_coder == 'device'
            n_tok = int(tokens.shape[0])
            if not device:
                tokens_h, ctx_h = tokens.cpu().numpy(), ctx.cpu().numpy().view(np.uint16)
            esc_h, hist_h, dc_h = esc.cpu().numpy().view(np.uint16), hist.cpu().numpy(), dc.cpu().tolist()
            t = self._tick('copies', t, dev)
            rows, table = frequency_rows(hist_h)
            if device:                            # the tokens and contexts stay where pcgc_raht_quantize wrote them
                steps = self.chunk_steps or max(1, ops.attr_rans_chunks(n_tok, 1))
                payload = ops.attr_rans_encode(table, ctx, tokens, steps)
                t = self._tick('device coder', t, dev)
            else:
                payload = ops.rc_encode_ctx(table, ctx_h, tokens_h) if n_tok else b''
            blob = _container(CODERS[self.attribute_coder], tree.n, ql, qc, dc_h, rows, table, n_tok, payload, esc_h)
            _dump(self.filename + postfix + SUFFIX, blob)
            self._tick('host coder', t)
        return {'bits_A': 8 * len(blob), 'tokens': n_tok, 'escapes': int(esc_h.size), 'payload_bytes': len(payload), 'tree': tree}

    @torch.no_grad()
    def decode(self, coords, postfix='', tree=None):
        """the colours of `_A.bin` for the rows of coords (the geometry the encoder coded them on) -> uint8 [N,3] device tensor in the row
        order of coords.  PcgcError on a stream that is cut, extended, damaged or not made for this geometry."""
        coords = self._coords(coords)
        dev = coords.device
        path = self.filename + postfix + SUFFIX
        with torch.cuda.device(dev):
            tree = self._tree(coords, tree)
            t = self._tick(None, 0.0, dev)
            version, ql, qc, dc, table, payload, esc = read_container(path, tree.n, tree.bucket)
            if version == VERSION_DEVICE:         # every host check has passed; the tokens are decoded where they are used
                t = self._tick('host coder', t)
                try:
                    tokens_d, n_escape = ops.attr_rans_decode(table, tree, payload, 3 * (tree.n - 1))
                except PcgcError as e:
                    raise PcgcError(f'{path}: {e}') from None
                if n_escape != esc.size:
                    raise PcgcError(f'{path}: {n_escape} escape tokens but {esc.size} escapes')
                t = self._tick('device coder', t, dev)
            else:
                tokens = _host_tokens(path, table, tree.bucket, payload, esc)
                t = self._tick('host coder', t)
                tokens_d = torch.from_numpy(np.ascontiguousarray(tokens)).to(dev)
            esc_d = torch.from_numpy(esc.view(np.int16).copy()).to(dev)
            t = self._tick('copies', t, dev)
            Hhat = ops.raht_dequantize(tree, tokens_d, esc_d, ql, qc)
            t = self._tick('dequantise', t, dev)
            rgb = ops.raht_inverse(tree, Hhat, dc, form=self.form)
            self._tick('inverse', t, dev)
        return rgb

    # ---- a batch of frames in one pass: the files and colours of frame-by-frame coding, the device work done once
    @staticmethod
    def _batch_args(coords, postfixes, qstep=0, qstep_chroma=None):
        """everything about a batch that can be refused without the device -> (B, q_luma [B], q_chroma [B])"""
        if isinstance(postfixes, str) or postfixes is None:
            raise ValueError('postfixes: a list of one distinct string per frame')
        postfixes = list(postfixes)
        B = len(postfixes)
        if not 1 <= B <= ops.RAHT_MAX_FRAMES:
            raise ValueError(f'{B} frames: a batch holds 1 .. {ops.RAHT_MAX_FRAMES} (code larger sets in several batches)')
        if len(set(postfixes)) != B or not all(isinstance(p, str) for p in postfixes):
            raise ValueError(f'postfixes {postfixes}: one distinct string per frame')

        def steps(q, what):
            q = [q] * B if isinstance(q, (int, np.integer)) and not isinstance(q, bool) else list(q) if hasattr(q, '__len__') else None
            if q is None or len(q) != B:
                raise ValueError(f'{what}: an integer or a sequence of {B}, one per frame')
            if not all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) and 0 <= v <= 255 for v in q):
                raise ValueError(f'{what} {q}: integers in 0 .. 255')
            return [int(v) for v in q]
        ql = steps(qstep, 'qstep')
        qc = ql if qstep_chroma is None else steps(qstep_chroma, 'qstep_chroma')
        if torch.is_tensor(coords) and coords.dim() == 2 and coords.shape[0] > ops.RAHT_MAX_POINTS:
            raise ValueError(f'{coords.shape[0]} rows: a batch holds 2^24 at most')
        if torch.is_tensor(coords) and (coords.dim() != 2 or coords.shape[1] != 4):
            raise ValueError(f'a batch takes coordinates [N,4] rows (frame, x, y, z), got {tuple(coords.shape)}')
        return B, ql, qc

    def _batch_tree(self, coords, B, tree):
        if tree is None:
            tree = ops.raht_tree_batch(coords, B, times=self.times)
        elif tree.n != coords.shape[0] or getattr(tree, 'frames', None) != B:
            raise ValueError(f'AttributeCoder: a tree of {tree.n} leaves for {coords.shape[0]} rows in {B} frames')
        return tree

    @torch.no_grad()
    def encode_batch(self, coords, rgb, qstep, qstep_chroma=None, postfixes=('',), tree=None):
        """coords int32 [N,4] device rows (b, x, y, z), b = 0 .. B - 1 in any order, B = len(postfixes) = 1 .. 16 frames of at least one
        row each; rgb uint8 [N,3] in the same row order; qstep, qstep_chroma: an int or B ints -> writes `filename + postfixes[b] + '_A.bin'`
        for every b, byte for byte what encode writes for frame b alone; -> B records {bits_A, tokens, escapes, payload_bytes}.  One key
        build and sort, one tree build, one transform, one quantiser pass and (attribute_coder='device') one coder launch sequence for the
        batch; 'host' brings tokens and contexts down once and codes each frame's slice on coder._batch_pool.  tree:
        ops.raht_tree_batch(coords, B) when the caller holds it already."""
        from .coder import _batch_pool
        B, ql, qc = self._batch_args(coords, postfixes, qstep, qstep_chroma)
        coords = self._coords(coords)
        dev = coords.device
        with torch.cuda.device(dev):
            tree = self._batch_tree(coords, B, tree)
            t = self._tick(None, 0.0, dev)
            H, dc = ops.raht_forward_batch(tree, rgb, form=self.form)
            t = self._tick('forward', t, dev)
            tokens, ctx, esc, hist = ops.raht_quantize_batch(tree, H, ql, qc)
            t = self._tick('quantise', t, dev)
            device = self.attribute_coder == 'device'
            tok = tree.tok
            if not device:
                tokens_h, ctx_h = tokens.cpu().numpy(), ctx.cpu().numpy().view(np.uint16)
            hist_h, dc_h = hist.cpu().numpy(), dc.cpu().tolist()
            n_esc = hist_h[:, :, ESCAPE].sum(1).astype(np.int64)           # frame b's escapes follow those of the frames before it
            esc_at = np.concatenate([[0], np.cumsum(n_esc)])
            esc_h = esc[:int(esc_at[-1])].cpu().numpy().view(np.uint16)
            t = self._tick('copies', t, dev)
            made = [frequency_rows(hist_h[b]) for b in range(B)]
            if device:                            # the tokens and contexts stay where pcgc_raht_quantize_batch wrote them
                payloads = ops.attr_rans_encode_batch(np.stack([m[1] for m in made]), ctx, tokens, tok, self.chunk_steps)
                t = self._tick('device coder', t, dev)
            else:
                def one(b):                       # a frame's slice on a host thread (the native coder releases the GIL)
                    mine = slice(int(tok[b]), int(tok[b + 1]))
                    return ops.rc_encode_ctx(made[b][1], ctx_h[mine], tokens_h[mine]) if tok[b + 1] > tok[b] else b''
                payloads = list(_batch_pool().map(one, range(B)))
            records = []
            for b in range(B):
                (rows, table), n_tok, e = made[b], int(tok[b + 1] - tok[b]), esc_h[esc_at[b]:esc_at[b + 1]]
                blob = _container(CODERS[self.attribute_coder], n_tok // 3 + 1, ql[b], qc[b], dc_h[b], rows, table, n_tok, payloads[b], e)
                _dump(self.filename + postfixes[b] + SUFFIX, blob)
                records.append({'bits_A': 8 * len(blob), 'tokens': n_tok, 'escapes': int(e.size), 'payload_bytes': len(payloads[b])})
            self._tick('host coder', t)
        return records

    @torch.no_grad()
    def decode_batch(self, coords, postfixes=('',), tree=None):
        """the colours of `filename + postfixes[b] + '_A.bin'`, b = 0 .. B - 1, for the rows (b, x, y, z) of coords -> uint8 [N,3] device
        tensor in the row order of coords: per frame what decode returns.  Every item is read in the version its file has (version-1
        payloads on the host threads of coder._batch_pool, version-2 payloads in one launch sequence on the device); the host checks of
        all items run before anything is launched.  PcgcError naming the file that is cut, extended, damaged or not made for its frame."""
        from .coder import _batch_pool
        B, _, _ = self._batch_args(coords, postfixes)
        coords = self._coords(coords)
        dev = coords.device
        paths = [self.filename + p + SUFFIX for p in postfixes]
        with torch.cuda.device(dev):
            tree = self._batch_tree(coords, B, tree)
            t = self._tick(None, 0.0, dev)
            tok, rows = tree.tok, np.diff(tree.starts)
            items = [read_container(paths[b], int(rows[b]), tree.bucket[b]) for b in range(B)]
            for b in range(B):
                if items[b][0] == VERSION_DEVICE:
                    try:
                        ops.attr_rans_layout(items[b][5], int(tok[b + 1] - tok[b]))
                    except PcgcError as e:
                        raise PcgcError(f'{paths[b]}: {e}') from None
            esc = np.concatenate([it[6] for it in items]) if B else np.zeros(0, np.uint16)
            n_esc = [int(it[6].size) for it in items]
            host = [b for b in range(B) if items[b][0] == VERSION]
            tokens_d = None
            if host:                              # version-1 items: decoded on the host, their slices go up in one copy
                tokens_h = np.zeros(int(tok[-1]), np.int16)
                for b, got in zip(host, _batch_pool().map(lambda b: _host_tokens(paths[b], items[b][4], tree.bucket[b], items[b][5], items[b][6]), host)):
                    tokens_h[tok[b]:tok[b + 1]] = got
                tokens_d = torch.from_numpy(tokens_h).to(dev)
            t = self._tick('host coder', t)
            if len(host) < B:                     # version-2 items: decoded where they are used, all of them in one launch sequence
                tokens_d, n_escape = ops.attr_rans_decode_batch(np.stack([it[4] for it in items]), tree,
                                                                [it[5] if it[0] == VERSION_DEVICE else None for it in items], tokens=tokens_d,
                                                                names=paths)
                for b in range(B):
                    if items[b][0] == VERSION_DEVICE and int(n_escape[b]) != n_esc[b]:
                        raise PcgcError(f'{paths[b]}: {int(n_escape[b])} escape tokens but {n_esc[b]} escapes')
                t = self._tick('device coder', t, dev)
            esc_d = torch.from_numpy(esc.view(np.int16).copy()).to(dev)
            t = self._tick('copies', t, dev)
            try:
                Hhat = ops.raht_dequantize_batch(tree, tokens_d, esc_d, n_esc, [it[1] for it in items], [it[2] for it in items])
            except PcgcError as e:
                raise PcgcError(f'{self.filename}{list(postfixes)}{SUFFIX}: {e}') from None
            t = self._tick('dequantise', t, dev)
            rgb = ops.raht_inverse_batch(tree, Hhat, [it[3] for it in items], form=self.form)
            self._tick('inverse', t, dev)
        return rgb


def attribute_bits(prefix, postfix=''):
    """bits of `_A.bin` of one coded cloud"""
    return os.path.getsize(prefix + postfix + SUFFIX) * 8


# ------------------------------------------------------------------------------------------------ CLI
def run(filedir, outdir, qstep, qstep_chroma=None, attribute_coder='host', chunk_steps=CHUNK_STEPS):
    """colours -> `_A.bin` -> colours on the file's own geometry; prints bits per point and the colour PSNR"""
    from .coder import device, _Stopwatch
    from .data_utils import read_ply_ascii_with_colours, write_ply_ascii_geo_rgb
    from .pc_error import colour_psnr_device, lattice_coords
    from .sparse import require_gpu
    require_gpu(device)
    xyz, rgb = read_ply_ascii_with_colours(filedir)
    if rgb is None:
        raise ValueError(f'{filedir} has no colours (red green blue)')
    os.makedirs(outdir, exist_ok=True)
    prefix = os.path.join(outdir, os.path.split(filedir)[-1].split('.')[0])
    print(prefix)
    a, ca = lattice_coords(xyz, device), torch.from_numpy(rgb).to(device)
    coder = AttributeCoder(prefix, attribute_coder=attribute_coder, chunk_steps=chunk_steps)
    with _Stopwatch('Enc Time'):
        record = coder.encode(a, ca, qstep, qstep_chroma)
    with _Stopwatch('Dec Time'):
        cb = coder.decode(a)
    print(f'{SUFFIX}:\t {record["bits_A"]} bits\t {round(record["bits_A"] / len(a), 3)} bpp')
    metric = colour_psnr_device(a, ca, a, cb)
    print('Colour PSNR (Y):\t', metric['c[0],PSNRF'])
    print('Colour PSNR (U, V):\t', metric['c[1],PSNRF'], metric['c[2],PSNRF'])
    write_ply_ascii_geo_rgb(prefix + '_dec.ply', xyz, cb.cpu().numpy())
    return record, metric


def run_batch(filedirs, outdir, qstep, qstep_chroma=None, attribute_coder='host', chunk_steps=CHUNK_STEPS):
    """several clouds collated into one batch and coded with encode_batch / decode_batch: per file the figures and the `_dec.ply` of run"""
    from .coder import device, _Stopwatch
    from .data_utils import read_ply_ascii_with_colours, write_ply_ascii_geo_rgb
    from .pc_error import colour_psnr_device, lattice_coords
    from .sparse import require_gpu
    require_gpu(device)
    names = [os.path.split(f)[-1].split('.')[0] for f in filedirs]
    if len(set(names)) != len(names):
        raise ValueError(f'{names}: the files of a batch need distinct names, they name the outputs')
    clouds = [read_ply_ascii_with_colours(f) for f in filedirs]
    for f, (_, rgb) in zip(filedirs, clouds):
        if rgb is None:
            raise ValueError(f'{f} has no colours (red green blue)')
    os.makedirs(outdir, exist_ok=True)
    prefix = os.path.join(outdir, '')
    parts = [lattice_coords(xyz, device, batch=b) for b, (xyz, _) in enumerate(clouds)]
    a, ca = torch.cat(parts), torch.from_numpy(np.concatenate([rgb for _, rgb in clouds])).to(device)
    coder = AttributeCoder(prefix, attribute_coder=attribute_coder, chunk_steps=chunk_steps)
    with _Stopwatch('Enc Time'):
        records = coder.encode_batch(a, ca, qstep, qstep_chroma, postfixes=names)
    with _Stopwatch('Dec Time'):
        cb = coder.decode_batch(a, postfixes=names)
    metrics, at = [], 0
    for b, (xyz, _) in enumerate(clouds):
        rows = slice(at, at + len(xyz))
        at += len(xyz)
        print(prefix + names[b])
        print(f'{SUFFIX}:\t {records[b]["bits_A"]} bits\t {round(records[b]["bits_A"] / len(xyz), 3)} bpp')
        single = torch.cat([torch.zeros_like(a[rows, :1]), a[rows, 1:]], 1)
        metric = colour_psnr_device(single, ca[rows], single, cb[rows])
        print('Colour PSNR (Y):\t', metric['c[0],PSNRF'])
        print('Colour PSNR (U, V):\t', metric['c[1],PSNRF'], metric['c[2],PSNRF'])
        write_ply_ascii_geo_rgb(prefix + names[b] + '_dec.ply', xyz, cb[rows].cpu().numpy())
        metrics.append(metric)
    return records, metrics


def main(argv=None):
    import argparse
    p = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("--filedir", required=True, nargs='+',
                   help="an ASCII PLY of distinct voxels with red green blue; several (up to 16): collated and coded as one batch")
    p.add_argument("--qstep", type=int, required=True, help="quantiser step of the luma channel, 0 .. 255 (0: lossless)")
    p.add_argument("--qstep_chroma", type=int, default=None, help="quantiser step of Co and Cg (default: --qstep)")
    p.add_argument("--outdir", default='./output')
    p.add_argument("--attribute_coder", choices=sorted(CODERS), default='host',
                   help="host: the payload coded by the host range coder (_A.bin version 1); device: interleaved rANS on the GPU (version 2)")
    p.add_argument("--chunk_steps", type=int, default=CHUNK_STEPS, help="device coder: steps per chunk of 64 lanes (0: one chunk)")
    p.add_argument("--voxelize", metavar='B', type=int, default=None,
                   help="the files are raw clouds (float coordinates in any unit, ASCII or binary PLY, several points per voxel): voxelise "
                        "each to B bits first (voxelize.py; _vox.ply and _V.bin are written), then code _vox.ply")
    p.add_argument("--merge", choices=('mean', 'first'), default='mean', help="with --voxelize: the colour of a voxel, the mean of its points or its first point")
    p.add_argument("--devoxelize", action='store_true', help="with --voxelize: also write _dec_units.ply, the decoded cloud in the input's units (by _V.bin)")
    from . import clean
    clean.add_arguments(p)
    args = p.parse_args(argv)
    if args.voxelize is not None and not 1 <= args.voxelize <= 20:
        p.error(f'--voxelize {args.voxelize}: a bit depth in 1 .. 20')
    if args.devoxelize and args.voxelize is None:
        p.error('--devoxelize needs --voxelize')
    clean.check_arguments(p, args)
    raw = []
    if args.voxelize is not None:                        # every raw cloud becomes its _vox.ply; the flow below takes those files
        from . import voxelize
        raw = [voxelize.in_front(f, args.outdir, args.voxelize, args.merge) for f in args.filedir]
        args.filedir = [vox for vox, _ in raw]
    if args.clean is not None:                           # every voxelised cloud becomes its _clean.ply
        args.filedir = [clean.in_front(f, args.outdir, args) for f in args.filedir]
        raw = [(f, raw_prefix) for f, (_, raw_prefix) in zip(args.filedir, raw)]
    if len(args.filedir) == 1:
        run(args.filedir[0], args.outdir, args.qstep, args.qstep_chroma, args.attribute_coder, args.chunk_steps)
    else:
        run_batch(args.filedir, args.outdir, args.qstep, args.qstep_chroma, args.attribute_coder, args.chunk_steps)
    if args.devoxelize:
        for vox, raw_prefix in raw:
            voxelize.write_units(raw_prefix, os.path.join(args.outdir, os.path.split(vox)[-1].split('.')[0]) + '_dec.ply')


if __name__ == '__main__':
    main()
