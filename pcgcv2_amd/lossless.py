"""Lossless mode: the lossy codec's four files plus `_O.bin`, the true occupancy of every candidate voxel of the three decoder levels,
range-coded under the probability the decoder's own logit gives it (occupancy_model.py).  A lossy decoder still decodes the four files;
a lossless one reads `_O.bin` as well, prunes by the coded bits instead of by top-k, and returns the input's voxel set exactly.

Why it works: the decoder's kernels are bit-for-bit reproducible (no floating-point atomics, one fmaf chain per output row whatever kernel
family runs it), so an encoder that runs the decoder network on the latent AS THE DECODER RECONSTRUCTS IT — from the int16 symbols and
min_v, on the sorted stride-8 level — and prunes every level by the truth sees the very logits the decoder will see.  Both sides go through
the same two functions below (`_latent_level`, `_logits`).

`_O.bin`, little endian:
    4s  magic "PCGL" | u32 version (1) | u32 CRC-32 of the format tables (occupancy_model.table_crc)
    3 x (u64 candidate rows, u64 payload bytes)          levels at stride 4, 2, 1; rows of level l + 1 = 8 x occupied rows of level l
    3 payloads                                           ops.rc_encode_ctx of the level's bits (0 empty, 1 occupied) in candidate-row
                                                         order, symbol i under CDF row ctx[i]
Level l + 1's contexts need level l decoded, so the payloads are separate streams.

Version 2 (`occupancy_coder='device'`) keeps the head and the table and codes each payload ON THE DEVICE by interleaved rANS
(csrc/occupancy_rans.hip; the layout is in include/pcgc_hip.h): the context words never leave the device, the decoded bits never reach the
host, only the coded bytes cross the bus.  A payload is cut into chunks of 64 x S rows, one wave each; every chunk costs up to 64 x 64 + 32
bits beyond its ideal length, so S (`chunk_steps`, recorded in the stream) trades rate against parallelism.  `decode` reads either version
whatever the constructor said.

Integrity.  A version-1 payload is decoded and coded again, and must give the same bytes: every cut, extended or damaged stream is
refused.  Version 2 has the check rANS offers: per chunk, the stored states must lie in [2^31, 2^63), exactly the declared number of words
must be consumed and all 64 lanes must end at their initial state 2^31.  The tables' lengths are checked against the file, so cuts and
extensions are refused; damage inside a chunk's words escapes when the lanes that read it still end at 2^31 with the word count intact —
unlikely (a damaged lane has to land on one value of 2^32 and more), not impossible.  A decoder that needs certainty asks for version 1.

Batches.  `encode_batch`, `estimate_batch` and `decode_batch` code the items of a collated batch (sequences, the octant blocks of a large
cloud) in one pass: Coder.encode_batch / the batch's latent, then the decoder network ONCE per level on the batch, whose levels are the
concatenation of the items' levels.  Item b's candidates of a level are a contiguous run of rows, so ops.occ_symbols_segments keeps one
pair of sums per item and the device coder (ops.occ_rans_encode_batch / occ_rans_decode_batch) one payload per item, its chunks beside the
other items' in the same launches, never straddling items.  Every file is byte for byte what `encode` of the item alone writes, in both
versions and at every `chunk_steps`; a decode_batch may mix versions, and either side reads the other's files.

    python -m pcgcv2_amd.lossless --ckptdir CKPT --filedir CLOUD.ply [--outdir DIR] [--occupancy_coder {host,device}] [--chunk_steps S]
    python -m pcgcv2_amd.lossless --ckptdir CKPT --filedir A.ply B.ply C.ply ...      up to 16 files, coded as one batch
"""
import os
import struct
import time

import numpy as np
import torch

from . import occupancy_model, ops
from ._lib import PcgcError
from .coder import Coder, _batch_pool, _check_batch_size, _dump, _slurp, stream_bits, STREAMS
from .data_utils import isin_mask
from .sparse import CoordMap, SparseTensor, require_gpu

SUFFIX = '_O.bin'
MAGIC, VERSION = b'PCGL', 1
VERSION_DEVICE = 2                                # payloads coded by ops.occ_rans_encode
CODERS = {'host': VERSION, 'device': VERSION_DEVICE}
CHUNK_STEPS = 4096                                # S of a version-2 payload unless the caller says otherwise
_HEAD = struct.Struct('<4sII')
_LEVELS = struct.Struct('<6Q')                    # (rows, bytes) of the three levels
LEVELS = 3


class LosslessCoder():
    """Coder(model, filename) plus the occupancy stream.  encode / estimate / decode: one frame per call; the _batch methods: a collated
    batch.  occupancy_coder: 'host' writes version 1 (the host range
    coder), 'device' version 2 (rANS on the device) in chunks of 64 x chunk_steps rows (None: CHUNK_STEPS; 0: one chunk per level)."""

    def __init__(self, model, filename, occupancy_coder='host', chunk_steps=None):
        if occupancy_coder not in CODERS:
            raise ValueError(f'occupancy_coder {occupancy_coder!r}: one of {sorted(CODERS)}')
        self.occupancy_coder = occupancy_coder
        self.chunk_steps = CHUNK_STEPS if chunk_steps is None else int(chunk_steps)
        if not 0 <= self.chunk_steps <= ops.RANS_MAX_STEPS:
            raise ValueError(f'chunk_steps {chunk_steps}: 0 (one chunk per level) or 1 .. 2^24')
        self.model = model
        self.filename = filename
        self.coder = Coder(model, filename)
        self._cdf = occupancy_model.cdf_rows()
        self.times = None                         # measurement hook (tools/lossless_time.py): a dict -> seconds per phase, with synchronisation

    # ---- measurement hook ---------------------------------------------------------------------------------------------------------------
    def _tick(self, phase, t0, dev=None):
        if self.times is None:
            return 0.0
        if dev is not None:
            torch.cuda.synchronize(dev)
        now = time.perf_counter()
        if phase is not None:
            self.times[phase] = self.times.get(phase, 0.0) + now - t0
        return now

    # ---- what both sides run ------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _latent_level(sym_d, min_v, coords8):
        """the latent as a decoder holds it: features from the int16 symbols and min_v, on the sorted stride-8 level"""
        lvl8 = coords8 if isinstance(coords8, CoordMap) else CoordMap(coords8, 8, unique=True)
        if len(lvl8) != sym_d.shape[0]:
            raise PcgcError(f'{len(lvl8)} stride-8 coordinates but {sym_d.shape[0]} latent rows')
        if len(lvl8) and lvl8._prepared_up is None:
            lvl8.prepare_up()
        if not isinstance(min_v, (list, tuple)):
            return SparseTensor(features=ops.desymbolize(sym_d, min_v), coordinate_map=lvl8)
        # a batch: every item has its own symbol offset (Coder._decode_batch_latent builds the same rows on the decoder's side)
        feats, off = torch.empty(sym_d.shape, dtype=torch.float32, device=sym_d.device), 0
        for rows, lo in zip(lvl8.batch_rows, min_v):
            feats[off:off + rows] = ops.desymbolize(sym_d[off:off + rows], lo)
            off += rows
        return SparseTensor(features=feats, coordinate_map=lvl8)

    def _logits(self, out, l):
        """decoder level l up to its classification head -> (candidates with their features, logits [8 n, 1])"""
        dec = self.model.decoder
        out = getattr(dec, f'up{l}')(out, relu=True)
        out = getattr(dec, f'conv{l}')(out, relu=True)
        out = getattr(dec, f'block{l}')(out)
        return out, getattr(dec, f'conv{l}_cls')(out).F

    # ---- encoder ------------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _single_frame(x):
        if not isinstance(x, SparseTensor):
            raise TypeError('LosslessCoder codes a SparseTensor')
        if len(x) == 0:
            raise ValueError('LosslessCoder: an empty cloud')
        if len(x.cmap.batch_rows) != 1:
            raise ValueError(f'LosslessCoder codes one frame at a time; got a batch of {len(x.cmap.batch_rows)} items')

    def _truth_levels(self, x):
        """the encoder pyramid's levels at stride 4, 2, 1 (of the cloud as Coder.encode ingests it: the sets are the input's)"""
        xi = self.coder._ingest(x)
        xi.cmap.build_pyramid(3)
        l2 = xi.cmap.down()[0]
        return xi, [l2.down()[0], l2, xi.cmap]

    def _enhance(self, x, y, code):
        """run the decoder network on the latent y (sorted, as Coder.encode returns it) under teacher forcing by the truth alone
        -> (record, payloads or None)"""
        dev = x.device
        t = self._tick(None, 0.0, dev)
        _, truths = self._truth_levels(x)
        min_v, _, sym_h = ops.quantize_symbols(y.F)
        out = self._latent_level(torch.from_numpy(sym_h).to(dev), min_v, y.C)
        t = self._tick('copies', t, dev)
        rows, units, payloads, chunks = [], 0, [], []
        on_device = code and self.occupancy_coder == 'device'
        for l in range(LEVELS):
            out, logits = self._logits(out, l)
            truth = isin_mask(out.cmap.C, truths[l])
            t = self._tick('network', t, dev)
            packed, sums = ops.occ_symbols(logits, truth)
            t = self._tick('k_occ_symbols', t, dev)
            candidates = packed.shape[0]
            if on_device:                         # the words stay on the device; the counts come with the payload's length
                steps = self.chunk_steps or max(1, ops.occ_rans_chunks(candidates, 1))
                payload, occupied, cost = ops.occ_rans_encode(packed, steps, sums)
                chunks.append(ops.occ_rans_chunks(candidates, steps))
                t = self._tick('k_occ_rans_encode', t, dev)
            else:
                words, occupied, cost = ops.occ_words_host(packed, sums)
                t = self._tick('copies', t, dev)
            if occupied != len(truths[l]):
                raise PcgcError(f'lossless encode: level {l} holds {len(truths[l])} voxels but {occupied} of its {candidates} candidates are '
                                'among them: the input is not a set of distinct voxels of one frame')
            rows.append(candidates)
            units += cost
            if on_device:
                payloads.append(payload)
            elif code:
                payloads.append(ops.rc_encode_ctx(self._cdf, words >> 1, words & 1))
                t = self._tick('host coder', t)
            out = self.model.decoder.pruning(out, truth, n_keep=occupied)
            t = self._tick('network', t, dev)
        record = {'est_units_O': units, 'est_bits_O': units / occupancy_model.COST_UNIT, 'rows': rows}
        if on_device:
            record['chunks'] = chunks
        return record, payloads

    @torch.no_grad()
    def encode(self, x, postfix=''):
        """Coder.encode(x, postfix) unchanged, then `_O.bin` -> {bits_O, est_bits_O, rows (candidates per level), ...}"""
        self._single_frame(x)
        with torch.cuda.device(x.device):
            t = self._tick(None, 0.0, x.device)
            y = self.coder.encode(x, postfix)
            self._tick('lossy encode', t, x.device)
            record, payloads = self._enhance(x, y, code=True)
            t = self._tick(None, 0.0)
            sizes = [v for r, p in zip(record['rows'], payloads) for v in (r, len(p))]
            blob = _HEAD.pack(MAGIC, CODERS[self.occupancy_coder], occupancy_model.table_crc()) + _LEVELS.pack(*sizes) + b''.join(payloads)
            _dump(self.filename + postfix + SUFFIX, blob)
            self._tick('host coder', t)
        record['bits_O'] = 8 * len(blob)
        record['payload_bytes'] = [len(p) for p in payloads]
        return record

    @torch.no_grad()
    def estimate(self, x):
        """est_bits_O of encode(x) — the ideal length of the occupancy stream in bits — without writing anything"""
        self._single_frame(x)
        with torch.cuda.device(x.device):
            xi, _ = self._truth_levels(x)
            lvl8 = xi.cmap.build_pyramid(3)
            y_list = self.model.encoder(xi)
            order = ops.sort_zyx(lvl8.C)                                     # (the order Coder.encode codes the latent in)
            y = SparseTensor(ops.gather_feats(y_list[0].F, order), coordinate_map=CoordMap(ops.gather_coords(lvl8.C, order), lvl8.stride, unique=True))
            return self._enhance(x, y, code=False)[0]['est_bits_O']

    # ---- encoder, collated batches -------------------------------------------------------------------------------------
    # B clouds through ONE pass: Coder.encode_batch, then the decoder network once per level on the batch.  A level's candidates are 8 per
    # parent in parent order, so item b is the contiguous rows [row[b], row[b + 1]); the batch index is part of every coordinate, so the truth
    # mask is per item; ops.occ_symbols_segments and ops.occ_rans_encode_batch keep one pair of sums and one payload per item.  Every file is
    # byte for byte what encode() of the item alone writes: a context depends on its own logit, a logit on its own item's rows only.
    def _enhance_batch(self, x, y, code):
        """_enhance over a collated batch -> (one record per item, one list of three payloads per item, or None)"""
        dev = x.device
        t = self._tick(None, 0.0, dev)
        _, truths = self._truth_levels(x)
        B = len(y.cmap.batch_rows)
        ranges, sym_h = ops.quantize_symbols_segments(y.F, y.cmap.batch_rows)
        out = self._latent_level(torch.from_numpy(sym_h).to(dev), [lo for lo, _ in ranges], y.cmap)
        t = self._tick('copies', t, dev)
        on_device = code and self.occupancy_coder == 'device'
        records = [{'est_units_O': 0, 'rows': []} for _ in range(B)]
        payloads, pending = [[] for _ in range(B)], []
        for l in range(LEVELS):
            out, logits = self._logits(out, l)
            truth = isin_mask(out.cmap.C, truths[l])
            t = self._tick('network', t, dev)
            rows, want = out.cmap.batch_rows, truths[l].batch_rows
            packed, sums = ops.occ_symbols_segments(logits, rows, truth)
            t = self._tick('k_occ_symbols', t, dev)
            if on_device:                         # the words and the finished payloads stay on the device; lengths and counts come in one small copy
                lay = ops.occ_rans_batch_layout(rows, self.chunk_steps)
                coded, occupied, cost = ops.occ_rans_encode_batch(packed, rows, self.chunk_steps, sums, fetch=False)
                t = self._tick('k_occ_rans_encode', t, dev)
            else:
                words, occupied, cost = ops.occ_words_host_segments(packed, sums)
                t = self._tick('copies', t, dev)
            for b in range(B):
                if occupied[b] != want[b]:
                    raise PcgcError(f'lossless encode_batch: item {b}: level {l} holds {want[b]} voxels but {int(occupied[b])} of its {rows[b]} '
                                    'candidates are among them: the item is not a set of distinct voxels of one frame')
                records[b]['rows'].append(int(rows[b]))
                records[b]['est_units_O'] += int(cost[b])
                if on_device:
                    records[b].setdefault('chunks', []).append(int(lay['chunks'][b]))
            if on_device:
                pending.append(coded)
            elif code:
                edge = np.concatenate([[0], np.cumsum(rows)])
                coded = list(_batch_pool().map(lambda b: ops.rc_encode_ctx(self._cdf, words[edge[b]:edge[b + 1]] >> 1, words[edge[b]:edge[b + 1]] & 1),
                                               range(B)))
                for b in range(B):
                    payloads[b].append(coded[b])
                t = self._tick('host coder', t)
            out = self.model.decoder.pruning(out, truth, n_keep=int(sum(want)), keep_per_item=list(want))
            t = self._tick('network', t, dev)
        if pending:                               # the three levels' payloads in one copy, after the last level's launches
            for level in ops.occ_rans_payloads(pending):
                for b in range(B):
                    payloads[b].append(level[b])
            t = self._tick('copies', t, dev)
        for r in records:
            r['est_bits_O'] = r['est_units_O'] / occupancy_model.COST_UNIT
        return records, payloads if code else None

    @torch.no_grad()
    def encode_batch(self, x, postfixes):
        """x: collated sparse tensor (item index in column 0, items contiguous, 1 to coder.MAX_BATCH_ITEMS items); postfixes[b]: file postfix
        of item b.  Coder.encode_batch(x, postfixes), then one `_O.bin` per item -> a list of encode()'s records.  Every file is byte for byte
        what encode() of the item alone writes.  PcgcError naming the item whose occupied count disagrees with its truth level."""
        postfixes = _check_items(x, postfixes, 'encode_batch')
        with torch.cuda.device(x.device):
            t = self._tick(None, 0.0, x.device)
            if len(x.cmap.batch_rows) != len(postfixes):
                raise ValueError(f'encode_batch: {len(postfixes)} postfixes for a batch of {len(x.cmap.batch_rows)} items')
            y = self.coder.encode_batch(x, postfixes)
            self._tick('lossy encode', t, x.device)
            records, payloads = self._enhance_batch(x, y, code=True)
            t = self._tick(None, 0.0)
            for record, mine, postfix in zip(records, payloads, postfixes):
                sizes = [v for r, p in zip(record['rows'], mine) for v in (r, len(p))]
                blob = _HEAD.pack(MAGIC, CODERS[self.occupancy_coder], occupancy_model.table_crc()) + _LEVELS.pack(*sizes) + b''.join(mine)
                _dump(self.filename + postfix + SUFFIX, blob)
                record['bits_O'] = 8 * len(blob)
                record['payload_bytes'] = [len(p) for p in mine]
            self._tick('host coder', t)
        return records

    @torch.no_grad()
    def estimate_batch(self, x):
        """est_bits_O of every item of a collated batch, each equal to estimate() of the item alone, without writing anything"""
        _check_items(x, None, 'estimate_batch')
        with torch.cuda.device(x.device):
            xi, _ = self._truth_levels(x)
            lvl8 = xi.cmap.build_pyramid(3)
            _check_batch_size(len(lvl8.batch_rows), 'estimate_batch')
            y_list = self.model.encoder(xi)
            order = ops.sort_zyx(lvl8.C, batch_major=True)                   # (the order Coder.encode_batch codes the latent in)
            cmap = CoordMap(ops.gather_coords(lvl8.C, order), lvl8.stride, unique=True)
            cmap._batch_rows = list(lvl8.batch_rows)
            y = SparseTensor(ops.gather_feats(y_list[0].F, order), coordinate_map=cmap)
            return [r['est_bits_O'] for r in self._enhance_batch(x, y, code=False)[0]]

    # ---- decoder ------------------------------------------------------------------------------------------------------------------------
    def _read_stream(self, postfix):
        """-> (candidate rows, payloads) of the three levels, of either version"""
        return self._read_versioned(postfix)[1:]

    def _read_versioned(self, postfix):
        """-> (version, candidate rows, payloads); a version-2 payload's head and tables are checked against its rows and size here"""
        path = self.filename + postfix + SUFFIX
        blob = _slurp(path)
        if len(blob) < _HEAD.size + _LEVELS.size:
            raise PcgcError(f'{path}: {len(blob)} bytes, shorter than its header')
        magic, version, crc = _HEAD.unpack_from(blob, 0)
        if magic != MAGIC:
            raise PcgcError(f'{path}: not an occupancy stream (magic {magic!r})')
        if version not in CODERS.values():
            raise PcgcError(f'{path}: version {version}; this decoder reads versions {sorted(CODERS.values())}')
        if crc != occupancy_model.table_crc():
            raise PcgcError(f'{path}: coded with other probability tables (CRC-32 {crc:08x}, here {occupancy_model.table_crc():08x})')
        sizes = _LEVELS.unpack_from(blob, _HEAD.size)
        rows, nbytes = sizes[0::2], sizes[1::2]
        if len(blob) != _HEAD.size + _LEVELS.size + sum(nbytes):
            raise PcgcError(f'{path}: {len(blob)} bytes, but the header declares payloads of {list(nbytes)} bytes')
        offs = np.cumsum([_HEAD.size + _LEVELS.size] + list(nbytes))
        payloads = [blob[offs[l]:offs[l + 1]] for l in range(LEVELS)]
        if version == VERSION_DEVICE:
            for l in range(LEVELS):
                try:
                    ops.occ_rans_layout(payloads[l], rows[l])
                except PcgcError as e:
                    raise PcgcError(f'{path}: level {l}: {e}') from None
        return version, rows, payloads

    @torch.no_grad()
    def decode(self, postfix=''):
        """reads `_C.bin`, `_F.bin`, `_H.bin` and `_O.bin` (either version) -> the stride-1 sparse tensor whose coordinate set is the
        input's.  Raises PcgcError on a stream that is cut, extended or inconsistent.  A version-1 stream with damaged payload bytes is
        always refused, never decoded to a cloud; a version-2 stream is refused when a chunk fails its check (the module docstring says
        what that check can and cannot see)."""
        dev = require_gpu(next(self.model.decoder.parameters()).device)
        with torch.cuda.device(dev):
            return self._decode(postfix, dev)

    def _decode(self, postfix, dev):
        t = self._tick(None, 0.0, dev)
        version, rows, payloads = self._read_versioned(postfix)
        fc = self.coder.feature_coder
        sym_h, min_v = fc.decode_symbols(postfix=postfix, device=dev)
        lvl8 = self.coder._decode_geometry(postfix, dev, torch.cuda.current_stream(dev))
        t = self._tick('host coder', t, dev)
        out = self._latent_level(torch.from_numpy(np.ascontiguousarray(sym_h)).to(dev), min_v, lvl8)
        t = self._tick('copies', t, dev)
        parents = len(out)
        for l in range(LEVELS):
            if rows[l] != 8 * parents:
                raise PcgcError(f'{self.filename + postfix + SUFFIX}: level {l} declares {rows[l]} candidate rows; the level above has '
                                f'{parents} voxels, i.e. {8 * parents} candidates')
            out, logits = self._logits(out, l)
            t = self._tick('network', t, dev)
            packed, _ = ops.occ_symbols(logits)
            t = self._tick('k_occ_symbols', t, dev)
            if version == VERSION_DEVICE:         # the bits never reach the host: the mask is the kernel's
                try:
                    mask, parents = ops.occ_rans_decode(packed, payloads[l], rows[l])
                except PcgcError as e:
                    raise PcgcError(f'{self.filename + postfix + SUFFIX}: level {l}: {e}') from None
                t = self._tick('k_occ_rans_decode', t, dev)
            else:
                words, _, _ = ops.occ_words_host(packed, None)
                t = self._tick('copies', t, dev)
                bits = ops.rc_decode_ctx(self._cdf, words >> 1, payloads[l])
                t = self._tick('host coder', t)
                parents = int(bits.sum())
                mask = torch.from_numpy(bits.astype(np.uint8)).to(dev)
                t = self._tick('copies', t, dev)
            if parents == 0:
                raise PcgcError(f'{self.filename + postfix + SUFFIX}: level {l} decodes to no voxel at all')
            out = self.model.decoder.pruning(out, mask, n_keep=parents)
            t = self._tick('network', t, dev)
        return out


    # ---- decoder, collated batches --------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def decode_batch(self, postfixes):
        """reads the files of every item (each `_O.bin` in the version it has) and decodes them in ONE decoder pass -> list of stride-1
        sparse tensors (batch column 0 each), equal to decode() of the item alone.  Every host check of every item — magic, version, CRC,
        lengths, the version-2 heads, rows of the first level against the item's latent — runs before the batch's level is uploaded;
        rows of a later level are checked against the level above once that is decoded.  A refusal names the item's file and the level."""
        postfixes = _check_items(None, postfixes, 'decode_batch')
        dev = require_gpu(next(self.model.decoder.parameters()).device)
        with torch.cuda.device(dev):
            return self._decode_batch(postfixes, dev)

    def _decode_batch(self, postfixes, dev):
        t = self._tick(None, 0.0, dev)
        B = len(postfixes)
        paths = [self.filename + p + SUFFIX for p in postfixes]
        streams = [self._read_versioned(p) for p in postfixes]               # (version, rows, payloads) per item, checked
        for b, (_, rows, _) in enumerate(streams):
            for l in range(1, LEVELS):                                       # rows of a level = 8 x occupied rows of the level above: at least a multiple of 8
                if rows[l] % 8:
                    raise PcgcError(f'{paths[b]}: level {l} declares {rows[l]} candidate rows, not a multiple of 8')

        def against(level, parents):
            for b in range(B):
                if streams[b][1][level] != 8 * parents[b]:
                    raise PcgcError(f'{paths[b]}: level {level} declares {streams[b][1][level]} candidate rows; the level above has '
                                    f'{parents[b]} voxels, i.e. {8 * parents[b]} candidates')

        out, _ = self.coder._decode_batch_latent(postfixes, dev, on_rows=lambda rows8: against(0, rows8))
        t = self._tick('host coder', t, dev)
        device_items = [b for b in range(B) if streams[b][0] == VERSION_DEVICE]
        host_items = [b for b in range(B) if streams[b][0] != VERSION_DEVICE]
        parents = list(out.cmap.batch_rows)
        for l in range(LEVELS):
            against(l, parents)
            out, logits = self._logits(out, l)
            t = self._tick('network', t, dev)
            rows = out.cmap.batch_rows
            edge = np.concatenate([[0], np.cumsum(rows)])
            packed, _ = ops.occ_symbols_segments(logits, rows)
            mask = torch.empty(int(edge[-1]), dtype=torch.uint8, device=dev)
            t = self._tick('k_occ_symbols', t, dev)
            if device_items:                      # one launch sequence for the version-2 items; the bits never reach the host
                _, occupied = ops.occ_rans_decode_batch(packed, rows, [streams[b][2][l] if streams[b][0] == VERSION_DEVICE else None for b in range(B)],
                                                        mask=mask, names=[f'{path}: level {l}' for path in paths])
                parents = [int(v) for v in occupied]
                t = self._tick('k_occ_rans_decode', t, dev)
            if host_items:                        # one copy of the contexts down, the items' payloads on the pool, their bits up in one copy
                words = packed.cpu().numpy().view(np.uint16)
                t = self._tick('copies', t, dev)

                def one(b):
                    try:
                        return ops.rc_decode_ctx(self._cdf, words[edge[b]:edge[b + 1]] >> 1, streams[b][2][l])
                    except PcgcError as e:
                        raise PcgcError(f'{paths[b]}: level {l}: {e}') from None
                bits = list(_batch_pool().map(one, host_items))
                t = self._tick('host coder', t)
                up = torch.from_numpy(np.concatenate(bits).astype(np.uint8)).to(dev)
                at = 0
                for b, mine in zip(host_items, bits):
                    mask[edge[b]:edge[b + 1]] = up[at:at + len(mine)]
                    at += len(mine)
                    parents[b] = int(mine.sum())
                t = self._tick('copies', t, dev)
            for b in range(B):
                if parents[b] == 0:
                    raise PcgcError(f'{paths[b]}: level {l} decodes to no voxel at all')
            out = self.model.decoder.pruning(out, mask, n_keep=sum(parents), keep_per_item=parents)
            t = self._tick('network', t, dev)
        return Coder._split_items(out)


def _check_items(x, postfixes, what):
    """the arguments of a batch call that the host can judge -> the postfixes as a list"""
    if postfixes is not None:
        postfixes = list(postfixes)
        _check_batch_size(len(postfixes), what)
        if len(set(postfixes)) != len(postfixes):
            raise ValueError(f'{what}: the postfixes name the items\' files and must differ, got {postfixes}')
    if x is not None or postfixes is None:
        if not isinstance(x, SparseTensor):
            raise TypeError('LosslessCoder codes a SparseTensor')
        if len(x) == 0:
            raise ValueError('LosslessCoder: an empty cloud')
    return postfixes


def occupancy_bits(prefix, postfix=''):
    """bits of `_O.bin` of one coded cloud"""
    return os.path.getsize(prefix + postfix + SUFFIX) * 8


def same_voxels(a, b):
    """True iff two [n, 4] coordinate tensors hold the same set of rows"""
    if a.shape != b.shape:
        return False
    a, b = a.contiguous(), b.contiguous()
    return bool(torch.equal(ops.gather_coords(a, ops.sort_zyx(a)), ops.gather_coords(b, ops.sort_zyx(b))))


# ------------------------------------------------------------------------------------------------ CLI
def run(ckptdir, filedir, outdir, occupancy_coder='host', chunk_steps=None, attributes=None, attribute_coder='host'):
    """encode, decode, check set equality, print the bpp of each file and the total.  attributes = (Q, Qc): also `_A.bin`, the file's colours
    on the decoded (= the input's) voxel set (attributes.py), its payload coded by attribute_coder ('host' or 'device'); `_dec.ply` then
    carries the colours decoded from it."""
    from .coder import device, _Stopwatch, _code_attributes
    from .data_utils import load_sparse_tensor, write_ply_ascii_geo, write_ply_ascii_geo_rgb
    from .pcc_model import PCCModel
    x = load_sparse_tensor(filedir, device)
    os.makedirs(outdir, exist_ok=True)
    prefix = os.path.join(outdir, os.path.split(filedir)[-1].split('.')[0])
    print(prefix)
    if not os.path.exists(ckptdir):
        raise FileNotFoundError(ckptdir)
    model = PCCModel().to(device)
    model.load_state_dict(torch.load(ckptdir, map_location=device)['model'])
    print('load checkpoint from \t', ckptdir)
    coder = LosslessCoder(model=model, filename=prefix, occupancy_coder=occupancy_coder, chunk_steps=chunk_steps)
    with _Stopwatch('Enc Time'):
        record = coder.encode(x)
    with _Stopwatch('Dec Time'):
        x_dec = coder.decode()
    exact = same_voxels(x.C, x_dec.C)
    names = STREAMS + (SUFFIX,)
    bits = np.append(stream_bits(prefix), occupancy_bits(prefix))
    bpps = (bits / len(x)).round(3)
    for name, b, bpp in zip(names, bits, bpps):
        print(f'{name}:\t {b} bits\t {bpp} bpp')
    print('bits:\t', sum(bits), '\nbpps:\t', sum(bpps).round(3))
    print('ideal bits of _O.bin:\t', round(record['est_bits_O'], 1), '\ncandidate rows:\t', record['rows'])
    print('lossless:\t', 'exact' if exact else 'MISMATCH')
    if attributes is not None:
        rgb_dec, colour, bits_a = _code_attributes(filedir, prefix, x_dec, attributes, attribute_coder)
        print('bits _A.bin:\t', bits_a, '\nbpp _A.bin:\t', round(bits_a / len(x), 3))
        print('Colour PSNR (Y):\t', colour['c[0],PSNRF'])
        write_ply_ascii_geo_rgb(prefix + '_dec.ply', x_dec.C.detach().cpu().numpy()[:, 1:], rgb_dec.cpu().numpy())
    else:
        write_ply_ascii_geo(prefix + '_dec.ply', x_dec.C.detach().cpu().numpy()[:, 1:])
    if not exact:
        raise PcgcError(f'{prefix}: the decoded voxel set differs from the input ({len(x_dec)} against {len(x)} voxels)')
    return record


def run_batch(ckptdir, filedirs, outdir, occupancy_coder='host', chunk_steps=None, attributes=None, attribute_coder='host'):
    """several clouds collated into one batch and coded with encode_batch / decode_batch: per file the lines of run and its `_dec.ply`.
    attributes = (Q, Qc): the files' colours on the decoded voxel sets through AttributeCoder.encode_batch / decode_batch."""
    from .coder import device, _Stopwatch
    from .data_utils import load_sparse_tensor, read_ply_ascii_with_colours, write_ply_ascii_geo, write_ply_ascii_geo_rgb
    from .pcc_model import PCCModel
    filedirs = list(filedirs)
    _check_batch_size(len(filedirs), 'run_batch')
    names = [os.path.split(f)[-1].split('.')[0] for f in filedirs]
    if len(set(names)) != len(names):
        raise ValueError(f'{names}: the files of a batch need distinct names, they name the outputs')
    clouds = [load_sparse_tensor(f, device) for f in filedirs]
    coords = torch.cat([torch.cat([torch.full_like(x.C[:, :1], b), x.C[:, 1:]], 1) for b, x in enumerate(clouds)]).contiguous()
    batch = SparseTensor(torch.ones((len(coords), 1), device=device), coordinates=coords, tensor_stride=1, device=device)
    os.makedirs(outdir, exist_ok=True)
    prefix = os.path.join(outdir, '')
    if not os.path.exists(ckptdir):
        raise FileNotFoundError(ckptdir)
    model = PCCModel().to(device)
    model.load_state_dict(torch.load(ckptdir, map_location=device)['model'])
    print('load checkpoint from \t', ckptdir)
    coder = LosslessCoder(model=model, filename=prefix, occupancy_coder=occupancy_coder, chunk_steps=chunk_steps)
    with _Stopwatch('Enc Time'):
        records = coder.encode_batch(batch, names)
    with _Stopwatch('Dec Time'):
        decoded = coder.decode_batch(names)
    colours = None
    if attributes is not None:
        from .attributes import AttributeCoder
        from .pc_error import colour_psnr_device, lattice_coords, nn_both, recolour_device
        carried, inputs = [], []
        for b, f in enumerate(filedirs):
            xyz, rgb = read_ply_ascii_with_colours(f)
            if rgb is None:
                raise ValueError(f'{f} has no colours (red green blue): --attributes needs them')
            mine = decoded[b].C.detach().contiguous()
            a, ca = lattice_coords(xyz, device), torch.from_numpy(rgb).to(device)
            nn = nn_both(a, mine)
            carried.append(recolour_device(a, ca, mine, nn=nn))
            inputs.append((a, ca, nn))
        where = torch.cat([torch.cat([torch.full_like(d.C[:, :1], b), d.C[:, 1:]], 1) for b, d in enumerate(decoded)]).contiguous()
        attribute_coder_ = AttributeCoder(prefix, attribute_coder=attribute_coder)
        records_a = attribute_coder_.encode_batch(where, torch.cat(carried), *attributes, postfixes=names)
        colours = attribute_coder_.decode_batch(where, postfixes=names)
    wrong, at = [], 0
    for b, (x, x_dec) in enumerate(zip(clouds, decoded)):
        stem = prefix + names[b]
        print(stem)
        exact = same_voxels(x.C, x_dec.C)
        bits = np.append(stream_bits(stem), occupancy_bits(stem))
        bpps = (bits / len(x)).round(3)
        for name, n_bits, bpp in zip(STREAMS + (SUFFIX,), bits, bpps):
            print(f'{name}:\t {n_bits} bits\t {bpp} bpp')
        print('bits:\t', sum(bits), '\nbpps:\t', sum(bpps).round(3))
        print('ideal bits of _O.bin:\t', round(records[b]['est_bits_O'], 1), '\ncandidate rows:\t', records[b]['rows'])
        print('lossless:\t', 'exact' if exact else 'MISMATCH')
        if colours is not None:
            rgb_dec = colours[at:at + len(x_dec)]
            at += len(x_dec)
            a, ca, nn = inputs[b]
            print('bits _A.bin:\t', records_a[b]['bits_A'], '\nbpp _A.bin:\t', round(records_a[b]['bits_A'] / len(x), 3))
            print('Colour PSNR (Y):\t', colour_psnr_device(a, ca, x_dec.C.detach().contiguous(), rgb_dec, nn=nn)['c[0],PSNRF'])
            write_ply_ascii_geo_rgb(stem + '_dec.ply', x_dec.C.detach().cpu().numpy()[:, 1:], rgb_dec.cpu().numpy())
        else:
            write_ply_ascii_geo(stem + '_dec.ply', x_dec.C.detach().cpu().numpy()[:, 1:])
        if not exact:
            wrong.append(f'{stem} ({len(x_dec)} against {len(x)} voxels)')
    if wrong:
        raise PcgcError(f'the decoded voxel set differs from the input: {", ".join(wrong)}')
    return records


def main(argv=None):
    import argparse
    p = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("--ckptdir", default='ckpts/r3_0.10bpp.pth')
    p.add_argument("--filedir", default=['../../../testdata/8iVFB/longdress_vox10_1300.ply'], nargs='+',
                   help="the cloud; several files (up to 16) are collated and coded as one batch (encode_batch / decode_batch)")
    p.add_argument("--outdir", default='./output')
    p.add_argument("--occupancy_coder", choices=sorted(CODERS), default='host',
                   help="who codes _O.bin: the host range coder (version 1) or interleaved rANS on the device (version 2)")
    p.add_argument("--chunk_steps", type=int, default=None,
                   help="device coder: rows per chunk / 64 (0: one chunk per level); default lossless.CHUNK_STEPS")
    p.add_argument("--attributes", metavar='Q[,Qc]', default=None,
                   help="also write _A.bin, the colour stream (attributes.py): the files' colours on the decoded voxel sets, quantiser step Q "
                        "(Qc for chroma; 0 .. 255, 0: lossless)")
    p.add_argument("--attribute_coder", choices=('host', 'device'), default='host', help="with --attributes: who codes the payload of _A.bin")
    args = p.parse_args(argv)
    if args.attributes is not None:
        try:
            q = [int(v) for v in args.attributes.split(',')]
            if not 1 <= len(q) <= 2 or not all(0 <= v <= 255 for v in q):
                raise ValueError
        except ValueError:
            p.error(f'--attributes {args.attributes}: Q or Q,Qc with integers in 0 .. 255')
        args.attributes = (q[0], q[-1])
    if len(args.filedir) == 1:
        run(args.ckptdir, args.filedir[0], args.outdir, args.occupancy_coder, args.chunk_steps, args.attributes, args.attribute_coder)
    else:
        run_batch(args.ckptdir, args.filedir, args.outdir, args.occupancy_coder, args.chunk_steps, args.attributes, args.attribute_coder)


if __name__ == '__main__':
    main()
