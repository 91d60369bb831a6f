#!/usr/bin/env python3
"""Time of one lossless encode and decode (pcgcv2_amd/lossless.py) on the bench frame (shell10, 786 632 points), synthetic weights, warm, in
this fresh process: the median of --repeat runs end to end, next to one lossy Coder.encode + decode pair in the same process, and — from a
second set of runs with a device synchronisation between the phases — the split into network, k_occ_symbols, host coder and copies.
Also: candidate rows per level, bits of `_O.bin` against its ideal length, bpp (synthetic weights: says nothing about trained models), and
the gap between the ideal length and loss.get_bce on the same forward point.  Both forms of `_O.bin` are timed in this one process: the host
range coder (version 1) and rANS on the device (version 2, phases k_occ_rans_encode / k_occ_rans_decode) in chunks of 64 x --chunk_steps rows;
--occupancy_coder says which of the two fills the top-level figures (and the --trace run), the other is reported under `other_coder`.
With --trace it re-runs itself once under `rocprofv3 --kernel-trace --stats` (a fresh child process) and prints the k_occ_* rows.
With --batch B it does one thing instead: encode_batch + decode_batch of B translated copies of the cloud against B frame-by-frame calls,
both coders, per phase and per whole call, with bits per file and the byte / voxel equality.
    tools/lossless_time.py [--cloud NAME] [--repeat K] [--occupancy_coder {host,device}] [--chunk_steps S[,S..]] [--trace] [--batch B]"""
import argparse, csv, glob, json, os, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument('--cloud', default='shell10')
ap.add_argument('--repeat', type=int, default=7)
ap.add_argument('--occupancy_coder', choices=('host', 'device'), default='device')
ap.add_argument('--chunk_steps', default='', help='S of the device coder (0: one chunk per level); a comma-separated list adds a table of '
                'medians and sizes over these values; default: lossless.CHUNK_STEPS')
ap.add_argument('--batch', type=int, default=0, help='B: one encode_batch + decode_batch of B translated copies of the cloud against B frame-by-frame calls '
                'in this process, both coders: ms per phase and per whole call, bits per file, same bytes / same voxels (nothing else is run)')
ap.add_argument('--trace', action='store_true', help='also one rocprofv3 --kernel-trace --stats run of two encode + decode pairs (child process)')
ap.add_argument('--one-call', action='store_true', help=argparse.SUPPRESS)
args = ap.parse_args()


def trace_table():
    with tempfile.TemporaryDirectory() as d:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '--', sys.executable, os.path.abspath(__file__),
               '--cloud', args.cloud, '--occupancy_coder', args.occupancy_coder, '--chunk_steps', args.chunk_steps, '--one-call']
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise SystemExit('rocprofv3 failed:\n' + r.stderr[-2000:])
        rows = []
        for path in glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True):
            rows += list(csv.DictReader(open(path)))
    return [{'kernel': r['Name'][:60], 'calls': int(r['Calls']), 'total_us': round(float(r['TotalDurationNs']) / 1e3, 1),
             'mean_us': round(float(r['AverageNs']) / 1e3, 1)} for r in rows if 'k_occ_' in r.get('Name', '')]


import numpy as np
import torch
import pcgcv2_amd
pcgcv2_amd.configure_host_threads()
from pcgcv2_amd import lossless, ops, synthetic
from pcgcv2_amd.coder import Coder, stream_bits
from pcgcv2_amd.data_utils import isin_mask
from pcgcv2_amd.pcc_model import PCCModel
from pcgcv2_amd.sparse import SparseTensor

dev = torch.device('cuda:0')
model = PCCModel().to(dev)
model.load_state_dict(synthetic.synthetic_state_dict())
pts = synthetic.cloud(args.cloud, device=dev)
coords = torch.cat([torch.zeros((len(pts), 1), dtype=torch.int32, device=dev), pts], 1).contiguous()
x = SparseTensor(torch.ones((len(pts), 1), device=dev), coordinates=coords, tensor_stride=1, device=dev)
tmp = tempfile.TemporaryDirectory()
prefix = os.path.join(tmp.name, 'frame')
steps_list = [int(v) for v in args.chunk_steps.split(',') if v != ''] or [None]
coders = {'host': lossless.LosslessCoder(model, prefix + '_host'),
          'device': lossless.LosslessCoder(model, prefix + '_device', occupancy_coder='device', chunk_steps=steps_list[0])}
other = 'host' if args.occupancy_coder == 'device' else 'device'
exact, lossy = coders[args.occupancy_coder], Coder(model, prefix + '_lossy')

if args.one_call:
    for _ in range(2):
        exact.encode(x); exact.decode()
    torch.cuda.synchronize()
    raise SystemExit(0)


def median_ms(fn, runs):
    fn(); torch.cuda.synchronize()                                    # (warm: code objects, derived tables, allocator)
    times = []
    for _ in range(runs):
        torch.cuda.synchronize(); t = time.perf_counter(); fn(); torch.cuda.synchronize(); times.append(time.perf_counter() - t)
    return round(float(np.median(times)) * 1e3, 3)


def phases_ms(fn, runs, coder=None):
    coder = coder or exact
    out = []
    for _ in range(runs):
        coder.times = {}
        fn(); torch.cuda.synchronize()
        out.append(coder.times)
    coder.times = None
    return {k: round(float(np.median([o.get(k, 0.0) for o in out])) * 1e3, 3) for k in out[0]}


def batch_report(B):
    """B copies of the cloud, each translated by a few voxels (so that levels, contexts and payloads differ), as one collated batch against
    the same B clouds frame by frame (the single-frame path), in this one process"""
    runs = max(args.repeat, 5)
    shifts = [torch.tensor([0, 3 * b, 5 * b, 7 * b], dtype=torch.int32, device=dev) for b in range(B)]
    singles = [SparseTensor(torch.ones((len(pts), 1), device=dev), coordinates=(coords + s).contiguous(), tensor_stride=1, device=dev) for s in shifts]
    both = torch.cat([torch.cat([torch.full_like(t.C[:, :1], b), t.C[:, 1:]], 1) for b, t in enumerate(singles)]).contiguous()
    batch = SparseTensor(torch.ones((len(both), 1), device=dev), coordinates=both, tensor_stride=1, device=dev)
    postfixes = [f'_{b}' for b in range(B)]
    suffixes = ('_C.bin', '_F.bin', '_H.bin', '_num_points.bin', lossless.SUFFIX)
    out = {'cloud': args.cloud, 'points_per_frame': len(pts), 'frames': B, 'runs': runs, 'chunk_steps': coders['device'].chunk_steps,
           'weights': 'synthetic (the rate says nothing about trained models)'}
    for name in ('host', 'device'):
        kw = dict(occupancy_coder=name, chunk_steps=steps_list[0])
        together, alone = lossless.LosslessCoder(model, prefix + '_batch_' + name, **kw), lossless.LosslessCoder(model, prefix + '_alone_' + name, **kw)
        enc_alone = lambda: [alone.encode(t, p) for t, p in zip(singles, postfixes)]
        dec_alone = lambda: [alone.decode(p) for p in postfixes]
        records, records_alone = together.encode_batch(batch, postfixes), enc_alone()
        decoded, decoded_alone = together.decode_batch(postfixes), dec_alone()
        r = {'bits_O_per_file': [rec['bits_O'] for rec in records], 'chunks_per_file': [rec.get('chunks') for rec in records],
             'candidate_rows_per_file': [rec['rows'] for rec in records],
             'same_bytes': all(open(together.filename + p + s, 'rb').read() == open(alone.filename + p + s, 'rb').read() for p in postfixes for s in suffixes),
             'same_records': records == records_alone,
             'same_voxels': all(lossless.same_voxels(a.C, t.C) and lossless.same_voxels(b.C, t.C) for a, b, t in zip(decoded, decoded_alone, singles)),
             'median_ms': {'encode_batch': median_ms(lambda: together.encode_batch(batch, postfixes), runs), 'encode_frame_by_frame': median_ms(enc_alone, runs),
                           'decode_batch': median_ms(lambda: together.decode_batch(postfixes), runs), 'decode_frame_by_frame': median_ms(dec_alone, runs)},
             'phases_ms_synchronised': {'encode_batch': phases_ms(lambda: together.encode_batch(batch, postfixes), runs, together),
                                        'encode_frame_by_frame': phases_ms(enc_alone, runs, alone),
                                        'decode_batch': phases_ms(lambda: together.decode_batch(postfixes), runs, together),
                                        'decode_frame_by_frame': phases_ms(dec_alone, runs, alone)}}
        out[name] = r
    return out


if args.batch:
    print(json.dumps(batch_report(args.batch), indent=1))
    raise SystemExit(0)

runs = max(args.repeat, 5)
record = exact.encode(x)
out = exact.decode()
report = {'cloud': args.cloud, 'points': len(pts), 'runs': runs, 'weights': 'synthetic (the rate says nothing about trained models)',
          'exact': lossless.same_voxels(out.C, x.C), 'candidate_rows': record['rows'],
          'bits_O': record['bits_O'], 'ideal_bits_O': round(record['est_bits_O'], 1), 'bpp_O': round(record['bits_O'] / len(pts), 4),
          'bpp_lossy_files': round(float(stream_bits(exact.filename).sum()) / len(pts), 4),
          'occupancy_coder': args.occupancy_coder, 'chunk_steps': coders['device'].chunk_steps, 'chunks': record.get('chunks')}
report['median_ms'] = {'lossless_encode': median_ms(lambda: exact.encode(x), runs), 'lossless_decode': median_ms(exact.decode, runs),
                       'lossy_encode': median_ms(lambda: lossy.encode(x), runs), 'lossy_decode': median_ms(lossy.decode, runs)}
report['phases_ms_synchronised'] = {'encode': phases_ms(lambda: exact.encode(x), runs), 'decode': phases_ms(exact.decode, runs)}
second = coders[other]
second_record = second.encode(x)
report['other_coder'] = {'occupancy_coder': other, 'exact': lossless.same_voxels(second.decode().C, x.C), 'bits_O': second_record['bits_O'],
                         'chunks': second_record.get('chunks'),
                         'median_ms': {'lossless_encode': median_ms(lambda: second.encode(x), runs), 'lossless_decode': median_ms(second.decode, runs)},
                         'phases_ms_synchronised': {'encode': phases_ms(lambda: second.encode(x), runs, second),
                                                    'decode': phases_ms(second.decode, runs, second)}}
if len(steps_list) > 1:                                               # the S table: medians and size of `_O.bin` per chunk_steps
    table = []
    for steps in steps_list:
        c = lossless.LosslessCoder(model, prefix + '_steps', occupancy_coder='device', chunk_steps=steps)
        r = c.encode(x)
        table.append({'chunk_steps': steps, 'chunks': r['chunks'], 'bits_O': r['bits_O'], 'exact': lossless.same_voxels(c.decode().C, x.C),
                      'lossless_encode_ms': median_ms(lambda: c.encode(x), runs), 'lossless_decode_ms': median_ms(c.decode, runs),
                      'k_occ_rans_encode_ms': phases_ms(lambda: c.encode(x), runs, c).get('k_occ_rans_encode'),
                      'k_occ_rans_decode_ms': phases_ms(c.decode, runs, c).get('k_occ_rans_decode')})
    report['chunk_steps_table'] = table

# the same forward point through loss.get_bce: teacher forcing by the truth alone, BCE of every level's logits in bits
with torch.no_grad():
    xi, truths = exact._truth_levels(x)
    y = exact.coder.encode(x)
    min_v, _, sym_h = ops.quantize_symbols(y.F)
    level = exact._latent_level(torch.from_numpy(sym_h).to(dev), min_v, y.C)
    bce_bits, candidates = 0.0, 0
    for l in range(lossless.LEVELS):
        level, logits = exact._logits(level, l)
        truth = isin_mask(level.cmap.C, truths[l])
        bce_bits += float(ops.bce_logits(logits, truth)[0].item())
        candidates += logits.shape[0]
        level = model.decoder.pruning(level, truth, n_keep=len(truths[l]))
report['bce_bits_same_point'] = round(bce_bits, 1)
report['ideal_minus_bce_bits_per_candidate'] = (record['est_bits_O'] - bce_bits) / candidates
report['first_order_bound_bits_per_candidate'] = (1 / 32) / float(np.log(2.0))
if args.trace:
    report['kernel_trace'] = trace_table()
print(json.dumps(report, indent=1))
