#!/usr/bin/env python3
"""Time of the colour codec (pcgcv2_amd/attributes.py, csrc/raht.hip) on the bench frame (shell10, 786 632 points, the colour field of
tools/recolour_time.py), warm, in this fresh process: the median of --repeat runs of AttributeCoder.encode and decode per phase (keys + sort,
tree, forward, quantise, copies, host coder; host coder, copies, dequantise, inverse), for both forms of the transform (one launch per split
bit | tiles), the forward and inverse transforms alone in both forms, and for scale: the numpy definition on the same cloud, carrying the
colours onto the decoded cloud (shared and own searches) and the lossy geometry decode.  With --trace it re-runs itself once under
`rocprofv3 --kernel-trace --stats` (a fresh child process) and prints the table of the k_raht_ kernels.
    tools/attributes_time.py [--cloud NAME] [--qstep Q] [--repeat K] [--no-host] [--trace]
With --attribute_coder device it times the device coder of `_A.bin` version 2 instead: version 1 first, then per value of
--chunk_steps the chunks, the bits of `_A.bin` and their excess over version 1, encode and decode as whole calls and the synchronised time
of the coder phase, all in this one process, the decoded colours compared with version 1's.
    tools/attributes_time.py --attribute_coder device [--chunk_steps 1024,4096,16384,0] [--cloud NAME] [--qstep Q] [--repeat K]
With --batch B it times ONE encode_batch + decode_batch of B copies of the cloud (the noise of the colour field drawn with another seed per
copy, so the streams differ) against B frame-by-frame encode + decode calls, in this one process: the median per phase of
both, the bits of every file, and whether the batch wrote the same bytes and decoded the same colours.
    tools/attributes_time.py --batch B [--attribute_coder device] [--cloud NAME] [--qstep Q] [--repeat K]"""
import argparse, csv, glob, json, os, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument('--cloud', default='shell10')
ap.add_argument('--qstep', type=int, default=8)
ap.add_argument('--repeat', type=int, default=11)
ap.add_argument('--no-host', action='store_true', help='skip the numpy definition (seconds on the bench frame)')
ap.add_argument('--trace', action='store_true', help='also one rocprofv3 --kernel-trace --stats run of two calls per form (child process)')
ap.add_argument('--attribute_coder', choices=('host', 'device'), default='host', help='device: time the device coder over --chunk_steps instead')
ap.add_argument('--chunk_steps', default='1024,4096,16384,0', help='with --attribute_coder device: steps per chunk, comma separated (0: one chunk)')
ap.add_argument('--batch', type=int, default=0, help='time encode_batch / decode_batch of this many copies against frame-by-frame calls')
ap.add_argument('--one-call', action='store_true', help=argparse.SUPPRESS)
args = ap.parse_args()


def trace_table():
    with tempfile.TemporaryDirectory() as d:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '--', sys.executable, os.path.abspath(__file__),
               '--cloud', args.cloud, '--qstep', str(args.qstep), '--one-call']
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise SystemExit('rocprofv3 failed:\n' + r.stderr[-2000:])
        rows = []
        for path in glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True):
            rows += list(csv.DictReader(open(path)))
    out = [{'kernel': r['Name'][:60], 'calls': int(r['Calls']), 'total_us': round(float(r['TotalDurationNs']) / 1e3, 1),
            'mean_us': round(float(r['AverageNs']) / 1e3, 1)} for r in rows if any(k in r.get('Name', '') for k in ('k_raht_', 'k_scan_', 'rocprim'))]
    return sorted(out, key=lambda r: -r['total_us'])


import numpy as np
import torch
import pcgcv2_amd
pcgcv2_amd.configure_host_threads()
from pcgcv2_amd import ops, synthetic
from pcgcv2_amd import pc_error as pe
from pcgcv2_amd.attributes import AttributeCoder

dev = torch.device('cuda:0')
pts = synthetic.cloud(args.cloud, device=dev)
a = torch.cat([torch.zeros((len(pts), 1), dtype=torch.int32, device=dev), pts], 1).contiguous()
t = pts.double() / float(pts.max() + 1)                              # a smooth colour field plus noise, like a textured surface
rgb = torch.stack([255 * t[:, 0], 127.5 * (1 + torch.sin(40 * t[:, 1])), 255 * t[:, 2] * t[:, 0]], 1)
ca = (rgb + torch.randint(-12, 13, rgb.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(1))).round().clamp(0, 255).to(torch.uint8)
tmp = tempfile.TemporaryDirectory()
prefix = os.path.join(tmp.name, 'f')

if args.one_call:
    for form in ops.RAHT_FORMS:
        coder = AttributeCoder(prefix, form=form)
        for _ in range(2):
            coder.encode(a, ca, args.qstep)
            coder.decode(a)
    torch.cuda.synchronize()
    raise SystemExit(0)

runs = max(args.repeat, 10)


def median_ms(fn):
    fn(); torch.cuda.synchronize()                                    # (warm: code objects, allocator)
    times = []
    for _ in range(runs):
        torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); times.append(time.perf_counter() - t0)
    return round(float(np.median(times)) * 1e3, 3)


def phases(fn, coder):
    """median per phase of the coder's own synchronised stopwatch, and of the whole call without it"""
    fn()
    rows = []
    for _ in range(runs):
        coder.times = {}
        fn()
        rows.append(coder.times)
    coder.times = None
    out = {k: round(float(np.median([r.get(k, 0.0) for r in rows])) * 1e3, 3) for k in rows[0]}
    out['sum of phases'] = round(sum(out.values()), 3)
    out['whole call, no stopwatch'] = median_ms(fn)
    return out


if args.batch:
    from pcgcv2_amd.attributes import CHUNK_STEPS
    B = args.batch
    noise = lambda seed: torch.randint(-12, 13, rgb.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(seed))
    colours = [(rgb + noise(1 + b)).round().clamp(0, 255).to(torch.uint8) for b in range(B)]
    frames = [torch.cat([torch.full((len(pts), 1), b, dtype=torch.int32, device=dev), pts], 1) for b in range(B)]
    shuffle = torch.randperm(B * len(pts), device=dev, generator=torch.Generator(device=dev).manual_seed(7))       # frames interleaved
    a_all, c_all = torch.cat(frames)[shuffle].contiguous(), torch.cat(colours)[shuffle].contiguous()
    postfixes = [f'_{b}' for b in range(B)]
    single = AttributeCoder(prefix + 's', attribute_coder=args.attribute_coder)
    batch = AttributeCoder(prefix + 'b', attribute_coder=args.attribute_coder)

    def single_encode():
        for b in range(B):
            single.encode(a, colours[b], args.qstep, postfix=postfixes[b])

    def single_decode():
        return [single.decode(a, postfix=postfixes[b]) for b in range(B)]

    report = {'cloud': args.cloud, 'frames': B, 'points_per_frame': len(a), 'qstep': args.qstep, 'runs': runs, 'form': ops.RAHT_FORM,
              'attribute_coder': args.attribute_coder, 'chunk_steps': CHUNK_STEPS,
              'frame_by_frame_ms': {'encode': phases(single_encode, single), 'decode': phases(single_decode, single)},
              'batch_ms': {'encode': phases(lambda: batch.encode_batch(a_all, c_all, args.qstep, postfixes=postfixes), batch),
                           'decode': phases(lambda: batch.decode_batch(a_all, postfixes=postfixes), batch)}}
    report['bits_A'] = {'frame_by_frame': [8 * os.path.getsize(prefix + 's' + p + '_A.bin') for p in postfixes],
                        'batch': [8 * os.path.getsize(prefix + 'b' + p + '_A.bin') for p in postfixes]}
    report['same_bytes'] = all(open(prefix + 's' + p + '_A.bin', 'rb').read() == open(prefix + 'b' + p + '_A.bin', 'rb').read() for p in postfixes)
    got, want = batch.decode_batch(a_all, postfixes=postfixes), single_decode()
    back = torch.empty_like(got)
    back[shuffle] = got                                               # row b len(pts) + i: frame b's row i
    report['same_colours'] = all(bool(torch.equal(back[b * len(pts):(b + 1) * len(pts)], want[b])) for b in range(B))
    whole = lambda side, kind: report[kind][side]['whole call, no stopwatch']
    report['speedup'] = {side: round(whole(side, 'frame_by_frame_ms') / whole(side, 'batch_ms'), 3) for side in ('encode', 'decode')}
    print(json.dumps(report, indent=1))
    raise SystemExit(0)

if args.attribute_coder == 'device':
    from pcgcv2_amd.attributes import CHUNK_STEPS
    report = {'cloud': args.cloud, 'points': len(a), 'tokens': 3 * (len(a) - 1), 'qstep': args.qstep, 'runs': runs, 'form': ops.RAHT_FORM,
              'default_chunk_steps': CHUNK_STEPS, 'device_coder': []}
    host = AttributeCoder(prefix + 'v1')
    report['version_1'] = {'encode_ms': phases(lambda: host.encode(a, ca, args.qstep), host), 'decode_ms': phases(lambda: host.decode(a), host),
                           'bits_A': 8 * os.path.getsize(prefix + 'v1_A.bin')}
    want = host.decode(a)
    for S in [int(v) for v in args.chunk_steps.split(',')]:
        coder = AttributeCoder(prefix + f'v2_{S}', attribute_coder='device', chunk_steps=S)
        enc, dec = phases(lambda: coder.encode(a, ca, args.qstep), coder), phases(lambda: coder.decode(a), coder)
        bits = 8 * os.path.getsize(prefix + f'v2_{S}_A.bin')
        steps = S or -(-report['tokens'] // 64)
        report['device_coder'].append({
            'chunk_steps': S, 'chunks': ops.attr_rans_chunks(report['tokens'], steps), 'bits_A': bits,
            'excess_over_version_1_percent': round(100.0 * (bits - report['version_1']['bits_A']) / report['version_1']['bits_A'], 3),
            'encode_ms': enc, 'decode_ms': dec, 'coder_phase_ms': {'encode': enc['device coder'], 'decode': dec['device coder']},
            'same_colours_as_version_1': bool(torch.equal(coder.decode(a), want)),
            'faster_than_version_1': {'encode': enc['whole call, no stopwatch'] < report['version_1']['encode_ms']['whole call, no stopwatch'],
                                      'decode': dec['whole call, no stopwatch'] < report['version_1']['decode_ms']['whole call, no stopwatch']}})
    print(json.dumps(report, indent=1))
    raise SystemExit(0)

report = {'cloud': args.cloud, 'points': len(a), 'qstep': args.qstep, 'runs': runs, 'tile_leaves': ops.raht_tile_leaves(),
          'default_form': ops.RAHT_FORM, 'encode_ms': {}, 'decode_ms': {}, 'forward_ms': {}, 'inverse_ms': {}}
tree = ops.raht_tree(a)
report['crossing_gaps'] = int(tree.cross[-1])
report['populated_split_bits'] = int(np.count_nonzero(np.diff(tree.bucket)))
blobs = {}
for form in ops.RAHT_FORMS:
    coder = AttributeCoder(prefix + form, form=form)
    report['encode_ms'][form] = phases(lambda: coder.encode(a, ca, args.qstep), coder)
    report['decode_ms'][form] = phases(lambda: coder.decode(a), coder)
    blobs[form] = open(prefix + form + '_A.bin', 'rb').read()
    H, dc = ops.raht_forward(tree, ca, form=form)
    dc = dc.cpu().tolist()
    report['forward_ms'][form] = median_ms(lambda: ops.raht_forward(tree, ca, form=form))
    report['inverse_ms'][form] = median_ms(lambda: ops.raht_inverse(tree, H, dc, form=form))
report['both_forms_same_bytes'] = len(set(blobs.values())) == 1
record = AttributeCoder(prefix).encode(a, ca, args.qstep)
cb = AttributeCoder(prefix).decode(a)
report['bits_per_point'] = round(record['bits_A'] / len(a), 4)
report['payload_bytes'], report['escapes'] = record['payload_bytes'], record['escapes']
metric = pe.colour_psnr_device(a, ca, a, cb)
report['colour_psnr_y_u_v'] = [metric[f'c[{k}],PSNRF'] for k in range(3)]
for form in ops.RAHT_FORMS:
    for side in ('encode_ms', 'decode_ms'):
        p = report[side][form]
        p['share of host coder and copies'] = round((p.get('host coder', 0.0) + p.get('copies', 0.0)) / p['sum of phases'], 3)

if not args.no_host:
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import raht_reference as R
    pts_h, rgb_h = pts.cpu().numpy().astype(np.int64), ca.cpu().numpy()
    t0 = time.perf_counter(); blob, rec = R.encode(pts_h, rgb_h, args.qstep, args.qstep, ops.rc_encode_ctx, ops.crc32); t_def = time.perf_counter() - t0
    report['numpy_definition_encode_ms'] = round(t_def * 1e3, 1)
    report['equal_to_definition'] = bool(blob == blobs[ops.RAHT_FORM] and np.array_equal(rec, cb.cpu().numpy()))
    report['host_cpus'] = pcgcv2_amd.effective_cpus()

# for scale, from the same process: the colours carried onto what the synthetic-weight codec decodes, and that decode
from pcgcv2_amd.coder import Coder
from pcgcv2_amd.pcc_model import PCCModel
from pcgcv2_amd.sparse import SparseTensor
model = PCCModel().to(dev)
model.load_state_dict(synthetic.synthetic_state_dict())
geometry = Coder(model, prefix + 'g')
geometry.encode(SparseTensor(torch.ones((len(pts), 1), device=dev), coordinates=a, tensor_stride=1, device=dev))
b = geometry.decode().C.detach().contiguous()
nn = pe.nn_both(a, b)
report['for_scale_ms'] = {'recolour_shared_searches': median_ms(lambda: pe.recolour_device(a, ca, b, nn=nn)),
                          'recolour_own_searches': median_ms(lambda: pe.recolour_device(a, ca, b)),
                          'lossy_geometry_decode': median_ms(lambda: geometry.decode())}
if args.trace:
    report['kernel_trace'] = trace_table()
print(json.dumps(report, indent=1))
