#!/usr/bin/env python3
"""Time of ops.voxelize on a synthetic raw cloud, warm, in this fresh process: shell10's voxels (786 632) jittered to three float32 points
each, in metres, with colours, voxelised to 10 bits.  Reports the median of --repeat whole calls, the ms per phase (bounds, quantise, sort,
merge, copies; each phase synchronised, so their sum exceeds the whole call), the numpy definition (tests/voxelize_reference.py) of the
same call on this host's CPUs, and whether the two agree.  With --trace it re-runs itself once under `rocprofv3 --kernel-trace --stats`
(a fresh child process) and prints the kernels' table.      tools/voxelize_time.py [--cloud NAME] [--bits B] [--per-voxel K] [--repeat R]
[--no-host] [--trace]"""
import argparse, csv, glob, json, os, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

ap = argparse.ArgumentParser()
ap.add_argument('--cloud', default='shell10')
ap.add_argument('--bits', type=int, default=10)
ap.add_argument('--per-voxel', type=int, default=3, help='raw points per voxel of the cloud')
ap.add_argument('--merge', default='mean', choices=('mean', 'first'))
ap.add_argument('--repeat', type=int, default=11)
ap.add_argument('--no-host', action='store_true', help='skip the numpy definition')
ap.add_argument('--trace', action='store_true', help='also one rocprofv3 --kernel-trace --stats run of two calls (child process)')
ap.add_argument('--one-call', action='store_true', help=argparse.SUPPRESS)
args = ap.parse_args()


def trace_table():
    with tempfile.TemporaryDirectory() as d:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '--', sys.executable, os.path.abspath(__file__),
               '--cloud', args.cloud, '--bits', str(args.bits), '--per-voxel', str(args.per_voxel), '--merge', args.merge, '--one-call']
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise SystemExit('rocprofv3 failed:\n' + r.stderr[-2000:])
        rows = []
        for path in glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True):
            rows += list(csv.DictReader(open(path)))
    out = [{'kernel': r['Name'][:60], 'calls': int(r['Calls']), 'total_us': round(float(r['TotalDurationNs']) / 1e3, 1),
            'mean_us': round(float(r['AverageNs']) / 1e3, 1)} for r in rows]
    return sorted(out, key=lambda r: -r['total_us'])[:16]


import numpy as np
import torch
import pcgcv2_amd
pcgcv2_amd.configure_host_threads()
from pcgcv2_amd import ops, synthetic

dev = torch.device('cuda:0')
cells = synthetic.cloud(args.cloud).numpy().astype(np.float64)
rng = np.random.default_rng(0)
raw = np.concatenate([cells + rng.uniform(-0.45, 0.45, cells.shape) for _ in range(args.per_voxel)])
order = rng.permutation(len(raw))
raw = (raw[order] * 0.002 + np.array([3.0, -1.5, 0.25])).astype(np.float32)            # 2 mm voxels, a scanner's frame
rgb = rng.integers(0, 256, (len(raw), 3)).astype(np.uint8)
points, colours = torch.from_numpy(raw).to(dev), torch.from_numpy(rgb).to(dev)


def call(times=None):
    return ops.voxelize(points, colours, args.bits, merge=args.merge, times=times)


if args.one_call:
    call(); call()
    torch.cuda.synchronize()
    raise SystemExit(0)

call(); torch.cuda.synchronize()                                       # (warm: code objects, allocator)
runs = max(args.repeat, 10)
whole, phases = [], []
for _ in range(runs):
    torch.cuda.synchronize(); t = time.perf_counter(); got = call(); torch.cuda.synchronize(); whole.append(time.perf_counter() - t)
for _ in range(runs):
    times = {}
    call(times)
    phases.append(times)
report = {'cloud': args.cloud, 'raw_points': len(raw), 'bits': args.bits, 'merge': args.merge, 'voxels': int(len(got.counts)),
          'largest_count': int(got.counts.max().item()), 'runs': runs, 'median_ms': {'whole_call': round(float(np.median(whole)) * 1e3, 3)}}
for phase in ('bounds', 'quantise', 'sort', 'merge', 'copies'):
    report['median_ms'][phase] = round(float(np.median([p[phase] for p in phases])) * 1e3, 3)
if not args.no_host:
    import voxelize_reference as V
    t = time.perf_counter(); ref = V.voxelize(raw, rgb, args.bits, merge=args.merge); t_ref = time.perf_counter() - t
    report['numpy_definition_ms'] = round(t_ref * 1e3, 1)
    report['host_cpus'] = pcgcv2_amd.effective_cpus()
    report['equal_to_definition'] = bool(
        np.array_equal(got.coords.cpu().numpy(), ref.coords) and np.array_equal(got.counts.cpu().numpy(), ref.counts) and
        np.array_equal(got.voxel_of.cpu().numpy(), ref.voxel_of) and np.array_equal(got.colours.cpu().numpy(), ref.colours) and
        list(got.origin) == ref.origin.tolist() and got.scale == ref.scale)
if args.trace:
    report['kernel_trace'] = trace_table()
print(json.dumps(report, indent=1))
