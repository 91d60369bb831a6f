#!/usr/bin/env python3
"""Time of ops.estimate_normals on the bench frame (shell10, 786 632 points) at r2 = 16, warm, in this fresh process: the median of --repeat
runs without and with a prebuilt D2Index, for both mappings of the moments pass (one wave per occupied 4 x 4 x 4 cell, the default, and one
thread per voxel), next to the numpy / scipy definition (tests/normals_reference.py) of the same call on this host's CPUs, and whether the
two agree.  With --trace it re-runs itself once under `rocprofv3 --kernel-trace --stats` (a fresh child process) and prints the normals
kernels' table for both mappings.      tools/normals_time.py [--cloud NAME] [--r2 R2] [--repeat K] [--no-host] [--trace]"""
import argparse, csv, glob, json, os, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

ap = argparse.ArgumentParser()
ap.add_argument('--cloud', default='shell10')
ap.add_argument('--r2', type=int, default=16)
ap.add_argument('--repeat', type=int, default=11)
ap.add_argument('--no-host', action='store_true', help='skip the numpy / scipy definition (it takes tens of seconds on the bench frame)')
ap.add_argument('--trace', action='store_true', help='also one rocprofv3 --kernel-trace --stats run of two calls per mapping (child process)')
ap.add_argument('--one-call', action='store_true', help=argparse.SUPPRESS)
args = ap.parse_args()


def trace_table():
    with tempfile.TemporaryDirectory() as d:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '--', sys.executable, os.path.abspath(__file__),
               '--cloud', args.cloud, '--r2', str(args.r2), '--one-call']
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise SystemExit('rocprofv3 failed:\n' + r.stderr[-2000:])
        rows = []
        for path in glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True):
            rows += list(csv.DictReader(open(path)))
    out = [{'kernel': r['Name'][:60], 'calls': int(r['Calls']), 'total_us': round(float(r['TotalDurationNs']) / 1e3, 1),
            'mean_us': round(float(r['AverageNs']) / 1e3, 1)} for r in rows if 'k_nrm_' in r.get('Name', '')]
    return sorted(out, key=lambda r: -r['total_us'])


import numpy as np
import torch
import pcgcv2_amd
pcgcv2_amd.configure_host_threads()
from pcgcv2_amd import ops, synthetic

dev = torch.device('cuda:0')
pts = synthetic.cloud(args.cloud, device=dev)
coords = torch.cat([torch.zeros((len(pts), 1), dtype=torch.int32, device=dev), pts], 1).contiguous()
MAPPINGS = (('wave_per_cell', 0), ('thread_per_voxel', 1))

if args.one_call:
    for _, mode in MAPPINGS:
        ops.lib().pcgc_set_normals_mapping(mode)
        ops.estimate_normals(coords, args.r2); ops.estimate_normals(coords, args.r2)
    torch.cuda.synchronize()
    raise SystemExit(0)


def median_ms(fn):
    fn(); torch.cuda.synchronize()                                    # (warm: code objects, ball table, allocator)
    times = []
    for _ in range(max(args.repeat, 10)):
        torch.cuda.synchronize(); t = time.perf_counter(); fn(); torch.cuda.synchronize(); times.append(time.perf_counter() - t)
    return round(float(np.median(times)) * 1e3, 3)


index = ops.D2Index(coords)
report = {'cloud': args.cloud, 'points': len(pts), 'r2': args.r2, 'runs': max(args.repeat, 10), 'median_ms': {}}
results = {}
for name, mode in MAPPINGS:
    ops.lib().pcgc_set_normals_mapping(mode)
    report['median_ms'][name] = {'with_index_build': median_ms(lambda: ops.estimate_normals(coords, args.r2)),
                                 'prebuilt_index': median_ms(lambda: ops.estimate_normals(coords, args.r2, index=index))}
    results[name] = [t.cpu().numpy() for t in ops.estimate_normals(coords, args.r2, index=index, want_moments=True)]
ops.lib().pcgc_set_normals_mapping(0)
report['median_ms']['d2_index_alone'] = median_ms(lambda: ops.D2Index(coords))
report['mappings_bitwise_equal'] = all(a.tobytes() == b.tobytes() for a, b in zip(*results.values()))
if not args.no_host:
    import normals_reference as nr
    rows = coords.cpu().numpy()
    t = time.perf_counter(); ref = nr.estimate_normals(rows, args.r2); t_ref = time.perf_counter() - t
    nrm, lam, count, valid, mom = results['wave_per_cell']
    sel = ref['valid'] & (ref['gap'] >= 1e-6)
    report['numpy_definition_ms'] = round(t_ref * 1e3, 1)
    report['host_cpus'] = pcgcv2_amd.effective_cpus()
    report['moments_equal_to_definition'] = bool(np.array_equal(mom, ref['moments']) and np.array_equal(valid, ref['valid']))
    report['max_sin_to_definition'] = float(np.linalg.norm(np.cross(nrm[sel], ref['normals'][sel]), axis=1).max())
    report['invalid_rows'] = int((~valid).sum())
if args.trace:
    report['kernel_trace'] = trace_table()
print(json.dumps(report, indent=1))
