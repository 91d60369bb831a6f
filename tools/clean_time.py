#!/usr/bin/env python3
"""Time of ops.clean on synthetic clouds, warm, in this fresh process.  Per cloud: the median of --repeat whole calls, the ms
per phase (index, counts, map, components = the labelling rounds and the size histogram, select, compaction, copies; each phase
synchronised, so their sum exceeds the whole call), the number of labelling rounds, the numpy definition (tests/clean_reference.py) of the
same call on this host's CPUs, and whether the two agree.  --codec: Coder.encode + decode of the first cloud before and after the cleaning,
in one process (Mpoints/s and the bytes written; synthetic weights, so the bits mean nothing).  With --trace it re-runs itself once under
`rocprofv3 --kernel-trace --stats` (a fresh child process) and prints the kernels' table.
    tools/clean_time.py [--clouds noisy10,multi10,shell10] [--clean 4,8] [--r2 16] [--keep_largest 0] [--repeat R] [--no-host] [--codec] [--trace]"""
import argparse, csv, glob, json, os, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

ap = argparse.ArgumentParser()
ap.add_argument('--clouds', default='noisy10,multi10,shell10')
ap.add_argument('--clean', default='4,8', help='K,M: min_neighbours, min_component')
ap.add_argument('--r2', type=int, default=16)
ap.add_argument('--keep_largest', type=int, default=0)
ap.add_argument('--repeat', type=int, default=11)
ap.add_argument('--no-host', action='store_true', help='skip the numpy definition')
ap.add_argument('--codec', action='store_true', help='also Coder.encode + decode of the first cloud before and after the cleaning')
ap.add_argument('--steps', type=int, default=5, help='with --codec: timed encode + decode passes')
ap.add_argument('--trace', action='store_true', help='also one rocprofv3 --kernel-trace --stats run of two calls on the first cloud (child process)')
ap.add_argument('--one-call', action='store_true', help=argparse.SUPPRESS)
args = ap.parse_args()
K, M = (int(v) for v in args.clean.split(','))


def trace_table():
    with tempfile.TemporaryDirectory() as d:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '--', sys.executable, os.path.abspath(__file__),
               '--clouds', args.clouds.split(',')[0], '--clean', args.clean, '--r2', str(args.r2), '--keep_largest', str(args.keep_largest), '--one-call']
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
PHASES = ('index', 'counts', 'map', 'components', 'select', 'compaction', 'copies')


def rows_of(name):
    p = synthetic.cloud(name).numpy()
    return np.concatenate([np.zeros((len(p), 1), np.int32), p], 1)


def one_cloud(name):
    c = rows_of(name)
    coords = torch.from_numpy(c).to(dev)
    call = lambda times=None: ops.clean(coords, None, r2=args.r2, min_neighbours=K, min_component=M, keep_largest=args.keep_largest, times=times)
    if args.one_call:
        call(); call()
        torch.cuda.synchronize()
        raise SystemExit(0)
    call(); torch.cuda.synchronize()                                   # (warm: code objects, allocator, ball table)
    runs = max(args.repeat, 10)
    whole, phases = [], []
    for _ in range(runs):
        torch.cuda.synchronize(); t = time.perf_counter(); got = call(); torch.cuda.synchronize(); whole.append(time.perf_counter() - t)
    for _ in range(runs):
        times = {}
        call(times)
        phases.append(times)
    rep = {'cloud': name, 'rows': len(c), 'r2': args.r2, 'min_neighbours': K, 'min_component': M, 'keep_largest': args.keep_largest,
           'removed_density': got.removed_density, 'removed_component': got.removed_component, 'components': got.n_components,
           'rows_out': int(len(got.coords)), 'rounds': got.rounds, 'runs': runs, 'median_ms': {'whole_call': round(float(np.median(whole)) * 1e3, 3)}}
    for phase in PHASES:
        rep['median_ms'][phase] = round(float(np.median([p.get(phase, 0.0) for p in phases])) * 1e3, 3)
    if not args.no_host:
        import clean_reference as R
        t = time.perf_counter(); ref = R.clean(c, None, args.r2, K, M, args.keep_largest); t_ref = time.perf_counter() - t
        rep['numpy_definition_ms'] = round(t_ref * 1e3, 1)
        rep['equal_to_definition'] = bool(all(np.array_equal(getattr(got, f).cpu().numpy(), getattr(ref, f)) for f in ('keep', 'neighbours', 'labels', 'sizes', 'coords'))
                                          and (got.removed_density, got.removed_component, got.n_components) == (ref.removed_density, ref.removed_component, ref.n_components))
    return rep, coords, got.coords


def codec(before, after):
    """Coder.encode + decode of both clouds, one process: Mpoints/s over --steps passes after one warm pass, and the bytes of the files"""
    from pcgcv2_amd.coder import Coder
    from pcgcv2_amd.pcc_model import PCCModel
    from pcgcv2_amd.sparse import SparseTensor
    model = PCCModel().to(dev)
    model.load_state_dict(synthetic.synthetic_state_dict())
    out = {}
    with tempfile.TemporaryDirectory(dir='/dev/shm' if os.path.isdir('/dev/shm') else None) as tmp:
        coder = Coder(model, os.path.join(tmp, 'u'))
        for tag, c in (('before', before), ('after', after)):
            x = SparseTensor(torch.ones((len(c), 1), device=dev), coordinates=c.contiguous(), tensor_stride=1, device=dev, assume_unique=True)
            dts = []
            for step in range(args.steps + 1):
                x.cmap.drop_caches()
                torch.cuda.synchronize(); t = time.perf_counter()
                coder.encode(x, postfix='_' + tag)
                y = coder.decode(postfix='_' + tag)
                torch.cuda.synchronize(); dts.append(time.perf_counter() - t)
            files = {f: os.path.getsize(os.path.join(tmp, f)) for f in sorted(os.listdir(tmp)) if f.startswith('u_' + tag)}
            out[tag] = {'points': len(c), 'decoded_points': len(y), 'Mpoints_s': round(len(c) / float(np.median(dts[1:])) / 1e6, 2),
                        'ms_per_step': round(float(np.median(dts[1:])) * 1e3, 2), 'file_bytes': files, 'bytes': sum(files.values())}
    out['note'] = 'synthetic weights: the bits are meaningless, only the counts of symbols and coordinates move'
    return out


report = {'host_cpus': pcgcv2_amd.effective_cpus(), 'clouds': []}
first = None
for name in args.clouds.split(','):
    rep, coords, kept = one_cloud(name)
    report['clouds'].append(rep)
    first = first or (coords, kept)
if args.codec:
    report['codec_' + args.clouds.split(',')[0]] = codec(*first)
if args.trace:
    report['kernel_trace'] = trace_table()
print(json.dumps(report, indent=1))
