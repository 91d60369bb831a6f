#!/usr/bin/env python3
"""Time of ops.partition on shell10 and on the scaled vox12 cloud of bench.py's `blocks` config, warm, in this fresh process.
Per cloud and per max_num (chosen to give about 8 and about 64 blocks): the median of --repeat whole calls, the ms per phase (bounds, coarse,
cut, fine, assign, order, copies; each phase synchronised, so their sum exceeds the whole call), rounds and blocks, the numpy definition
(tests/partition_reference.py) and shard.split_octants on this host's CPUs in the same process (both on rows already on the host), and
whether device and definition agree.
--codec: BlockCoder.encode + decode next to the whole-cloud Coder pair on the first cloud (ms, bits, D1 PSNR; synthetic weights, so the bits
mean nothing).  With --trace it re-runs itself once under `rocprofv3 --kernel-trace --stats` (a fresh child process) and prints the kernels'
table.
    tools/partition_time.py [--clouds shell10,blocks] [--repeat R] [--no-host] [--codec] [--trace]"""
import argparse, csv, glob, json, os, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

ap = argparse.ArgumentParser()
ap.add_argument('--clouds', default='shell10,blocks', help="names of synthetic clouds; 'blocks' = shell12 scaled by 0.375, the cloud of bench.py --config blocks")
ap.add_argument('--repeat', type=int, default=11)
ap.add_argument('--no-host', action='store_true', help='skip the numpy definition and shard.split_octants')
ap.add_argument('--codec', action='store_true', help='also BlockCoder.encode + decode next to Coder.encode + decode of the first cloud')
ap.add_argument('--steps', type=int, default=5, help='with --codec: timed encode + decode passes')
ap.add_argument('--trace', action='store_true', help='also one rocprofv3 --kernel-trace --stats run of two calls on the first cloud (child process)')
ap.add_argument('--one-call', action='store_true', help=argparse.SUPPRESS)
args = ap.parse_args()


def trace_table():
    with tempfile.TemporaryDirectory() as d:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '--', sys.executable, os.path.abspath(__file__),
               '--clouds', args.clouds.split(',')[0], '--one-call']
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
from pcgcv2_amd import ops, shard, synthetic

dev = torch.device('cuda:0')


def rows_of(name):
    """-> int32 [N,4] device rows (batch 0) of a named cloud"""
    from pcgcv2_amd.data_utils import scale_sparse_tensor
    from pcgcv2_amd.sparse import SparseTensor
    p = synthetic.cloud('shell12' if name == 'blocks' else name)
    c = torch.cat([torch.zeros((len(p), 1), dtype=torch.int32), p.int()], 1)
    x = SparseTensor(torch.ones((len(c), 1)), coordinates=c, tensor_stride=1, device=dev)
    if name == 'blocks':
        x = scale_sparse_tensor(x, 0.375)
    return x.C.contiguous()


def one_cloud(name):
    coords = rows_of(name)
    n = len(coords)
    if args.one_call:
        ops.partition(coords, max(1, n // 8)); ops.partition(coords, max(1, n // 8))
        torch.cuda.synchronize()
        raise SystemExit(0)
    host = coords.cpu().numpy()
    reps = []
    for target in (8, 64):
        max_num = max(1, -(-n // target))                               # halving down to at most n / target rows a block: about `target` blocks
        call = lambda times=None: ops.partition(coords, max_num, times=times)
        call(); torch.cuda.synchronize()                               # (warm: code objects, allocator)
        runs = max(args.repeat, 10)
        whole, phases = [], []
        for _ in range(runs):
            torch.cuda.synchronize(); t = time.perf_counter(); got = call(); torch.cuda.synchronize(); whole.append(time.perf_counter() - t)
        for _ in range(runs):
            times = {}
            call(times)
            phases.append(times)
        rep = {'cloud': name, 'rows': n, 'max_num': max_num, 'blocks': int(len(got.table)), 'rounds': got.rounds, 'oversize': got.oversize,
               'largest': int(got.table[:, 1].max()), 'smallest': int(got.table[:, 1].min()), 'runs': runs,
               'median_ms': {'whole_call': round(float(np.median(whole)) * 1e3, 3)}}
        for phase in ops.PARTITION_PHASES:
            rep['median_ms'][phase] = round(float(np.median([p.get(phase, 0.0) for p in phases])) * 1e3, 3)
        if not args.no_host:
            import partition_reference as R
            t = time.perf_counter(); ref = R.partition(host, max_num); t_ref = time.perf_counter() - t
            rep['numpy_definition_ms'] = round(t_ref * 1e3, 1)
            rep['equal_to_definition'] = bool(np.array_equal(got.block_of.cpu().numpy(), ref.block_of) and np.array_equal(got.perm.cpu().numpy(), ref.perm)
                                              and np.array_equal(got.table.cpu().numpy(), ref.table) and (got.rounds, got.oversize) == (ref.rounds, ref.oversize))
            levels = 1 if target == 8 else 2
            t = time.perf_counter(); parts = shard.split_octants(host, levels=levels); t_oct = time.perf_counter() - t
            rep['split_octants'] = {'levels': levels, 'blocks': len(parts), 'largest': max(len(p) for p in parts), 'ms': round(t_oct * 1e3, 1)}
        reps.append(rep)
    return reps, coords


def codec(coords):
    """BlockCoder.encode + decode at about 8 blocks next to Coder.encode + decode of the whole cloud, one process: ms over --steps passes after
    one warm pass, the bits written and the D1 PSNR of each decoded cloud against the input"""
    from pcgcv2_amd.coder import Coder, stream_bits
    from pcgcv2_amd.partition import BlockCoder, block_bits
    from pcgcv2_amd.pc_error import d1_psnr_device
    from pcgcv2_amd.pcc_model import PCCModel
    from pcgcv2_amd.sparse import SparseTensor
    model = PCCModel().to(dev)
    model.load_state_dict(synthetic.synthetic_state_dict())
    n = len(coords)
    res = 1 << int(np.ceil(np.log2(int(coords[:, 1:].max()) + 1)))
    out = {}
    with tempfile.TemporaryDirectory(dir='/dev/shm' if os.path.isdir('/dev/shm') else None) as tmp:
        whole, blocked = Coder(model, os.path.join(tmp, 'w')), BlockCoder(model, os.path.join(tmp, 'b'), max(1, -(-n // 8)), batch_items=8)
        x = SparseTensor(torch.ones((n, 1), device=dev), coordinates=coords, tensor_stride=1, device=dev, assume_unique=True)
        for tag, pair in (('whole', whole), ('blocked', blocked)):
            dts = []
            for step in range(args.steps + 1):
                x.cmap.drop_caches()
                torch.cuda.synchronize(); t = time.perf_counter()
                pair.encode(x)
                y = pair.decode()
                torch.cuda.synchronize(); dts.append(time.perf_counter() - t)
            bits = int(stream_bits(os.path.join(tmp, 'w')).sum()) if tag == 'whole' else block_bits(os.path.join(tmp, 'b'))
            m = d1_psnr_device(x.C, y.C, res)
            out[tag] = {'points': n, 'decoded_points': len(y), 'ms_per_step': round(float(np.median(dts[1:])) * 1e3, 2),
                        'Mpoints_s': round(n / float(np.median(dts[1:])) / 1e6, 2), 'bits': bits, 'bpp': round(bits / n, 4),
                        'd1_psnr': round(m['mseF,PSNR (p2point)'], 3), 'd1_mse': round(m['mseF      (p2point)'], 5)}
    out['note'] = 'synthetic weights: the bits are meaningless, only the counts of symbols and coordinates move'
    return out


report = {'host_cpus': pcgcv2_amd.effective_cpus(), 'clouds': []}
first = None
for name in args.clouds.split(','):
    reps, coords = one_cloud(name)
    report['clouds'] += reps
    first = coords if first is None else first
if args.codec:
    report['codec_' + args.clouds.split(',')[0]] = codec(first)
if args.trace:
    report['kernel_trace'] = trace_table()
print(json.dumps(report, indent=1))
