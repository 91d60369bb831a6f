#!/usr/bin/env python3
"""Time of carrying colours onto a decoded cloud and of the colour metric on the bench frame (shell10, 786 632 points, against what the
synthetic-weight codec decodes from it), warm, in this fresh process: the median of --repeat runs of pc_error.recolour_device and
pc_error.colour_psnr_device with the two nearest-neighbour searches shared (nn=) and not shared, the two searches alone, next to the host
numpy / scipy route (pc_error.recolour, pc_error.colour_psnr) on this host's CPUs, whether they agree, and the coloured-PLY writer against a
pandas writer.  With --trace it re-runs itself once under `rocprofv3 --kernel-trace --stats` (a fresh child process) and prints the table of
the colour and search kernels.      tools/recolour_time.py [--cloud NAME] [--repeat K] [--no-host] [--trace]"""
import argparse, csv, glob, json, os, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument('--cloud', default='shell10')
ap.add_argument('--repeat', type=int, default=11)
ap.add_argument('--no-host', action='store_true', help='skip the host numpy / scipy route (seconds on the bench frame)')
ap.add_argument('--trace', action='store_true', help='also one rocprofv3 --kernel-trace --stats run of two calls (child process)')
ap.add_argument('--one-call', action='store_true', help=argparse.SUPPRESS)
args = ap.parse_args()


def trace_table():
    with tempfile.TemporaryDirectory() as d:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '--', sys.executable, os.path.abspath(__file__),
               '--cloud', args.cloud, '--one-call']
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise SystemExit('rocprofv3 failed:\n' + r.stderr[-2000:])
        rows = []
        for path in glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True):
            rows += list(csv.DictReader(open(path)))
    out = [{'kernel': r['Name'][:60], 'calls': int(r['Calls']), 'total_us': round(float(r['TotalDurationNs']) / 1e3, 1),
            'mean_us': round(float(r['AverageNs']) / 1e3, 1)} for r in rows if any(k in r.get('Name', '') for k in ('k_attr_', 'k_colour_', 'k_d2_'))]
    return sorted(out, key=lambda r: -r['total_us'])


import numpy as np
import torch
import pcgcv2_amd
pcgcv2_amd.configure_host_threads()
from pcgcv2_amd import ops, synthetic
from pcgcv2_amd import pc_error as pe
from pcgcv2_amd.coder import Coder
from pcgcv2_amd.data_utils import write_ply_ascii_geo_rgb
from pcgcv2_amd.pcc_model import PCCModel
from pcgcv2_amd.sparse import SparseTensor

dev = torch.device('cuda:0')
pts = synthetic.cloud(args.cloud, device=dev)
a = torch.cat([torch.zeros((len(pts), 1), dtype=torch.int32, device=dev), pts], 1).contiguous()
model = PCCModel().to(dev)
model.load_state_dict(synthetic.synthetic_state_dict())
with tempfile.TemporaryDirectory() as d:
    coder = Coder(model, os.path.join(d, 'f'))
    coder.encode(SparseTensor(torch.ones((len(pts), 1), device=dev), coordinates=a, tensor_stride=1, device=dev))
    b = coder.decode().C.detach().contiguous()
t = pts.double() / float(pts.max() + 1)                              # a smooth colour field plus noise, like a textured surface
rgb = torch.stack([255 * t[:, 0], 127.5 * (1 + torch.sin(40 * t[:, 1])), 255 * t[:, 2] * t[:, 0]], 1)
ca = (rgb + torch.randint(-12, 13, rgb.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(1))).round().clamp(0, 255).to(torch.uint8)

if args.one_call:
    for _ in range(2):
        nn = pe.nn_both(a, b)
        cb = pe.recolour_device(a, ca, b, nn=nn)
        pe.colour_psnr_device(a, ca, b, cb, nn=nn)
    torch.cuda.synchronize()
    raise SystemExit(0)


def median_ms(fn):
    fn(); torch.cuda.synchronize()                                    # (warm: code objects, allocator)
    times = []
    for _ in range(max(args.repeat, 10)):
        torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); times.append(time.perf_counter() - t0)
    return round(float(np.median(times)) * 1e3, 3)


nn = pe.nn_both(a, b)
cb = pe.recolour_device(a, ca, b, nn=nn)
metric = pe.colour_psnr_device(a, ca, b, cb, nn=nn)
report = {'cloud': args.cloud, 'points_source': len(a), 'points_target': len(b), 'runs': max(args.repeat, 10),
          'median_ms': {'two_searches_alone': median_ms(lambda: pe.nn_both(a, b)),
                        'recolour_shared_searches': median_ms(lambda: pe.recolour_device(a, ca, b, nn=nn)),
                        'recolour_own_searches': median_ms(lambda: pe.recolour_device(a, ca, b)),
                        'metric_shared_searches': median_ms(lambda: pe.colour_psnr_device(a, ca, b, cb, nn=nn)),
                        'metric_own_searches': median_ms(lambda: pe.colour_psnr_device(a, ca, b, cb)),
                        'd2_normals_transfer_for_comparison': median_ms(lambda: ops.d2_normals(len(b), nn[0], ca.double(), nn[1]))},
          'colour_psnr_y_u_v': [metric[f'c[{k}],PSNRF'] for k in range(3)],
          'two_runs_bitwise_equal': bool(torch.equal(cb, pe.recolour_device(a, ca, b, nn=nn)))}
a_h, b_h, ca_h, cb_h = a[:, 1:].cpu().numpy(), b[:, 1:].cpu().numpy(), ca.cpu().numpy(), cb.cpu().numpy()
if not args.no_host:
    t0 = time.perf_counter(); host_cb = pe.recolour(a_h, ca_h, b_h); t_rec = time.perf_counter() - t0
    t0 = time.perf_counter(); host_m = pe.colour_psnr(a_h, ca_h, b_h, cb_h); t_met = time.perf_counter() - t0
    report['host_numpy_ms'] = {'recolour': round(t_rec * 1e3, 1), 'metric': round(t_met * 1e3, 1)}
    report['host_cpus'] = pcgcv2_amd.effective_cpus()
    report['recolour_equal_to_host'] = bool(np.array_equal(host_cb, cb_h))
    report['metric_equal_to_host'] = all(np.float64(metric[k]).tobytes() == np.float64(host_m[k]).tobytes() for k in metric)
with tempfile.TemporaryDirectory() as d:
    import pandas as pd
    t0 = time.perf_counter(); write_ply_ascii_geo_rgb(os.path.join(d, 'n.ply'), b_h, cb_h); t_native = time.perf_counter() - t0
    t0 = time.perf_counter()
    with open(os.path.join(d, 'p.ply'), 'w', newline='') as f:
        f.write('ply\nformat ascii 1.0\nelement vertex %d\n' % len(b_h) + ''.join(f'property float {c}\n' for c in 'xyz') +
                ''.join(f'property uchar {c}\n' for c in ('red', 'green', 'blue')) + 'end_header\n')
        pd.DataFrame(np.concatenate([b_h.astype(np.int64), cb_h.astype(np.int64)], 1)).to_csv(f, sep=' ', header=False, index=False, lineterminator='\n')
    t_pandas = time.perf_counter() - t0
    report['ply_writer_ms'] = {'native': round(t_native * 1e3, 1), 'pandas': round(t_pandas * 1e3, 1),
                               'same_bytes': open(os.path.join(d, 'n.ply'), 'rb').read() == open(os.path.join(d, 'p.ply'), 'rb').read()}
if args.trace:
    report['kernel_trace'] = trace_table()
print(json.dumps(report, indent=1))
