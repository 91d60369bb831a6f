#!/usr/bin/env python3
"""Time of the renderer on a synthetic cloud, warm, in this fresh process: 6 faces at --size^2 (1024), at point sizes 1 and 3.
Per point size: the median of --repeat whole render() calls and of view_metric(), the ms per phase (clear, splat, resolve, each launched alone
on the same buffers and synchronised, so their sum exceeds the whole call; metric; copies = the matrices up and the refusal count down; PNG =
six files encoded on the host), the atomics the splat sent in one call next to their ceiling N V (2r+1)^2 (the difference is the early-outs
and the clipped pixels), the numpy definition (tests/render_reference.py) of the same call on this host's CPUs, and whether the two agree.
With --trace it re-runs itself once under `rocprofv3 --kernel-trace --stats` (a fresh child process) and prints the kernels' table.
    tools/render_time.py [--cloud shell10] [--size 1024] [--point_sizes 1,3] [--repeat R] [--no-host] [--trace]"""
import argparse, csv, glob, json, os, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

ap = argparse.ArgumentParser()
ap.add_argument('--cloud', default='shell10')
ap.add_argument('--size', type=int, default=1024)
ap.add_argument('--point_sizes', default='1,3')
ap.add_argument('--repeat', type=int, default=11)
ap.add_argument('--no-host', action='store_true', help='skip the numpy definition')
ap.add_argument('--trace', action='store_true', help='also one rocprofv3 --kernel-trace --stats run of two calls per point size (child process)')
ap.add_argument('--one-call', action='store_true', help=argparse.SUPPRESS)
args = ap.parse_args()


def trace_table():
    with tempfile.TemporaryDirectory() as d:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '--', sys.executable, os.path.abspath(__file__),
               '--cloud', args.cloud, '--size', str(args.size), '--point_sizes', args.point_sizes, '--one-call']
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
from pcgcv2_amd import ops, render, synthetic
from pcgcv2_amd._lib import lib, check

dev = torch.device('cuda:0')
p = synthetic.cloud(args.cloud).numpy()
c = np.concatenate([np.zeros((len(p), 1), np.int32), p], 1)
rgb = np.stack([p[:, 0], p[:, 1], p[:, 2]], 1).astype(np.uint8)
bits = render.bits_for(p)
coords, colours = torch.from_numpy(c).to(dev), torch.from_numpy(rgb).to(dev)
n, V, S = len(c), 6, args.size
matrices = render.view_matrices('faces', bits, S)
planes = render.depth_planes(matrices, bits)


def med(f, runs):
    ts = []
    for _ in range(runs):
        torch.cuda.synchronize(); t = time.perf_counter(); f(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t)
    return round(float(np.median(ts)) * 1e3, 3)


def one_size(ps):
    r = (ps - 1) // 2
    call = lambda times=None: render.render(coords, colours, 'faces', S, bits, ps, batch_items=1, times=times)
    a = call()
    b = render.render(coords[::2].contiguous(), colours[::2].contiguous(), a.matrices, S, bits, ps, batch_items=1)
    render.view_metric(a, b); torch.cuda.synchronize()                  # (warm: code objects, allocator)
    if args.one_call:
        call(); render.view_metric(a, b); torch.cuda.synchronize()
        return None
    runs = max(args.repeat, 10)
    rep = {'point_size': ps, 'runs': runs, 'median_ms': {'whole_call': med(call, runs), 'metric': med(lambda: ops.render_metric(a, b), runs)}}
    copies = []
    for _ in range(runs):
        times = {}
        call(times)
        copies.append(times['copies'])
    rep['median_ms']['copies'] = round(float(np.median(copies)) * 1e3, 3)
    # the phases alone, on buffers of their own
    L, s = lib(), torch.cuda.current_stream().cuda_stream
    m_dev, p_dev = torch.from_numpy(matrices).to(dev), torch.from_numpy(planes).to(dev)
    image = torch.empty((1, V, S, S, 3), dtype=torch.uint8, device=dev)
    depth, index = (torch.empty((1, V, S, S), dtype=torch.int32, device=dev) for _ in range(2))
    mask = torch.empty((1, V, S, S), dtype=torch.uint8, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    issued = torch.zeros(1, dtype=torch.int64, device=dev)
    ws_bytes = int(L.pcgc_render_workspace_bytes(1, V, S, S))
    ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=dev)
    phase = lambda which, count=None: check(L.pcgc_render(coords.data_ptr(), colours.data_ptr(), n, 1, V, S, S, r, m_dev.data_ptr(), p_dev.data_ptr(),
                                                          0xFFFFFF, index.data_ptr(), depth.data_ptr(), mask.data_ptr(), image.data_ptr(), bad.data_ptr(),
                                                          None if count is None else count.data_ptr(), which, ws.data_ptr(), ws_bytes, s), 'render')
    per = {'clear': [], 'splat': [], 'resolve': []}
    for _ in range(runs):
        for name, which in (('clear', 1), ('splat', 2), ('resolve', 4)):
            torch.cuda.synchronize(); t = time.perf_counter(); phase(which); torch.cuda.synchronize(); per[name].append(time.perf_counter() - t)
    for name in per:
        rep['median_ms'][name] = round(float(np.median(per[name])) * 1e3, 3)
    assert all(torch.equal(x, y) for x, y in ((image, a.image), (depth, a.depth), (index, a.index), (mask, a.mask.view(torch.uint8))))
    phase(1); phase(2, issued); torch.cuda.synchronize()
    rep['splat_atomics'] = {'sent': int(issued.item()), 'ceiling_N_V_(2r+1)^2': n * V * ps * ps, 'covered_pixels': int(a.mask.sum().item())}
    images = a.image[0].cpu().numpy()
    t = time.perf_counter()
    data = [render.png_bytes(im) for im in images]
    rep['median_ms']['png_six_files'] = round((time.perf_counter() - t) * 1e3, 1)
    rep['png_bytes'] = sum(len(d) for d in data)
    m = render.view_metric(a, b)['mean']
    rep['against_every_second_row'] = {k: (None if np.isinf(v) else round(v, 4)) for k, v in m.items()}
    if not args.no_host:
        import render_reference as R
        t = time.perf_counter(); ref = R.render_views(c, rgb, 'faces', bits, S, r); t_ref = time.perf_counter() - t
        rep['numpy_definition_ms'] = round(t_ref * 1e3, 1)
        rep['equal_to_definition'] = bool(all(np.array_equal(getattr(a, f).cpu().numpy(), getattr(ref, f)) for f in ('index', 'depth', 'mask', 'image')))
    return rep


report = {'host_cpus': pcgcv2_amd.effective_cpus(), 'cloud': args.cloud, 'rows': n, 'bits': bits, 'views': V, 'size': S, 'point_sizes': []}
for ps in (int(v) for v in args.point_sizes.split(',')):
    rep = one_size(ps)
    if rep is not None:
        report['point_sizes'].append(rep)
if args.one_call:
    raise SystemExit(0)
if args.trace:
    report['kernel_trace'] = trace_table()
print(json.dumps(report, indent=1))
