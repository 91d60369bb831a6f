#!/usr/bin/env python3
"""One training step on the bench frame (shell10, vox10) with synthetic weights, from ONE fresh process with a warm-up: ms per
PCCModel.forward_train (+ loss.sum_loss), per backward and per Adam step (HIP events around each phase of K steps), next to the
teacher-forced forward without a graph.  With --trace it re-runs itself once under `rocprofv3 --kernel-trace --stats` (a fresh child
process) and prints the per-kernel table of the backward pass's kernels, with pcgc_conv_wgrad's fraction of the fp32 MFMA peak from
algorithmic flops 2 P Cin Cout per layer.      tools/train_step_time.py [--steps K] [--warmup W] [--cloud NAME] [--trace]"""
import argparse, csv, glob, json, os, subprocess, sys, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument('--steps', type=int, default=10)
ap.add_argument('--warmup', type=int, default=3)
ap.add_argument('--cloud', default='shell10')
ap.add_argument('--trace', action='store_true', help='also one rocprofv3 --kernel-trace --stats run of a single step (child process)')
ap.add_argument('--one-step', action='store_true', help=argparse.SUPPRESS)
args = ap.parse_args()

GRAD_KERNELS = ('k_conv_wgrad', 'k_wgrad_sum', 'k_kmap_invert', 'k_relu_bwd', 'k_scatter_rows', 'k_bce_bwd', 'k_eb_bwd')


def trace_table():
    with tempfile.TemporaryDirectory() as d:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '--', sys.executable, os.path.abspath(__file__),
               '--cloud', args.cloud, '--one-step']
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise SystemExit('rocprofv3 failed:\n' + r.stderr[-2000:])
        rows = []
        for path in glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True):
            rows += list(csv.DictReader(open(path)))
    out = []
    for r in rows:
        name = r.get('Name', '')
        if any(k in name for k in GRAD_KERNELS):
            out.append({'kernel': name[:90], 'calls': int(r['Calls']), 'total_us': round(float(r['TotalDurationNs']) / 1e3, 1),
                        'mean_us': round(float(r['AverageNs']) / 1e3, 1)})
    return sorted(out, key=lambda r: -r['total_us'])


import torch
import pcgcv2_amd
pcgcv2_amd.configure_host_threads()
from pcgcv2_amd import loss, ops, synthetic
from pcgcv2_amd.pcc_model import PCCModel
from pcgcv2_amd.sparse import SparseTensor

dev = torch.device('cuda:0')
pts = synthetic.cloud(args.cloud, device=dev)
coords = torch.cat([torch.zeros((len(pts), 1), dtype=torch.int32, device=dev), pts], 1).contiguous()
model = PCCModel().to(dev); model.load_state_dict(synthetic.synthetic_state_dict())
x = SparseTensor(torch.ones((len(pts), 1), device=dev), coordinates=coords, tensor_stride=1, device=dev)
gen = torch.Generator(device=dev); gen.manual_seed(0)
opt = torch.optim.Adam([{'params': m.parameters(), 'lr': 8e-4} for m in model._modules.values()], betas=(0.9, 0.999), weight_decay=1e-4)


def step(ev=None):
    mark = (lambda i: ev[i].record()) if ev else (lambda i: None)
    opt.zero_grad()
    mark(0)
    out = model.forward_train(x, generator=gen)
    total, _, _ = loss.sum_loss(out, len(x))
    mark(1)
    total.backward()
    mark(2)
    opt.step()
    mark(3)


if args.one_step:
    step(); torch.cuda.synchronize()
    sys.exit(0)

for _ in range(args.warmup):
    step()
torch.cuda.synchronize()
acc = [0.0, 0.0, 0.0]
for _ in range(args.steps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    step(ev)
    torch.cuda.synchronize()
    for i in range(3):
        acc[i] += ev[i].elapsed_time(ev[i + 1])
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(args.steps):
    model(x, training=True, generator=gen)
e1.record(); torch.cuda.synchronize()
report = {'cloud': args.cloud, 'points': len(x), 'steps': args.steps, 'warmup': args.warmup,
          'ms_forward_train': round(acc[0] / args.steps, 3), 'ms_backward': round(acc[1] / args.steps, 3), 'ms_adam': round(acc[2] / args.steps, 3),
          'ms_step': round(sum(acc) / args.steps, 3), 'ms_teacher_forced_forward': round(e0.elapsed_time(e1) / args.steps, 3),
          'peak_memory_MiB': round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)}

# pcgc_conv_wgrad per layer shape, timed on its own on the recorded forward point: algorithmic flops 2 P Cin Cout against the fp32 MFMA peak
record = {}
out = model.forward_train(x, generator=gen, record=record)
loss.sum_loss(out, len(x))[0].backward()
shapes = {}
for name, e in record.items():
    if 'gy' not in e or e.get('kind') not in ('k3', 'k1', 'down'):
        continue
    nbr, xin, gy = e['map'], e['x'], e['gy'].contiguous()
    key = (e['kind'], xin.shape[1], gy.shape[1], gy.shape[0])
    if key in shapes:
        continue
    pairs = int((nbr >= 0).sum()) if nbr is not None else gy.shape[0]
    for _ in range(2):
        ops.conv_wgrad(nbr, xin, gy)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(5):
        ops.conv_wgrad(nbr, xin, gy)
    t1.record(); torch.cuda.synchronize()
    us = t0.elapsed_time(t1) / 5 * 1e3
    flops = 2.0 * pairs * key[1] * key[2]
    shapes[key] = {'layer': name, 'kind': key[0], 'Cin': key[1], 'Cout': key[2], 'rows': key[3], 'pairs': pairs, 'us': round(us, 1),
                   'tflops': round(flops / us / 1e6, 2), 'fraction_of_fp32_mfma_peak': round(flops / us / 1e6 / ops.MFMA_F32_PEAK_TFLOPS, 4)}
report['conv_wgrad'] = sorted(shapes.values(), key=lambda r: -r['us'])
if args.trace:
    report['kernel_trace'] = trace_table()
print(json.dumps(report, indent=1))
