#!/usr/bin/env python3
"""What a training batch costs before the step starts, from ONE fresh process: 64 synthetic clouds at resolution 127 (perturbed shells on a
128^3 grid, written once as ASCII PLY to a temporary directory), batch size 8.  ms per batch DELIVERED, i.e. until coords and feats lie
on the device where Trainer._tensor's SparseTensor wants them (one synchronise per epoch), for
  (a) train.PlyLoader, the route of `python -m pcgcv2_amd.train` without a loader flag: the baseline;
  (b) data_loader's host cache with num_workers 0 and 4, first epoch (files) and second (cache);
  (c) data_loader's device cache, first epoch (files -> arena) and second (arena alone);
next to the ms of one Trainer.step on such a batch, and ops.collate_rows alone (device events) against the bytes it reads and writes.
Every epoch figure is the least of --repeat fresh loaders.  With --trace it re-runs itself once under `rocprofv3 --kernel-trace --stats`
(a fresh child process) and prints k_collate_rows' row.      tools/data_loader_time.py [--clouds N] [--batch_size B] [--repeat K] [--trace]"""
import argparse, atexit, csv, glob, json, os, shutil, subprocess, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument('--clouds', type=int, default=64)
ap.add_argument('--batch_size', type=int, default=8)
ap.add_argument('--repeat', type=int, default=3)
ap.add_argument('--steps', type=int, default=10, help='Trainer.step calls timed (after 3 of warm-up)')
ap.add_argument('--trace', action='store_true', help='also one rocprofv3 --kernel-trace --stats run of two device-cache epochs (child process)')
ap.add_argument('--one-call', action='store_true', help=argparse.SUPPRESS)
args = ap.parse_args()

HBM_PEAK_TBS = 8.0               # MI355X HBM3E


def trace_table():
    with tempfile.TemporaryDirectory() as d:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '--', sys.executable, os.path.abspath(__file__),
               '--clouds', str(args.clouds), '--batch_size', str(args.batch_size), '--one-call']
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise SystemExit('rocprofv3 failed:\n' + r.stderr[-2000:])
        rows = []
        for path in glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True):
            rows += list(csv.DictReader(open(path)))
    return [{'kernel': r['Name'][:60], 'calls': int(r['Calls']), 'total_us': round(float(r['TotalDurationNs']) / 1e3, 1),
             'mean_us': round(float(r['AverageNs']) / 1e3, 2)} for r in rows if 'k_collate_rows' in r.get('Name', '')]


import torch
import pcgcv2_amd
pcgcv2_amd.configure_host_threads()
from pcgcv2_amd import data_loader as dl, ops, synthetic, train
from pcgcv2_amd.data_utils import write_ply_ascii_geo
from pcgcv2_amd.pcc_model import PCCModel
from pcgcv2_amd.trainer import Trainer, TrainingConfig

dev = torch.device('cuda:0')
tmp = tempfile.mkdtemp()
atexit.register(shutil.rmtree, tmp, True)
files, rows = [], []
for i in range(args.clouds):
    pts = synthetic._shell(128, 40.0 + 0.25 * (i % 64), 3.0, (2 + i % 4, 3 + i % 5)).numpy()
    files.append(os.path.join(tmp, f'cloud_{i:03d}.ply'))
    write_ply_ascii_geo(files[-1], pts)
    rows.append(len(pts))


def epoch_ms(loader):
    """ms per batch of one pass, every batch brought to the device as Trainer._tensor would"""
    torch.cuda.synchronize()
    t = time.perf_counter()
    n = 0
    for coords, feats in loader:
        coords, feats = torch.as_tensor(coords).to(dev), torch.as_tensor(feats).float().to(dev)
        n += 1
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / n


def two_epochs(make):
    firsts, seconds = [], []
    for _ in range(args.repeat):
        loader = make()
        firsts.append(epoch_ms(loader))
        seconds.append(epoch_ms(loader))
    return round(min(firsts), 3), round(min(seconds), 3)


def loader(**kw):
    return lambda: dl.make_data_loader(dl.PCDataset(files), batch_size=args.batch_size, shuffle=False, **kw)


if args.one_call:
    ld = loader(num_workers=0, device_cache=True, device=dev)()
    epoch_ms(ld); epoch_ms(ld)
    raise SystemExit(0)

epoch_ms(loader(num_workers=0, device_cache=True, device=dev)())          # (loads the code object, starts the allocator)
report = {'clouds': args.clouds, 'batch_size': args.batch_size, 'rows_per_cloud': {'min': min(rows), 'mean': round(sum(rows) / len(rows)), 'max': max(rows)},
          'ply_bytes': sum(os.path.getsize(f) for f in files), 'repeat': args.repeat, 'ms_per_batch': {}}
ms = report['ms_per_batch']
ms['a_ply_loader'], ms['a_ply_loader_again'] = two_epochs(lambda: train.PlyLoader(files, args.batch_size, shuffle=False))
for w in (0, 4):
    ms[f'b_host_cache_workers{w}_epoch1'], ms[f'b_host_cache_workers{w}_epoch2'] = two_epochs(loader(num_workers=w))
for w in (0, 4):
    ms[f'c_device_cache_workers{w}_epoch1'], ms[f'c_device_cache_workers{w}_epoch2'] = two_epochs(loader(num_workers=w, device_cache=True, device=dev))

# one Trainer.step on such a batch
config = TrainingConfig(logdir=os.path.join(tmp, 'logs'), ckptdir=os.path.join(tmp, 'ckpts'), init_ckpt='', alpha=1., beta=1., lr=8e-4, check_time=10)
trainer = Trainer(config=config, model=PCCModel(), device=dev)
trainer.model.load_state_dict(synthetic.synthetic_state_dict())
optimizer = trainer.set_optimizer()
ld = loader(num_workers=0, device_cache=True, device=dev)()
batch = next(iter(ld))
x = trainer._tensor(*batch)
for _ in range(3):
    trainer.step(x, optimizer)
torch.cuda.synchronize()
t = time.perf_counter()
for _ in range(args.steps):
    trainer.step(x, optimizer)
torch.cuda.synchronize()
report['trainer_step'] = {'rows': len(x), 'ms': round((time.perf_counter() - t) * 1e3 / args.steps, 3)}
t = time.perf_counter()
for _ in range(args.steps):
    trainer._tensor(*batch)
torch.cuda.synchronize()
report['trainer_tensor_ms'] = round((time.perf_counter() - t) * 1e3 / args.steps, 3)

# collate_rows alone: the first batch's items, device events around 100 launches
items = [(*ld.arena.table[i][:3], 0, ld.arena.table[i][4]) for i in range(min(args.batch_size, len(files)))]
n = sum(i[1] for i in items)
out = (torch.empty((n, 4), dtype=torch.int32, device=dev), torch.empty((n, 1), dtype=torch.float32, device=dev))
for _ in range(10):
    ops.collate_rows(ld.arena.buf, items, out=out)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(100):
    ops.collate_rows(ld.arena.buf, items, out=out)
e1.record(); torch.cuda.synchronize()
us = e0.elapsed_time(e1) / 100 * 1e3
moved = sum(3 * i[2] * i[1] for i in items) + 20 * n
report['collate_rows'] = {'rows': n, 'bytes_read': moved - 20 * n, 'bytes_written': 20 * n, 'us_per_launch_back_to_back': round(us, 2),
                          'GB_per_s': round(moved / us / 1e3, 1), 'fraction_of_hbm_peak': round(moved / us / 1e6 / HBM_PEAK_TBS, 4),
                          'us_at_hbm_peak': round(moved / HBM_PEAK_TBS / 1e6, 2)}
if args.trace:
    report['kernel_trace'] = trace_table()
print(json.dumps(report, indent=1))
