#!/usr/bin/env python3
"""PCCModel.forward on the bench frame (shell10, vox10) in both decoder modes: training=False (top-k pruning, what the codec computes) and
training=True (top-k | ground truth: every true voxel survives whatever the weights, so the finer levels carry the neighbourhood of a real
surface instead of what random logits keep).  Prints, from ONE fresh process: ms per forward (warm-up, then HIP events around K steps) next
to one Coder.encode + decode step for scale, the rows and the mean k3 neighbours per row of each decoder level, and the rate estimate
get_bits next to the size of the `_F.bin` the coder writes for the same cloud.      tools/teacher_forced.py [--steps K] [--warmup W] [--cloud NAME]"""
import argparse, json, os, sys, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import pcgcv2_amd
pcgcv2_amd.configure_host_threads()
from pcgcv2_amd import loss, ops, synthetic
from pcgcv2_amd.pcc_model import PCCModel
from pcgcv2_amd.coder import Coder
from pcgcv2_amd.sparse import SparseTensor

ap = argparse.ArgumentParser()
ap.add_argument('--steps', type=int, default=10)
ap.add_argument('--warmup', type=int, default=3)
ap.add_argument('--cloud', default='shell10')
args = ap.parse_args()
dev = torch.device('cuda:0')
pts = synthetic.shell(args.cloud, device=dev)
coords = torch.cat([torch.zeros((len(pts), 1), dtype=torch.int32, device=dev), pts], 1).contiguous()
model = PCCModel().to(dev); model.load_state_dict(synthetic.synthetic_state_dict())
x = SparseTensor(torch.ones((len(pts), 1), device=dev), coordinates=coords, tensor_stride=1, device=dev)
gen = torch.Generator(device=dev); gen.manual_seed(0)


def timed(fn):
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.steps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.steps


def levels(out):
    """rows and mean k3 neighbours per row (the row itself included) of the three candidate levels the decoder convolves on"""
    res = []
    for cls in out['out_cls_list']:
        parent = cls.cmap.origin[1]
        res.append({'stride': cls.cmap.stride, 'rows': len(cls), 'k3_neighbours_per_row': round(ops.child_pairs(parent.k3) / len(cls), 3)})
    return res


report = {'cloud': args.cloud, 'points': len(x), 'steps': args.steps, 'warmup': args.warmup}
for name, training in (('inference', False), ('teacher_forced', True)):
    ms = timed(lambda: model(x, training=training, generator=gen))
    out = model(x, training=training, generator=gen)
    report[name] = {'ms_per_forward': round(ms, 3), 'out_rows': len(out['out']), 'levels': levels(out)}
    rec = loss.evaluate(model, x, training=training, generator=gen)
    report[name]['evaluate'] = rec
with tempfile.TemporaryDirectory() as d:
    coder = Coder(model, os.path.join(d, 'f'))

    def step():
        coder.encode(x); coder.decode()
    report['coder_encode_decode_ms'] = round(timed(step), 3)
    report['F_bin_bits_per_point'] = round(8 * os.path.getsize(os.path.join(d, 'f_F.bin')) / len(x), 5)
report['estimated_bits_per_point'] = round(report['inference']['evaluate']['bpp'], 5)
print(json.dumps(report, indent=1))
