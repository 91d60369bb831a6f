#!/usr/bin/env python3
"""Time of the device D2 metric (pc_error.d2_psnr_device) against the host d2_psnr on the bench frame: shell10 with outward normals against the
cloud the synthetic-weight codec decodes from it (as tools/d1_time.py), plus the device D1 for scale."""
import os, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import pcgcv2_amd
pcgcv2_amd.configure_host_threads()
from pcgcv2_amd import synthetic
from pcgcv2_amd.pcc_model import PCCModel
from pcgcv2_amd.coder import Coder
from pcgcv2_amd.sparse import SparseTensor
from pcgcv2_amd.pc_error import d1_psnr_device, d2_psnr_device, d2_psnr
dev = torch.device('cuda:0')
pts = synthetic.shell('shell10', device=dev)
coords = torch.cat([torch.zeros((len(pts), 1), dtype=torch.int32, device=dev), pts], 1).contiguous()
model = PCCModel().to(dev); model.load_state_dict(synthetic.synthetic_state_dict())
coder = Coder(model, os.path.join(tempfile.mkdtemp(), 'f'))
x = SparseTensor(torch.ones((len(pts), 1), device=dev), coordinates=coords, tensor_stride=1, device=dev)
coder.encode(x); out = coder.decode()
a = coords[:, 1:].cpu().numpy()
v = a - a.mean(0)
na = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32).astype(np.float64)
na_dev = torch.from_numpy(na).to(dev)
for name, fn in (('device D1', lambda: d1_psnr_device(coords, out.C, 1024)), ('device D2', lambda: d2_psnr_device(coords, na_dev, out.C, 1024))):
    times = []
    for _ in range(5):
        torch.cuda.synchronize(); t = time.perf_counter(); m = fn(); torch.cuda.synchronize(); times.append(time.perf_counter() - t)
    print(f'{name}: {min(times) * 1e3:.2f} ms (min of 5, median {sorted(times)[2] * 1e3:.2f} ms)  {len(a)} vs {len(out)} points')
md = m
t = time.perf_counter(); mh = d2_psnr(a, na, out.C[:, 1:].cpu().numpy(), 1024); th = time.perf_counter() - t
print(f'host D2: {th:.2f} s  ({pcgcv2_amd.effective_cpus()} CPUs)')
p2point = [k for k in mh if 'p2point' in k]
p2plane = [k for k in mh if 'p2plane' in k]
print('p2point identical', all(md[k] == mh[k] for k in p2point),
      ' p2plane max rel diff', max(abs(md[k] - mh[k]) / abs(mh[k]) for k in p2plane if mh[k]))
print('mseF,PSNR (p2point)', round(md['mseF,PSNR (p2point)'], 4), ' mseF,PSNR (p2plane)', round(md['mseF,PSNR (p2plane)'], 4))
