#!/usr/bin/env python3
"""Time of one generate_dataset.mesh2pc on a synthetic mesh (an icosahedron subdivided 6 times: 81 920 triangles, written as an OFF file
so that the native reader is timed too), 4e5 samples at resolution 255, split into file parse / upload + CDF / voxelize / copy-out, with the
numpy definition (tests/mesh_reference.py) of the same call for scale.  With --trace it re-runs itself once under
`rocprofv3 --kernel-trace --stats` (a fresh child process) and prints the mesh kernels' table.
    tools/generate_dataset_time.py [--n_points N] [--resolution R] [--levels L] [--repeat K] [--trace]"""
import argparse, csv, glob, json, os, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
ap = argparse.ArgumentParser()
ap.add_argument('--n_points', type=int, default=400000)
ap.add_argument('--resolution', type=int, default=255)
ap.add_argument('--levels', type=int, default=6, help='subdivisions of the icosahedron: 20 * 4^levels triangles')
ap.add_argument('--repeat', type=int, default=5)
ap.add_argument('--trace', action='store_true', help='also one rocprofv3 --kernel-trace --stats run of a single mesh2pc (child process)')
ap.add_argument('--one-call', action='store_true', help=argparse.SUPPRESS)
args = ap.parse_args()


def trace_table():
    with tempfile.TemporaryDirectory() as d:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '--', sys.executable, os.path.abspath(__file__),
               '--n_points', str(args.n_points), '--resolution', str(args.resolution), '--levels', str(args.levels), '--one-call']
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise SystemExit('rocprofv3 failed:\n' + r.stderr[-2000:])
        rows = []
        for path in glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True):
            rows += list(csv.DictReader(open(path)))
    out = [{'kernel': r['Name'][:60], 'calls': int(r['Calls']), 'total_us': round(float(r['TotalDurationNs']) / 1e3, 1),
            'mean_us': round(float(r['AverageNs']) / 1e3, 1)} for r in rows if 'k_mesh_' in r.get('Name', '')]
    return sorted(out, key=lambda r: -r['total_us'])


import numpy as np
import torch
import mesh_reference as mr
from pcgcv2_amd import generate_dataset as gd, ops


def icosphere(levels):
    p = (1 + 5 ** 0.5) / 2
    v = np.array([[-1, p, 0], [1, p, 0], [-1, -p, 0], [1, -p, 0], [0, -1, p], [0, 1, p], [0, -1, -p], [0, 1, -p],
                  [p, 0, -1], [p, 0, 1], [-p, 0, -1], [-p, 0, 1]], dtype=np.float64)
    f = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
                  [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]], dtype=np.int64)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    for _ in range(levels):
        e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
        edges, inv = np.unique(e, axis=0, return_inverse=True)
        mid = v[edges[:, 0]] + v[edges[:, 1]]
        mid /= np.linalg.norm(mid, axis=1, keepdims=True)
        m = len(v) + inv.reshape(3, -1)                  # midpoints of edges (01), (12), (20) of every face
        v = np.concatenate([v, mid])
        f = np.concatenate([np.stack([f[:, 0], m[0], m[2]], 1), np.stack([f[:, 1], m[1], m[0]], 1), np.stack([f[:, 2], m[2], m[1]], 1),
                            np.stack([m[0], m[1], m[2]], 1)])
    return v, f.astype(np.int32)


dev = torch.device('cuda:0')
verts, faces = icosphere(args.levels)
tmp = tempfile.mkdtemp()
path = os.path.join(tmp, 'icosphere.off')
mr.write_off(path, verts, [tuple(t) for t in faces])
seed, n, res = 0, args.n_points, args.resolution
R = gd.get_rotate_matrix(np.random.default_rng(seed))


def sync():
    torch.cuda.synchronize()


def one_call():
    t0 = time.perf_counter()
    v, f = gd.read_mesh(path)
    t1 = time.perf_counter()
    dv, df = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    cdf = ops.mesh_area_cdf(dv, df)
    sync(); t2 = time.perf_counter()
    rows = ops.mesh_voxelize(dv, df, cdf, seed, n, R, res)
    sync(); t3 = time.perf_counter()
    out = rows[:, 1:].cpu().numpy()
    t4 = time.perf_counter()
    return out, cdf, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)


if args.one_call:
    one_call(); one_call()
    raise SystemExit(0)

runs = [one_call() for _ in range(args.repeat + 1)][1:]          # (the first call loads the code objects)
best = [min(r[2][k] for r in runs) * 1e3 for k in range(4)]
out, cdf = runs[-1][0], runs[-1][1].cpu().numpy()
t = time.perf_counter(); whole = gd.mesh2pc(path, n, res, seed=seed); sync(); t_whole = time.perf_counter() - t
t = time.perf_counter(); ref = mr.voxelize(verts, faces, cdf, seed, n, R, res); t_ref = time.perf_counter() - t
report = {'mesh': {'vertices': len(verts), 'triangles': len(faces), 'file_bytes': os.path.getsize(path)}, 'n_points': n, 'resolution': res,
          'voxels': len(out), 'ms_min_of_%d' % args.repeat: {'file_parse': round(best[0], 3), 'upload_cdf': round(best[1], 3),
                                                            'voxelize': round(best[2], 3), 'copy_out': round(best[3], 3),
                                                            'sum': round(sum(best), 3)},
          'mesh2pc_ms': round(t_whole * 1e3, 3), 'numpy_definition_ms': round(t_ref * 1e3, 1),
          'equal_to_definition': bool(np.array_equal(out, ref) and np.array_equal(whole, ref))}
if args.trace:
    report['kernel_trace'] = trace_table()
print(json.dumps(report, indent=1))
