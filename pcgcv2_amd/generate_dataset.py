"""Training clouds from triangle meshes on the GPU (reference generate_dataset.py): sample points on each mesh, rotate them randomly,
normalise to a cube, round and de-duplicate, write one PLY per mesh — what `python -m pcgcv2_amd.train --dataset 'clouds/*.ply'` reads.

The reference samples with open3d (std::mt19937 through library distributions), which cannot be reproduced.  The sampling here is this
project's own exact fp64 definition with a counter-based generator (csrc/mesh.hip); the steps after it are mesh2pc's
(generate_dataset.py:27-35) operation for operation.  Meshes are read natively (csrc/mesh_io.cpp: ASCII OFF and OBJ).

    python -m pcgcv2_amd.generate_dataset --mesh_root ModelNet40 --out dataset [--num_mesh 100 --n_points 400000 --resolution 127 --seed 0]
"""
import os
import random
import time

import numpy as np
import torch

from . import ops
from ._lib import lib, PcgcError
from .data_utils import write_ply_ascii_geo


class MeshFormatError(PcgcError):
    """the file is not a well-formed (or is a truncated) ASCII OFF / OBJ mesh"""


class MeshIndexError(PcgcError):
    """a face names a vertex the file does not have"""


def read_mesh(mesh_filedir):
    """-> vertices float64 [V,3], triangles int32 [T,3] (polygons fanned).  FileNotFoundError / MeshFormatError / MeshIndexError."""
    # One parse (the C entry also answers a sizes-only call): a vertex takes at least 6 bytes of text and a triangle at least 2 (one more
    # index of a polygon), so the file size bounds both counts; the untouched tail of the two buffers is never paged in.
    try:
        size = os.path.getsize(mesh_filedir)
    except OSError:
        raise FileNotFoundError(mesh_filedir) from None
    verts = np.empty((size // 6 + 1, 3), dtype=np.float64)
    faces = np.empty((size // 2 + 1, 3), dtype=np.int32)
    counts = np.zeros(2, dtype=np.int64)
    rc = int(lib().pcgc_mesh_read(os.fsencode(mesh_filedir), verts.ctypes.data, len(verts), faces.ctypes.data, len(faces), counts.ctypes.data))
    if rc == -1:
        raise FileNotFoundError(mesh_filedir)
    if rc == -4:
        raise MeshIndexError(f'{mesh_filedir}: a face names a vertex that does not exist')
    if rc == -5:
        raise PcgcError(f'{mesh_filedir}: file grew while reading')
    if rc != 0:
        raise MeshFormatError(f'{mesh_filedir}: malformed or truncated OFF / OBJ mesh')
    return verts[:int(counts[0])].copy(), faces[:int(counts[1])].copy()


def _device(device):
    return torch.device(device if device is not None else 'cuda')


def _upload(mesh_filedir, device):
    verts, faces = read_mesh(mesh_filedir)
    if len(verts) == 0 or len(faces) == 0:
        raise MeshFormatError(f'{mesh_filedir}: no triangles')
    verts, faces = torch.from_numpy(verts).to(device), torch.from_numpy(faces).to(device)
    cdf = ops.mesh_area_cdf(verts, faces)
    total = float(cdf[-1].item())
    if not (total > 0 and np.isfinite(total)):
        raise PcgcError(f'{mesh_filedir}: the total area of the mesh is {total}')
    return verts, faces, cdf


def sample_points(mesh_filedir, n_points=4e5, resolution=255, *, seed=0, device=None):
    """generate_dataset.py:7-16: int(n_points) points spread uniformly over the surface -> float64 [N,3] numpy.  (`resolution` is unused,
    as in the reference.)  Raises where the reference prints and returns None."""
    verts, faces, cdf = _upload(mesh_filedir, _device(device))
    _, pts = ops.mesh_sample(verts, faces, cdf, seed, 0, int(n_points), want_tri=False)
    return pts.cpu().numpy()


def get_rotate_matrix(rng=None):
    """generate_dataset.py:18-23: a random orthogonal matrix (Q of a Gaussian matrix, first axis flipped with probability 1/2), fp64 on
    the host.  rng: a numpy Generator; None draws from numpy's global state as the reference does."""
    m = np.eye(3, dtype='float32')
    if rng is None:
        m[0, 0] *= np.random.randint(0, 2) * 2 - 1
        g = np.random.randn(3, 3)
    else:
        m[0, 0] *= int(rng.integers(0, 2)) * 2 - 1
        g = rng.standard_normal((3, 3))
    return np.dot(m, np.linalg.qr(g)[0])


def mesh2pc(mesh_filedir, n_points, resolution, *, seed=0, rotation=None, device=None):
    """generate_dataset.py:25-36 -> int [M,3] numpy: the distinct voxels, ordered by (z, y, x) (the same set as the reference's
    np.unique, which orders x first).  `seed` fixes the samples and, unless `rotation` (3x3, applied as points . R) is given, the rotation."""
    if not 1 <= int(resolution) <= 1023:
        raise ValueError(f'resolution must be in 1 .. 1023, got {resolution}')
    if int(n_points) < 1:
        raise ValueError(f'n_points must be at least 1, got {n_points}')
    verts, faces, cdf = _upload(mesh_filedir, _device(device))
    if rotation is None:
        rotation = get_rotate_matrix(np.random.default_rng(seed))
    rows = ops.mesh_voxelize(verts, faces, cdf, seed, int(n_points), rotation, int(resolution))
    return rows[:, 1:].cpu().numpy().astype('int')


def generate_dataset(mesh_filedirs, pc_rootdir, out_filetype, n_points=4e5, resolution=255, *, seed=0, device=None):
    """generate_dataset.py:38-57: mesh idx (seed `seed + idx`) -> pc_rootdir/{idx}_{stem}.ply.  A mesh that cannot be read or has no area
    is reported with its reason and skipped."""
    if out_filetype == 'h5':
        raise ValueError("out_filetype 'h5' needs h5py, which this package does not use: write 'ply' (train.py reads PLY)")
    if out_filetype != 'ply':
        raise ValueError(f"out_filetype must be 'ply', got {out_filetype!r}")
    start_time = time.time()
    for idx, mesh_filedir in enumerate(mesh_filedirs):
        try:
            points = mesh2pc(mesh_filedir, n_points, resolution, seed=seed + idx, device=device)
        except (OSError, PcgcError) as e:
            print('ERROR generate_dataset', idx, mesh_filedir, f'{type(e).__name__}: {e}', '!' * 8)
            continue
        pc_filedir = os.path.join(pc_rootdir, str(idx) + '_' + os.path.split(mesh_filedir)[-1].split('.')[0] + '.ply')
        write_ply_ascii_geo(pc_filedir, points)
        if idx % 100 == 0:
            print('=' * 20, idx, round((time.time() - start_time) / 60.), 'mins', '=' * 20)
    return


def traverse_path_recursively(rootdir):
    """generate_dataset.py:59-73: every file below rootdir"""
    filedirs = []

    def gci(filepath):
        for fi in os.listdir(filepath):
            fi_d = os.path.join(filepath, fi)
            if os.path.isdir(fi_d):
                gci(fi_d)
            else:
                filedirs.append(fi_d)

    gci(rootdir)
    return filedirs


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description='ModelNet-style meshes (.off / .obj) -> voxelised training clouds (.ply)')
    ap.add_argument('--mesh_root', required=True, help='directory searched recursively for .off and .obj meshes')
    ap.add_argument('--out', required=True, help='directory the clouds are written to')
    ap.add_argument('--num_mesh', type=int, default=100, help='meshes drawn at random (all of them if there are fewer)')
    ap.add_argument('--n_points', type=int, default=int(4e5))
    ap.add_argument('--resolution', type=int, default=127)
    ap.add_argument('--seed', type=int, default=0)
    args = ap.parse_args(argv)
    input_filedirs = traverse_path_recursively(rootdir=args.mesh_root)
    mesh_filedirs = sorted(f for f in input_filedirs if os.path.splitext(f)[1].lower() in ('.off', '.obj'))
    mesh_filedirs = random.Random(args.seed).sample(mesh_filedirs, min(args.num_mesh, len(mesh_filedirs)))
    print('mesh_filedirs:\n', len(input_filedirs), len(mesh_filedirs))
    os.makedirs(args.out, exist_ok=True)
    generate_dataset(mesh_filedirs, args.out, 'ply', args.n_points, args.resolution, seed=args.seed)
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
