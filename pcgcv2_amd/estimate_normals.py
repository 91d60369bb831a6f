"""`python -m pcgcv2_amd.estimate_normals --filedir in.ply --out out.ply [--r2 16] [--orient centroid|none|x,y,z]`: normals of a voxelised
ASCII PLY estimated on the GPU (pc_error.estimate_normals_device), written next to the coordinates as `nx ny nz` (float32) so that any
cloud can be given to the D2 (point-to-plane) metric.  The reference has no such tool: it assumes clouds whose normals were estimated
elsewhere.  Rows without a valid normal (fewer than three neighbours, or all of them on one line) are written with (0, 0, 0)."""
import argparse
import time


def parse_orient(text):
    """'centroid' | 'none' | 'x,y,z' -> 'centroid' | None | (x, y, z)"""
    t = text.strip().lower()
    if t == 'centroid':
        return 'centroid'
    if t == 'none':
        return None
    try:
        view = tuple(float(v) for v in t.split(','))
    except ValueError:
        view = ()
    if len(view) != 3:
        raise argparse.ArgumentTypeError(f"orient is 'centroid', 'none' or a viewpoint 'x,y,z', got {text!r}")
    return view


def parser():
    p = argparse.ArgumentParser(description=__doc__.split('\n\n')[0], formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('--filedir', required=True, help='input ASCII PLY (integer coordinates)')
    p.add_argument('--out', required=True, help='output ASCII PLY with x y z nx ny nz')
    p.add_argument('--r2', type=int, default=16, help='squared radius of the neighbourhood, 1 .. 64')
    p.add_argument('--orient', type=parse_orient, default='centroid',
                   help="sign of the normals: away from the centroid, 'none' (largest component positive) or towards a viewpoint x,y,z")
    return p


def main(argv=None):
    args = parser().parse_args(argv)
    if not 1 <= args.r2 <= 64:
        raise SystemExit(f'--r2 must be in 1 .. 64, got {args.r2}')
    import torch
    from .data_utils import write_ply_ascii_geo_normals
    from .pc_error import estimate_normals_device, lattice_coords, read_ply_ascii_with_normals
    xyz, _ = read_ply_ascii_with_normals(args.filedir)
    coords = lattice_coords(xyz, torch.device('cuda'))
    estimate_normals_device(coords, args.r2, args.orient)              # (warm: library load, ball table)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    normals, _, _, valid = estimate_normals_device(coords, args.r2, args.orient)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    write_ply_ascii_geo_normals(args.out, xyz, normals.cpu().numpy())
    invalid = len(xyz) - int(valid.sum().item())
    print(f'{len(xyz)} points, {invalid} rows without a valid normal, {ms:.2f} ms (r2 = {args.r2}) -> {args.out}')
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
