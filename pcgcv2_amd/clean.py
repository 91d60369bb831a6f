"""Outlier and fragment removal of a voxelised cloud on the GPU (csrc/clean.hip; the definition is tests/clean_reference.py):
what every point-cloud toolchain does straight after voxelising a scanner's cloud.  The reference has no such stage: it assumes clouds that
were cleaned elsewhere.

    stage 1, density     neighbours = the other voxels within squared distance r2; a row with fewer than min_neighbours goes
    stage 2, components  the 26-connected components of the survivors; a component with fewer than min_component rows goes, and with
                         keep_largest = n only the n largest of each batch item stay (ties to the smaller label)

One pass: nothing is counted again after rows go.  labels = the smallest input row of the row's component.

    python -m pcgcv2_amd.clean --filedir vox.ply [--r2 16] [--min_neighbours K] [--min_component M] [--keep_largest n] [--out clean.ply]
"""
import os

import torch

from . import ops
from .ops import Cleaned                                        # noqa: F401  (the record clean returns)


def clean(coords, colours=None, r2=16, min_neighbours=0, min_component=1, keep_largest=0, times=None):
    """ops.clean: device tensors coords int32 [N,4] (batch, x, y, z) of distinct voxels and colours uint8 [N,3] or None -> Cleaned(keep bool
    [N], neighbours, labels, sizes int32 [N], coords [M,4], colours [M,3] or None, removed_density, removed_component, n_components, rounds)"""
    return ops.clean(coords, colours, r2=r2, min_neighbours=min_neighbours, min_component=min_component, keep_largest=keep_largest, times=times)


def connected_components(coords):
    """stage 2 on all rows: coords int32 [N,4] of distinct voxels -> (labels int32 [N], sizes int32 [N], number of components)"""
    return ops.connected_components(coords)


# ------------------------------------------------------------------------------------------------ files
def clean_file(filedir, out, r2=16, min_neighbours=0, min_component=1, keep_largest=0, device=None):
    """voxelised PLY (integer coordinates, with or without colours) -> the cleaned ASCII PLY `out` (colours carried); -> Cleaned"""
    from .data_utils import read_ply_with_colours, write_ply_ascii_geo, write_ply_ascii_geo_rgb
    from .pc_error import lattice_coords
    from .sparse import require_gpu
    device = torch.device('cuda') if device is None else device
    require_gpu(device)
    xyz, rgb = read_ply_with_colours(filedir)
    c = clean(lattice_coords(xyz, device), None if rgb is None else torch.from_numpy(rgb).to(device), r2=r2, min_neighbours=min_neighbours,
              min_component=min_component, keep_largest=keep_largest)
    kept = c.coords[:, 1:].cpu().numpy()
    if rgb is None:
        write_ply_ascii_geo(out, kept)
    else:
        write_ply_ascii_geo_rgb(out, kept, c.colours.cpu().numpy())
    return c


def describe(c):
    """the one line the tools print: rows in, removed by density, removed by component, components, rows out"""
    return (f'clean:\t {len(c.keep)} rows in, {c.removed_density} removed by density, {c.removed_component} removed by component, '
            f'{c.n_components} components, {len(c.coords)} rows out')


def parse_clean(text):
    """'K,M' of --clean -> (min_neighbours, min_component)"""
    import argparse
    try:
        v = tuple(int(t) for t in text.split(','))
    except ValueError:
        v = ()
    if len(v) != 2 or v[0] < 0 or v[1] < 1:
        raise argparse.ArgumentTypeError(f'--clean is K,M (min_neighbours >= 0, min_component >= 1), got {text!r}')
    return v


def add_arguments(p):
    """--clean K,M [--clean_r2 R] [--keep_largest n] of voxelize.py, coder.py and attributes.py"""
    p.add_argument("--clean", metavar='K,M', type=parse_clean, default=None,
                   help="clean the voxelised cloud first (clean.py; after --voxelize when both are given): rows with fewer than K neighbours "
                        "go, then components of fewer than M rows; _clean.ply is written and the flow takes that file")
    p.add_argument("--clean_r2", type=int, default=16, help="with --clean: squared radius of the neighbour count, 1 .. 64")
    p.add_argument("--keep_largest", type=int, default=0, help="with --clean: keep only the n largest components (0: all)")


def check_arguments(p, args):
    if args.clean is None:
        if args.keep_largest or args.clean_r2 != 16:
            p.error('--clean_r2 and --keep_largest need --clean')
        return
    if not 1 <= args.clean_r2 <= ops.NORMALS_MAX_R2:
        p.error(f'--clean_r2 {args.clean_r2}: 1 .. {ops.NORMALS_MAX_R2}')
    if args.keep_largest < 0:
        p.error(f'--keep_largest {args.keep_largest}: at least 0')


def in_front(filedir, outdir, args):
    """`--clean K,M` of coder.py and attributes.py: the voxelised file cleaned into `<prefix>_clean.ply`, prefix = outdir / the file's name
    -> the path of `_clean.ply`, which the flow then takes as its --filedir"""
    os.makedirs(outdir, exist_ok=True)
    out = os.path.join(outdir, os.path.split(filedir)[-1].split('.')[0]) + '_clean.ply'
    c = clean_file(filedir, out, args.clean_r2, args.clean[0], args.clean[1], args.keep_largest)
    print(describe(c))
    if len(c.coords) == 0:
        raise ValueError(f'--clean {args.clean[0]},{args.clean[1]}: none of the {len(c.keep)} rows of {filedir} is left ({c.removed_density} removed by '
                         f'density, {c.removed_component} by component): nothing to code')
    return out


# ------------------------------------------------------------------------------------------------ CLI
def parser():
    import argparse
    p = argparse.ArgumentParser(description='remove isolated voxels and small components from a voxelised PLY on the GPU',
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('--filedir', required=True, help='input PLY: integer coordinates (a voxelised cloud), with or without red green blue')
    p.add_argument('--r2', type=int, default=16, help='squared radius of the neighbour count, 1 .. 64')
    p.add_argument('--min_neighbours', type=int, default=0, help='rows with fewer other voxels within the radius go (0: none)')
    p.add_argument('--min_component', type=int, default=1, help='26-connected components of the survivors with fewer rows go (1: none)')
    p.add_argument('--keep_largest', type=int, default=0, help='keep only the n largest components (0: all)')
    p.add_argument('--out', default=None, help='output ASCII PLY (default: the input name + _clean.ply)')
    return p


def main(argv=None):
    p = parser()
    args = p.parse_args(argv)
    if not 1 <= args.r2 <= ops.NORMALS_MAX_R2:
        p.error(f'--r2 {args.r2}: 1 .. {ops.NORMALS_MAX_R2}')
    if args.min_neighbours < 0 or args.min_component < 1 or args.keep_largest < 0:
        p.error('--min_neighbours >= 0, --min_component >= 1, --keep_largest >= 0')
    out = args.out or os.path.splitext(args.filedir)[0] + '_clean.ply'
    print(describe(clean_file(args.filedir, out, args.r2, args.min_neighbours, args.min_component, args.keep_largest)))
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
