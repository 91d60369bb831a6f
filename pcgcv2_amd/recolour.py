"""Carry the colours of one cloud onto the geometry of another on the GPU:

    python -m pcgcv2_amd.recolour --source src.ply --target dec.ply --out dec_rgb.ply [--metric]

Every point of the target takes the mean, rounded half up, of the colours of the source points that have it as a nearest neighbour (all of
them at the nearest distance, up to 30); a target no source point chose takes that of its own nearest source points (pc_error.recolour_device,
DESIGN.md 8f).  --metric prints the colour distortion of the pair as `pc_error_d -c 1` reports it (pc_error.colour_psnr_device): the two
nearest-neighbour searches are shared."""
import torch

from .data_utils import read_ply_ascii_with_colours, write_ply_ascii_geo_rgb
from .pc_error import colour_psnr_device, lattice_coords, nn_both, recolour_device


def recolour_file(source, target, out, metric=False):
    """-> the colour columns (dict) with metric=True, else None"""
    xyz, rgb = read_ply_ascii_with_colours(source)
    if rgb is None:
        raise ValueError(f'{source} has no colours (red green blue)')
    t_xyz, _ = read_ply_ascii_with_colours(target)
    device = torch.device('cuda')
    a, b, ca = lattice_coords(xyz, device), lattice_coords(t_xyz, device), torch.from_numpy(rgb).to(device)
    nn = nn_both(a, b)
    cb = recolour_device(a, ca, b, nn=nn)
    write_ply_ascii_geo_rgb(out, t_xyz, cb.cpu().numpy())
    return colour_psnr_device(a, ca, b, cb, nn=nn) if metric else None


def main(argv=None):
    import argparse
    p = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    p.add_argument('--source', required=True, help='ASCII PLY with x y z and red green blue')
    p.add_argument('--target', required=True, help='ASCII PLY whose points receive the colours')
    p.add_argument('--out', required=True, help='the target with colours')
    p.add_argument('--metric', action='store_true', help='print the colour distortion between source and recoloured target')
    args = p.parse_args(argv)
    m = recolour_file(args.source, args.target, args.out, metric=args.metric)
    print('wrote', args.out)
    if m is not None:
        for k, name in enumerate('YUV'):
            print(f'Colour PSNR ({name}):\t', m[f'c[{k}],PSNRF'])
        print('Colour h.PSNR (R G B):\t', *[m[f'h.c[{k}],PSNRF'] for k in range(3)])
    return m


if __name__ == '__main__':
    main()
