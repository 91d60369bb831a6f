"""Rate-distortion sweep (the role of the reference's `test.py`): one cloud through a list of checkpoints, one CSV row per
rate, files namespaced by the per-rate postfix `_r{i}` (test.py:38).  `test(...)` keeps the reference's signature and CSV
column names; `sweep(...)` is the underlying generator.

What differs in execution: the input tensor — and its optional down-scaled version — is built once, and because the
encoder's geometry pyramid and kernel maps depend only on the coordinates they are built by the first rate and reused by
all others (they are cached on the tensor's coordinate levels).  D2 (point-to-plane) columns need normals in the
input PLY (as the reference's `pc_error(..., normal=True)` does) and are computed natively when no `pc_error_d` binary is installed.  Checkpoints may be paths or in-memory state dicts.

metric='host' (the default) computes D1 / D2 like the reference: pc_error() on the input PLY and the decoded PLY.  metric='device' computes
the same columns on the GPU (pc_error.d2_psnr_device, or d1_psnr_device for a cloud without normals): the input's raw rows and normals are
read and uploaded once, the decoded cloud is taken from the decoder's tensor directly (its PLY is still written), no pc_error_d is run.

estimate_normals=R2 (`--estimate_normals [R2]`, off by default; metric='device' only): a cloud WITHOUT normals gets the D2 columns too, from
normals estimated on the GPU over neighbourhoods of squared radius R2 (pc_error.estimate_normals_device).  Two more columns say which normals
a row used: `normals` ('file' or 'estimated') and `normals_r2`.  D2 from estimated normals compares across our own rates and runs, not with
published figures computed from a dataset's own normals.  The host metric has no estimator: it raises for such a cloud.

colour=True (`--colour`, off by default): the input's colours (red green blue) are carried onto every decoded cloud (pc_error.recolour_device
with metric='device', sharing the two nearest-neighbour searches with D2; pc_error.recolour with metric='host'), `_dec.ply` is written with
them, and the row gains the 36 colour columns of `pc_error_d -c 1` (pc_error.COLOUR_COLUMNS) — the colour distortion the geometry loss
induces.  The columns are the same both ways.  An input without colours raises ValueError.

views=VIEWS (`--views [VIEWS]`, off by default; metric='device' only): the projection metrics of render.py.  The input is
rendered once into the views ('faces', 'turntable:N', 'yaw,pitch;...') of the cube [0, 2^ceil(log2 res))^3, every decoded cloud is rendered
with the same matrices, and the row gains `view_depth_psnr` and `view_iou` and, with colour=True, `view_psnr_y` (the pictures then show the
carried colours, else the depth shade): the figures of all views' sums added up."""
import os
import time

import numpy as np
import pandas as pd
import torch

from .coder import Coder, stream_bits
from .data_utils import (load_sparse_tensor, ply_has_colours, read_ply_ascii_with_colours, scale_sparse_tensor, write_ply_ascii_geo,
                         write_ply_ascii_geo_rgb)
from .pc_error import (COLOUR_COLUMNS, D1_COLUMNS, colour_psnr_device, d1_psnr_device, d2_psnr_device, lattice_coords, nn_both, pc_error,
                       ply_has_normals, read_ply_ascii_with_normals, recolour, recolour_device)
from .pcc_model import PCCModel

device = torch.device('cuda' if torch.cuda.is_available() else 'cpu')

REFERENCE_CKPTS = ['./ckpts/r1_0.025bpp.pth', './ckpts/r2_0.05bpp.pth', './ckpts/r3_0.10bpp.pth', './ckpts/r4_0.15bpp.pth',
                   './ckpts/r5_0.25bpp.pth', './ckpts/r6_0.3bpp.pth', './ckpts/r7_0.4bpp.pth']


def _state_dict(ckpt):
    if isinstance(ckpt, (str, os.PathLike)):
        if not os.path.exists(ckpt):
            raise FileNotFoundError(ckpt)
        return torch.load(ckpt, map_location=device)['model']
    return ckpt


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.time()
    out = fn()
    torch.cuda.synchronize()
    return out, round(time.time() - t0, 3)


def sweep(filedir, ckpts, outdir, scaling_factor=1.0, rho=1.0, res=1024, metric='host', estimate_normals=None, colour=False, views=None):
    """Yield one single-row DataFrame per checkpoint (columns as in the reference's results/*.csv).  metric: 'host' or 'device',
    estimate_normals: None or the squared radius R2, colour: carry the input's colours and report their distortion, views: None or the view
    list of the projection metrics (module doc)."""
    if metric not in ('host', 'device'):
        raise ValueError(f"metric must be 'host' or 'device', got {metric!r}")
    if views is not None and metric != 'device':
        raise ValueError("views (the projection metrics) are rendered on the GPU: use metric='device'")
    if colour and not ply_has_colours(filedir):
        raise ValueError(f'{filedir} has no colours (red green blue): colour=True needs them')
    estimated = estimate_normals is not None and not ply_has_normals(filedir)
    if estimated and metric != 'device':
        raise ValueError(f"{filedir} has no normals (nx ny nz) and the host metric cannot estimate them: use metric='device'")
    x = load_sparse_tensor(filedir, device)
    os.makedirs(outdir, exist_ok=True)
    prefix = os.path.join(outdir, os.path.split(filedir)[-1].split('.')[0])
    x_in = scale_sparse_tensor(x, factor=scaling_factor) if scaling_factor != 1 else x
    model = PCCModel().to(device)
    with_normals = ply_has_normals(filedir)       # (test.py:74-75 always asks for D2: its test clouds carry normals; a cloud without them gets D1 only)
    if metric == 'device':                        # the file's rows as the host metric reads them (not the deduplicated x), uploaded once
        a_xyz, a_nrm = read_ply_ascii_with_normals(filedir)
        a_dev = lattice_coords(a_xyz, device)
        na_dev = torch.from_numpy(a_nrm).to(device) if with_normals else None
    if colour:                                    # the raw rows again, with their colours (duplicates included, as the metric reads them)
        c_xyz, c_rgb = read_ply_ascii_with_colours(filedir)
        ca_dev = torch.from_numpy(c_rgb).to(device) if metric == 'device' else None
    if views is not None:                         # the input's pictures, once; every rate is rendered with their matrices
        from . import render
        view_bits = max(1, (int(res) - 1).bit_length())
        view_in = render.render(a_dev, ca_dev if colour else None, views, bits=view_bits, batch_items=1)
    for rate, ckpt in enumerate(ckpts, start=1):
        model.load_state_dict(_state_dict(ckpt))
        coder = Coder(model=model, filename=prefix)
        tag = f'_r{rate}'
        _, t_enc = _timed(lambda: coder.encode(x_in, postfix=tag))
        x_dec, t_dec = _timed(lambda: coder.decode(postfix=tag, rho=rho))
        if scaling_factor != 1:
            x_dec = scale_sparse_tensor(x_dec, factor=1.0 / scaling_factor)
        bits = stream_bits(prefix, tag)
        bpps = (bits / len(x)).round(3)
        dec_ply = prefix + tag + '_dec.ply'
        dec_xyz = x_dec.C.detach().cpu().numpy()[:, 1:]
        if not colour:
            write_ply_ascii_geo(dec_ply, dec_xyz)
        if metric == 'device':
            b_dev = x_dec.C.detach().contiguous()
            nn = nn_both(a_dev, b_dev) if colour else None          # both searches once: D2, the recolouring and the colour metric read them
            if estimated:
                m = d2_psnr_device(a_dev, {'r2': estimate_normals}, b_dev, res, nn=nn)
                row = pd.DataFrame([{k: m[k] for k in m if k not in ('normals_r2', 'normals_invalid')}])
            else:
                m = d2_psnr_device(a_dev, na_dev, b_dev, res, nn=nn) if with_normals else d1_psnr_device(a_dev, b_dev, res)
                row = pd.DataFrame([{k: m[k] for k in (m if with_normals else D1_COLUMNS)}])
            if colour:
                cb_dev = recolour_device(a_dev, ca_dev, b_dev, nn=nn)
                write_ply_ascii_geo_rgb(dec_ply, dec_xyz, cb_dev.cpu().numpy())
                mc = colour_psnr_device(a_dev, ca_dev, b_dev, cb_dev, nn=nn)
                for k in COLOUR_COLUMNS:
                    row[k] = mc[k]
            if views is not None:
                view_dec = render.render(b_dev, cb_dev if colour else None, view_in.matrices, view_in.depth.shape[2:], view_bits, batch_items=1)
                mv = render.view_metric(view_in, view_dec)['mean']
                row['view_depth_psnr'], row['view_iou'] = mv['depth_psnr'], mv['iou']
                if colour:
                    row['view_psnr_y'] = mv['psnr_y']
        else:
            if colour:
                write_ply_ascii_geo_rgb(dec_ply, dec_xyz, recolour(c_xyz, c_rgb, dec_xyz))
            row = pc_error(filedir, dec_ply, res=res, normal=with_normals, show=False, **({'color': True} if colour else {}))
        row["num_points(input)"], row["num_points(output)"], row["resolution"] = len(x), len(x_dec), res
        row["bits"], row["bpp"] = sum(bits).round(3), sum(bpps).round(3)
        row["bpp(coords)"], row["bpp(feats)"] = bpps[0], bpps[1]
        row["time(enc)"], row["time(dec)"] = t_enc, t_dec
        if estimate_normals is not None:
            row["normals"], row["normals_r2"] = ('estimated', int(estimate_normals)) if estimated else ('file', None)
        yield row


def test(filedir, ckptdir_list, outdir, resultdir, scaling_factor=1.0, rho=1.0, res=1024, verbose=True, metric='host', estimate_normals=None,
         colour=False, views=None):
    """Reference entry point (test.py:13): runs the sweep, rewrites `<resultdir>/<cloud>.csv` after every rate.  metric: 'host' | 'device';
    estimate_normals: None | R2; colour: False | True; views: None | a view list (module doc)."""
    os.makedirs(resultdir, exist_ok=True)
    csv_name = os.path.join(resultdir, os.path.split(filedir)[-1].split('.')[0] + '.csv')
    rows, table = [], None
    for rate, row in enumerate(sweep(filedir, ckptdir_list, outdir, scaling_factor, rho, res, metric, estimate_normals, colour, views), start=1):
        rows.append(row)
        table = pd.concat(rows, ignore_index=True)
        table.to_csv(csv_name, index=False)
        if verbose:
            seen = '' if views is None else f'view depth {row["view_depth_psnr"][0]:.4f} dB  view IoU {row["view_iou"][0]:.6f}  ' + \
                (f'view Y {row["view_psnr_y"][0]:.4f} dB  ' if colour else '')
            print(f'[r{rate}] bpp {row["bpp"][0]}  D1 {row["mseF,PSNR (p2point)"][0]:.4f} dB  {seen}enc {row["time(enc)"][0]} s  '
                  f'dec {row["time(dec)"][0]} s  -> {csv_name}')
    return table


def plot_rd(table, title, path):
    """R-D curve like test.py:123-136 (optional: needs matplotlib)."""
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    fig, _ = plt.subplots(figsize=(7, 4))
    curves = [("mseF,PSNR (p2point)", "D1", 'red'), ("mseF,PSNR (p2plane)", "D2", 'blue')]
    for col, label, colour in curves:
        if col in table:
            plt.plot(np.array(table["bpp"]), np.array(table[col]), label=label, marker='x', color=colour)
    plt.title(title); plt.xlabel('bpp'); plt.ylabel('PSNR'); plt.grid(ls='-.'); plt.legend(loc='lower right')
    fig.savefig(path)


def main(argv=None):
    import argparse
    parser = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("--filedir", default='../../../testdata/8iVFB/longdress_vox10_1300.ply')
    parser.add_argument("--outdir", default='./output')
    parser.add_argument("--resultdir", default='./results')
    parser.add_argument("--scaling_factor", type=float, default=1.0, help='scaling_factor')
    parser.add_argument("--res", type=int, default=1024, help='resolution')
    parser.add_argument("--rho", type=float, default=1.0, help='the ratio of the number of output points to the number of input points')
    parser.add_argument("--ckpts", nargs='*', default=REFERENCE_CKPTS)
    parser.add_argument("--metric", choices=('host', 'device'), default='host',
                        help='where D1 / D2 are computed: host (pc_error on the PLY files, as the reference) or device (GPU)')
    parser.add_argument("--estimate_normals", nargs='?', type=int, const=16, default=None, metavar='R2',
                        help='with --metric device: D2 for a cloud without normals, from normals estimated on the GPU over neighbourhoods '
                             'of squared radius R2 (1 .. 64, 16 when no value is given)')
    parser.add_argument("--colour", action='store_true',
                        help='carry the colours of the input onto every decoded cloud (written into _dec.ply) and report their distortion')
    from . import render
    parser.add_argument("--views", metavar='VIEWS', nargs='?', type=render.views_argument, const='faces', default=None,
                        help="with --metric device: the projection metrics (render.py) over these views ('faces', 'turntable:N' or "
                             "'yaw,pitch;...'): the columns view_depth_psnr and view_iou and, with --colour, view_psnr_y")
    args = parser.parse_args(argv)
    if args.views is not None and args.metric != 'device':
        parser.error('--views needs --metric device')
    table = test(args.filedir, args.ckpts, args.outdir, args.resultdir, scaling_factor=args.scaling_factor, rho=args.rho, res=args.res,
                 metric=args.metric, estimate_normals=args.estimate_normals, colour=args.colour, views=args.views)
    name = os.path.split(args.filedir)[-1][:-4]
    try:
        plot_rd(table, name, os.path.join(args.resultdir, name + '.jpg'))
    except ImportError:
        pass


if __name__ == '__main__':
    main()
