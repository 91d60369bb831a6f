"""Clouds rendered into views on the GPU (csrc/render.hip; the definition is tests/render_reference.py): a deterministic
z-buffer splat of the rows into several orthographic views, PNG files of the pictures, and the projection metrics of two renderings (the
PSNR of the views of a decoded cloud against the views of the input, the depth PSNR and the silhouette IoU).  The reference has no renderer.

A view is a 3x4 integer matrix M in Q16: (u, v, d) = (M[:, :3] . (x, y, z) + M[:, 3]) >> 16 (a floor); u counts columns to the right, v rows
downwards, the smallest d is in front.  view_matrices builds the matrices on the host, and that is the only place where floating point
appears: the device and the definition consume the integers.

    faces       the six axis views of the cube [0, 2^bits)^3, FACES = +x -x +y -y +z -z.  A face is named by the direction the camera LOOKS
                along; what it shows is seen from outside the cube, not mirrored.  With L = 2^bits, s = size / L (a power of two) and every
                product floored:
                    +x   u = s (L-1-y)   v = s (L-1-z)   d = s x            -x   u = s y         v = s (L-1-z)   d = s (L-1-x)
                    +y   u = s x         v = s (L-1-z)   d = s y            -y   u = s (L-1-x)   v = s (L-1-z)   d = s (L-1-y)
                    +z   u = s x         v = s y         d = s z            -z   u = s (L-1-x)   v = s y         d = s (L-1-z)
                (z points up in the four side views; with size == L pixel (u, v) of +z is the column (x, y) of the lattice)
    yaw,pitch   degrees: an oblique orthographic view about the cube centre c = (L-1)/2.  right = (cos yaw, sin yaw, 0), forward = (-sin yaw
                cos pitch, cos yaw cos pitch, -sin pitch), up = right x forward (0,0 is +y; a positive pitch looks down); u = W/2 + k right .
                (p-c), v = H/2 - k up . (p-c), d = k forward . (p-c) (negative in front of the centre); k fits the cube's bounding sphere
                into the image less the margin the Q16 rounding can move a corner by
    turntable:N N such views at yaw = 360 k / N, pitch TURNTABLE_PITCH
A view list is any of these joined by ';' (or a list of such strings), for instance 'faces;30,20'.

    python -m pcgcv2_amd.render --filedir cloud.ply [--against ref.ply] [--views faces|turntable:N|yaw,pitch;...] [--bits B] [--size S]
                                [--point_size P] [--out prefix] [--sheet]
"""
import math
import os
import struct
import zlib

import numpy as np

FACES = ('+x', '-x', '+y', '-y', '+z', '-z')
# face -> (axis, flipped) of u, v, d: flipped is L - 1 - coordinate
_FACE_AXES = {'+x': ((1, True), (2, True), (0, False)), '-x': ((1, False), (2, True), (0, True)),
              '+y': ((0, False), (2, True), (1, False)), '-y': ((0, True), (2, True), (1, True)),
              '+z': ((0, False), (1, False), (2, False)), '-z': ((0, True), (1, False), (2, True))}
TURNTABLE_PITCH = 15.0
MAX_SLICES, MAX_SIDE, MAX_POINT_SIZE, COORD_BITS = 64, 4096, 9, 21          # (ops.RENDER_*: restated so this part imports without the library)
MAX_ENTRY, MAX_TRANSLATION = 1 << 20, 1 << 60
SHADE_SPAN = 200                                                            # the depth shade: 255 at the near plane, 55 at the far plane
DEPTH_DIFF_LIMIT = 1 << 19
SUMS = ('union', 'intersection', 'sse_r', 'sse_g', 'sse_b', 'sse_y', 'sse_depth', 'depth_out_of_range')
FIGURES = ('psnr_y', 'psnr_r', 'psnr_g', 'psnr_b', 'depth_psnr', 'iou')


# ------------------------------------------------------------------------------------------------ views (host only)
def parse_views(views):
    """'faces', 'turntable:N', a face name, 'yaw,pitch', joined by ';', or a list of such -> [('face', name) | ('oblique', yaw, pitch)]"""
    if isinstance(views, str):
        tokens = [t.strip() for t in views.split(';')]
    else:
        tokens = []
        for v in views:
            if isinstance(v, str):
                tokens += [t.strip() for t in v.split(';')]
            elif isinstance(v, (tuple, list)) and len(v) == 2:
                tokens.append(f'{float(v[0])!r},{float(v[1])!r}')
            else:
                raise ValueError(f'views: {v!r} is neither a string nor a (yaw, pitch) pair')
    out = []
    for t in tokens:
        if t == 'faces':
            out += [('face', f) for f in FACES]
        elif t in FACES:
            out.append(('face', t))
        elif t.startswith('turntable:'):
            try:
                n = int(t[len('turntable:'):])
            except ValueError:
                n = 0
            if not 1 <= n <= MAX_SLICES:
                raise ValueError(f'views: {t!r}: turntable:N with N in 1 .. {MAX_SLICES}')
            out += [('oblique', 360.0 * k / n, TURNTABLE_PITCH) for k in range(n)]
        else:
            try:
                yaw, pitch = (float(v) for v in t.split(','))
            except ValueError:
                raise ValueError(f"views: {t!r} is none of 'faces', a face ({' '.join(FACES)}), 'turntable:N' and 'yaw,pitch'") from None
            if not (math.isfinite(yaw) and -90.0 <= pitch <= 90.0):
                raise ValueError(f'views: {t!r}: a finite yaw and a pitch in -90 .. 90 degrees')
            out.append(('oblique', yaw, pitch))
    if not 1 <= len(out) <= MAX_SLICES:
        raise ValueError(f'views: {len(out)} views; 1 .. {MAX_SLICES}')
    return out


def _shape(size):
    """size: S or (H, W) -> (H, W)"""
    hw = (size, size) if isinstance(size, (int, np.integer)) and not isinstance(size, bool) else tuple(size)
    if len(hw) != 2 or not all(isinstance(v, (int, np.integer)) and 1 <= v <= MAX_SIDE for v in hw):
        raise ValueError(f'size {size!r}: S or (H, W) with each side in 1 .. {MAX_SIDE}')
    return int(hw[0]), int(hw[1])


def _q16(v):
    return int(round(v * 65536.0))


def view_matrices(views, bits, size):
    """The Q16 matrices of a view list (module doc) for the cube [0, 2^bits)^3 and an image of `size` = S or (H, W) pixels -> int64 [V,3,4],
    range-checked (check_matrices).  A face view scales by min(H, W) / 2^bits, which must be a power of two of at least 2^-16, and is
    centred in the longer side."""
    if isinstance(bits, bool) or not isinstance(bits, (int, np.integer)) or not 1 <= bits <= COORD_BITS:
        raise ValueError(f'bits {bits!r}: an integer in 1 .. {COORD_BITS}')
    H, W = _shape(size)
    L, S = 1 << int(bits), min(H, W)
    out = []
    for spec in parse_views(views):
        M = np.zeros((3, 4), np.int64)
        if spec[0] == 'face':
            if S & (S - 1) or (S << 16) % L:
                raise ValueError(f'face views: the shorter side {S} over 2^{bits} must be a power of two of at least 2^-16')
            s16 = (S << 16) // L
            for row, ((axis, flipped), off) in enumerate(zip(_FACE_AXES[spec[1]], ((W - S) // 2, (H - S) // 2, 0))):
                M[row, axis] = -s16 if flipped else s16
                M[row, 3] = (s16 * (L - 1) if flipped else 0) + (off << 16)
        else:
            yaw, pitch = math.radians(spec[1]), math.radians(spec[2])
            right = np.array([math.cos(yaw), math.sin(yaw), 0.0])
            forward = np.array([-math.sin(yaw) * math.cos(pitch), math.cos(yaw) * math.cos(pitch), -math.sin(pitch)])
            up = np.cross(right, forward)
            margin = 0.5 + 3.0 * L / 131072.0                                   # half a pixel, and three entries off by 2^-17 each
            k = (S / 2.0 - margin) / (math.sqrt(3.0) / 2.0 * L)
            if k * 65536.0 < 1.0:
                raise ValueError(f'oblique views: a {H} x {W} image is too small for 2^{bits} in Q16 (the scale rounds to nothing)')
            c = (L - 1) / 2.0
            for row, (axis_vec, centre) in enumerate(((right, W / 2.0), (-up, H / 2.0), (forward, 0.0))):
                M[row, :3] = [_q16(k * a) for a in axis_vec]
                M[row, 3] = _q16(centre - k * c * float(axis_vec.sum()))
        out.append(M)
    out = np.stack(out)
    check_matrices(out)
    return out


def _extremes(row, top):
    """the least and the largest value of row[:3] . p + row[3] over p in [0, top]^3 (Python integers)"""
    lo = hi = int(row[3])
    for m in row[:3]:
        lo, hi = lo + min(0, int(m)) * top, hi + max(0, int(m)) * top
    return lo, hi


def check_matrices(matrices):
    """ValueError unless matrices is int64 [V,3,4] with 1 <= V <= 64, |3x3 entries| <= 2^20, |translations| <= 2^60 and d inside int32 for
    every coordinate in [0, 2^21): what the kernel's 64-bit products and its 32-bit depth field need"""
    M = np.asarray(matrices)
    if M.dtype != np.int64 or M.ndim != 3 or M.shape[1:] != (3, 4) or not 1 <= M.shape[0] <= MAX_SLICES:
        raise ValueError(f'matrices must be int64 [V,3,4] with V in 1 .. {MAX_SLICES}, got {M.dtype} {M.shape}')
    for k, m in enumerate(M):
        if max(abs(int(v)) for v in m[:, :3].ravel()) > MAX_ENTRY:
            raise ValueError(f'view {k}: an entry of the 3x3 part exceeds 2^20 in magnitude')
        if max(abs(int(v)) for v in m[:, 3]) > MAX_TRANSLATION:
            raise ValueError(f'view {k}: a translation exceeds 2^60 in magnitude')
        lo, hi = _extremes(m[2], (1 << COORD_BITS) - 1)
        if (lo >> 16) < -(1 << 31) or (hi >> 16) > (1 << 31) - 1:
            raise ValueError(f'view {k}: d leaves int32 for coordinates in [0, 2^{COORD_BITS}) ({lo >> 16} .. {hi >> 16})')


def depth_planes(matrices, bits):
    """near, far of the depth shade: the least and the largest d over the cube [0, 2^bits)^3 -> int32 [V,2].  The shade of a pixel is the
    grey level 255 - (200 * clamp(d - near, 0, span)) // span, span = max(far - near, 1)"""
    top = (1 << int(bits)) - 1
    return np.array([[v >> 16 for v in _extremes(m[2], top)] for m in np.asarray(matrices)], np.int32).reshape(-1, 2)


# ------------------------------------------------------------------------------------------------ rendering (device)
def render(coords, colours=None, views='faces', size=None, bits=None, point_size=1, background=(255, 255, 255), batch_items=None, times=None):
    """coords int32 [N,4] (batch, x, y, z) device tensor (rows in any order, repeats allowed), colours uint8 [N,3] or None (the depth shade)
    -> ops.Rendered(image uint8 [B,V,H,W,3], depth int32 [B,V,H,W], index int32 (the row a pixel shows, -1: background), mask bool,
    matrices int64 [V,3,4]), every tensor on the device.  views: a view list (module doc) or int64 [V,3,4] matrices used as they are (those
    of another rendering, to compare with it); bits: the cube is [0, 2^bits)^3, default the smallest that holds the largest coordinate;
    size: S or (H, W), default 2^bits, at most 4096; point_size: 1, 3, .. 9 pixels; batch_items: B, default the largest batch index + 1."""
    import torch
    from . import ops
    if not torch.is_tensor(coords) or not coords.is_cuda:
        raise ops.PcgcError('render: coords must be a ROCm device tensor (no CPU fallback exists)')
    if coords.dtype != torch.int32 or coords.dim() != 2 or coords.shape[1] != 4:
        raise ValueError(f'render: coords must be int32 [N,4], got {coords.dtype} {tuple(coords.shape)}')
    if isinstance(point_size, bool) or not isinstance(point_size, (int, np.integer)) or not 1 <= point_size <= MAX_POINT_SIZE or point_size % 2 == 0:
        raise ValueError(f'render: point_size {point_size!r}: an odd integer in 1 .. {MAX_POINT_SIZE}')
    n = coords.shape[0]
    if (bits is None or batch_items is None) and n:
        top = coords.max(0).values.cpu().tolist()
    if batch_items is None:
        batch_items = top[0] + 1 if n else 1
    if bits is None:
        bits = max(1, int(max(top[1:])).bit_length()) if n else 1
    if size is None:
        size = min(1 << bits, MAX_SIDE)
    H, W = _shape(size)
    if isinstance(views, np.ndarray) or torch.is_tensor(views):
        matrices = np.ascontiguousarray(views.cpu().numpy() if torch.is_tensor(views) else views)
        check_matrices(matrices)
    else:
        matrices = view_matrices(views, bits, (H, W))
    return ops.render(coords, colours, matrices, depth_planes(matrices, bits), batch_items, H, W, (int(point_size) - 1) // 2, background, times=times)


def _psnr(peak, count, sse):
    return math.inf if sse == 0 else 10.0 * math.log10(peak * peak * count / sse)


def figures(sums, width):
    """one row of the integer sums SUMS -> {psnr_y, psnr_r, psnr_g, psnr_b (peak 255, the mean over the union of the masks), depth_psnr
    (peak = the image width, the mean over their intersection), iou}; an SSE of 0 gives inf, an empty union the IoU 1"""
    s = dict(zip(SUMS, (int(v) for v in sums)))
    out = {f'psnr_{c}': _psnr(255.0, s['union'], s[f'sse_{c}']) for c in 'yrgb'}
    out['depth_psnr'] = _psnr(float(width), s['intersection'], s['sse_depth'])
    out['iou'] = s['intersection'] / s['union'] if s['union'] else 1.0
    return out


def metric_from_sums(sums, width):
    """int64 [B,V,8] sums -> {'sums': them, each of FIGURES: float64 [B,V], 'mean': the FIGURES of the sums added up over items and views}"""
    sums = np.asarray(sums, np.int64)
    if int(sums[..., 7].sum()):
        raise ValueError(f'view_metric: {int(sums[..., 7].sum())} pixels differ in depth by 2^19 or more: the depth SSE is not defined for them')
    per = [[figures(s, width) for s in item] for item in sums]
    out = {'sums': sums, 'mean': figures(sums.reshape(-1, len(SUMS)).sum(0), width)}
    for f in FIGURES:
        out[f] = np.array([[p[f] for p in item] for item in per], np.float64).reshape(sums.shape[:2])
    return out


def view_metric(a, b):
    """two renderings of the same views (equal matrices and shapes) -> metric_from_sums of the device's integer sums: per (item, view) and
    'mean' values of psnr_y, psnr_r, psnr_g, psnr_b, depth_psnr and iou, and 'sums', the raw integers"""
    import torch
    from . import ops
    if a.matrices.shape != b.matrices.shape or not torch.equal(a.matrices, b.matrices):
        raise ValueError('view_metric: the two renderings have different view matrices')
    return metric_from_sums(ops.render_metric(a, b).cpu().numpy(), a.depth.shape[3])


def describe(name, f):
    """one metric line of the tools"""
    return (f'{name}:\t Y {f["psnr_y"]:.4f} dB  R {f["psnr_r"]:.4f} dB  G {f["psnr_g"]:.4f} dB  B {f["psnr_b"]:.4f} dB  '
            f'depth {f["depth_psnr"]:.4f} dB  IoU {f["iou"]:.6f}')


# ------------------------------------------------------------------------------------------------ pictures (host only)
def _chunk(kind, data):
    return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data) & 0xFFFFFFFF)


def png_bytes(image):
    """uint8 [H,W,3] (numpy array or tensor) -> the bytes of an 8-bit RGB PNG: IHDR, one IDAT (filter 0 on every row), IEND"""
    a = image.cpu().numpy() if hasattr(image, 'cpu') else np.asarray(image)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f'write_png: the image must be uint8 [H,W,3], got {a.dtype} {a.shape}')
    H, W = a.shape[:2]
    rows = np.zeros((H, 1 + 3 * W), np.uint8)
    rows[:, 1:] = a.reshape(H, 3 * W)
    return (b'\x89PNG\r\n\x1a\n' + _chunk(b'IHDR', struct.pack('>IIBBBBB', W, H, 8, 2, 0, 0, 0)) + _chunk(b'IDAT', zlib.compress(rows.tobytes(), 6))
            + _chunk(b'IEND', b''))


def write_png(path, image):
    with open(path, 'wb') as f:
        f.write(png_bytes(image))


def sheet(rendered, item=0, background=(255, 255, 255)):
    """the views of one batch item tiled into one picture, row by row, ceil(sqrt(V)) to a row -> uint8 [rows H, columns W, 3] (numpy)"""
    images = rendered.image[item].cpu().numpy()
    V, H, W = images.shape[:3]
    cols = int(math.ceil(math.sqrt(V)))
    rows = (V + cols - 1) // cols
    out = np.empty((rows * H, cols * W, 3), np.uint8)
    out[:] = np.asarray(background, np.uint8)
    for k in range(V):
        out[k // cols * H:(k // cols + 1) * H, k % cols * W:(k % cols + 1) * W] = images[k]
    return out


def write_views(prefix, rendered, as_sheet=False, item=0, background=(255, 255, 255)):
    """`<prefix>_view<k>.png` for every view of the item, or `<prefix>_sheet.png` -> the paths"""
    if as_sheet:
        write_png(prefix + '_sheet.png', sheet(rendered, item, background))
        return [prefix + '_sheet.png']
    images = rendered.image[item].cpu().numpy()
    paths = [f'{prefix}_view{k}.png' for k in range(len(images))]
    for path, image in zip(paths, images):
        write_png(path, image)
    return paths


# ------------------------------------------------------------------------------------------------ files
def bits_for(*clouds):
    """the smallest bit depth whose cube holds the largest coordinate of the clouds (float [n,3] arrays)"""
    top = max([int(c.max()) for c in clouds if len(c)] + [0])
    return max(1, top.bit_length())


def render_pair(xyz_a, rgb_a, xyz_b, rgb_b, views='faces', size=None, bits=None, point_size=1, background=(255, 255, 255), device=None):
    """two clouds as the PLY readers give them, rendered with the same matrices; colours are used when both have them -> (a, b, metric)"""
    import torch
    from .pc_error import lattice_coords
    from .sparse import require_gpu
    device = torch.device('cuda') if device is None else device
    require_gpu(device)
    bits = bits_for(xyz_a, xyz_b) if bits is None else bits
    coloured = rgb_a is not None and rgb_b is not None
    up = lambda rgb: torch.from_numpy(rgb).to(device) if coloured else None
    a = render(lattice_coords(xyz_a, device), up(rgb_a), views, size, bits, point_size, background, batch_items=1)
    b = render(lattice_coords(xyz_b, device), up(rgb_b), a.matrices, a.depth.shape[2:], bits, point_size, background, batch_items=1)
    return a, b, view_metric(a, b)


def after_coding(filedir, decoded, prefix, views):
    """`--render [VIEWS]` of coder.py: the input file and the decoded file rendered with the same matrices into `<prefix>_in_view<k>.png`
    and `<prefix>_dec_view<k>.png` (colours when both files carry them, else the depth shade), and the three lines of the mean figures"""
    from .data_utils import read_ply_with_colours
    a, b, m = render_pair(*read_ply_with_colours(filedir), *read_ply_with_colours(decoded), views=views)
    write_views(prefix + '_in', a)
    write_views(prefix + '_dec', b)
    print('View PSNR (Y):\t', m['mean']['psnr_y'])
    print('View depth PSNR:\t', m['mean']['depth_psnr'])
    print('View IoU:\t', m['mean']['iou'])
    return m


# ------------------------------------------------------------------------------------------------ CLI
def views_argument(text):
    """argparse type of a view list: the text, checked"""
    import argparse
    try:
        parse_views(text)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e)) from None
    return text


def parser():
    import argparse
    p = argparse.ArgumentParser(description='render a voxelised PLY into views on the GPU; with --against, the projection metrics of the pair',
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('--filedir', required=True, help='input PLY: integer coordinates, with or without red green blue')
    p.add_argument('--against', default=None, help='a second PLY rendered with the same matrices: one metric line per view and one for the mean')
    p.add_argument('--views', type=views_argument, default='faces', help="'faces', 'turntable:N', a face (+x .. -z) or 'yaw,pitch' in degrees, joined by ';'")
    p.add_argument('--bits', type=int, default=None, help='the cube is [0, 2^bits)^3 (default: the smallest that holds both files)')
    p.add_argument('--size', type=int, default=None, help='pixels per side, 1 .. 4096 (default: 2^bits, at most 4096)')
    p.add_argument('--point_size', type=int, default=1, help='pixels a point covers per side: 1, 3, 5, 7 or 9')
    p.add_argument('--out', default=None, help='prefix of the PNG files (default: the input name without its extension)')
    p.add_argument('--sheet', action='store_true', help='one picture of all views, <prefix>_sheet.png, instead of <prefix>_view<k>.png')
    return p


def parse_args(argv=None):
    p = parser()
    args = p.parse_args(argv)
    if args.bits is not None and not 1 <= args.bits <= COORD_BITS:
        p.error(f'--bits {args.bits}: 1 .. {COORD_BITS}')
    if args.size is not None and not 1 <= args.size <= MAX_SIDE:
        p.error(f'--size {args.size}: 1 .. {MAX_SIDE}')
    if not 1 <= args.point_size <= MAX_POINT_SIZE or args.point_size % 2 == 0:
        p.error(f'--point_size {args.point_size}: 1, 3, 5, 7 or 9')
    return args


def main(argv=None):
    import torch
    from .data_utils import read_ply_with_colours
    from .pc_error import lattice_coords
    from .sparse import require_gpu
    args = parse_args(argv)
    prefix = args.out or os.path.splitext(args.filedir)[0]
    xyz, rgb = read_ply_with_colours(args.filedir)
    if args.against is None:
        device = torch.device('cuda')
        require_gpu(device)
        bits = bits_for(xyz) if args.bits is None else args.bits
        a = render(lattice_coords(xyz, device), None if rgb is None else torch.from_numpy(rgb).to(device), args.views, args.size, bits,
                   args.point_size, batch_items=1)
        for path in write_views(prefix, a, args.sheet):
            print(path)
        return 0
    xyz_b, rgb_b = read_ply_with_colours(args.against)
    a, b, m = render_pair(xyz, rgb, xyz_b, rgb_b, args.views, args.size, args.bits, args.point_size)
    for path in write_views(prefix, a, args.sheet) + write_views(prefix + '_against', b, args.sheet):
        print(path)
    for k in range(a.depth.shape[1]):
        print(describe(f'view {k}', {f: m[f][0, k] for f in FIGURES}))
    print(describe('mean', m['mean']))
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
