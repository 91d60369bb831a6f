"""D1 (point-to-point) and D2 (point-to-plane) geometry distortion (reference pc_error.py:27-74 -> external mpeg-pcc-dmetric 0.13.4 binary).

`pc_error(infile1, infile2, res)` keeps the reference's signature and DataFrame column names.  If a `pc_error_d`
executable is installed (env PCGC_PC_ERROR or next to this file) it is invoked exactly like the reference does;
otherwise the metric is computed natively (exact nearest neighbours on the integer lattice), pinned to the binary's
output by tests/golden/d1_metric.npz (D1) and tests/golden/d2_metric.npz (D2: the reference's test.py:74-75 asks for it with
`normal=True`; normals come from infile1, as with the binary's `-n infile1`).  The metric sits outside the timed encode/decode path
(coder.py:180-182)."""
import os
import subprocess
import numpy as np
import pandas as pd

rootdir = os.path.split(__file__)[0]


def _exe():
    p = os.environ.get('PCGC_PC_ERROR') or os.path.join(rootdir, 'pc_error_d')
    return p if os.path.isfile(p) and os.access(p, os.X_OK) else None


def number_in_line(line):
    number = None
    for item in line.split(' '):
        try:
            number = float(item)
        except ValueError:
            continue
    return number


D1_COLUMNS = ['mse1      (p2point)', 'mse1,PSNR (p2point)', 'h.       1(p2point)', 'h.,PSNR  1(p2point)',
              'mse2      (p2point)', 'mse2,PSNR (p2point)', 'h.       2(p2point)', 'h.,PSNR  2(p2point)',
              'mseF      (p2point)', 'mseF,PSNR (p2point)', 'h.        (p2point)', 'h.,PSNR   (p2point)']     # what pc_error() reports for D1


def d1_sums(a, b):
    """-> (sum of squared NN distances a->b, max) with an exact KD-tree search (scipy, host)."""
    from scipy.spatial import cKDTree
    d, _ = cKDTree(np.asarray(b, dtype=np.float64)).query(np.asarray(a, dtype=np.float64), workers=-1)
    d2 = np.rint(d * d)                      # integer lattices: squared distances are integers
    return float(d2.sum()), float(d2.max() if len(d2) else 0.0)


def d1_psnr(a, b, res):
    """mseF,PSNR (p2point) = 10*log10(3*peak^2 / max(mse1, mse2)), peak = res-1 (pc_error.py:49)."""
    s1, h1 = d1_sums(a, b)
    s2, h2 = d1_sums(b, a)
    mse1, mse2 = s1 / len(a), s2 / len(b)
    peak = float(res - 1)
    psnr = lambda m: float(10 * np.log10(3 * peak * peak / m)) if m > 0 else float('inf')
    return {'mse1      (p2point)': mse1, 'mse1,PSNR (p2point)': psnr(mse1), 'h.       1(p2point)': h1, 'h.,PSNR  1(p2point)': psnr(h1),
            'mse2      (p2point)': mse2, 'mse2,PSNR (p2point)': psnr(mse2), 'h.       2(p2point)': h2, 'h.,PSNR  2(p2point)': psnr(h2),
            'mseF      (p2point)': max(mse1, mse2), 'mseF,PSNR (p2point)': psnr(max(mse1, mse2)),
            'h.        (p2point)': max(h1, h2), 'h.,PSNR   (p2point)': psnr(max(h1, h2))}


# ---- D2 (point-to-plane), as mpeg-pcc-dmetric 0.13.4 computes it with `-n infile1` (averageNormals on, its default).  Restated from the tool's
# behaviour and pinned to its output (golden G6):
#   * normals of B ("scaleNormals"): every point of A adds its normal to its nearest neighbour(s) in B — ALL neighbours at the nearest distance, up
#     to 30 — and a point of B takes the average of what it received; a point of B that received nothing takes the average normal of its own
#     nearest neighbour(s) in A;
#   * A -> B: for a in A with nearest neighbour(s) b in B (ties as above): c2p(a) = mean over the tied b of ((a - b) . n_b)^2; mse = mean over A,
#     h. = max over A.  B -> A the same with A's own normals.  PSNR = 10 log10(3 peak^2 / mse), peak = res - 1.
_D2_TIES = 30


def _nn_ties(tree, q, chunk=1 << 15):
    """for every query point: indices of its up to 30 nearest neighbours in `tree`, squared distances, and which of them tie with the nearest"""
    k = min(_D2_TIES, tree.n)
    pts = tree.data
    for s in range(0, len(q), chunk):
        qq = q[s:s + chunk]
        _, idx = tree.query(qq, k=k, workers=-1)
        idx = idx.reshape(len(qq), k)
        e = qq[:, None, :] - pts[idx]
        d2 = (e * e).sum(-1)                                     # (exact for lattice points: ties are compared as the tool compares them)
        yield s, idx, e, d2, d2 == d2[:, :1]


def d2_estimate_normals(a, na, b):
    """normals of cloud b from those of cloud a (the tool's scaleNormals)"""
    from scipy.spatial import cKDTree
    a, b, na = np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(na, np.float64)
    acc, cnt = np.zeros((len(b), 3)), np.zeros(len(b), np.int64)
    for s, idx, _, _, same in _nn_ties(cKDTree(b), a):
        rows, cols = np.nonzero(same)
        np.add.at(acc, idx[rows, cols], na[s + rows])
        np.add.at(cnt, idx[rows, cols], 1)
    nb = np.zeros((len(b), 3))
    got = cnt > 0
    nb[got] = acc[got] / cnt[got, None]
    lone = np.nonzero(~got)[0]
    if len(lone):
        for s, idx, _, _, same in _nn_ties(cKDTree(a), b[lone]):
            w = same.astype(np.float64)
            nb[lone[s:s + len(idx)]] = (na[idx] * w[:, :, None]).sum(1) / w.sum(1, keepdims=True)
    return nb


def d2_sums(p, q, nq):
    """p -> q with q's normals: (sum of c2c, max c2c, sum of c2p, max c2p)"""
    from scipy.spatial import cKDTree
    p, q, nq = np.asarray(p, np.float64), np.asarray(q, np.float64), np.asarray(nq, np.float64)
    s_c2c = s_c2p = 0.0
    h_c2c = h_c2p = 0.0
    for _, idx, e, d2, same in _nn_ties(cKDTree(q), p):
        proj = (e * nq[idx]).sum(-1) ** 2
        w = same.astype(np.float64)
        c2p = (proj * w).sum(1) / w.sum(1)
        s_c2c += float(d2[:, 0].sum()); s_c2p += float(c2p.sum())
        h_c2c = max(h_c2c, float(d2[:, 0].max())); h_c2p = max(h_c2p, float(c2p.max()))
    return s_c2c, h_c2c, s_c2p, h_c2p


def d2_psnr(a, na, b, res):
    """every column the reference parses from `pc_error_d -a A -b B -n A` (pc_error.py:37-47): p2point and p2plane, computed on the host"""
    nb = d2_estimate_normals(a, na, b)
    s1, h1, p1, _ = d2_sums(a, b, nb)
    s2, h2, p2, _ = d2_sums(b, a, na)
    mse1, mse2, pl1, pl2 = s1 / len(a), s2 / len(b), p1 / len(a), p2 / len(b)
    peak = float(res - 1)
    psnr = lambda m: float(10 * np.log10(3 * peak * peak / m)) if m > 0 else float('inf')
    return {'mse1      (p2point)': mse1, 'mse1,PSNR (p2point)': psnr(mse1), 'h.       1(p2point)': h1, 'h.,PSNR  1(p2point)': psnr(h1),
            'mse2      (p2point)': mse2, 'mse2,PSNR (p2point)': psnr(mse2), 'h.       2(p2point)': h2, 'h.,PSNR  2(p2point)': psnr(h2),
            'mseF      (p2point)': max(mse1, mse2), 'mseF,PSNR (p2point)': psnr(max(mse1, mse2)),
            'h.        (p2point)': max(h1, h2), 'h.,PSNR   (p2point)': psnr(max(h1, h2)),
            'mse1      (p2plane)': pl1, 'mse1,PSNR (p2plane)': psnr(pl1), 'mse2      (p2plane)': pl2, 'mse2,PSNR (p2plane)': psnr(pl2),
            'mseF      (p2plane)': max(pl1, pl2), 'mseF,PSNR (p2plane)': psnr(max(pl1, pl2))}


def ply_has_normals(path):
    """True iff the ASCII PLY's vertex element declares nx, ny and nz (header scan only)"""
    names = []
    try:
        with open(path, 'rb') as f:
            for line in f:
                t = line.decode('ascii', 'replace').split()
                if t and t[0] == 'property':
                    names.append(t[-1])
                elif t and t[0] == 'end_header':
                    break
    except OSError:
        return False
    return all(c in names for c in ('nx', 'ny', 'nz'))


def read_ply_ascii_with_normals(path):
    """ASCII PLY -> (coordinates float64 [n, 3], normals float64 [n, 3] or None): the vertex properties x y z and, when present, nx ny nz
    (read as the tool reads them: single precision)"""
    names, n, skip = [], 0, 0
    with open(path, 'rb') as f:
        in_vertex = False
        for line in f:
            skip += 1
            t = line.decode('ascii', 'replace').split()
            if not t:
                continue
            if t[0] == 'element':
                in_vertex = t[1] == 'vertex'
                if in_vertex:
                    n = int(t[2])
            elif t[0] == 'property' and in_vertex:
                names.append(t[-1])
            elif t[0] == 'end_header':
                break
    if not all(c in names for c in 'xyz'):
        raise ValueError(f'{path}: no x / y / z vertex properties')
    data = pd.read_csv(path, sep=r'\s+', header=None, skiprows=skip, nrows=n, dtype=np.float64, engine='c').to_numpy()
    xyz = data[:, [names.index(c) for c in 'xyz']]
    if not all(c in names for c in ('nx', 'ny', 'nz')):
        return xyz, None
    nrm = data[:, [names.index(c) for c in ('nx', 'ny', 'nz')]].astype(np.float32).astype(np.float64)
    return xyz, nrm


def d1_psnr_device(a, b, res, radius=12):
    """Same metrics as d1_psnr, computed on the GPU from two device coordinate tensors [N,4] (or sparse tensors' .C):
    exact nearest neighbours by ascending-distance probes of the coordinate hash (pcgc_d1_nn).  Points farther than `radius`
    voxels from the other cloud (never the case for codec outputs) are finished on the host."""
    from . import ops
    out = []
    for p, q in ((a, b), (b, a)):
        s, m, u = ops.d1_nn(p, q, radius)
        s, m, u = float(s.item()), float(m.item()), int(u.item())
        if u:                                               # rare: finish the far points exactly on the host
            pc, qc = p[:, 1:].cpu().numpy(), q[:, 1:].cpu().numpy()
            from scipy.spatial import cKDTree
            d, _ = cKDTree(qc.astype(np.float64)).query(pc.astype(np.float64), workers=-1)
            d2 = np.rint(d * d)
            s, m = float(d2.sum()), float(d2.max())
        out.append((s, m))
    (s1, h1), (s2, h2) = out
    mse1, mse2 = s1 / a.shape[0], s2 / b.shape[0]
    peak = float(res - 1)
    psnr = lambda v: float(10 * np.log10(3 * peak * peak / v)) if v > 0 else float('inf')
    return {'mse1      (p2point)': mse1, 'mse1,PSNR (p2point)': psnr(mse1), 'h.       1(p2point)': h1, 'h.,PSNR  1(p2point)': psnr(h1),
            'mse2      (p2point)': mse2, 'mse2,PSNR (p2point)': psnr(mse2), 'h.       2(p2point)': h2, 'h.,PSNR  2(p2point)': psnr(h2),
            'mseF      (p2point)': max(mse1, mse2), 'mseF,PSNR (p2point)': psnr(max(mse1, mse2)),
            'h.        (p2point)': max(h1, h2), 'h.,PSNR   (p2point)': psnr(max(h1, h2)),
            'sse1': s1, 'sse2': s2}


def lattice_coords(xyz, device, batch=0):
    """float [n,3] coordinates (as read_ply_ascii_with_normals returns them) -> int32 [n,4] (batch, x, y, z) device tensor.  The device
    metrics work on the integer lattice: a non-integer coordinate raises instead of being rounded."""
    import torch
    xyz = np.asarray(xyz, dtype=np.float64)
    if xyz.size and not np.array_equal(xyz, np.rint(xyz)):
        bad = int(np.count_nonzero((xyz != np.rint(xyz)).any(1)))
        raise ValueError(f'{bad} of {len(xyz)} points have non-integer coordinates: the device metric needs voxelised clouds')
    out = np.empty((len(xyz), 4), np.int32)
    out[:, 0] = batch
    out[:, 1:] = xyz
    return torch.from_numpy(out).to(device)


def estimate_normals_device(coords, r2=16, orient='centroid'):
    """Normals of a voxelised cloud estimated on the GPU: coords int32 [N,4] (batch, x, y, z) device tensor (or a sparse tensor), r2 the
    integer squared radius of the neighbourhood (1 .. 64), orient 'centroid' | (x, y, z) viewpoint | None.
    -> (normals float64 [N,3], lam float64 [N,3], count int32 [N], valid bool [N]), see ops.estimate_normals."""
    from . import ops
    return ops.estimate_normals(coords, r2=r2, orient=orient)


def d2_psnr_device(a, na, b, res, nn=None):
    """The columns of d2_psnr, computed on the GPU: a, b int32 [N,4] (batch, x, y, z) device tensors (or sparse tensors' .C), na the normals of
    a ([Na,3], float32 or float64, used as fp64) — or 'estimate' / a dict {'r2': .., 'orient': ..} of estimate_normals_device's options: the
    normals are then estimated on a (ops.estimate_normals, through the index of a that the search builds anyway) and the result gains
    `normals_r2` and `normals_invalid` (rows of a without a valid normal: they enter as (0, 0, 0)).  Such figures compare across our own
    rates and runs, not with published D2 computed from a dataset's own normals.  Neighbours are searched within the same batch index only.
    Every row is a point of its own (duplicated rows are counted and appear in tie sets).  Tie sets: every point of the other cloud at the
    nearest squared distance, at most 30 — when more tie (e.g. 48 lattice points at d2 = 14) the 30 with the LOWEST row indices, as
    oracle/pcgc_oracle.py:d2_metrics keeps them (the host d2_psnr's k = 30 KD-tree query keeps an unspecified subset in that case).  Exact at
    any distance: points the cell tables cannot settle are searched again with a larger table, then exhaustively (ops.d2_nn).
    p2point columns equal d2_psnr's exactly (integer distances); p2plane columns to rounding (sums of the same terms in another order).
    nn = (ops.d2_nn(a, b), ops.d2_nn(b, a)) when the caller has searched already (nn_both): the colour functions read the same tie sets."""
    import torch
    from . import ops
    a, b = (t.C if hasattr(t, 'C') else t for t in (a, b))
    a, b = a.contiguous(), b.contiguous()
    if a.shape[0] == 0 or b.shape[0] == 0:
        raise ValueError('d2_psnr_device: empty point cloud')
    estimate = None
    if isinstance(na, (str, dict)):
        if isinstance(na, str) and na != 'estimate':
            raise ValueError(f"d2_psnr_device: normals are a tensor, 'estimate' or a dict of estimate_normals_device's options, got {na!r}")
        estimate = {'r2': 16, 'orient': 'centroid', **(na if isinstance(na, dict) else {})}
        if set(estimate) != {'r2', 'orient'}:
            raise ValueError(f"d2_psnr_device: unknown normal-estimation options {sorted(set(estimate) - {'r2', 'orient'})}")
    elif na.shape != (a.shape[0], 3):
        raise ValueError(f'd2_psnr_device: normals {tuple(na.shape)} do not match {a.shape[0]} points')
    ops.check_coords(a, 'd2_psnr_device: a'); ops.check_coords(b, 'd2_psnr_device: b')
    ia = ops.D2Index(a) if nn is None or estimate is not None else None
    extra = {}
    if estimate is not None:
        na, _, _, ok = ops.estimate_normals(a, estimate['r2'], estimate['orient'], index=ia)
        extra = {'normals_r2': int(estimate['r2']), 'normals_invalid': a.shape[0] - int(ok.sum().item())}
    na = torch.as_tensor(na).to(device=a.device, dtype=torch.float64).contiguous()
    ab, ba = nn if nn is not None else (ops.d2_nn(a, ops.D2Index(b)), ops.d2_nn(b, ia))
    nb = ops.d2_normals(b.shape[0], ab, na, ba)
    sums = []
    for p, q, nq, nn in ((a, b, nb, ab), (b, a, na, ba)):
        sm, s = ops.d2_reduce(nn[0], ops.d2_c2p(p, q, nq, nn))
        sums.append((sm, s))
    (sm1, p1), (sm2, p2) = [(sm.cpu().tolist(), float(s.item())) for sm, s in sums]
    s1, h1, s2, h2 = float(sm1[0]), float(sm1[1]), float(sm2[0]), float(sm2[1])
    mse1, mse2, pl1, pl2 = s1 / a.shape[0], s2 / b.shape[0], p1 / a.shape[0], p2 / b.shape[0]
    peak = float(res - 1)
    psnr = lambda m: float(10 * np.log10(3 * peak * peak / m)) if m > 0 else float('inf')
    return {'mse1      (p2point)': mse1, 'mse1,PSNR (p2point)': psnr(mse1), 'h.       1(p2point)': h1, 'h.,PSNR  1(p2point)': psnr(h1),
            'mse2      (p2point)': mse2, 'mse2,PSNR (p2point)': psnr(mse2), 'h.       2(p2point)': h2, 'h.,PSNR  2(p2point)': psnr(h2),
            'mseF      (p2point)': max(mse1, mse2), 'mseF,PSNR (p2point)': psnr(max(mse1, mse2)),
            'h.        (p2point)': max(h1, h2), 'h.,PSNR   (p2point)': psnr(max(h1, h2)),
            'mse1      (p2plane)': pl1, 'mse1,PSNR (p2plane)': psnr(pl1), 'mse2      (p2plane)': pl2, 'mse2,PSNR (p2plane)': psnr(pl2),
            'mseF      (p2plane)': max(pl1, pl2), 'mseF,PSNR (p2plane)': psnr(max(pl1, pl2)), **extra}

# ---- Colours: carrying them onto another geometry, and the colour distortion `pc_error_d -c 1` prints.  Tie sets as above (every
# row of the other cloud at the nearest squared distance, at most 30, the 30 LOWEST rows when more tie: here the host functions keep exactly
# those, so host and device agree on every input).
#   * recolour: a target takes the mean, rounded half up, of the colours of the sources whose tie set holds it; a target no source chose takes
#     that of its own tie set among the sources (scaleNormals' rule, on integers);
#   * distortion A -> B: each a against round_half_up(mean colour of its tie set in B); c[k] = mean over A of the squared difference of BT.709
#     Y, U, V on [0, 1], h.c[k] = max over A of the squared difference of R, G, B in 8-bit units.
# Everything is integer arithmetic until the last division: the YUV matrix times 10^4 is integral, so a squared difference is an integer over
# (255 * 10^4)^2, the sums are exact, and host and device produce the same doubles.
COLOUR_COLUMNS = [f'{h}c[{k}],{w}{d}' for d in '12F' for h, w in (('', '    '), ('', 'PSNR'), ('h.', '    '), ('h.', 'PSNR')) for k in range(3)]
_YUV_1E4 = np.array([[2126, 7152, 722], [-1146, -3854, 5000], [5000, -4542, -458]], np.int64)       # BT.709, times 10^4
_YUV_DEN = (255 * 10 ** 4) ** 2


def _tie_sets(pts, q, chunk=1 << 15):
    """for every row of q (float64 [m,3]): the rows of pts at its nearest squared distance, ascending, at most 30 (the lowest).
    yields (first row of the chunk, idx [m,w], same bool [m,w]): same marks the columns of idx that belong to the tie set"""
    from scipy.spatial import cKDTree
    tree = cKDTree(pts)
    k = min(_D2_TIES + 1, tree.n)
    for s in range(0, len(q), chunk):
        qq = q[s:s + chunk]
        _, idx = tree.query(qq, k=k, workers=-1)
        idx = idx.reshape(len(qq), k)
        e = qq[:, None, :] - pts[idx]
        d2 = (e * e).sum(-1)                                     # (exact on the lattice)
        same = d2 == d2.min(1, keepdims=True)
        order = np.argsort(np.where(same, idx, np.iinfo(np.int64).max), axis=1, kind='stable')
        idx, same = np.take_along_axis(idx, order, 1), np.take_along_axis(same, order, 1)
        for i in np.nonzero(same.sum(1) > _D2_TIES)[0]:          # more than 30 may tie: every row at that distance, the 30 lowest kept
            r2 = d2[i].min()
            cand = np.asarray(tree.query_ball_point(qq[i], np.sqrt(r2) + 1e-6), np.int64)
            cand = np.sort(cand[((pts[cand] - qq[i]) ** 2).sum(1) == r2])[:_D2_TIES]
            idx[i, :len(cand)], same[i] = cand, False
            same[i, :len(cand)] = True
        yield s, idx[:, :_D2_TIES], same[:, :_D2_TIES]


def _round_mean(total, count):
    """round_half_up(total / count) on integers"""
    return (2 * total + count) // (2 * count)


def _check_attr(attr, n, what, channels=None):
    attr = np.asarray(attr)
    if attr.dtype != np.uint8:
        raise ValueError(f'{what}: attributes must be uint8, got {attr.dtype}')
    if attr.ndim != 2 or attr.shape[0] != n or not (1 <= attr.shape[1] <= 4 if channels is None else attr.shape[1] == channels):
        raise ValueError(f'{what}: {n} points need attributes [{n},{"1..4" if channels is None else channels}], got {tuple(attr.shape)}')
    return attr


def recolour(src, attr_src, dst):
    """Attributes of the cloud dst ([nt,3]) from those of src ([ns,3], attr_src uint8 [ns,C], C = 1 .. 4), on the host.  -> uint8 [nt,C]"""
    src, dst = np.asarray(src, np.float64).reshape(-1, 3), np.asarray(dst, np.float64).reshape(-1, 3)
    if len(src) == 0 or len(dst) == 0:
        raise ValueError('recolour: empty point cloud')
    attr = _check_attr(attr_src, len(src), 'recolour').astype(np.int64)
    acc, cnt = np.zeros((len(dst), attr.shape[1]), np.int64), np.zeros(len(dst), np.int64)
    for s, idx, same in _tie_sets(dst, src):
        rows, cols = np.nonzero(same)
        np.add.at(acc, idx[rows, cols], attr[s + rows])
        np.add.at(cnt, idx[rows, cols], 1)
    out = np.zeros(acc.shape, np.int64)
    got = cnt > 0
    out[got] = _round_mean(acc[got], cnt[got, None])
    lone = np.nonzero(~got)[0]
    if len(lone):
        for s, idx, same in _tie_sets(src, dst[lone]):
            m = same.sum(1)[:, None]
            out[lone[s:s + len(idx)]] = _round_mean((attr[idx] * same[:, :, None]).sum(1), m)
    return out.astype(np.uint8)


def colour_sums(p, cp, q, cq):
    """p -> q: (the three sums over p of the squared YUV differences times (255 * 10^4)^2, as Python integers; the three maxima of the squared
    RGB differences)"""
    p, q = np.asarray(p, np.float64).reshape(-1, 3), np.asarray(q, np.float64).reshape(-1, 3)
    cp, cq = np.asarray(cp).astype(np.int64), np.asarray(cq).astype(np.int64)
    total, high = [0, 0, 0], np.zeros(3, np.int64)
    for s, idx, same in _tie_sets(q, p):
        mean = _round_mean((cq[idx] * same[:, :, None]).sum(1), same.sum(1)[:, None])
        d = cp[s:s + len(idx)] - mean
        y = d @ _YUV_1E4.T
        y2 = y * y                                               # below 2^43: summed as low and high words, exact at any size
        for k in range(3):
            total[k] += (int((y2[:, k] >> 32).sum()) << 32) + int((y2[:, k] & 0xFFFFFFFF).sum())
        high = np.maximum(high, (d * d).max(0))
    return total, [int(v) for v in high]


def _colour_columns(t1, h1, n1, t2, h2, n2):
    """the 36 columns from the exact sums and maxima of both directions"""
    out = {}
    mse = {'1': [t / (_YUV_DEN * n1) for t in t1], '2': [t / (_YUV_DEN * n2) for t in t2]}      # (int / int: correctly rounded)
    hd = {'1': [float(h) for h in h1], '2': [float(h) for h in h2]}
    mse['F'] = [max(a, b) for a, b in zip(mse['1'], mse['2'])]
    hd['F'] = [max(a, b) for a, b in zip(hd['1'], hd['2'])]
    psnr = lambda peak2, v: float(10 * np.log10(peak2 / v)) if v > 0 else float('inf')
    for d in '12F':
        for k in range(3):
            out[f'c[{k}],    {d}'] = mse[d][k]
            out[f'c[{k}],PSNR{d}'] = psnr(1.0, mse[d][k])
            out[f'h.c[{k}],    {d}'] = hd[d][k]
            out[f'h.c[{k}],PSNR{d}'] = psnr(255.0 * 255.0, hd[d][k])
    return {c: out[c] for c in COLOUR_COLUMNS}


def colour_psnr(a, ca, b, cb):
    """every colour column `pc_error_d -a A -b B -c 1 --hausdorff=1` prints (COLOUR_COLUMNS), computed on the host: a, b [n,3] coordinates,
    ca, cb uint8 [n,3] RGB"""
    a, b = np.asarray(a).reshape(-1, 3), np.asarray(b).reshape(-1, 3)
    if len(a) == 0 or len(b) == 0:
        raise ValueError('colour_psnr: empty point cloud')
    ca, cb = _check_attr(ca, len(a), 'colour_psnr', 3), _check_attr(cb, len(b), 'colour_psnr', 3)
    t1, h1 = colour_sums(a, ca, b, cb)
    t2, h2 = colour_sums(b, cb, a, ca)
    return _colour_columns(t1, h1, len(a), t2, h2, len(b))


def _device_cloud(t, what):
    from . import ops
    t = t.C if hasattr(t, 'C') else t
    t = t.contiguous()
    if t.dim() != 2 or t.shape[1] != 4:
        raise ValueError(f'{what}: coordinates must be [N,4] (batch, x, y, z), got {tuple(t.shape)}')
    if t.shape[0] == 0:
        raise ValueError(f'{what}: empty point cloud')
    ops.check_coords(t, what)
    return t


def _device_attr(attr, cloud, what, channels=None):
    import torch
    attr = torch.as_tensor(attr)
    if attr.dtype != torch.uint8:
        raise ValueError(f'{what}: attributes must be uint8, got {attr.dtype}')
    n = cloud.shape[0]
    if attr.dim() != 2 or attr.shape[0] != n or not (1 <= attr.shape[1] <= 4 if channels is None else attr.shape[1] == channels):
        raise ValueError(f'{what}: {n} points need attributes [{n},{"1..4" if channels is None else channels}], got {tuple(attr.shape)}')
    return attr.to(cloud.device).contiguous()


def nn_both(a, b):
    """(d2_nn(a, b), d2_nn(b, a)) of two [N,4] device clouds: the `nn=` argument of recolour_device and colour_psnr_device"""
    from . import ops
    ia, ib = ops.D2Index(a), ops.D2Index(b)
    return ops.d2_nn(a, ib), ops.d2_nn(b, ia)


def recolour_device(src, attr_src, dst, nn=None):
    """recolour on the GPU: src, dst int32 [N,4] (batch, x, y, z) device tensors (or sparse tensors), attr_src uint8 [ns,C], C = 1 .. 4;
    neighbours within the same batch index only.  nn = (d2_nn(src, dst), d2_nn(dst, src)) when the caller has searched already (nn_both).
    Exact, bitwise reproducible.  -> uint8 [nt,C] device tensor"""
    from . import ops
    src, dst = _device_cloud(src, 'recolour_device: src'), _device_cloud(dst, 'recolour_device: dst')
    attr = _device_attr(attr_src, src, 'recolour_device')
    st, ts = nn if nn is not None else nn_both(src, dst)
    return ops.attr_transfer(dst.shape[0], st, attr, ts)


def colour_psnr_device(a, ca, b, cb, nn=None):
    """The columns of colour_psnr computed on the GPU: a, b int32 [N,4] device tensors (or sparse tensors), ca, cb uint8 [n,3];
    nn = (d2_nn(a, b), d2_nn(b, a)) when the caller has searched already.  The sums are exact integers: every column equals colour_psnr's."""
    import torch
    from . import ops
    a, b = _device_cloud(a, 'colour_psnr_device: a'), _device_cloud(b, 'colour_psnr_device: b')
    ca, cb = _device_attr(ca, a, 'colour_psnr_device', 3), _device_attr(cb, b, 'colour_psnr_device', 3)
    ab, ba = nn if nn is not None else nn_both(a, b)
    sums = torch.stack([ops.colour_reduce(*ops.colour_dist(ca, cb, ab)), ops.colour_reduce(*ops.colour_dist(cb, ca, ba))]).cpu().tolist()
    (t1, h1), (t2, h2) = [([(r[3 + k] << 32) + r[k] for k in range(3)], r[6:9]) for r in sums]
    return _colour_columns(t1, h1, a.shape[0], t2, h2, b.shape[0])


def _colour_files(infile1, infile2):
    from .data_utils import read_ply_ascii_with_colours
    out = []
    for f in (infile1, infile2):
        xyz, rgb = read_ply_ascii_with_colours(f)
        if rgb is None:
            raise ValueError(f'{f} has no colours (red green blue): the colour distortion needs them in both clouds, as `pc_error_d -c 1` does')
        out += [xyz, rgb]
    return out


def pc_error(infile1, infile2, res, normal=False, show=False, color=False):
    """color=True adds COLOUR_COLUMNS (`-c 1`): both files need red green blue."""
    exe = _exe()
    if color:
        from .data_utils import ply_has_colours
        for f in (infile1, infile2):
            if not ply_has_colours(f):
                raise ValueError(f'{f} has no colours (red green blue): the colour distortion needs them in both clouds')
    if exe is None:
        from .data_utils import read_ply_ascii_geo
        if color:
            base = pc_error(infile1, infile2, res, normal=normal, show=show)
            return pd.concat([base, pd.DataFrame([colour_psnr(*_colour_files(infile1, infile2))])], axis=1)
        if normal:
            a, na = read_ply_ascii_with_normals(infile1)
            if na is None:
                raise ValueError(f'{infile1} has no normals (nx ny nz): point-to-plane (D2) needs them, as `pc_error_d -n` does')
            return pd.DataFrame([d2_psnr(a, na, read_ply_ascii_with_normals(infile2)[0], res)])
        return pd.DataFrame([d1_psnr(read_ply_ascii_geo(infile1), read_ply_ascii_geo(infile2), res)])
    headers = ['mse1      (p2point)', 'mse1,PSNR (p2point)', 'h.       1(p2point)', 'h.,PSNR  1(p2point)',
               'mse2      (p2point)', 'mse2,PSNR (p2point)', 'h.       2(p2point)', 'h.,PSNR  2(p2point)',
               'mseF      (p2point)', 'mseF,PSNR (p2point)', 'h.        (p2point)', 'h.,PSNR   (p2point)']
    p2plane = ['mse1      (p2plane)', 'mse1,PSNR (p2plane)', 'mse2      (p2plane)', 'mse2,PSNR (p2plane)',
               'mseF      (p2plane)', 'mseF,PSNR (p2plane)']
    cmd = [exe, '-a', infile1, '-b', infile2, '--hausdorff=1', '--resolution=' + str(res - 1)]
    if normal:
        headers += p2plane
        cmd += ['-n', infile1]
    if color:
        cmd += ['-c', '1']
    out = subprocess.run(cmd, stdout=subprocess.PIPE).stdout.decode('utf-8', 'replace')
    results = {}
    for line in out.splitlines():
        if show:
            print(line)
        for key in headers:
            if line.find(key) != -1:
                results[key] = number_in_line(line)
        # the colour labels are matched whole ('c[0],    1' is a substring of 'h.c[0],    1')
        if color and ':' in line and line.split(':')[0].strip() in COLOUR_COLUMNS:
            results[line.split(':')[0].strip()] = number_in_line(line)
    if color:                                                    # (the geometry columns first, as the native route orders them)
        results = {k: results[k] for k in headers + COLOUR_COLUMNS if k in results}
    return pd.DataFrame([results])
