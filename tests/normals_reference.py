"""The definition of the estimated normals ("Estimated normals"; pcgcv2_amd/csrc/normals.hip) in numpy / scipy, independent of the
device code: per batch a ball query on the DISTINCT voxels (a KD-tree, or an occupancy grid where the cloud's box is small), integer
moments, np.linalg.eigh on the integer scatter matrix as float64, the orientation rules.  tools/normals_time.py times it as the host side of the comparison."""
import numpy as np

MOMENT_NAMES = ('k', 'sx', 'sy', 'sz', 'sxx', 'syy', 'szz', 'sxy', 'sxz', 'syz')
GRID_CELLS = 1 << 24      # boxes up to this many voxels are searched through a dense occupancy grid (full neighbourhoods cost no lists)


def _moments_grid(pts, r2):
    """the same moments from a padded occupancy grid: one gather per lattice offset of the ball"""
    r = int(np.sqrt(r2))
    lo = pts.min(0) - r
    occ = np.zeros(tuple(pts.max(0) + r + 1 - lo), bool)
    q = pts - lo
    occ[q[:, 0], q[:, 1], q[:, 2]] = True
    out = np.zeros((len(pts), 10), np.int64)
    ax = np.arange(-r, r + 1)
    for dx in ax:
        for dy in ax:
            for dz in ax:
                if dx * dx + dy * dy + dz * dz > r2:
                    continue
                hit = occ[q[:, 0] + dx, q[:, 1] + dy, q[:, 2] + dz].astype(np.int64)
                out += hit[:, None] * np.array([1, dx, dy, dz, dx * dx, dy * dy, dz * dz, dx * dy, dx * dz, dy * dz], np.int64)
    return out


def _moments_of_batch(pts, r2, method='auto', chunk=1 << 16):
    """pts: distinct voxels int64 [n,3] of one batch -> moments int64 [n,10] over d = q - p, |d|^2 <= r2 (p itself included)"""
    if method == 'grid' or (method == 'auto' and np.prod((pts.max(0) - pts.min(0) + 17).astype(np.float64)) <= GRID_CELLS):
        return _moments_grid(pts, r2)
    from scipy.spatial import cKDTree
    n = len(pts)
    out = np.zeros((n, 10), np.int64)
    tree = cKDTree(pts.astype(np.float64))
    radius = float(np.sqrt(r2)) + 1e-6                                 # (a superset: the integer test below decides)
    for s in range(0, n, chunk):
        p = pts[s:s + chunk]
        lists = tree.query_ball_point(p.astype(np.float64), radius, workers=-1, return_sorted=False)
        lens = np.fromiter((len(l) for l in lists), np.int64, len(lists))
        idx = np.concatenate([np.asarray(l, np.int64) for l in lists]) if lens.sum() else np.zeros(0, np.int64)
        row = np.repeat(np.arange(len(p)), lens)
        d = pts[idx] - p[row]
        keep = (d * d).sum(1) <= r2
        d, row = d[keep], row[keep]
        cols = [np.ones(len(d), np.int64), d[:, 0], d[:, 1], d[:, 2], d[:, 0] ** 2, d[:, 1] ** 2, d[:, 2] ** 2,
                d[:, 0] * d[:, 1], d[:, 0] * d[:, 2], d[:, 1] * d[:, 2]]
        for j, c in enumerate(cols):                                   # (sums far below 2^53: exact in the float64 bincount adds in)
            out[s:s + len(p), j] = np.rint(np.bincount(row, weights=c.astype(np.float64), minlength=len(p))).astype(np.int64)
    return out


def scatter(m):
    """moments int64 [n,10] -> S int64 [n,3,3] = k sum(d d^T) - (sum d)(sum d)^T"""
    k = m[:, 0]
    sxx, syy, szz = k * m[:, 4] - m[:, 1] ** 2, k * m[:, 5] - m[:, 2] ** 2, k * m[:, 6] - m[:, 3] ** 2
    sxy, sxz, syz = k * m[:, 7] - m[:, 1] * m[:, 2], k * m[:, 8] - m[:, 1] * m[:, 3], k * m[:, 9] - m[:, 2] * m[:, 3]
    return np.stack([np.stack([sxx, sxy, sxz], 1), np.stack([sxy, syy, syz], 1), np.stack([sxz, syz, szz], 1)], 1)


def _largest_component_sign(n):
    """(sign that makes the component of largest magnitude positive (the first one on ties), margin to the runner-up magnitude)"""
    a = np.abs(n)
    j = np.argmax(a, 1)                                                # (first occurrence on ties)
    big = n[np.arange(len(n)), j]
    srt = np.sort(a, 1)
    return np.where(big < 0, -1.0, 1.0), srt[:, 2] - srt[:, 1]


def estimate_normals(coords, r2=16, orient='centroid', method='auto'):
    """coords: int [N,4] (batch, x, y, z), rows in any order, duplicates allowed.  -> dict of per-ROW arrays: moments int64 [N,10], count,
    valid, lam float64 [N,3] ascending, normals float64 [N,3] (oriented; zeros where not valid), gap = (lam1 - lam0) / lam2 (0 where lam2 = 0),
    dot = the orientation rule's dot product divided by the length of its direction vector (for orient=None: the margin by which the largest
    component leads): tests compare signs only where |dot| is well above rounding.  method: 'auto' | 'kdtree' | 'grid' (how neighbours are found)."""
    coords = np.asarray(coords, np.int64)
    if not 1 <= r2 <= 64:
        raise ValueError('r2 outside 1 .. 64')
    uniq, inv = np.unique(coords, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    n = len(uniq)
    mom = np.zeros((n, 10), np.int64)
    direction = np.zeros((n, 3), np.float64)
    for b in np.unique(uniq[:, 0]):
        sel = np.nonzero(uniq[:, 0] == b)[0]
        pts = uniq[sel, 1:]
        mom[sel] = _moments_of_batch(pts, r2, method)
        if isinstance(orient, str):
            if orient != 'centroid':
                raise ValueError(orient)
            direction[sel] = (len(pts) * pts - pts.sum(0)).astype(np.float64)      # N_b p - sum q: exact integers
        elif orient is not None:
            direction[sel] = np.asarray(orient, np.float64) - pts.astype(np.float64)
    S = scatter(mom)
    minors = (S[:, 0, 0] * S[:, 1, 1] - S[:, 0, 1] ** 2) + (S[:, 0, 0] * S[:, 2, 2] - S[:, 0, 2] ** 2) + (S[:, 1, 1] * S[:, 2, 2] - S[:, 1, 2] ** 2)
    valid = (mom[:, 0] >= 3) & (minors != 0)
    lam, vec = np.linalg.eigh(S.astype(np.float64))
    nrm = vec[:, :, 0].copy()
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    none_sign, none_margin = _largest_component_sign(nrm)
    if orient is None:
        sign, dot = none_sign, none_margin
    else:
        raw = nrm[:, 0] * direction[:, 0] + nrm[:, 1] * direction[:, 1] + nrm[:, 2] * direction[:, 2]
        sign = np.where(raw < 0, -1.0, np.where(raw > 0, 1.0, none_sign))
        length = np.linalg.norm(direction, axis=1)
        dot = np.where(length > 0, raw / np.maximum(length, 1e-300), 0.0)
    nrm = nrm * sign[:, None] + 0.0
    nrm[~valid] = 0.0
    with np.errstate(invalid='ignore', divide='ignore'):
        gap = np.where(lam[:, 2] > 0, (lam[:, 1] - lam[:, 0]) / lam[:, 2], 0.0)
    return {'moments': mom[inv], 'count': mom[inv, 0].astype(np.int32), 'valid': valid[inv], 'lam': lam[inv], 'normals': nrm[inv],
            'gap': gap[inv], 'dot': dot[inv], 'S': S[inv]}
