"""The definitions of DESIGN.md 8f restated in numpy / scipy, for the colour tests: tie sets, recolouring, colour distortion.

Tie sets are those of ops.d2_nn and oracle d2_metrics: the tie set of p in Q is every row of Q at the nearest squared distance (duplicated rows
are points of their own), at most 30 rows, the 30 lowest original rows when more tie.  Clouds here are [n,3] integer arrays of ONE batch item;
`shifted` turns [n,4] (batch, x, y, z) rows into that by moving item b by b * 10^4 along x, so that no cross-item neighbour can be nearest."""
import numpy as np
from scipy.spatial import cKDTree

TIES = 30
YUV = np.array([[0.2126, 0.7152, 0.0722], [-0.1146, -0.3854, 0.5], [0.5, -0.4542, -0.0458]])
COLUMNS = [f'{h}c[{k}],{w}{d}' for d in '12F' for h, w in (('', '    '), ('', 'PSNR'), ('h.', '    '), ('h.', 'PSNR')) for k in range(3)]


def shifted(c4):
    c4 = np.asarray(c4, np.int64)
    out = c4[:, 1:].copy()
    out[:, 0] += c4[:, 0] * 10 ** 4
    return out


def tie_sets(p, q):
    """-> list over the rows of p: int64 array of the rows of q in its tie set, ascending"""
    p, q = np.asarray(p, np.int64), np.asarray(q, np.int64)
    k = min(TIES + 1, len(q))
    _, idx = cKDTree(q.astype(np.float64)).query(p.astype(np.float64), k=k)
    idx = idx.reshape(len(p), k)
    d2 = ((p[:, None, :] - q[idx]) ** 2).sum(-1)
    out = []
    for i in range(len(p)):
        best = d2[i].min()
        if (d2[i] == best).sum() > TIES:                       # the query may have missed rows at that distance: look at every row of q
            rows = np.nonzero(((q - p[i]) ** 2).sum(1) == best)[0]
        else:
            rows = np.sort(idx[i][d2[i] == best])
        out.append(rows[:TIES])
    return out


def max_tie_set(p, q):
    """the largest number of rows of q at the nearest distance of a row of p, counted up to 31 (a k = 31 query)"""
    p, q = np.asarray(p, np.int64), np.asarray(q, np.int64)
    k = min(TIES + 1, len(q))
    _, idx = cKDTree(q.astype(np.float64)).query(p.astype(np.float64), k=k)
    d2 = ((p[:, None, :] - q[idx.reshape(len(p), k)]) ** 2).sum(-1)
    return int((d2 == d2.min(1, keepdims=True)).sum(1).max())


def round_half_up_mean(values):
    """per channel (2 sum + n) // (2 n) of an integer array [n,C]"""
    values = np.asarray(values, np.int64)
    n = len(values)
    return (2 * values.sum(0) + n) // (2 * n)


def recolour(s, attr_s, t):
    """attributes uint8 [nt,C] of T from those of S"""
    attr_s = np.asarray(attr_s)
    assert attr_s.dtype == np.uint8 and attr_s.ndim == 2 and len(attr_s) == len(s)
    received = [[] for _ in range(len(t))]
    for i, rows in enumerate(tie_sets(s, t)):                  # R(t) = { s : t is in the tie set of s in T }
        for r in rows:
            received[r].append(i)
    own = None
    out = np.zeros((len(t), attr_s.shape[1]), np.uint8)
    for j in range(len(t)):
        if received[j]:
            out[j] = round_half_up_mean(attr_s[received[j]])
        else:
            if own is None:
                own = tie_sets(t, s)
            out[j] = round_half_up_mean(attr_s[own[j]])
    return out


def to_yuv(rgb):
    out = (np.asarray(rgb, np.float64) @ YUV.T) / 255.0
    out[:, 1:] += 0.5
    return out


def one_way(p, cp, q, cq):
    """-> (mean over p of the squared Y, U, V differences [3], max over p of the squared R, G, B differences [3])"""
    cp, cq = np.asarray(cp, np.int64), np.asarray(cq, np.int64)
    mean = np.stack([round_half_up_mean(cq[rows]) for rows in tie_sets(p, q)])
    dy = (to_yuv(cp) - to_yuv(mean)) ** 2
    return dy.mean(0), ((cp - mean) ** 2).max(0).astype(np.float64)


def colour_metric(a, ca, b, cb):
    """the 36 columns `pc_error_d -c 1 --hausdorff=1` prints"""
    m1, h1 = one_way(a, ca, b, cb)
    m2, h2 = one_way(b, cb, a, ca)
    mse = {'1': m1, '2': m2, 'F': np.maximum(m1, m2)}
    hd = {'1': h1, '2': h2, 'F': np.maximum(h1, h2)}
    psnr = lambda peak2, v: float(10 * np.log10(peak2 / v)) if v > 0 else float('inf')
    out = {}
    for d in '12F':
        for k in range(3):
            out[f'c[{k}],    {d}'] = float(mse[d][k])
            out[f'c[{k}],PSNR{d}'] = psnr(1.0, mse[d][k])
            out[f'h.c[{k}],    {d}'] = float(hd[d][k])
            out[f'h.c[{k}],PSNR{d}'] = psnr(255.0 ** 2, hd[d][k])
    return {c: out[c] for c in COLUMNS}


def golden_key(case, column):
    """name under which tests/golden/colour_metric.npz stores a printed value"""
    return f'p{case}_' + column.replace(' ', '').replace(',', '_')
