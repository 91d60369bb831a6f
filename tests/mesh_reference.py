"""The definition of this project's mesh sampling and voxelisation, restated in numpy.  csrc/mesh.hip must EQUAL it.

open3d's sample_points_uniformly (the reference's generate_dataset.py:11) draws from std::mt19937 through library distributions and
cannot be reproduced, so the sampling arithmetic is defined here, exactly, in fp64, with a counter-based generator: sample i is a pure
function of (seed, i).  Every step after sampling is mesh2pc's (generate_dataset.py:27-35), operation for operation.  numpy evaluates
each elementwise operation with one IEEE rounding and never fuses a multiply with an add; the products of `points . R` are written out
because a BLAS dot may.
"""
import math

import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85          # Philox4x32-10 (Random123)
MASK = np.uint64(0xFFFFFFFF)

KNOWN_ANSWERS = [                                                        # Random123's kat_vectors for philox4x32 10
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def philox(ctr, key):
    """ctr [n,4] uint32, key (k0, k1) -> [n,4] uint32; all arithmetic in uint64 masked to 32 bits"""
    c = [np.asarray(ctr)[:, i].astype(np.uint64) for i in range(4)]
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & MASK]
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return np.stack(c, 1).astype(np.uint32)


def uniforms(seed, first, n):
    """-> u0 in [0,1), u, v in (0,1) of samples first .. first+n-1, all exact in fp64"""
    i = np.uint64(first) + np.arange(n, dtype=np.uint64)
    ctr = np.stack([i & MASK, i >> np.uint64(32), np.zeros(n, np.uint64), np.zeros(n, np.uint64)], 1)
    w = philox(ctr, (int(seed) & 0xFFFFFFFF, int(seed) >> 32)).astype(np.uint64)
    u0 = ((w[:, 0] << np.uint64(20)) | (w[:, 1] >> np.uint64(12))).astype(np.float64) * 2.0 ** -52
    u = (w[:, 2].astype(np.float64) + 0.5) * 2.0 ** -32
    v = (w[:, 3].astype(np.float64) + 0.5) * 2.0 ** -32
    return u0, u, v


def areas(verts, faces):
    A, B, C = (verts[faces[:, k]] for k in range(3))
    e1, e2 = B - A, C - A
    cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    return 0.5 * np.sqrt((cx * cx + cy * cy) + cz * cz)


def fsum_cdf(area):
    """the exactly rounded inclusive sums (math.fsum of every prefix, in O(T): fsum's partials carried along)"""
    out, partials = np.empty(len(area)), []
    for t, x in enumerate(area.tolist()):
        i = 0
        for y in partials:                               # Shewchuk's grow-expansion, as math.fsum does it
            if abs(x) < abs(y):
                x, y = y, x
            hi = x + y
            lo = y - (hi - x)
            if lo:
                partials[i] = lo
                i += 1
            x = hi
        partials[i:] = [x]
        out[t] = math.fsum(partials)
    return out


def sample(verts, faces, cdf, seed, first, n):
    """-> tri int32 [n], points float64 [n,3]"""
    u0, u, v = uniforms(seed, first, n)
    T = len(cdf)
    t = np.minimum(np.searchsorted(cdf, u0 * cdf[T - 1], side='right'), T - 1)
    fold = u + v > 1
    u, v = np.where(fold, 1 - u, u), np.where(fold, 1 - v, v)
    A, B, C = (verts[faces[t, k]] for k in range(3))
    p = (A + u[:, None] * (B - A)) + v[:, None] * (C - A)
    return t.astype(np.int32), p


def voxelize(verts, faces, cdf, seed, n, R, resolution):
    """-> int32 [M,3]: the distinct voxels ordered by (z, y, x), z most significant"""
    _, p = sample(verts, faces, cdf, seed, 0, n)
    R = np.asarray(R, dtype=np.float64)
    q = np.stack([(p[:, 0] * R[0, j] + p[:, 1] * R[1, j]) + p[:, 2] * R[2, j] for j in range(3)], 1)
    mn = np.min(q)
    d = q - mn
    mx = np.max(d)
    if not mx > 0:
        raise ValueError('max == 0')
    vox = np.round((d / mx) * resolution).astype(np.int32)
    vox = np.unique(vox, axis=0)
    return vox[np.lexsort((vox[:, 0], vox[:, 1], vox[:, 2]))]


# ------------------------------------------------------------------------------------------------ test meshes
CUBE_VERTS = np.array([[x, y, z] for z in (0, 1) for y in (0, 1) for x in (0, 1)], dtype=np.float64)
CUBE_QUADS = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]


def fan(polys):
    return np.array([(p[0], p[i], p[i + 1]) for p in polys for i in range(1, len(p) - 1)], dtype=np.int32)


def cube():
    return CUBE_VERTS.copy(), fan(CUBE_QUADS)


def random_mesh(T, seed, lo=-1.0, hi=1.0):
    rng = np.random.default_rng(seed)
    V = max(4, T // 2)
    verts = rng.uniform(lo, hi, (V, 3))
    faces = rng.integers(0, V, (T, 3)).astype(np.int32)
    return verts, faces


def fixed_rotation():
    """one fixed rotation built like get_rotate_matrix (QR of a Gaussian matrix, first axis flipped)"""
    m = np.eye(3, dtype='float32')
    m[0, 0] = -1
    return np.dot(m, np.linalg.qr(np.random.default_rng(12345).standard_normal((3, 3)))[0])


def write_off(path, verts, polys, glued=False):
    with open(path, 'w') as f:
        f.write(('OFF' if glued else 'OFF\n') + f'{len(verts)} {len(polys)} 0\n')
        for v in verts:
            f.write(' '.join(repr(float(x)) for x in v) + '\n')
        for p in polys:
            f.write(f'{len(p)} ' + ' '.join(str(int(i)) for i in p) + '\n')


def write_obj(path, verts, polys):
    with open(path, 'w') as f:
        for v in verts:
            f.write('v ' + ' '.join(repr(float(x)) for x in v) + '\n')
        for p in polys:
            f.write('f ' + ' '.join(str(int(i) + 1) for i in p) + '\n')
