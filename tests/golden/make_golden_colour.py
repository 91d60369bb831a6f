"""Regenerates tests/golden/colour_metric.npz: the colour lines mpeg-pcc-dmetric 0.13.4 prints with `-c 1 --hausdorff=1` on four small pairs of
coloured clouds.  Needs the reference checkout for its vendored pc_error_d binary (nothing of it is copied here, only what it prints):

    python tests/golden/make_golden_colour.py --reference DIR

The binary keeps an unspecified subset when more than 30 rows tie at the nearest distance, so the generator asserts through a k = 31 query that
no tie set of any case, in either direction, exceeds 30: the fixture is one the binary alone settles."""
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

if '--reference' not in sys.argv[1:-1]:
    sys.exit('usage: make_golden_colour.py --reference DIR')
REF = os.path.abspath(sys.argv[sys.argv.index('--reference') + 1])
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
from colour_reference import COLUMNS, TIES, golden_key, max_tie_set      # noqa: E402


def write_coloured(path, pts, rgb):
    with open(path, 'w') as f:
        f.write('ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n'
                'property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n' % len(pts))
        for q, c in zip(pts, rgb):
            f.write('%d %d %d %d %d %d\n' % (q[0], q[1], q[2], c[0], c[1], c[2]))


def shell(res, radius, thick):
    g = np.stack(np.meshgrid(*[np.arange(res)] * 3, indexing='ij'), -1).reshape(-1, 3)
    r = np.linalg.norm(g - res / 2.0, axis=1)
    return g[np.abs(r - radius) < thick]


def gradient(pts, res):
    """a smooth colour: each channel a slow function of position"""
    t = pts.astype(np.float64) / res
    rgb = np.stack([255 * t[:, 0], 127.5 * (1 + np.sin(6 * t[:, 1])), 255 * (t[:, 2] * t[:, 0])], 1)
    return np.clip(np.rint(rgb), 0, 255).astype(np.uint8)


def main():
    rng = np.random.default_rng(8)
    random_colours = lambda n: rng.integers(0, 256, size=(n, 3)).astype(np.uint8)
    cases = []
    a = shell(64, 20, 0.7)                                       # thin shell; B: jittered by one voxel, 50 points fewer
    b = np.unique(np.clip(a + rng.integers(-1, 2, size=a.shape), 0, 63), axis=0)[:len(a) - 50]
    cases.append((a, random_colours(len(a)), b, random_colours(len(b)), 64))
    a = shell(128, 30, 1.2)                                      # thicker shell; B: shifted up to three voxels (many distance ties); smooth colours
    b = np.unique(np.clip(a + rng.integers(-3, 4, size=a.shape), 0, 127), axis=0)
    cases.append((a, gradient(a, 128), b, gradient(b[:, ::-1], 128), 128))
    a = shell(64, 18, 0.6)                                       # identical clouds and colours: zeros, infinite PSNR
    ca = random_colours(len(a))
    cases.append((a, ca, a.copy(), ca.copy(), 64))
    a = np.unique(rng.integers(0, 128, size=(4000, 3)), axis=0)  # scattered points against a sparser jitter
    b = np.unique(np.clip(a + rng.integers(-2, 3, size=a.shape), 0, 127), axis=0)
    b = b[rng.random(len(b)) < 0.6]
    cases.append((a, random_colours(len(a)), b, random_colours(len(b)), 128))
    out = {'n_cases': np.array(len(cases))}
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, 'pc_error_d'); shutil.copy(os.path.join(REF, 'pc_error_d'), exe); os.chmod(exe, 0o755)
        for i, (a, ca, b, cb, res) in enumerate(cases):
            assert max_tie_set(a, b) <= TIES and max_tie_set(b, a) <= TIES, f'case {i}: a tie set exceeds {TIES}'
            pa, pb = os.path.join(d, f'a{i}.ply'), os.path.join(d, f'b{i}.ply')
            write_coloured(pa, a, ca); write_coloured(pb, b, cb)
            text = subprocess.run([exe, '-a', pa, '-b', pb, '-c', '1', '--hausdorff=1', '--resolution=' + str(res - 1)],
                                  stdout=subprocess.PIPE, check=True).stdout.decode('utf-8', 'replace')
            printed = {}
            for line in text.splitlines():
                label = line.split(':')[0].strip()
                if ':' in line and label in COLUMNS:
                    printed[label] = float(line.split(':')[1])
            assert sorted(printed) == sorted(COLUMNS), f'case {i}: the binary printed {sorted(printed)}'
            out[f'p{i}_a'], out[f'p{i}_b'] = a.astype(np.int16), b.astype(np.int16)
            out[f'p{i}_ca'], out[f'p{i}_cb'], out[f'p{i}_res'] = ca, cb, np.array(res)
            for c in COLUMNS:
                out[golden_key(i, c)] = np.array(printed[c])
            if i == 0:
                kept = '\n'.join(l for l in text.splitlines() if d not in l) + '\n'      # (without the lines that echo the temporary paths)
                out['p0_stdout'] = np.frombuffer(kept.encode(), np.uint8)                # one captured output, for the parser's test
    np.savez_compressed(os.path.join(OUT, 'colour_metric.npz'), **out)


if __name__ == '__main__':
    main()
