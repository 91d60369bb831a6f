"""Cleaning a voxelised cloud, the parts that need no GPU: the definition (tests/clean_reference.py) against brute force (an N x N adjacency
matrix with a breadth-first search, N x N squared distances), the figures pinned for the project's own clouds, hand-made cases, every
refusal with its count, CLI parsing, and the C-ABI entries' refusals before anything is touched."""
import numpy as np
import pytest

import clean_reference as R
from pcgcv2_amd import _lib, attributes, clean, coder, synthetic, voxelize as vox


def _rows(xyz, batch=0):
    xyz = np.asarray(xyz, np.int32).reshape(-1, 3)
    return np.concatenate([np.full((len(xyz), 1), batch, np.int32), xyz], 1)


def _named(name, order='raster'):
    return _rows(synthetic.cloud(name, order=order, seed=3).numpy())


# ---- the definition against brute force ---------------------------------------------------------------------------------------------------
def _brute(c, r2, min_neighbours, min_component, keep_largest):
    c = c.astype(np.int64)
    n = len(c)
    d = c[:, None, 1:] - c[None, :, 1:]
    same = (c[:, None, 0] == c[None, :, 0]) & ~np.eye(n, dtype=bool)
    neighbours = (((d * d).sum(2) <= r2) & same).sum(1)
    keep1 = neighbours >= min_neighbours
    adjacent = (np.abs(d).max(2) == 1) & same & keep1[:, None] & keep1[None, :]
    labels, sizes = np.full(n, -1), np.zeros(n, np.int64)
    for i in range(n):                                                         # rows ascend: an unlabelled row is its component's smallest
        if keep1[i] and labels[i] < 0:
            seen, front = {i}, [i]
            while front:
                front = [int(j) for f in front for j in np.flatnonzero(adjacent[f]) if j not in seen and not seen.add(int(j))]
            members = sorted(seen)
            labels[members], sizes[members] = i, len(members)
    keep = keep1 & (sizes >= min_component)
    if keep_largest:
        for b in np.unique(c[:, 0]):
            roots = [i for i in range(n) if labels[i] == i and c[i, 0] == b]
            roots.sort(key=lambda i: (-sizes[i], i))
            keep &= ~((c[:, 0] == b) & ~np.isin(labels, roots[:keep_largest]))
    return keep, neighbours, labels, sizes


def _cloud(n, seed, box=12):
    rng = np.random.default_rng(seed)
    cells = rng.permutation(box ** 3)[:n]
    return np.stack([cells % box, cells // box % box, cells // (box * box)], 1)


@pytest.mark.parametrize('n', [40, 150, 300])
@pytest.mark.parametrize('r2,k,m,largest', [(16, 0, 1, 0), (3, 2, 1, 0), (16, 4, 3, 0), (1, 1, 2, 2), (64, 30, 1, 1), (9, 0, 2, 3)])
def test_definition_against_brute_force(n, r2, k, m, largest):
    c = _rows(_cloud(n, n + r2))
    got = R.clean(c, None, r2, k, m, largest)
    keep, neighbours, labels, sizes = _brute(c, r2, k, m, largest)
    assert np.array_equal(got.neighbours, neighbours) and np.array_equal(got.labels, labels) and np.array_equal(got.sizes, sizes)
    assert np.array_equal(got.keep, keep) and np.array_equal(got.coords, c[keep])
    assert got.removed_density == (neighbours < k).sum() and got.removed_density + got.removed_component == n - keep.sum()
    assert got.n_components == (labels == np.arange(n)).sum()
    assert got.neighbours.dtype == got.labels.dtype == got.sizes.dtype == np.int32 and got.keep.dtype == bool


def test_two_batch_items_that_overlap_in_space():
    a, b = _cloud(140, 1), _cloud(160, 2)
    c = np.concatenate([_rows(a, 0), _rows(b, 5)])
    c = c[np.random.default_rng(3).permutation(len(c))]
    assert len(np.unique(c[:, 1:], axis=0)) < len(c)                           # some voxels are in both items
    for args in ((16, 0, 1, 0), (6, 3, 2, 0), (16, 0, 1, 2)):
        got = R.clean(c, None, *args)
        keep, neighbours, labels, sizes = _brute(c, *args)
        assert np.array_equal(got.neighbours, neighbours) and np.array_equal(got.labels, labels) and np.array_equal(got.sizes, sizes)
        assert np.array_equal(got.keep, keep)
    lab = R.clean(c, None).labels
    assert (c[lab, 0] == c[:, 0]).all()                                        # no component crosses the items


# ---- pinned figures (scipy.ndimage.label with the full 3 x 3 x 3 structure, and a direct count) -------------------------------------------
def test_pinned_multi_s():
    c = _named('multi_s')
    labels, sizes, n_components = R.connected_components(c)
    assert len(c) == 15733 and n_components == 3
    assert sorted(np.bincount(labels)[np.unique(labels)].tolist(), reverse=True) == [15426, 280, 27]
    assert sorted(set(sizes.tolist()), reverse=True) == [15426, 280, 27]


def test_pinned_noisy_s():
    c = _named('noisy_s')
    got = R.clean(c, None, r2=16)
    per_component = np.bincount(got.labels)[np.unique(got.labels)]
    assert len(c) == 11086 and got.n_components == 843 == len(per_component)
    assert (per_component == 1).sum() == 803 and per_component.max() == 10204
    assert (got.neighbours < 4).sum() == 480 and (got.neighbours < 8).sum() == 535
    assert R.clean(c, None, 16, 4, 1).removed_density == 480 and R.clean(c, None, 16, 8, 1).removed_density == 535


def test_pinned_shell7():
    c = _named('shell7')
    assert R.connected_components(c)[2] == 1 and R.neighbour_counts(c, 16).min() == 35


# ---- hand-made cases ----------------------------------------------------------------------------------------------------------------------
def test_label_is_the_smallest_row_under_a_shuffle():
    xyz = np.array([[0, 0, 0], [1, 1, 1], [2, 2, 1], [9, 9, 9], [9, 10, 9], [20, 0, 0]])      # components {0,1,2}, {3,4}, {5}
    for seed in range(5):
        perm = np.random.default_rng(seed).permutation(6)
        labels, sizes, n = R.connected_components(_rows(xyz[perm]))
        where = np.argsort(perm)                                               # where[j]: the row that holds voxel j
        for group in ([0, 1, 2], [3, 4], [5]):
            assert set(labels[where[group]].tolist()) == {int(where[group].min())}
            assert set(sizes[where[group]].tolist()) == {len(group)}
        assert n == 3


def test_keep_largest_ties_go_to_the_smaller_label():
    xyz = np.array([[30, 0, 0], [0, 0, 0], [1, 0, 0], [10, 0, 0], [11, 0, 0], [20, 0, 0], [21, 0, 0], [21, 1, 0]])
    c = _rows(xyz)                                                             # sizes: {5,6,7} = 3, {1,2} = 2, {3,4} = 2, {0} = 1
    assert R.clean(c, None, keep_largest=1).keep.tolist() == [False] * 5 + [True] * 3
    assert R.clean(c, None, keep_largest=2).keep.tolist() == [False, True, True, False, False, True, True, True]      # label 1 before label 3
    assert R.clean(c, None, keep_largest=3).keep.tolist() == [False] + [True] * 7
    assert R.clean(c, None, keep_largest=4).keep.all() and R.clean(c, None, keep_largest=99).keep.all()
    assert R.clean(c, None, min_component=3, keep_largest=2).keep.tolist() == [False] * 5 + [True] * 3


def test_the_two_stages_in_order():
    # a bar of three: the ends have one neighbour within r2 = 1, the middle has two.  min_neighbours = 2 drops the ends, and the middle,
    # which passed with their help, is a singleton in stage 2: nothing is counted again
    c = _rows([[0, 0, 0], [1, 0, 0], [2, 0, 0]])
    got = R.clean(c, None, r2=1, min_neighbours=2, min_component=1)
    assert got.neighbours.tolist() == [1, 2, 1] and got.keep.tolist() == [False, True, False]
    assert got.labels.tolist() == [-1, 1, -1] and got.sizes.tolist() == [0, 1, 0] and got.n_components == 1
    got = R.clean(c, None, r2=1, min_neighbours=2, min_component=2)
    assert not got.keep.any() and (got.removed_density, got.removed_component) == (2, 1) and got.coords.shape == (0, 4)


def test_colours_and_empty():
    c = _rows([[0, 0, 0], [5, 5, 5], [0, 1, 0]])
    rgb = np.array([[1, 2, 3], [4, 5, 6], [7, 8, 9]], np.uint8)
    got = R.clean(c, rgb, min_component=2)
    assert got.colours.tolist() == [[1, 2, 3], [7, 8, 9]] and got.colours.dtype == np.uint8 and got.coords.tolist() == c[[0, 2]].tolist()
    none = R.clean(np.zeros((0, 4), np.int32), np.zeros((0, 3), np.uint8), min_neighbours=3)
    assert none.keep.shape == (0,) and none.coords.shape == (0, 4) and none.n_components == 0


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_count():
    ok = _rows([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0]])
    dup = ok.copy()
    dup[2], dup[3] = dup[0], dup[0]
    with pytest.raises(ValueError, match='2 of 4 rows repeat'):
        R.clean(dup, None)
    with pytest.raises(ValueError, match='2 of 4 rows repeat'):
        R.connected_components(dup)
    far = ok.copy()
    far[1, 1], far[2, 3], far[3, 2] = 1 << 20, -1, (1 << 20) - 1               # the last one is inside
    with pytest.raises(ValueError, match='2 of 4 rows are outside'):
        R.clean(far, None)
    batch = ok.copy()
    batch[0, 0], batch[1, 0], batch[2, 0] = 16, -1, 15
    with pytest.raises(ValueError, match='2 of 4 rows are outside'):
        R.clean(batch, None)
    for kw in (dict(r2=0), dict(r2=65), dict(r2=True), dict(r2=4.0), dict(min_neighbours=-1), dict(min_component=0), dict(keep_largest=-1),
               dict(min_component=1.5)):
        with pytest.raises(ValueError, match=list(kw)[0]):
            R.clean(ok, None, **kw)
    with pytest.raises(ValueError, match='colours'):
        R.clean(ok, np.zeros((3, 3), np.uint8))
    with pytest.raises(ValueError, match='int32'):
        R.clean(ok.astype(np.int64), None)

    class Big:                                                                 # 2^24 + 1 rows without the memory
        ndim, shape, dtype = 2, ((1 << 24) + 1, 4), np.dtype(np.int32)

        def __len__(self):
            return self.shape[0]

        def __array__(self, dtype=None, copy=None):
            return np.lib.stride_tricks.as_strided(np.zeros(1, np.int32), self.shape, (0, 0))
    with pytest.raises(ValueError, match='16777217 rows'):
        R.check(Big())


# ---- CLI ----------------------------------------------------------------------------------------------------------------------------------
def test_cli_parsing(capsys):
    args = clean.parser().parse_args(['--filedir', 'vox.ply'])
    assert (args.r2, args.min_neighbours, args.min_component, args.keep_largest, args.out) == (16, 0, 1, 0, None)
    args = clean.parser().parse_args(['--filedir', 'vox.ply', '--r2', '9', '--min_neighbours', '4', '--min_component', '8', '--keep_largest', '2',
                                      '--out', 'c.ply'])
    assert (args.r2, args.min_neighbours, args.min_component, args.keep_largest, args.out) == (9, 4, 8, 2, 'c.ply')
    for bad in (['--r2', '0'], ['--r2', '65'], ['--min_neighbours', '-1'], ['--min_component', '0'], ['--keep_largest', '-1'], ['--r2', 'four']):
        with pytest.raises(SystemExit):
            clean.main(['--filedir', 'vox.ply'] + bad)
    assert clean.parse_clean('4,8') == (4, 8) and clean.parse_clean('0,1') == (0, 1)
    args = coder._parse_cli(['--filedir', 'raw.ply', '--voxelize', '9', '--clean', '4,8', '--clean_r2', '9', '--keep_largest', '1', '--lossless'])
    assert (args.voxelize, args.clean, args.clean_r2, args.keep_largest, args.lossless) == (9, (4, 8), 9, 1, True)
    args = coder._parse_cli(['--filedir', 'vox.ply'])                          # without the flag nothing moves
    assert (args.clean, args.clean_r2, args.keep_largest, args.voxelize, args.res) == (None, 16, 0, None, 1024)
    args = vox.parser().parse_args(['--filedir', 'raw.ply', '--bits', '7', '--clean', '2,3'])
    assert (args.clean, args.clean_r2, args.keep_largest) == ((2, 3), 16, 0)
    for bad in (['--clean', '4'], ['--clean', '4,0'], ['--clean', '-1,2'], ['--clean', 'a,b'], ['--clean', '4,8', '--clean_r2', '0'],
                ['--clean', '4,8', '--clean_r2', '65'], ['--clean', '4,8', '--keep_largest', '-1'], ['--keep_largest', '2'], ['--clean_r2', '9']):
        with pytest.raises(SystemExit):
            coder._parse_cli(['--filedir', 'vox.ply'] + bad)
        with pytest.raises(SystemExit):
            attributes.main(['--filedir', 'vox.ply', '--qstep', '0'] + bad)
        with pytest.raises(SystemExit):
            vox.main(['--filedir', 'raw.ply', '--bits', '7'] + bad)
    capsys.readouterr()


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------------
EXPORTS = ('pcgc_clean_neighbours', 'pcgc_components_workspace_bytes', 'pcgc_components', 'pcgc_clean_expand', 'pcgc_clean_select_workspace_bytes',
           'pcgc_clean_select', 'pcgc_clean_compact_colours')


def test_exports_and_refusals_before_anything_is_touched():
    import ctypes
    L = _lib.lib()
    for name in EXPORTS:
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    err = lambda: L.pcgc_last_error().decode()
    p = 64                                                                     # a pointer that is not null and must never be followed
    n_comp, rounds = ctypes.c_int64(7), ctypes.c_int32(7)
    refs = (ctypes.byref(n_comp), ctypes.byref(rounds))
    need = int(L.pcgc_components_workspace_bytes(1000))
    assert need >= 4000 and int(L.pcgc_components_workspace_bytes(0)) > 0
    assert L.pcgc_components(p, -1, p, p, *refs, p, need, None) == -2 and 'row count' in err()
    assert L.pcgc_components(p, (1 << 24) + 1, p, p, *refs, p, 1 << 40, None) == -2 and 'row count' in err()
    assert L.pcgc_components(p, 1000, p, p, *refs, p, need - 1, None) == -2 and 'too small' in err()
    for hole in range(3):
        a = [p, p, p]
        a[hole] = None
        assert L.pcgc_components(a[0], 1000, a[1], a[2], *refs, p, need, None) == -2 and 'null' in err()
    assert L.pcgc_components(p, 1000, p, p, *refs, None, need, None) == -2 and 'null' in err()
    assert L.pcgc_components(p, 1000, p, p, None, refs[1], p, need, None) == -2 and L.pcgc_components(p, 1000, p, p, refs[0], None, p, need, None) == -2
    assert (n_comp.value, rounds.value) == (7, 7)               # nothing was written
    nb = lambda n=10, r2=16, k=0, cap=16, hole=None: L.pcgc_clean_neighbours(*[None if j == hole else p for j in range(2)], n,
                                                                           *[None if j + 2 == hole else p for j in range(2)], cap,
                                                                           *[None if j + 4 == hole else p for j in range(3)], r2, k,
                                                                           *[None if j + 7 == hole else p for j in range(3)], None)
    assert nb(n=-1) == -2 and nb(n=(1 << 24) + 1) == -2 and nb(r2=0) == -2 and nb(r2=65) == -2 and nb(k=-1) == -2 and nb(cap=12) == -2 and nb(cap=0) == -2
    for hole in range(10):
        assert nb(hole=hole) == -2 and 'null' in err(), hole
    assert L.pcgc_clean_expand(p, p, p, p, p, -1, 0, p, p, None) == -2 and L.pcgc_clean_expand(p, p, p, p, p, 5, 6, p, p, None) == -2
    assert L.pcgc_clean_expand(None, p, p, p, p, 5, 5, p, p, None) == -2 and L.pcgc_clean_expand(p, p, None, p, p, 5, 5, p, p, None) == -2
    assert L.pcgc_clean_expand(p, p, p, p, p, 5, 5, None, p, None) == -2
    need = int(L.pcgc_clean_select_workspace_bytes(1000))
    assert need >= 17000
    assert L.pcgc_clean_select(p, p, p, -1, 1, 0, p, p, need, None) == -2 and L.pcgc_clean_select(p, p, p, 1000, 0, 0, p, p, need, None) == -2
    assert L.pcgc_clean_select(p, p, p, 1000, 1, -1, p, p, need, None) == -2
    assert L.pcgc_clean_select(p, p, p, 1000, 1, 0, p, p, need - 1, None) == -2 and 'too small' in err()
    assert L.pcgc_clean_select(None, p, p, 1000, 1, 0, p, p, need, None) == -2 and L.pcgc_clean_select(p, p, p, 1000, 1, 0, None, p, need, None) == -2
    assert L.pcgc_clean_select(p, p, p, 1000, 1, 0, p, None, need, None) == -2 and L.pcgc_clean_select(p + 4, p, p, 1000, 1, 0, p, p, need, None) == -2
    assert L.pcgc_clean_compact_colours(p, p, p, -1, p, None) == -2 and L.pcgc_clean_compact_colours(None, p, p, 5, p, None) == -2
    assert L.pcgc_clean_compact_colours(p, p, p, 5, None, None) == -2
