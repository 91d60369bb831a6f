"""pcgcv2_amd.data_loader on the host: the sampler's order, the collate function, the dataset's cache, the loader's length / order /
determinism / thread independence, the 48 symmetries against their numpy definition (restated HERE, not imported), and the CLI flags."""
import itertools
import os

import numpy as np
import pytest
import torch

from pcgcv2_amd import data_loader as dl
from pcgcv2_amd import train
from pcgcv2_amd.data_utils import read_h5_geo, write_h5_geo, write_ply_ascii_geo


def symmetry(v, s):
    """the issue's definition: perm = s % 6 into itertools.permutations(range(3)), flips = s // 6, e = the largest coordinate"""
    perm, flips, e = list(itertools.permutations(range(3)))[s % 6], s // 6, v.max()
    w = v.copy()
    for a in range(3):
        if flips >> a & 1:
            w[:, a] = e - v[:, a]
    return w[:, perm]


def cloud(i, n=40):
    """an asymmetric cloud of n distinct rows: no symmetry of the cube maps it to itself"""
    rng = np.random.default_rng(100 + i)
    pts = np.unique(rng.integers(0, 30 + i, (n, 3)) * np.array([1, 2, 3]) + np.array([0, 1, 5]), axis=0)
    return pts[rng.permutation(len(pts))].astype(np.int64)


@pytest.fixture
def files(tmp_path):
    def make(n, start=0):
        out = []
        for i in range(start, start + n):
            path = str(tmp_path / f'c{i:02d}.ply')
            write_ply_ascii_geo(path, cloud(i))
            out.append(path)
        return out
    return make


def batches(loader, limit=None):
    out = []
    for k, (c, f) in enumerate(loader):
        if limit is not None and k >= limit:
            break
        out.append((c.clone(), f.clone()))
    return out


def same(a, b):
    return len(a) == len(b) and all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(a, b))


def clouds_of(batch):
    c = batch[0].numpy()
    return [c[c[:, 0] == b, 1:] for b in range(int(c[:, 0].max()) + 1)]


# ---- InfSampler -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 2, 7])
def test_inf_sampler_order(n):
    source = list(range(n))
    torch.manual_seed(5)
    sampler = dl.InfSampler(source, shuffle=True)
    got = [next(sampler) for _ in range(2 * n + 1)]
    torch.manual_seed(5)
    want, perm = [], []
    for _ in range(2 * n + 1):
        if not perm:
            perm = torch.randperm(n).tolist()
        want.append(perm.pop())
    assert got == want
    assert len(sampler) == n and iter(sampler) is sampler
    plain = dl.InfSampler(source, shuffle=False)
    assert [next(plain) for _ in range(2 * n + 1)] == (list(range(n - 1, -1, -1)) * 3)[:2 * n + 1]


# ---- collate_pointcloud_fn ------------------------------------------------------------------------------------------------------------
def test_collate_drops_none_and_counts_kept_items():
    a, b = cloud(0), cloud(1)
    ones = lambda c: np.ones((len(c), 1), np.float32)
    coords, feats = dl.collate_pointcloud_fn([None, (a, ones(a)), None, (b, ones(b))])
    assert coords.dtype == torch.int32 and coords.shape == (len(a) + len(b), 4)
    assert feats.dtype == torch.float32 and feats.shape == (len(a) + len(b), 1) and bool((feats == 1).all())
    assert coords[:, 0].tolist() == [0] * len(a) + [1] * len(b)
    assert np.array_equal(coords[:, 1:].numpy(), np.concatenate([a, b]))
    with pytest.raises(ValueError, match='No data in the batch'):
        dl.collate_pointcloud_fn([None, None])
    with pytest.raises(ValueError, match='No data in the batch'):
        dl.collate_pointcloud_fn([])


# ---- PCDataset ------------------------------------------------------------------------------------------------------------------------
def test_dataset_caches_after_the_first_read(files):
    paths = files(2)
    ds = dl.PCDataset(paths)
    assert len(ds) == 2
    coords, feats = ds[1]
    assert np.array_equal(coords, cloud(1)) and np.issubdtype(coords.dtype, np.integer) and coords.shape[1] == 3
    assert feats.dtype == np.float32 and feats.shape == (len(coords), 1) and (feats == 1).all()
    os.remove(paths[1])
    again, _ = ds[1]
    assert np.array_equal(again, coords)
    os.remove(paths[0])
    with pytest.raises(FileNotFoundError):
        ds[0]


def test_dataset_refuses_an_unknown_suffix(tmp_path):
    path = str(tmp_path / 'cloud.xyz')
    open(path, 'w').write('1 2 3\n')
    with pytest.raises(ValueError, match='cloud.xyz'):
        dl.PCDataset([path])[0]


def test_h5_without_h5py_names_it(tmp_path):
    try:
        import h5py  # noqa: F401
    except ImportError:
        pass
    else:
        pytest.skip('h5py is installed: the round trip runs instead')
    with pytest.raises(ImportError, match='h5py'):
        dl.PCDataset([str(tmp_path / 'a.h5')])[0]
    with pytest.raises(ImportError, match='h5py'):
        write_h5_geo(str(tmp_path / 'a.h5'), cloud(0))


def test_h5_round_trip(tmp_path):
    pytest.importorskip('h5py')
    pts = cloud(0)
    path = str(tmp_path / 'a.h5')
    write_h5_geo(path, pts)
    assert np.array_equal(read_h5_geo(path), pts.astype('uint8').astype('int'))
    coords, feats = dl.PCDataset([path])[0]
    assert np.array_equal(coords, pts) and feats.shape == (len(pts), 1)


# ---- the loader on the host route -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 5, 16])
@pytest.mark.parametrize('batch_size', [1, 2, 16])
def test_len_and_one_pass_visits_every_cloud_once(files, n, batch_size):
    loader = dl.make_data_loader(dl.PCDataset(files(n)), batch_size=batch_size, shuffle=True, num_workers=0)
    assert len(loader) == -(-n // batch_size)
    got = batches(loader)
    assert len(got) == len(loader)
    seen = sorted(c.tobytes() for b in got for c in clouds_of(b))
    assert seen == sorted(cloud(i).astype(np.int32).tobytes() for i in range(n))
    assert all(len(clouds_of(b)) == batch_size for b in got[:-1])
    plain = batches(dl.make_data_loader(dl.PCDataset(files(n)), batch_size=batch_size, shuffle=False, num_workers=0))
    assert [c.tobytes() for b in plain for c in clouds_of(b)] == [cloud(i).astype(np.int32).tobytes() for i in range(n)]


@pytest.mark.parametrize('augment', [False, True])
def test_equal_seeds_and_any_worker_count_give_the_same_batches(files, augment):
    paths = files(7)
    runs = []
    for workers in (0, 4, 0):
        loader = dl.make_data_loader(dl.PCDataset(paths), batch_size=2, shuffle=True, num_workers=workers, augment=augment,
                                     generator=torch.Generator().manual_seed(11))
        runs.append(batches(loader) + batches(loader))              # two epochs: the second from the host cache
    assert same(runs[0], runs[1]) and same(runs[0], runs[2])
    assert not same(runs[0][:4], runs[0][4:])                       # (the second epoch is another permutation)
    other = dl.make_data_loader(dl.PCDataset(paths), batch_size=2, shuffle=True, num_workers=0, augment=augment,
                                generator=torch.Generator().manual_seed(12))
    assert not same(runs[0][:4], batches(other))


@pytest.mark.parametrize('workers', [0, 4])
def test_repeat_never_stops(files, workers):
    loader = dl.make_data_loader(dl.PCDataset(files(5)), batch_size=2, shuffle=False, num_workers=workers, repeat=True)
    got = batches(loader, limit=3 * len(loader) + 1)
    assert len(got) == 3 * len(loader) + 1
    order = [c.tobytes() for b in got for c in clouds_of(b)]
    want = [cloud(i).astype(np.int32).tobytes() for i in ([4, 3, 2, 1, 0] * 4)[:len(order)]]
    assert order == want                                            # (InfSampler without shuffle; batches run across its redraws)


def test_batch_size_17_raises_before_any_file_is_opened(tmp_path):
    ds = dl.PCDataset([str(tmp_path / 'missing.ply')])
    with pytest.raises(ValueError, match='batch_size'):
        dl.make_data_loader(ds, batch_size=17)
    with pytest.raises(ValueError, match='batch_size'):
        dl.make_data_loader(ds, batch_size=0)
    assert ds.cache == {}


def test_worker_count_is_capped_and_threads_end(files):
    import threading
    loader = dl.make_data_loader(dl.PCDataset(files(3)), batch_size=1, num_workers=64)
    assert loader.num_workers == 16
    it = iter(loader)
    next(it)
    it.close()
    assert not [t for t in threading.enumerate() if t.name.startswith('pcgc-loader')]


def test_augment_is_the_stated_symmetry_for_all_48_codes(files):
    paths = files(16)
    gen = torch.Generator().manual_seed(3)
    loader = dl.make_data_loader(dl.PCDataset(paths), batch_size=16, shuffle=False, num_workers=0, augment=True, generator=gen)
    mirror = torch.Generator().manual_seed(3)
    seen = set()
    for _ in range(40):                                             # 640 draws: all 48 codes turn up (checked below)
        (coords, feats), = batches(loader)
        codes = torch.randint(48, (16,), generator=mirror).tolist()
        seen.update(codes)
        for i, (got, s) in enumerate(zip(clouds_of((coords, feats)), codes)):
            assert np.array_equal(got, symmetry(cloud(i), s)), (i, s)
        assert bool((feats == 1).all())
    assert seen == set(range(48))
    # every code on one cloud, and: the 48 images of an asymmetric cloud are 48 different clouds
    v = cloud(0)
    images = [dl.apply_symmetry(v, s) for s in range(48)]
    assert all(np.array_equal(images[s], symmetry(v, s)) for s in range(48))
    assert len({np.unique(im, axis=0).tobytes() for im in images}) == 48
    assert np.array_equal(images[0], v) and all(im.min() >= 0 and im.max() <= v.max() for im in images)


def test_augment_refuses_a_negative_coordinate(tmp_path):
    path = str(tmp_path / 'neg.ply')
    write_ply_ascii_geo(path, np.array([[3, -1, 2], [0, 4, 5]]))
    loader = dl.make_data_loader(dl.PCDataset([path]), batch_size=1, shuffle=False, num_workers=0, augment=True)
    with pytest.raises(ValueError, match='negative'):
        next(iter(loader))
    (coords, _), = batches(dl.make_data_loader(dl.PCDataset([path]), batch_size=1, shuffle=False, num_workers=0))
    assert coords.tolist() == [[0, 3, -1, 2], [0, 0, 4, 5]]       # (legal without augment)


def test_pack_cloud_picks_the_narrowest_width():
    for hi, lo, width in [(255, 0, 1), (256, 0, 2), (65535, 0, 2), (65536, 0, 4), (2 ** 20 - 1, 0, 4), (7, -1, 4)]:
        pts = np.array([[lo, 1, hi], [2, hi, 3]], dtype=np.int64)
        packed, w, got_lo, got_hi = dl.pack_cloud(pts)
        assert (w, got_lo, got_hi) == (width, min(lo, 1), hi) and packed.dtype == np.uint8 and len(packed) == 6 * width
        dtype = {1: np.uint8, 2: np.uint16, 4: np.int32}[width]
        assert np.array_equal(packed.view(dtype).reshape(-1, 3), pts)
    assert dl.pack_cloud(np.zeros((0, 3), np.int64))[1] == 1


# ---- the CLI --------------------------------------------------------------------------------------------------------------------------
def test_train_flags():
    args = train.parse_args([])
    assert (args.num_workers, args.device_cache, args.augment) == (0, False, False)
    args = train.parse_args(['--num_workers', '4', '--device_cache', '--augment'])
    assert (args.num_workers, args.device_cache, args.augment) == (4, True, True)
