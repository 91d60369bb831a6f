"""The device-resident route of pcgcv2_amd.data_loader: ops.collate_rows against sparse_collate of the host arrays (exact), the 48
symmetries at every packing width against their numpy definition (restated here), the device-cache loader against the host loader
batch for batch, the arena's growth, and `python -m pcgcv2_amd.train --device_cache --augment` end to end."""
import glob
import itertools
import math
import os
import re

import numpy as np
import pytest
import torch

from pcgcv2_amd import data_loader as dl
from pcgcv2_amd import ops, synthetic, train
from pcgcv2_amd.data_utils import write_ply_ascii_geo
from pcgcv2_amd.pcc_model import PCCModel
from pcgcv2_amd.sparse import SparseTensor, sparse_collate

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
SENTINEL_I, SENTINEL_F, GUARD = -7777, -3.5, 64


def symmetry(v, s):
    """the stated definition: perm = s % 6 into itertools.permutations(range(3)), flips = s // 6, e = the largest coordinate"""
    perm, flips, e = list(itertools.permutations(range(3)))[s % 6], s // 6, v.max()
    w = v.copy()
    for a in range(3):
        if flips >> a & 1:
            w[:, a] = e - v[:, a]
    return w[:, perm]


def rows_at(width, n, seed):
    """n rows whose values span the width; the first rows carry its extremes, each on every axis in turn, and row 0 alone forces the width"""
    rng = np.random.default_rng(seed)
    lo, hi = {1: (0, 255), 2: (0, 65535), 4: (-5, 2 ** 20 - 1)}[width]
    pts = rng.integers(lo, hi + 1, (n, 3), dtype=np.int64)
    marks = {1: [255, 0, 17], 2: [65535, 256, 0, 255], 4: [-5, 2 ** 20 - 1, 65536, 65535, 256, 255, 0]}[width]
    for k in range(min(n, len(marks))):
        pts[k] = np.roll([marks[k], marks[(k + 1) % len(marks)], marks[(k + 2) % len(marks)]], k)
    return pts


class HostArena:
    """clouds packed as the loader packs them, behind `lead` bytes of another cloud, uploaded once"""

    def __init__(self, clouds, lead=48):
        self.clouds, self.items, chunks, used = clouds, [], [np.full(lead, 0xAB, np.uint8)], lead
        for c in clouds:
            packed, width, lo, hi = dl.pack_cloud(c)
            pad = -used % 16
            chunks.append(np.zeros(pad, np.uint8))
            self.items.append((used + pad, len(c), width, hi))
            chunks.append(packed)
            used += pad + len(packed)
        self.buf = torch.from_numpy(np.concatenate(chunks)).to(DEV)

    def collate(self, picks, codes=None):
        codes = [0] * len(picks) if codes is None else codes
        items = [(self.items[p][0], self.items[p][1], self.items[p][2], s, self.items[p][3]) for p, s in zip(picks, codes)]
        n = sum(i[1] for i in items)
        coords = torch.full((n + GUARD, 4), SENTINEL_I, dtype=torch.int32, device=DEV)
        feats = torch.full((n + GUARD, 1), SENTINEL_F, dtype=torch.float32, device=DEV)
        got = ops.collate_rows(self.buf, items, out=(coords, feats))
        assert got[0].shape == (n, 4) and got[1].shape == (n, 1)
        assert bool((coords[n:] == SENTINEL_I).all()) and bool((feats[n:] == SENTINEL_F).all()), 'rows past N were written'
        fresh = ops.collate_rows(self.buf, items)
        assert torch.equal(fresh[0], got[0]) and torch.equal(fresh[1], got[1])
        return got[0].cpu(), got[1].cpu()

    def expect(self, picks, codes=None):
        codes = [0] * len(picks) if codes is None else codes
        clouds = [symmetry(self.clouds[p], s) if s else self.clouds[p] for p, s in zip(picks, codes)]
        return sparse_collate(clouds, [np.ones((len(c), 1), np.float32) for c in clouds])


@pytest.fixture(scope='module')
def arena():
    """clouds 0..17: every row count of {1, 63, 64, 65, 257, 4099} at every width"""
    return HostArena([rows_at(w, n, 10 * w + k) for w in (1, 2, 4) for k, n in enumerate((1, 63, 64, 65, 257, 4099))])


PICKS = {
    'one-item': [5],
    'one-row': [0],
    'two-items-mixed-widths': [9, 3],
    'same-cloud-twice': [2, 2],
    'same-cloud-twice-between': [14, 1, 14],
    'sixteen-items': [0, 6, 12, 1, 7, 13, 2, 8, 14, 3, 9, 15, 4, 10, 16, 17],
    'sixteen-single-rows': [0, 6, 12] * 5 + [0],
}


@pytest.mark.parametrize('name', list(PICKS))
def test_collate_rows_equals_sparse_collate(arena, name):
    picks = PICKS[name]
    coords, feats = arena.collate(picks)
    want_c, want_f = arena.expect(picks)
    assert coords.dtype == torch.int32 and feats.dtype == torch.float32
    assert torch.equal(coords, want_c) and torch.equal(feats, want_f)
    assert bool((feats == 1.0).all())


def test_collate_rows_reads_the_extremes_of_every_width(arena):
    seen = set(np.unique(arena.collate(PICKS['sixteen-items'])[0][:, 1:].numpy()).tolist())
    assert {0, 255, 256, 65535, 65536, 2 ** 20 - 1, -5} <= seen
    assert [i[2] for i in arena.items] == [1] * 6 + [2] * 6 + [4] * 6 and all(i[0] % 16 == 0 and i[0] > 0 for i in arena.items)


def test_collate_rows_launches_nothing_for_nothing(arena):
    coords, feats = ops.collate_rows(arena.buf, [])
    assert coords.shape == (0, 4) and feats.shape == (0, 1) and coords.dtype == torch.int32 and feats.dtype == torch.float32
    coords, feats = ops.collate_rows(arena.buf, [(16, 0, 1, 0, 0), (32, 0, 4, 0, 0)])
    assert coords.shape == (0, 4) and feats.shape == (0, 1)
    empty_between = [(arena.items[1][0], 63, 1, 0, 255), (16, 0, 2, 0, 0), (arena.items[7][0], 63, 2, 0, 65535)]
    coords, _ = ops.collate_rows(arena.buf, empty_between)
    assert coords[:, 0].tolist() == [0] * 63 + [2] * 63            # (an item without rows still counts in the batch column)


def test_collate_rows_refuses_items_outside_the_arena(arena):
    n = arena.buf.numel()
    for item in [(n - 16, 4099, 4, 0, 0), (8, 1, 1, 0, 0), (0, 1, 3, 0, 0), (0, -1, 1, 0, 0), (-16, 1, 1, 0, 0)]:
        with pytest.raises(ops.PcgcError):
            ops.collate_rows(arena.buf, [item])
    with pytest.raises(ValueError):
        ops.collate_rows(arena.buf, [(0, 1, 1, 48, 0)])
    with pytest.raises(ValueError):
        ops.collate_rows(arena.buf, [(0, 1, 1, 0, 0)] * 17)


@pytest.mark.parametrize('width', [1, 2, 4])
def test_all_48_symmetries_at_each_width(width):
    base = rows_at(width, 65, 7)
    base[base < 0] = 3                                             # (a symmetry needs coordinates >= 0)
    assert dl.pack_cloud(base)[1] == width
    assert len({np.unique(symmetry(base, s), axis=0).tobytes() for s in range(48)}) == 48, 'the cloud is not asymmetric'
    a = HostArena([base])
    for first in range(0, 48, 16):
        codes = list(range(first, first + 16))
        coords, feats = a.collate([0] * 16, codes)
        want_c, want_f = a.expect([0] * 16, codes)
        assert torch.equal(coords, want_c) and torch.equal(feats, want_f)


# ---- the loader -----------------------------------------------------------------------------------------------------------------------
def small_cloud(i):
    rng = np.random.default_rng(200 + i)
    n = [1, 63, 64, 65, 257, 700, 5, 130, 1000, 300][i]
    pts = rng.integers(0, 40 + 3 * i, (n, 3)) * np.array([1, 2, 3]) + np.array([0, 1, 5])
    if i == 3:
        pts = np.concatenate([pts, pts[::2], pts[:5]])             # duplicate rows (SparseTensor collapses them)
    if i == 4:
        pts = pts[np.lexsort((pts[:, 0], pts[:, 1], pts[:, 2]))][::-1]       # sorted backwards
    if i == 7:
        pts = pts + np.array([70000, 300, 0])                      # wider than 8 (and 16) bits
    if i == 8:
        pts = pts + np.array([0, 300, 0])                          # 16 bits
    return np.ascontiguousarray(pts, dtype=np.int64)


@pytest.fixture
def ply_files(tmp_path):
    paths = []
    for i in range(10):
        paths.append(str(tmp_path / f'c{i}.ply'))
        write_ply_ascii_geo(paths[-1], small_cloud(i))
    return paths


def run(loader, epochs=2):
    return [[(c.cpu(), f.cpu(), c.device.type) for c, f in loader] for _ in range(epochs)]


def tensor_of(coords, feats):
    """Trainer._tensor's recipe"""
    return SparseTensor(features=torch.as_tensor(feats).float(), coordinates=torch.as_tensor(coords), tensor_stride=1, device=DEV)


@pytest.mark.parametrize('augment', [False, True], ids=['plain', 'augment'])
@pytest.mark.parametrize('shuffle', [False, True], ids=['ordered', 'shuffled'])
@pytest.mark.parametrize('batch_size', [1, 3, 16])
def test_device_cache_loader_equals_host_loader(ply_files, batch_size, shuffle, augment):
    make = lambda device_cache, workers: dl.make_data_loader(
        dl.PCDataset(ply_files), batch_size=batch_size, shuffle=shuffle, num_workers=workers, device_cache=device_cache, augment=augment,
        generator=torch.Generator().manual_seed(21), device=DEV if device_cache else None)
    host, device = run(make(False, 0)), run(make(True, 2))
    for h_epoch, d_epoch in zip(host, device):
        assert len(h_epoch) == len(d_epoch) == math.ceil(10 / batch_size)
        for (hc, hf, _), (dc, df, where) in zip(h_epoch, d_epoch):
            assert where == 'cuda' and dc.dtype == torch.int32 and df.dtype == torch.float32
            assert torch.equal(hc, dc) and torch.equal(hf, df)
    if batch_size == 3:                                            # the tensors the trainer builds from either route are the same
        loader = make(True, 0)
        for (hc, hf, _), (dc, df) in zip(host[0], loader):
            xh, xd = tensor_of(hc, hf), tensor_of(dc, df)
            assert len(xh) == len(xd) and torch.equal(xh.C, xd.C) and xh.has_unit_features() and xd.has_unit_features()
            assert len(xd) <= len(dc)
        assert any(len(tensor_of(c, f)) < len(c) for c, f, _ in host[0]), 'no batch holds the cloud with duplicate rows'


def test_second_epoch_reads_no_file(ply_files):
    loader = dl.make_data_loader(dl.PCDataset(ply_files), batch_size=3, shuffle=False, num_workers=2, device_cache=True, device=DEV)
    first = [(c.cpu(), f.cpu()) for c, f in loader]
    for path in ply_files:
        os.remove(path)
    second = [(c.cpu(), f.cpu()) for c, f in loader]
    assert len(first) == len(second) == 4
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(first, second))
    assert loader.dataset.cache == {}                              # (the device route keeps no second copy on the host)


def test_arena_doubles_and_keeps_every_cloud(ply_files, monkeypatch):
    monkeypatch.setattr(dl, 'ARENA_INITIAL_BYTES', 256)
    loader = dl.make_data_loader(dl.PCDataset(ply_files), batch_size=1, shuffle=False, num_workers=0, device_cache=True, device=DEV)
    list(loader)
    assert loader.arena.grown >= 2 and loader.arena.buf.numel() >= loader.arena.used
    assert all(offset % 16 == 0 for offset, *_ in loader.arena.table.values())
    assert [loader.arena.table[i][2] for i in range(10)] == [dl.pack_cloud(small_cloud(i))[1] for i in range(10)]
    assert {loader.arena.table[i][2] for i in range(10)} == {1, 2, 4}
    for i, (coords, feats) in enumerate(loader):                   # after all the growth: every cloud is still its file's rows
        assert np.array_equal(coords.cpu().numpy()[:, 1:], small_cloud(i)) and bool((coords[:, 0] == 0).all())
        assert bool((feats == 1).all()) and feats.shape == (len(small_cloud(i)), 1)


def test_device_cache_refuses_a_negative_coordinate_under_augment(tmp_path):
    path = str(tmp_path / 'neg.ply')
    write_ply_ascii_geo(path, np.array([[3, -1, 2], [0, 4, 5]]))
    loader = dl.make_data_loader(dl.PCDataset([path]), batch_size=1, shuffle=False, num_workers=0, device_cache=True, augment=True, device=DEV)
    with pytest.raises(ValueError, match='negative'):
        next(iter(loader))
    plain = dl.make_data_loader(dl.PCDataset([path]), batch_size=1, shuffle=False, num_workers=0, device_cache=True, device=DEV)
    assert next(iter(plain))[0].tolist() == [[0, 3, -1, 2], [0, 0, 4, 5]]


# ---- the CLI --------------------------------------------------------------------------------------------------------------------------
def test_train_main_with_device_cache_and_augment(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    os.makedirs('clouds')
    for i in range(6):                                             # six shells of shell6's size, each another surface
        pts = synthetic._shell(64, 15.0 + 0.5 * i, 1.1, (3 + i % 2, 5 - i % 3)).numpy()
        write_ply_ascii_geo(os.path.join('clouds', f's{i}.ply'), pts)
    train.main(['--dataset', os.path.join('clouds', '*.ply'), '--epoch', '1', '--batch_size', '2', '--device_cache', '--augment',
                '--prefix', 't'])
    ckpt = torch.load(os.path.join('ckpts', 't', 'epoch_0.pth'), map_location='cpu')
    PCCModel().load_state_dict(ckpt['model'])
    log = open(os.path.join('logs', 't', 'log.txt')).read()
    for tag in ('Train Epoch 0', 'Test Epoch 1'):                   # (Trainer.train counts the epoch up before Trainer.test records)
        block = log.split('=' * 10 + tag)[1]
        for key in ('bce', 'bpp'):
            value = float(re.search(r': ' + key + r': ([-+.\deEnaif]+)', block).group(1))
            assert math.isfinite(value) and value > 0, (tag, key, value)
    assert len(glob.glob(os.path.join('clouds', '*.ply'))) == 6
