"""Training data (reference data_loader.py): PCDataset, InfSampler, collate_pointcloud_fn and make_data_loader under the reference's names
and argument lists, plus what the reference leaves to torch.utils.data and this package does itself:

  * host route: clouds are parsed once into the dataset's host cache and collated by sparse_collate, as in the reference;
  * device route (device_cache=True): every cloud read so far lies packed in one uint8 arena on the GPU, and a batch is one launch of
    ops.collate_rows into fresh device tensors: after the first pass an epoch reads no file and copies nothing to the device;
  * augment=True: one of the 48 symmetries of the cube per batch item (`apply_symmetry`), the same definition on both routes.

`num_workers` counts host THREADS that parse files up to two batches ahead of the consumer (the native PLY parser runs outside the GIL).
No worker process is ever started: a forked child of a process that holds the GPU is not safe.  The batches do not depend on
`num_workers` or on thread timing: the order and the symmetry codes are drawn by the consuming thread, the threads only read files.
"""
import itertools
from collections import deque
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import ops
from .data_utils import read_h5_geo, read_ply_ascii_geo
from .sparse import sparse_collate

MAX_BATCH = 16                   # the coordinate key holds a 4-bit item index (ops.check_coords)
MAX_WORKERS = 16
LOOK_AHEAD = 2                   # batches whose files the threads may be parsing ahead of the consumer
ARENA_INITIAL_BYTES = 1 << 26    # the arena doubles from here
PERMS = tuple(itertools.permutations(range(3)))


class InfSampler:
    """An endless index iterator: pops from the end of a permutation of 0..n-1 and draws a new one when it is empty.  shuffle=True
    draws torch.randperm(n) (from `generator`, else the global one); shuffle=False uses 0..n-1, so the indices come as n-1 .. 0 again
    and again.  (The reference's InfSampler breaks with shuffle=False: it calls .tolist() on the integer n.)"""

    def __init__(self, data_source, shuffle=False, generator=None):
        self.data_source = data_source
        self.shuffle = shuffle
        self.generator = generator
        self.reset_permutation()

    def reset_permutation(self):
        n = len(self.data_source)
        self._perm = torch.randperm(n, generator=self.generator).tolist() if self.shuffle else list(range(n))

    def __iter__(self):
        return self

    def __next__(self):
        if len(self._perm) == 0:
            self.reset_permutation()
        return self._perm.pop()

    def __len__(self):
        return len(self.data_source)


def collate_pointcloud_fn(list_data):
    """[(coords [n, 3], feats [n, 1]) or None, ...] -> sparse_collate of the items that are not None: int32 [N, 4], float32 [N, 1]"""
    list_data = [data for data in list_data if data is not None]
    if len(list_data) == 0:
        raise ValueError('No data in the batch')
    coords, feats = list(zip(*list_data))
    return sparse_collate(coords, feats)


class PCDataset:
    """files -> (coords int [n, 3], feats float32 [n, 1] of ones); a cloud is read once and kept in a host cache."""

    def __init__(self, files):
        self.files = files
        self.cache = {}

    def __len__(self):
        return len(self.files)

    def read(self, idx):
        """the file's rows, past the cache"""
        filedir = self.files[idx]
        if filedir.endswith('.h5'):
            return read_h5_geo(filedir)
        if filedir.endswith('.ply'):
            return read_ply_ascii_geo(filedir)
        raise ValueError(f'{filedir}: a cloud is a .ply or an .h5 file')

    def __getitem__(self, idx):
        if idx not in self.cache:
            self.cache[idx] = self.read(idx)
        coords = self.cache[idx]
        return coords, np.ones((coords.shape[0], 1), dtype=np.float32)


def apply_symmetry(coords, code, extent=None):
    """Symmetry `code` (0..47) of the cube on int rows [n, 3]: perm = PERMS[code % 6], flips = code // 6; with e = `extent` (default: the
    largest coordinate over all three axes) a row v becomes w, w[a] = e - v[a] if flips >> a & 1 else v[a], then w[perm].  Exact on
    the lattice; coordinates stay in [0, e]."""
    coords = np.asarray(coords)
    if coords.size and coords.min() < 0:
        raise ValueError('augment: a cloud with a negative coordinate has no symmetry of the cube [0, e]^3')
    e = (int(coords.max()) if coords.size else 0) if extent is None else int(extent)
    perm, flips = PERMS[int(code) % 6], int(code) // 6
    w = coords.copy()
    for a in range(3):
        if flips >> a & 1:
            w[:, a] = e - coords[:, a]
    return w[:, list(perm)]


def pack_cloud(coords):
    """int rows [n, 3] -> (uint8 [3 n width] in file order, width, lowest, largest coordinate) at the narrowest of uint8 / uint16 / int32"""
    coords = np.asarray(coords).reshape(-1, 3)
    lo, hi = (int(coords.min()), int(coords.max())) if coords.size else (0, 0)
    if lo < -2 ** 31 or hi >= 2 ** 31:
        raise ValueError('a coordinate does not fit int32')
    dtype = np.uint8 if 0 <= lo and hi < 1 << 8 else np.uint16 if 0 <= lo and hi < 1 << 16 else np.int32
    packed = np.ascontiguousarray(coords, dtype=dtype)
    return packed.view(np.uint8).reshape(-1), packed.itemsize, lo, hi


class Arena:
    """Every cloud read so far, packed by pack_cloud, in ONE uint8 device tensor: clouds start on 16-byte boundaries, `table[idx]` =
    (byte offset, rows, width, lowest, extent) stays on the host, and a full arena doubles with a device-to-device copy."""

    def __init__(self, device, capacity=None):
        self.device = torch.device(device)
        self.buf = torch.empty(max(16, int(ARENA_INITIAL_BYTES if capacity is None else capacity)), dtype=torch.uint8, device=self.device)
        self.used, self.grown, self.table = 0, 0, {}

    def __contains__(self, idx):
        return idx in self.table

    def append(self, idx, packed, width, lo, hi):
        offset = -(-self.used // 16) * 16
        need = offset + len(packed)
        if need > self.buf.numel():
            capacity = self.buf.numel()
            while capacity < need:
                capacity *= 2
                self.grown += 1
            buf = torch.empty(capacity, dtype=torch.uint8, device=self.device)
            buf[:self.used].copy_(self.buf[:self.used])
            self.buf = buf
        if len(packed):
            self.buf[offset:need].copy_(torch.from_numpy(packed))
        self.used = need
        self.table[idx] = (offset, len(packed) // (3 * width), width, lo, hi)


class PointCloudLoader:
    """What make_data_loader returns: iterating yields (coords [N, 4], feats [N, 1]), the pairs Trainer.train / Trainer.test consume."""

    def __init__(self, dataset, batch_size, shuffle, num_workers, repeat, collate_fn, device_cache, augment, generator, device):
        self.batch_size = int(batch_size)
        if not 1 <= self.batch_size <= MAX_BATCH:
            raise ValueError(f'batch_size must be 1..{MAX_BATCH} (the coordinate key holds a 4-bit item index), got {batch_size}')
        if device_cache and collate_fn is not collate_pointcloud_fn:
            raise ValueError('device_cache=True collates on the GPU: it takes no collate_fn of the caller')
        self.dataset, self.shuffle, self.repeat, self.collate_fn = dataset, bool(shuffle), bool(repeat), collate_fn
        self.num_workers = max(0, min(int(num_workers), MAX_WORKERS))
        self.device_cache, self.augment, self.generator = bool(device_cache), bool(augment), generator
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None and device_cache else \
            (None if device is None else torch.device(device))
        self.sampler = InfSampler(dataset, self.shuffle, generator) if self.repeat else None
        self.arena = None

    def __len__(self):
        return (len(self.dataset) + self.batch_size - 1) // self.batch_size

    # ---- the plan: which clouds and which symmetries, drawn by the consuming thread alone
    def _plan(self):
        if self.repeat:
            batches = ([next(self.sampler) for _ in range(self.batch_size)] for _ in itertools.count()) if len(self.dataset) else iter(())
        else:
            n = len(self.dataset)
            order = torch.randperm(n, generator=self.generator).tolist() if self.shuffle else list(range(n))
            batches = (order[i:i + self.batch_size] for i in range(0, n, self.batch_size))
        for indices in batches:
            codes = torch.randint(48, (len(indices),), generator=self.generator).tolist() if self.augment else [0] * len(indices)
            yield indices, codes

    # ---- what a thread does: read one cloud (nothing, where the arena already holds it)
    def _load(self, idx):
        if not self.device_cache:
            return self.dataset[idx]
        if self.arena is not None and idx in self.arena:
            return None
        return pack_cloud(self.dataset.read(idx) if hasattr(self.dataset, 'read') else self.dataset[idx][0])

    # ---- what the consumer does with the loaded clouds of one batch
    def _deliver(self, indices, codes, loaded):
        if not self.device_cache:
            if self.augment:
                loaded = [(apply_symmetry(c, s), f) for (c, f), s in zip(loaded, codes)]
            coords, feats = self.collate_fn(loaded)
            return (coords, feats) if self.device is None else (coords.to(self.device), feats.to(self.device))
        if self.arena is None:
            self.arena = Arena(self.device)
        items = []
        for idx, code, packed in zip(indices, codes, loaded):
            if idx not in self.arena:
                self.arena.append(idx, *(packed if packed is not None else self._load(idx)))
            offset, rows, width, lo, hi = self.arena.table[idx]
            if self.augment and lo < 0:
                raise ValueError(f'augment: {self.dataset.files[idx] if hasattr(self.dataset, "files") else idx} has a negative coordinate')
            items.append((offset, rows, width, code, hi))
        return ops.collate_rows(self.arena.buf, items)

    def __iter__(self):
        plan = self._plan()
        if self.num_workers == 0:
            for indices, codes in plan:
                yield self._deliver(indices, codes, [self._load(i) for i in indices])
            return
        pool = ThreadPoolExecutor(max_workers=self.num_workers, thread_name_prefix='pcgc-loader')
        window = deque()
        try:
            while True:
                while len(window) <= LOOK_AHEAD:
                    step = next(plan, None)
                    if step is None:
                        break
                    window.append((step[0], step[1], [pool.submit(self._load, i) for i in step[0]]))
                if not window:
                    return
                indices, codes, futures = window.popleft()
                yield self._deliver(indices, codes, [f.result() for f in futures])
        finally:
            pool.shutdown(wait=True, cancel_futures=True)


def make_data_loader(dataset, batch_size=1, shuffle=True, num_workers=1, repeat=False, collate_fn=collate_pointcloud_fn, *,
                     device_cache=False, augment=False, generator=None, device=None):
    """data_loader.py:90-105 -> a PointCloudLoader (not a torch DataLoader).  len() = ceil(len(dataset) / batch_size), no drop_last.
    repeat=True never stops (InfSampler); otherwise every iter() is one pass in the order torch.randperm(n, generator=generator) if
    shuffle else 0..n-1.  num_workers: host threads parsing ahead (0: the consumer parses; at most 16; never processes).
    device_cache: batches come out of a device-resident arena as device tensors (`device`, default the current one).  augment: one of
    the 48 symmetries of the cube per batch item, torch.randint(48, (B,), generator=generator) per batch."""
    return PointCloudLoader(dataset, batch_size, shuffle, num_workers, repeat, collate_fn, device_cache, augment, generator, device)
