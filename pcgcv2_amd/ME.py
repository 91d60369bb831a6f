"""The part of MinkowskiEngine's Python surface that PCGCv2 touches, on the HIP operator set — `import pcgcv2_amd.ME as ME`.

The product's own network (pcgcv2_amd/autoencoder.py) fuses ReLU / bias / residual / concat into the producing kernels and never
goes through this module.  It exists so that code written against ME — the reference's `autoencoder.py` as it stands
(`ME.MinkowskiConvolution(in_channels=..., dimension=3)`, `ME.MinkowskiReLU(inplace=True)`, `ME.cat(a, b) + x`,
`ME.MinkowskiPruning()(data, mask)`), `data_utils.py` (`ME.SparseTensor(...)`, `ME.utils.sparse_collate`) — binds to the operators
unmodified.  Same results as the fused graph, bit for bit (tests/test_gpu_parity.py::test_me_facade_unfused_graph_equals_fused).

`ME.SparseTensor(features=, coordinate_map_key=, coordinate_manager=)` (pcc_model.py:18-23: a tensor that shares another's coordinates)
binds too: the key of a tensor is its coordinate level (sparse.CoordMap) and the manager a token that only has to be handed back.

Not provided: MinkowskiEngine's other layers.  The layers of this module record no autograd graph; the backward pass of the same
unfused operators lives in pcgcv2_amd/grad.py (`PCCModel.forward_train`), which pcgcv2_amd/trainer.py drives."""
import torch

from . import ops
from .nn import MinkowskiConvolution, MinkowskiGenerativeConvolutionTranspose          # noqa: F401  (ME-compatible parameters)
from .nn import MinkowskiPruning as _Pruning
from .sparse import SparseTensor as _SparseTensor, sparse_collate as _sparse_collate

__version__ = '0.5.4-pcgcv2_amd'


class _CoordinateManager:
    def __repr__(self):
        return 'CoordinateManager(pcgcv2_amd: the levels own their maps)'


COORDINATE_MANAGER = _CoordinateManager()


class SparseTensor(_SparseTensor):
    """ME.SparseTensor(features=, coordinates=, tensor_stride=, device=) plus the two operators autoencoder.py:55 applies to it."""

    def __init__(self, features, coordinates=None, tensor_stride=1, device=None, coordinate_map=None, assume_unique=False,
                 coordinate_map_key=None, coordinate_manager=None):
        if coordinate_map_key is not None:                       # share the coordinates of the tensor the key was taken from
            if coordinates is not None or coordinate_map is not None:
                raise ValueError('ME.SparseTensor: give coordinates or a coordinate_map_key, not both')
            if coordinate_manager is not None and coordinate_manager is not COORDINATE_MANAGER:
                raise ValueError('ME.SparseTensor: foreign coordinate_manager')
            coordinate_map = coordinate_map_key
        super().__init__(features, coordinates=coordinates, tensor_stride=tensor_stride, device=device, coordinate_map=coordinate_map,
                         assume_unique=assume_unique)

    @property
    def coordinate_map_key(self):
        """the tensor's coordinate level: what ME calls a coordinate-map key (pcc_model.py:20)"""
        return self.cmap

    @property
    def coordinate_manager(self):
        """ME keeps every level in one manager object; here each level owns its tables, so the manager is a token (pcc_model.py:21)"""
        return COORDINATE_MANAGER

    def __add__(self, other):
        if len(self) != len(other) or self.cmap is not other.cmap and not torch.equal(self.C, other.C):
            raise ValueError('SparseTensor + SparseTensor: the operands live on different coordinate levels')
        return SparseTensor(ops.add(self.F, other.F), coordinate_map=self.cmap)

    @property
    def _batchwise_row_indices(self):
        """row indices per batch item (data_utils.py:84 uses it in istopk)"""
        out, off = [], 0
        for r in self.cmap.batch_rows:
            out.append(torch.arange(off, off + r, device=self.device))
            off += r
        return out

    @property
    def decomposed_coordinates(self):
        """per batch item, its coordinates without the batch column (pcc_model.py:30)"""
        out, off = [], 0
        for r in self.cmap.batch_rows:
            out.append(self.C[off:off + r, 1:])
            off += r
        return out


def _wrap(x):
    """operator results are plain sparse tensors; hand them on as ME-style ones"""
    if isinstance(x, SparseTensor):
        return x
    y = SparseTensor.__new__(SparseTensor)
    y.__dict__.update(x.__dict__)
    return y


def _lift(cls):
    class Lifted(cls):
        def forward(self, *a, **k):
            return _wrap(super().forward(*a, **k))
    Lifted.__name__ = Lifted.__qualname__ = cls.__name__
    return Lifted


MinkowskiConvolution = _lift(MinkowskiConvolution)
MinkowskiGenerativeConvolutionTranspose = _lift(MinkowskiGenerativeConvolutionTranspose)


class MinkowskiPruning(_Pruning):
    """ME.MinkowskiPruning()(x, mask): keeps the rows where the boolean mask is set, order preserved (autoencoder.py:237,247)."""

    def forward(self, x, mask):
        m = mask.to(device=x.device)
        m = (m if m.dtype == torch.uint8 else m.to(torch.uint8)).contiguous()
        y = _wrap(super().forward(x, m))
        rows = x.cmap._batch_rows
        if rows is not None and len(rows) > 1:                       # per-item survivors, for the next stage's per-item top-k
            off, keep = 0, []
            cs = torch.cumsum(m.to(torch.int64), 0).cpu()
            for r in rows:
                keep.append(int(cs[off + r - 1] - (cs[off - 1] if off else 0)) if r else 0)
                off += r
            y.cmap._batch_rows = keep
        return y


class MinkowskiReLU(torch.nn.Module):
    def __init__(self, inplace=False):
        super().__init__()
        self.inplace = inplace

    def forward(self, x):
        return SparseTensor(ops.relu(x.F, inplace=self.inplace and x.F.is_contiguous()), coordinate_map=x.cmap)


def cat(*tensors):
    """ME.cat: channel concatenation of sparse tensors on the same coordinate level (autoencoder.py:55)."""
    first = tensors[0]
    for t in tensors[1:]:
        if len(t) != len(first):
            raise ValueError('ME.cat: the operands live on different coordinate levels')
    return SparseTensor(torch.cat([t.F for t in tensors], dim=1), coordinate_map=first.cmap)


class utils:
    sparse_collate = staticmethod(_sparse_collate)
