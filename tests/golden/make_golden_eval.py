#!/usr/bin/env python3
"""Generate tests/golden/eval_loss.npz from the reference implementation: `make_golden_eval.py --reference DIR`.

Like make_golden.py, this runs only where a checkout of the reference exists and none of the reference's Python travels: the script
imports `entropy_model`, `data_utils` and `loss` from it (with empty stub modules for MinkowskiEngine / torchac / h5py), feeds
them seeded inputs on plain tensors and SimpleNamespace stand-ins for sparse tensors, and stores inputs and outputs.

  bottleneck cases  b{i}_*   EntropyBottleneck.forward(y, quantize_mode=None) (entropy_model.py:132-140) and loss.get_bits
                             (loss.py:17-20) for default and perturbed parameters, on (a) integer latents, (b) integers plus uniform
                             noise, (c) values far in the tails, where the 1e-9 bound is hit — as the reference computes them in
                             fp32, and the same module's answer in fp64 (eb.double(), inputs.double())
  BCE cases         e{i}_*   data_utils.isin, loss.get_bce (fp32 and fp64 logits) and loss.get_cls_metrics of the top-k prediction
                             (data_utils.istopk with nums = ground-truth rows per batch item) on unique coordinates of two batch items
"""
import os, sys, types
import numpy as np
import torch

if '--reference' not in sys.argv[1:-1]:
    sys.exit('usage: make_golden_eval.py --reference DIR')
REF = os.path.abspath(sys.argv[sys.argv.index('--reference') + 1])
OUT = os.path.dirname(os.path.abspath(__file__))

for name in ('torchac', 'h5py', 'MinkowskiEngine'):
    sys.modules.setdefault(name, types.ModuleType(name))
sys.path.insert(0, REF)
import entropy_model as ref_em      # noqa: E402
import data_utils as ref_du         # noqa: E402
import loss as ref_loss             # noqa: E402


def pack_params(eb):
    """matrices 0..3, biases 0..3, factors 0..3, flattened (the order of make_golden.py's G1)"""
    return np.concatenate([p.detach().numpy().astype(np.float32).ravel() for lst in (eb._matrices, eb._biases, eb._factors) for p in lst])


def bottleneck_cases(out):
    rng = np.random.default_rng(515)
    ci = 0
    for seed, perturb in ((1234, False), (7, True)):
        np.random.seed(seed); torch.manual_seed(seed)
        eb = ref_em.EntropyBottleneck(8)
        if perturb:                                              # as G1 perturbs them
            with torch.no_grad():
                for f in eb._factors:
                    f.copy_(torch.empty_like(f).uniform_(-0.5, 0.5))
                for m in eb._matrices:
                    m.add_(torch.empty_like(m).uniform_(-0.3, 0.3))
        params = pack_params(eb)
        ints = rng.integers(-14, 15, size=(501, 8)).astype(np.float32)
        noisy = (rng.integers(-14, 15, size=(333, 8)) + rng.uniform(-0.5, 0.5, size=(333, 8))).astype(np.float32)
        tails = (rng.choice([-1.0, 1.0], size=(257, 8)) * rng.uniform(20.0, 400.0, size=(257, 8))).astype(np.float32)
        tails[::5] = rng.normal(0.0, 6.0, size=tails[::5].shape).astype(np.float32)      # ... mixed with ordinary values
        inputs = {'int': ints, 'noisy': noisy, 'tails': tails}
        res32 = {}
        with torch.no_grad():
            for kind, y in inputs.items():
                _, lik = eb(torch.from_numpy(y), quantize_mode=None)
                res32[kind] = (lik.numpy().copy(), float(ref_loss.get_bits(lik)))
            eb.double()
            for kind, y in inputs.items():
                _, lik64 = eb(torch.from_numpy(y).double(), quantize_mode=None)
                assert lik64.dtype == torch.float64
                lik32, bits32 = res32[kind]
                if kind == 'tails':
                    assert (lik32 == np.float32(1e-9)).any() and (lik64.numpy() == 1e-9).any(), 'the tails case must hit the bound'
                out[f'b{ci}_kind'] = np.array(kind)
                out[f'b{ci}_params'] = params
                out[f'b{ci}_y'] = y
                out[f'b{ci}_lik32'] = lik32
                out[f'b{ci}_bits32'] = np.float32(bits32)
                out[f'b{ci}_lik64'] = lik64.numpy().copy()
                out[f'b{ci}_bits64'] = np.float64(float(ref_loss.get_bits(lik64)))
                ci += 1
    out['n_bottleneck'] = np.array(ci)


class _Duck:
    """the attributes of an ME.SparseTensor that istopk touches (data_utils.py:77-89)"""
    def __init__(self, F, rows):
        self.F = F; self.device = F.device
        off = np.concatenate([[0], np.cumsum(rows)])
        self._batchwise_row_indices = [torch.arange(int(a), int(b)) for a, b in zip(off[:-1], off[1:])]
    def __len__(self): return len(self.F)


def bce_cases(out):
    rng = np.random.default_rng(616)
    ei = 0
    for n_per, hi, frac in (((1500, 1203), 64, 0.3), ((777, 2050), 1 << 20, 0.12), ((64, 65), 16, 0.6)):
        items, gts = [], []
        for b, n in enumerate(n_per):
            c = np.unique(rng.integers(0, hi, size=(n, 3)).astype(np.int32), axis=0)
            rng.shuffle(c)
            if b == 1:                                           # the same xyz as rows of item 0, in another batch item
                c[:20] = items[0][:20, 1:]
                c = c[np.sort(np.unique(c, axis=0, return_index=True)[1])]
            if hi == 1 << 20:                                    # both ends of the supported range
                c[0] = (0, 0, 0); c[1] = (hi - 1, hi - 1, hi - 1)
                c = c[np.sort(np.unique(c, axis=0, return_index=True)[1])]
            c4 = np.concatenate([np.full((len(c), 1), b, np.int32), c], 1)
            items.append(c4)
            pick = rng.random(len(c4)) < frac
            if b == 1:
                pick[:20] = rng.random(20) < 0.5                 # in the truth of one item only, mostly
            n_extra = min(30, len(c4) // 12)
            extra = np.concatenate([np.full((n_extra, 1), b, np.int32), rng.integers(0, hi, size=(n_extra, 3)).astype(np.int32)], 1)
            gts.append(np.concatenate([c4[pick], extra]))        # a truth row need not be a candidate
        coords = np.concatenate(items)
        gt = np.concatenate(gts)
        gt = gt[np.sort(np.unique(gt, axis=0, return_index=True)[1])]
        rows = [len(i) for i in items]
        nums = [int((gt[:, 0] == b).sum()) for b in range(len(items))]
        n = len(coords)
        logits = (rng.normal(0.0, 4.0, size=n)).astype(np.float32)
        logits[rng.integers(0, n, max(4, n // 60))] = 0.0
        logits[rng.integers(0, n, max(4, n // 60))] = -0.0
        logits[rng.integers(0, n, 10)] = rng.choice([-1.0, 1.0], 10).astype(np.float32) * rng.uniform(50, 3000, 10).astype(np.float32)
        logits[rng.integers(0, n, max(6, n // 40))] = np.float32(9.25)    # ties ...
        off = 0
        for r, k in zip(rows, nums):                             # ... none of which straddles the item's top-k threshold (torch.topk may
            v = np.sort(logits[off:off + r])[::-1]               #     take either of two equal values)
            assert 0 < k < r and v[k - 1] != v[k], 'reseed: a tie straddles the top-k threshold'
            off += r
        tC, tG = torch.from_numpy(coords), torch.from_numpy(gt)
        mask = ref_du.isin(tC, tG)
        F32 = torch.from_numpy(logits).reshape(-1, 1)
        data32 = types.SimpleNamespace(C=tC, F=F32, shape=F32.shape)
        data64 = types.SimpleNamespace(C=tC, F=F32.double(), shape=F32.shape)
        truth = types.SimpleNamespace(C=tG)
        with torch.no_grad():
            bce32 = ref_loss.get_bce(data32, truth)
            bce64 = ref_loss.get_bce(data64, truth)
        assert bce64.dtype == torch.float64
        pred = ref_du.istopk(_Duck(F32, rows), nums, rho=1.0)
        out[f'e{ei}_coords'] = coords
        out[f'e{ei}_truth'] = gt
        out[f'e{ei}_rows'] = np.array(rows)
        out[f'e{ei}_nums'] = np.array(nums)
        out[f'e{ei}_logits'] = logits
        out[f'e{ei}_isin'] = mask.numpy()
        out[f'e{ei}_bce32'] = np.float32(float(bce32))
        out[f'e{ei}_bce64'] = np.float64(float(bce64))
        out[f'e{ei}_pred'] = pred.numpy()
        out[f'e{ei}_metrics'] = np.array(ref_loss.get_cls_metrics(pred, mask), np.float64)
        ei += 1
    out['n_bce'] = np.array(ei)


if __name__ == '__main__':
    out = {}
    bottleneck_cases(out)
    bce_cases(out)
    out['torch_version'] = np.array(torch.__version__)
    path = os.path.join(OUT, 'eval_loss.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')
