#!/usr/bin/env python3
"""Generate tests/golden/loss_channels.npz from the reference implementation: `make_golden_loss_channels.py --reference DIR`.

Like make_golden_eval.py, this runs only where a checkout of the reference exists and none of the reference's Python travels: the script
imports `entropy_model` and `loss` from it (with empty stub modules for MinkowskiEngine / torchac / h5py), feeds them seeded inputs on
plain tensors and stores inputs and outputs.

  c{C}_*  for C in (1, 3, 5, 16): EntropyBottleneck(C) with perturbed parameters (as make_golden_eval.py perturbs them) on 67 rows that
          mix integers, integers plus uniform noise and a few values far in the tails, where the 1e-9 bound is hit.  Stored: the packed
          fp32 parameters (matrices 0..3 | biases 0..3 | factors 0..3), y, the module's fp64 likelihood and loss.get_bits (eb.double()),
          and the fp64 autograd gradients of get_bits — through Low_bound.backward (entropy_model.py:19-39) — with respect to y and to
          the packed parameters.
"""
import os, sys, types
import numpy as np
import torch

if '--reference' not in sys.argv[1:-1]:
    sys.exit('usage: make_golden_loss_channels.py --reference DIR')
REF = os.path.abspath(sys.argv[sys.argv.index('--reference') + 1])
OUT = os.path.dirname(os.path.abspath(__file__))

for name in ('torchac', 'h5py', 'MinkowskiEngine'):
    sys.modules.setdefault(name, types.ModuleType(name))
sys.path.insert(0, REF)
import entropy_model as ref_em      # noqa: E402
import loss as ref_loss             # noqa: E402

CHANNELS = (1, 3, 5, 16)
ROWS = 67


def pack_params(eb):
    return np.concatenate([p.detach().numpy().astype(np.float32).ravel() for lst in (eb._matrices, eb._biases, eb._factors) for p in lst])


if __name__ == '__main__':
    rng = np.random.default_rng(717)
    out = {'channels': np.array(CHANNELS)}
    for C in CHANNELS:
        np.random.seed(100 + C); torch.manual_seed(100 + C)
        eb = ref_em.EntropyBottleneck(C)
        with torch.no_grad():                                    # as make_golden_eval.py perturbs them
            for f in eb._factors:
                f.copy_(torch.empty_like(f).uniform_(-0.5, 0.5))
            for m in eb._matrices:
                m.add_(torch.empty_like(m).uniform_(-0.3, 0.3))
        params = pack_params(eb)
        y = rng.integers(-14, 15, size=(ROWS, C)).astype(np.float64)
        y[1::3] += rng.uniform(-0.5, 0.5, size=y[1::3].shape)
        tails = np.arange(5, ROWS, 11)
        y[tails] = rng.choice([-1.0, 1.0], size=(len(tails), C)) * rng.uniform(60.0, 400.0, size=(len(tails), C))
        y = y.astype(np.float32)
        eb.double()                                              # (the fp32 parameters, widened: exactly what was packed)
        assert np.array_equal(pack_params(eb), params)
        yt = torch.from_numpy(y).double().requires_grad_(True)
        _, lik = eb(yt, quantize_mode=None)
        assert lik.dtype == torch.float64 and lik.shape == (ROWS, C)
        at_bound = lik.detach().numpy() == 1e-9
        assert at_bound.any() and not at_bound.all(), 'reseed: the case must hit the bound on a few rows'
        bits = ref_loss.get_bits(lik)
        plist = [p for lst in (eb._matrices, eb._biases, eb._factors) for p in lst]
        grads = torch.autograd.grad(bits, [yt] + plist)
        assert all(g.dtype == torch.float64 for g in grads)
        out[f'c{C}_params'] = params
        out[f'c{C}_y'] = y
        out[f'c{C}_lik64'] = lik.detach().numpy().copy()
        out[f'c{C}_bits64'] = np.float64(float(bits.detach()))
        out[f'c{C}_gy'] = grads[0].numpy().copy()
        out[f'c{C}_gparams'] = np.concatenate([g.numpy().ravel() for g in grads[1:]])
    out['torch_version'] = np.array(torch.__version__)
    path = os.path.join(OUT, 'loss_channels.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')
