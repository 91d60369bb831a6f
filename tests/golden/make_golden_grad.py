#!/usr/bin/env python3
"""Generate tests/golden/grad_loss.npz from the reference implementation: `make_golden_grad.py --reference DIR`.

Like make_golden_eval.py, this runs only where a checkout of the reference exists and none of the reference's Python travels: the script
imports `entropy_model`, `data_utils` and `loss` from it (with empty stub modules for MinkowskiEngine / torchac / h5py) and lets the
reference's own modules, in fp64, differentiate the inputs of tests/golden/eval_loss.npz (which must exist: only results are stored here).

  bottleneck cases  b{i}_gy, b{i}_gparams   gradient of loss.get_bits(EntropyBottleneck.forward(y, quantize_mode=None)[1]) — through
                                            Low_bound.backward (entropy_model.py:19-39) — with respect to the latent y [n, 8] and the 12
                                            parameter tensors (packed matrices | biases | factors), for the three latent kinds of
                                            eval_loss.npz; "tails" hits the 1e-9 bound
  BCE cases         e{i}_glogits            gradient of loss.get_bce with respect to the fp64 logits
"""
import os, sys, types
import numpy as np
import torch

if '--reference' not in sys.argv[1:-1]:
    sys.exit('usage: make_golden_grad.py --reference DIR')
REF = os.path.abspath(sys.argv[sys.argv.index('--reference') + 1])
OUT = os.path.dirname(os.path.abspath(__file__))

for name in ('torchac', 'h5py', 'MinkowskiEngine'):
    sys.modules.setdefault(name, types.ModuleType(name))
sys.path.insert(0, REF)
import entropy_model as ref_em      # noqa: E402
import loss as ref_loss             # noqa: E402


def set_params(eb, packed):
    off = 0
    with torch.no_grad():
        for lst in (eb._matrices, eb._biases, eb._factors):
            for p in lst:
                n = p.numel()
                p.copy_(torch.from_numpy(packed[off:off + n].astype(np.float64)).reshape(p.shape))
                off += n
    assert off == len(packed)


if __name__ == '__main__':
    ev = np.load(os.path.join(OUT, 'eval_loss.npz'))
    out = {}
    for i in range(int(ev['n_bottleneck'])):
        np.random.seed(0)
        eb = ref_em.EntropyBottleneck(8).double()
        set_params(eb, ev[f'b{i}_params'])
        y = torch.from_numpy(ev[f'b{i}_y']).double().requires_grad_(True)
        _, lik = eb(y, quantize_mode=None)
        if str(ev[f'b{i}_kind']) == 'tails':
            assert (lik.detach().numpy() == 1e-9).any(), 'the tails case must hit the bound'
        bits = ref_loss.get_bits(lik)
        assert abs(float(bits) - float(ev[f'b{i}_bits64'])) <= 1e-12 * abs(float(bits))
        params = [p for lst in (eb._matrices, eb._biases, eb._factors) for p in lst]
        grads = torch.autograd.grad(bits, [y] + params)
        assert all(g.dtype == torch.float64 for g in grads)
        out[f'b{i}_gy'] = grads[0].numpy().copy()
        out[f'b{i}_gparams'] = np.concatenate([g.numpy().ravel() for g in grads[1:]])
    out['n_bottleneck'] = ev['n_bottleneck']
    for i in range(int(ev['n_bce'])):
        logits = torch.from_numpy(ev[f'e{i}_logits']).double().reshape(-1, 1).requires_grad_(True)
        data = types.SimpleNamespace(C=None, F=logits, shape=logits.shape)
        mask = torch.from_numpy(ev[f'e{i}_isin'])
        ref_loss.isin = lambda C, G, m=mask: m                   # (the membership mask is eval_loss.npz's e{i}_isin, computed by the reference)
        bce = ref_loss.get_bce(data, types.SimpleNamespace(C=None))
        assert abs(float(bce) - float(ev[f'e{i}_bce64'])) <= 1e-12 * abs(float(bce))
        out[f'e{i}_glogits'] = torch.autograd.grad(bce, [logits])[0].numpy().ravel().copy()
    out['n_bce'] = ev['n_bce']
    out['torch_version'] = np.array(torch.__version__)
    path = os.path.join(OUT, 'grad_loss.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')
