"""The case of the descent tests (a helper module): one small cloud, the seeded synthetic weights, twenty Adam steps with the reference's
default learning rate (train.py: --lr 8e-4; trainer.py:60-65: betas (0.9, 0.999), weight decay 1e-4) and the same noise at every step.
test_grad_cpu.py runs the fp64 definition through it, test_grad_device.py the device."""
import numpy as np
import torch

CLOUD = 'shell6'
STEPS = 20
LR = 8e-4
SEED = 1234


def cloud4():
    """[N, 4] int64 rows (batch 0, x, y, z) of the case's cloud, in the raster order the synthetic clouds come in"""
    from pcgcv2_amd.synthetic import cloud
    c = cloud(CLOUD).numpy().astype(np.int64)
    return np.concatenate([np.zeros((len(c), 1), np.int64), c], 1)


def adam(params):
    return torch.optim.Adam([{'params': list(params), 'lr': LR}], betas=(0.9, 0.999), weight_decay=1e-4)


def definition_descent(steps=STEPS):
    """-> (sum_loss before the first step, sum_loss after the last) of the fp64 definition"""
    import grad_reference as G
    import fp64_reference as R
    from pcgcv2_amd.synthetic import synthetic_state_dict
    c = cloud4()
    sd = G.state_dict_f64(synthetic_state_dict(seed=SEED))
    n8 = len(R.down_coords(R.down_coords(R.down_coords(c, 1), 2), 4))
    noise = torch.rand((n8, 8), dtype=torch.float64, generator=torch.Generator().manual_seed(SEED)) - 0.5
    opt = adam(sd.values())
    losses = []
    for _ in range(steps + 1):
        opt.zero_grad()
        loss = G.model_loss(sd, c, noise)[0]
        losses.append(float(loss))
        if len(losses) <= steps:
            loss.backward()
            opt.step()
    return losses[0], losses[-1]
