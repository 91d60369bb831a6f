"""The training graph of PCGCv2 restated in torch float64 on the CPU, for tests (a helper module, like fp64_reference.py): autograd
differentiates it, and the device's gradients (csrc/grad.hip, pcgcv2_amd/grad.py) are judged by the result.

Written from the formulas (reference autoencoder.py:52-57,138-147,251-273, entropy_model.py:19-39,82-140, loss.py:8-20,
trainer.py:127-134); it shares no code with the package.  Kernel maps come from fp64_reference.neighbour_map (binary search over
linearised coordinates), convolutions are index_select + matmul over the present pairs, the bottleneck is written out with a
Low_bound-style function.  tests/test_grad_cpu.py pins it by torch.autograd.gradcheck and by the reference's own fp64 gradients
(tests/golden/grad_loss.npz, 1e-12 relative) before the GPU is judged by it."""
import numpy as np
import torch

import fp64_reference as R

FILTERS = (1, 3, 3, 3, 1)
LN2 = float(np.log(2.0))
# what the reference divides by: torch.log(torch.tensor(2.0)) is an fp32 tensor even when the logits are fp64 (loss.py:13)
LN2_REFERENCE = float(np.log(np.float32(2.0), dtype=np.float32))
F64 = torch.float64


# ------------------------------------------------------------------------------------------------ bottleneck and losses
def eb_unpack(params, C=8):
    """packed parameters [44 C] (matrices 0..3 | biases 0..3 | factors 0..3) -> 12 views [C, fo, fi] / [C, fo, 1]"""
    out, off = [], 0
    shapes = [(C, FILTERS[i + 1], FILTERS[i]) for i in range(4)] + [(C, FILTERS[i + 1], 1) for i in range(4)] * 2
    for shp in shapes:
        n = int(np.prod(shp))
        out.append(params[off:off + n].reshape(shp))
        off += n
    assert off == params.numel()
    return out


def logits_cumulative(tensors, v):
    """v [n, C] -> logits [n, C]: four layers z <- softplus(M) z + b; z <- z + tanh(f) tanh(z)"""
    mats, biases, factors = tensors[0:4], tensors[4:8], tensors[8:12]
    z = v.t()[:, None, :]                                        # [C, 1, n]
    for M, b, f in zip(mats, biases, factors):
        z = torch.matmul(torch.nn.functional.softplus(M), z) + b
        z = z + torch.tanh(f) * torch.tanh(z)
    return z[:, 0, :].t()


class LowBound(torch.autograd.Function):
    """max(x, bound); the gradient passes where x >= bound (or where it is negative AND x >= bound is what remains of the reference's
    rule after its first line has zeroed every element below the bound, entropy_model.py:27-39).  passthrough=True: the mutation
    "clamp gradient passed through" of the device tests."""

    @staticmethod
    def forward(ctx, x, bound, passthrough):
        ctx.save_for_backward(x)
        ctx.bound, ctx.passthrough = bound, passthrough
        return torch.clamp(x, min=bound)

    @staticmethod
    def backward(ctx, g):
        x, = ctx.saved_tensors
        return (g if ctx.passthrough else g * (x >= ctx.bound).to(g.dtype)), None, None


def likelihood(tensors, y, bound=1e-9, passthrough=False):
    lo, up = logits_cumulative(tensors, y - 0.5), logits_cumulative(tensors, y + 0.5)
    s = -torch.sign(lo + up).detach()
    lik = torch.abs(torch.sigmoid(s * up) - torch.sigmoid(s * lo))
    return LowBound.apply(lik, bound, passthrough) if bound else lik


def bits(lik):
    return -torch.sum(torch.log2(lik))


def bce_bits(logits, mask, ln2=LN2):
    """sum_i max(x, 0) - x t + log1p(exp(-|x|)) = log(1 + exp(x)) - x t, in bits (written in the smooth form: the derivative of the
    max / |.| form at x = 0 is a subgradient convention, not sigmoid(0) - t)"""
    x = logits.reshape(-1)
    t = torch.as_tensor(np.asarray(mask, np.float64))
    return torch.sum(torch.logaddexp(torch.zeros_like(x), x) - x * t) / ln2


def eb_gradients(params, y, bound=1e-9, passthrough=False):
    """d bits / d y [n, C] and d bits / d params [44 C] (numpy fp64) at fp32 or fp64 inputs given as arrays"""
    p = torch.tensor(np.asarray(params, np.float64), requires_grad=True)
    v = torch.tensor(np.asarray(y, np.float64), requires_grad=True)
    b = bits(likelihood(eb_unpack(p, v.shape[1]), v, bound, passthrough))
    gy, gp = torch.autograd.grad(b, [v, p])
    return gy.numpy(), gp.numpy(), float(b.detach())


def eb_row_gradients(params, y, bound=1e-9):
    """d (row i's rate) / d params -> [n, 44 C] in the packing of `params`, in ONE backward pass: element (i, c) uses the 44 parameters of
    channel c only, so every element is evaluated as a channel of its own (n C channels, one row) holding a copy of its channel's
    parameters, and the gradient with respect to the copies is the Jacobian of the per-row rates with respect to the parameters."""
    y = np.asarray(y, np.float64)
    n, C = y.shape
    if n == 0:
        return np.zeros((0, 44 * C))
    p = torch.as_tensor(np.asarray(params, np.float64))
    idx = torch.arange(n * C) % C
    big = torch.cat([t[idx].reshape(-1) for t in eb_unpack(p, C)])
    _, g, _ = eb_gradients(big.numpy(), y.reshape(1, n * C), bound)
    return np.concatenate([t.reshape(n, -1).numpy() for t in eb_unpack(torch.from_numpy(g), n * C)], 1)


def bce_gradient(logits, mask, ln2=LN2):
    x = torch.tensor(np.asarray(logits, np.float64).ravel(), requires_grad=True)
    g, = torch.autograd.grad(bce_bits(x, mask, ln2), [x])
    return g.numpy()


# ------------------------------------------------------------------------------------------------ convolutions
def conv(nbr, x, W, b=None):
    """out[o] = b + sum_k x[nbr[k, o]] W[k] over the present pairs.  nbr: int array [K, n_out] (-1 = absent); W [K, Cin, Cout]"""
    nbr = np.asarray(nbr)
    xp = torch.cat([x, torch.zeros((1, x.shape[1]), dtype=x.dtype)], 0)
    idx = torch.as_tensor(np.where(nbr < 0, x.shape[0], nbr).astype(np.int64))
    y = None
    for k in range(nbr.shape[0]):
        t = xp.index_select(0, idx[k]) @ W[k]
        y = t if y is None else y + t
    return y if b is None else y + b.reshape(1, -1)


def up_map(n):
    """the generative transpose as a gather: output row 8 p + j reads input row p through offset j"""
    m = np.full((8, 8 * n), -1, np.int64)
    for j in range(8):
        m[j, j::8] = np.arange(n)
    return m


def conv_gradients(nbr, x, W, gy, bias=True):
    """(gW, gb, gx) of <conv(nbr, x, W, b), gy> by autograd, numpy fp64"""
    xt = torch.tensor(np.asarray(x, np.float64), requires_grad=True)
    Wt = torch.tensor(np.asarray(W, np.float64), requires_grad=True)
    bt = torch.zeros(W.shape[-1], dtype=F64, requires_grad=True)
    s = (conv(nbr, xt, Wt, bt) * torch.as_tensor(np.asarray(gy, np.float64))).sum()
    gW, gb, gx = torch.autograd.grad(s, [Wt, bt, xt])
    return gW.numpy(), gb.numpy(), gx.numpy()


# ------------------------------------------------------------------------------------------------ the model
def _k3(coords, stride):
    return R.k3_map(coords, stride)


def _c(sd, name, nbr, x, relu=False):
    W = sd[name + '.kernel']
    y = conv(nbr, x, W.reshape(1, *W.shape) if W.dim() == 2 else W, sd[name + '.bias'])
    return torch.relu(y) if relu else y


def inception_resnet(sd, name, nbr, x):
    ident = np.arange(x.shape[0])[None]
    a = _c(sd, name + '.conv0_1', nbr, _c(sd, name + '.conv0_0', nbr, x, True))
    h = _c(sd, name + '.conv1_1', nbr, _c(sd, name + '.conv1_0', ident, x, True), True)
    return torch.cat([a, _c(sd, name + '.conv1_2', ident, h)], 1) + x


def block(sd, name, nbr, x):
    for i in range(3):
        x = inception_resnet(sd, f'{name}.{i}', nbr, x)
    return x


def topk_mask(vals, k):
    v = np.asarray(vals, np.float64).ravel()
    mask = np.zeros(len(v), bool)
    mask[np.argsort(-v, kind='stable')[:int(min(len(v), k))]] = True
    return mask


def isin(data, truth):
    return R.lookup(truth, data) >= 0


def model_loss(sd, coords, noise, alpha=1.0, beta=1.0, bce_div='cls'):
    """sum_loss of trainer.py:127-134 for the cloud `coords` [N, 4] (batch, x, y, z; unique rows, items contiguous) with the all-ones
    feature, teacher-forced pruning and `noise` (tensor [N8, 8] in [-0.5, 0.5)) on the latent.  sd: fp64 tensors by state-dict name.
    -> (sum_loss, parts dict)"""
    coords = np.asarray(coords, np.int64)
    x = torch.ones((len(coords), 1), dtype=F64)
    levels, feats, stride = [coords], [], 1
    c = coords
    for i in range(3):
        x = _c(sd, f'encoder.conv{i}', _k3(c, stride), x, True)
        coarse = R.down_coords(c, stride)
        x = _c(sd, f'encoder.down{i}', R.neighbour_map(coarse, c, R.offsets(2) * stride), x, True)
        c, stride = coarse, 2 * stride
        x = block(sd, f'encoder.block{i}', _k3(c, stride), x)
        levels.append(c); feats.append(x)
    y = _c(sd, 'encoder.conv3', _k3(c, stride), x)
    y_q = y + noise
    eb = [sd[f'entropy_bottleneck._{kind}.{i}'] for kind in ('matrices', 'biases', 'factors') for i in range(4)]
    rate = bits(likelihood(eb, y_q)) / len(coords)
    truths = [levels[2], levels[1], levels[0]]
    bce_sum, bces, f = 0, [], y_q
    for l in range(3):
        kids = R.children_coords(c, stride)
        stride //= 2
        h = _c(sd, f'decoder.up{l}', up_map(len(c)), f, True)
        nbr = _k3(kids, stride)
        h = block(sd, f'decoder.block{l}', nbr, _c(sd, f'decoder.conv{l}', nbr, h, True))
        cls = _c(sd, f'decoder.conv{l}_cls', nbr, h)
        truth = isin(kids, truths[l])
        curr = bce_bits(cls, truth) / (len(kids) if bce_div == 'cls' else len(coords))
        bce_sum = bce_sum + curr
        bces.append(curr)
        keep = truth.copy()
        logits = cls.detach().numpy().ravel()
        for b in np.unique(kids[:, 0]):
            rows = np.nonzero(kids[:, 0] == b)[0]
            keep[rows[topk_mask(logits[rows], int((truths[l][:, 0] == b).sum()))]] = True
        c = kids[keep]
        f = h[torch.as_tensor(np.nonzero(keep)[0])]
    return alpha * bce_sum + beta * rate, {'bces': bces, 'bpp': rate, 'latent': y_q}


def state_dict_f64(sd, requires_grad=True):
    """a state dict (tensors or arrays) -> fp64 leaf tensors; the bottleneck's three alias keys are dropped (they are the last layer)"""
    out = {}
    for k, v in sd.items():
        if k in ('entropy_bottleneck.matrix', 'entropy_bottleneck.bias', 'entropy_bottleneck.factor'):
            continue
        out[k] = torch.tensor(np.asarray(v.detach().cpu() if hasattr(v, 'detach') else v, np.float64), requires_grad=requires_grad)
    return out
