"""The differentiable training graph (reference trainer.py:120-134: `out_set = model(x, training=True)` ... `sum_loss.backward()`).

torch.autograd.Functions over the UNFUSED operators — the graph the `ME.py` facade runs, which
tests/test_gpu_parity.py::test_me_facade_unfused_graph_equals_fused proves bit-equal to the fused one — so that `forward_train` returns
the values of `PCCModel.forward(x, training=True)` bit for bit and records what the backward pass reads.  Every gradient is computed by
libpcgc_hip.so (csrc/grad.hip and the forward gather convolution); torch only routes tensors (cat, column slices, accumulation of
gradients that meet at one tensor).  There is no eager fallback.

    operator                       weight / bias gradient            input gradient (always a gather, never a scatter)
    conv k3 (one level)            conv_wgrad(map, x, g)             conv_gather(map, g, W'),  W'[k] = W[26 - k]^T  (the map is its own
                                                                     transpose under k <-> 26 - k)
    conv k1                        conv_wgrad(None, x, g)            conv_gather(None, g, W^T)
    conv k2 s2 (down)              conv_wgrad(down map, x, g)        conv_gather(kmap_invert(down map), g, W[k]^T)
    generative transpose k2 s2     conv_up2_wgrad(x, g)              conv_gather(inv, g, W[k]^T),  inv[j][p] = 8 p + j
    ReLU epilogue                  g <- relu_bwd(g, y) first;   residual epilogue: the residual receives g;   bias: column sums of g
    pruning (row gather)           scatter_rows(g, kept rows)
    noise quantisation             gradient 1;   top-k | truth mask: a constant
"""
import torch

from . import ops
from .sparse import SparseTensor


def _rows(g):
    """a gradient as a 2-D view with unit column stride (autograd hands column slices of a cat on as they are)"""
    return g if g.stride(1) == 1 and g.stride(0) >= g.shape[1] else g.contiguous()


class _Map:
    """the kernel map of one convolution and, built on first use, its transpose"""

    def __init__(self, kind, nbr, n_in):
        self.kind, self.nbr, self.n_in = kind, nbr, int(n_in)           # kind: 'k3' | 'k1' | 'down'
        self._inv = None

    def transposed(self):
        if self.kind == 'down' and self._inv is None:
            self._inv = ops.kmap_invert(self.nbr, self.n_in)
        return self.nbr if self.kind == 'k3' else self._inv               # (k1: None = identity)


def transposed_kernel(W, kind):
    """the kernel of the input-gradient convolution: k3 W'[k] = W[26 - k]^T; k1 W^T; down / up W[k]^T"""
    if W.dim() == 2:
        return W.t().contiguous()
    Wt = W.transpose(1, 2)
    return (Wt.flip(0) if kind == 'k3' else Wt).contiguous()


class Conv(torch.autograd.Function):
    """relu?(conv(map, x, W) + bias (+ residual)) by pcgc_conv_gather (the all-ones first layer by pcgc_conv_gather_unit: same chain)"""

    @staticmethod
    def forward(ctx, x, W, bias, residual, kmap, relu, unit):
        if unit:
            y = ops.conv_gather_unit(kmap.nbr, W, bias, relu=relu)
        else:
            y = ops.conv_gather(kmap.nbr, x, W, bias, residual=residual, relu=relu)
        ctx.kmap, ctx.relu = kmap, relu
        ctx.save_for_backward(x, W, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, g):
        x, W, y = ctx.saved_tensors
        kmap = ctx.kmap
        g = _rows(g)
        if ctx.relu:
            g = ops.relu_bwd(g, y)
        gW, gb = ops.conv_wgrad(kmap.nbr, x, g)
        if W.dim() == 2:
            gW = gW[0]
        gx = None
        if ctx.needs_input_grad[0]:
            gx = ops.conv_gather(kmap.transposed(), g, transposed_kernel(W, kmap.kind), None, n_out=kmap.n_in)
        return gx, gW, gb, (g if ctx.needs_input_grad[3] else None), None, None, None


class UpConv(torch.autograd.Function):
    """relu?(generative transpose k2 s2 + bias): row 8 p + j = x[p] W[j]"""

    @staticmethod
    def forward(ctx, x, W, bias, relu):
        y = ops.conv_up2(x, W, bias, relu=relu)
        ctx.relu = relu
        ctx.save_for_backward(x, W, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, g):
        x, W, y = ctx.saved_tensors
        g = _rows(g)
        if ctx.relu:
            g = ops.relu_bwd(g, y)
        gW, gb = ops.conv_up2_wgrad(x, g)
        gx = None
        if ctx.needs_input_grad[0]:
            gx = ops.conv_gather(ops.kmap_up_inverse(x.shape[0], x.device), g, transposed_kernel(W, 'up'), None)
        return gx, gW, gb, None


class Prune(torch.autograd.Function):
    """MinkowskiPruning's feature rows: x[kept rows]; the mask is a constant"""

    @staticmethod
    def forward(ctx, x, mask, prefix, n):
        ctx.orig, ctx.n_in = ops.compact_index(mask, prefix, n), x.shape[0]
        return ops.compact_feats(x, mask, prefix, n)

    @staticmethod
    def backward(ctx, g):
        return ops.scatter_rows(_rows(g), ctx.orig, ctx.n_in), None, None, None


class NoiseQuantize(torch.autograd.Function):
    """EntropyBottleneck._quantize(mode='noise'): gradient 1"""

    @staticmethod
    def forward(ctx, y, eb, generator):
        return eb._quantize(y, 'noise', generator=generator)

    @staticmethod
    def backward(ctx, g):
        return g, None, None


class Bits(torch.autograd.Function):
    """scale * (-sum log2 max(likelihood(y), bound)) as one leaf: value and gradient both come from the fp64 chain of csrc/eb_logits.h
    (pcgc_eb_likelihood / pcgc_eb_likelihood_bwd), each rounded once.  params: the bottleneck's 12 tensors in packing order."""

    @staticmethod
    def forward(ctx, y, scale, bound, *params):
        packed = torch.cat([p.detach().reshape(-1) for p in params]).contiguous()
        bits = ops.eb_likelihood(y, packed, bound=bound, want_likelihood=False, want_bits=True)[1]
        ctx.scale, ctx.bound, ctx.shapes = float(scale), bound, [p.shape for p in params]
        ctx.save_for_backward(y, packed)
        return (bits[0] * float(scale)).float()

    @staticmethod
    def backward(ctx, g):
        y, packed = ctx.saved_tensors
        gy, gp = ops.eb_likelihood_bwd(y, packed, bound=ctx.bound, scale=ctx.scale * float(g))
        out, off = [], 0
        for s in ctx.shapes:
            out.append(gp[off:off + s.numel()].reshape(s))
            off += s.numel()
        return (gy, None, None) + tuple(out)


class BCE(torch.autograd.Function):
    """scale * loss.get_bce as one leaf (the truth mask is a constant)"""

    @staticmethod
    def forward(ctx, logits, mask, scale):
        ctx.scale = float(scale)
        ctx.save_for_backward(logits, mask)
        return (ops.bce_logits(logits, mask)[0][0] * float(scale)).float()

    @staticmethod
    def backward(ctx, g):
        logits, mask = ctx.saved_tensors
        return ops.bce_logits_bwd(logits, mask, scale=ctx.scale * float(g)), None, None


# ------------------------------------------------------------------------------------------------ the model (autoencoder.py) on those operators
class _Tape:
    def __init__(self, record):
        self.record = record

    def conv(self, name, m, feats, cmap, relu=False, residual=None, unit=False):
        k, s = m.kernel_size, m.stride
        if k == 3:
            kmap, out_map = self._k3(cmap), cmap
        elif k == 1:
            kmap, out_map = _Map('k1', None, len(cmap)), cmap
        else:
            coarse, down = cmap.down()
            kmap, out_map = _Map('down', down, len(cmap)), coarse
        y = Conv.apply(feats, m.kernel, m.bias, residual, kmap, relu, unit)
        self.note(name, x=feats, y=y, relu=relu, kind=kmap.kind, map=kmap.nbr, coords=cmap, out_coords=out_map, residual=residual)
        return y, out_map

    def _k3(self, cmap):
        hit = cmap.__dict__.get('_grad_k3')
        if hit is None or hit.nbr is not cmap.k3:
            hit = cmap.__dict__['_grad_k3'] = _Map('k3', cmap.k3, len(cmap))
        return hit

    def note(self, name, **kw):
        if self.record is not None:
            entry = self.record[name] = {k: (v.detach() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
            y = kw.get('y')
            if isinstance(y, torch.Tensor) and y.requires_grad:          # 'gy': the gradient that reaches the layer's output, once backward ran
                y.register_hook(lambda g, e=entry: e.__setitem__('gy', g.detach().clone()))

    def irn(self, name, blk, x, cmap):
        """autoencoder.py:52-57: cat(conv0_1(relu(conv0_0 x)), conv1_2(relu(conv1_1(relu(conv1_0 x))))) + x; the residual add is the
        epilogue of the two last convolutions on the column slices of x, as in the unfused forward graph"""
        c = x.shape[1]
        a, _ = self.conv(f'{name}.conv0_0', blk.conv0_0, x, cmap, relu=True)
        o0, _ = self.conv(f'{name}.conv0_1', blk.conv0_1, a, cmap, residual=x[:, :c // 2])
        b, _ = self.conv(f'{name}.conv1_0', blk.conv1_0, x, cmap, relu=True)
        b, _ = self.conv(f'{name}.conv1_1', blk.conv1_1, b, cmap, relu=True)
        o1, _ = self.conv(f'{name}.conv1_2', blk.conv1_2, b, cmap, residual=x[:, c // 2:])
        return torch.cat([o0, o1], dim=1)

    def block(self, name, seq, x, cmap):
        for i, blk in enumerate(seq):
            x = self.irn(f'{name}.{i}', blk, x, cmap)
        return x


def forward_train(model, x, generator=None, record=None):
    """PCCModel.forward(x, training=True) with an autograd graph: same dict, same values bit for bit (given the same generator state); the
    feature tensors carry a grad_fn.  out['likelihood'] is the forward's tensor; the rate term is differentiated as one leaf by
    loss.bits(out['likelihood']), which finds the latent it was evaluated at through the tensor's `_rate_of` attribute."""
    enc, dec, eb = model.encoder, model.decoder, model.entropy_bottleneck
    tape = _Tape(record)
    # encoder (autoencoder.py:138-147).  The first layer's weight gradient reads the input level's k3 map, which the codec's mapless
    # first layer never builds: cmap.k3 builds it here.
    f, cm = x.F, x.cmap
    outs = []
    for i in range(3):
        f, _ = tape.conv(f'encoder.conv{i}', getattr(enc, f'conv{i}'), f, cm, relu=True, unit=(i == 0 and x.has_unit_features()))
        f, cm = tape.conv(f'encoder.down{i}', getattr(enc, f'down{i}'), f, cm, relu=True)
        f = tape.block(f'encoder.block{i}', getattr(enc, f'block{i}'), f, cm)
        outs.append((f, cm))
    y, _ = tape.conv('encoder.conv3', enc.conv3, f, cm)
    ground_truth_list = [SparseTensor(o.detach(), coordinate_map=c) for o, c in (outs[1], outs[0])] + [x]
    nums_list = [list(gt.cmap.batch_rows) for gt in ground_truth_list]
    # bottleneck (pcc_model.py:15-24)
    eb._check_inputs(y)
    y_q = NoiseQuantize.apply(y, eb, generator)
    with torch.no_grad():
        likelihood = ops.eb_likelihood(y_q.detach(), eb.packed_params(y.device), bound=eb._likelihood_bound)[0]
    likelihood._rate_of = (y_q, eb)
    tape.note('entropy_bottleneck', x=y_q, likelihood=likelihood, coords=cm)
    # decoder (autoencoder.py:251-273), teacher-forced pruning
    f, cls_list, latent_map = y_q, [], cm
    for l in range(3):
        up = getattr(dec, f'up{l}')
        h = UpConv.apply(f, up.kernel, up.bias, True)
        tape.note(f'decoder.up{l}', x=f, y=h, relu=True, kind='up', coords=cm)
        cm = cm.up()
        h, _ = tape.conv(f'decoder.conv{l}', getattr(dec, f'conv{l}'), h, cm, relu=True)
        h = tape.block(f'decoder.block{l}', getattr(dec, f'block{l}'), h, cm)
        cls, _ = tape.conv(f'decoder.conv{l}_cls', getattr(dec, f'conv{l}_cls'), h, cm)
        cls_list.append(SparseTensor(cls, coordinate_map=cm))
        with torch.no_grad():
            pruned = dec.prune_voxel(SparseTensor(h.detach(), coordinate_map=cm), SparseTensor(cls.detach(), coordinate_map=cm), nums_list[l],
                                     ground_truth_list[l], True)
        _, _, mask, prefix = pruned.cmap.origin
        tape.note(f'decoder.prune{l}', mask=mask, coords=cm, out_coords=pruned.cmap)
        if l < 2:                                   # (the last stage hands on coordinates; no loss reads its features: they stay lazy)
            f = Prune.apply(h, mask, prefix, len(pruned.cmap))
        cm = pruned.cmap
    return {'out': pruned,
            'out_cls_list': cls_list,
            'prior': SparseTensor(y_q, coordinate_map=latent_map),
            'likelihood': likelihood,
            'ground_truth_list': ground_truth_list}
