"""PCCModel (reference pcc_model.py:8-45): container wiring Encoder [1,16,32,64,32,8], Decoder [8,64,32,16] and
EntropyBottleneck(8).  coder.Coder drives the encode/decode path; `forward` / `get_likelihood` are the forward half of the
reference's training graph (rate estimate, per-scale logits, teacher-forced pruning).  They run under torch.no_grad(); `forward_train` is the
same graph with a backward pass (pcgcv2_amd/grad.py), which pcgcv2_amd/trainer.py drives."""
import torch

from .autoencoder import Encoder, Decoder
from .entropy_model import EntropyBottleneck
from .sparse import SparseTensor


class PCCModel(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.encoder = Encoder(channels=[1, 16, 32, 64, 32, 8])
        self.decoder = Decoder(channels=[8, 64, 32, 16])
        self.entropy_bottleneck = EntropyBottleneck(8)

    def load_state_dict(self, state_dict, strict=True, **kw):
        from . import conventions
        self.entropy_bottleneck.invalidate()
        return super().load_state_dict(conventions.permute_state_dict(state_dict), strict=strict, **kw)

    def weights_changed(self):
        """The cache contract's explicit call (pcgcv2_amd/derived.py): the kernels read re-laid-out copies of the weights, rebuilt when a
        parameter's (data_ptr, _version) changes.  Writes through `.data` (`p.data.mul_(s)`, `p.data.copy_(w)`) change neither — call
        this after them, before the next forward / encode / decode.  Also available on every conv, block and the bottleneck."""
        from . import derived
        derived.weights_changed(self)

    @torch.no_grad()
    def get_likelihood(self, data, quantize_mode, generator=None):
        """pcc_model.py:15-24 -> (the quantised latent on data's coordinate level, likelihood [N, 8])."""
        data_F, likelihood = self.entropy_bottleneck(data.F, quantize_mode=quantize_mode, generator=generator)
        return SparseTensor(data_F, coordinate_map=data.cmap), likelihood

    @torch.no_grad()
    def forward(self, x, training=True, generator=None):
        """pcc_model.py:26-45.  training=True: uniform noise on the latent (`generator`: optional torch.Generator on x's device) and
        top-k | ground-truth pruning in the decoder; training=False: rounding and top-k pruning, i.e. what encode + decode compute.
        Forward values only — under torch.no_grad(), nothing can be back-propagated."""
        y_list = self.encoder(x)
        y = y_list[0]
        ground_truth_list = y_list[1:] + [x]
        nums_list = [list(gt.cmap.batch_rows) for gt in ground_truth_list]
        y_q, likelihood = self.get_likelihood(y, quantize_mode='noise' if training else 'symbols', generator=generator)
        out_cls_list, out = self.decoder(y_q, nums_list, ground_truth_list, training)
        return {'out': out,
                'out_cls_list': out_cls_list,
                'prior': y_q,
                'likelihood': likelihood,
                'ground_truth_list': ground_truth_list}

    def forward_train(self, x, generator=None, record=None):
        """forward(x, training=True) with an autograd graph (pcgcv2_amd/grad.py): the same dict with bit-equal values given the same
        generator state; the feature tensors carry a grad_fn, and loss.bce / loss.bits of the result can be back-propagated to all 224
        parameters.  record: optional dict that receives, per state-dict module name, what that layer's backward reads plus the level
        coordinates and kept masks (tests)."""
        from . import grad
        return grad.forward_train(self, x, generator=generator, record=record)

    def state_dict_reference(self):
        """state_dict() in the reference's layout: whatever load_state_dict permutes on the way in (the kernel-offset convention), undone"""
        from . import conventions
        return conventions.permute_state_dict({k: v.detach().clone() for k, v in self.state_dict().items()})


if __name__ == '__main__':
    print(PCCModel())
