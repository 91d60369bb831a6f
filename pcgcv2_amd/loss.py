"""Losses and classification metrics of the training graph (reference loss.py:1-41) and the record Trainer.test keeps per cloud
(trainer.py:78-101), on the HIP operator set: same names and argument lists, so `from loss import get_bce, get_bits, get_metrics` binds.

get_bce / get_bits / the metrics give forward values only and run under torch.no_grad(); `bce`, `bits` and `sum_loss` are their differentiable
counterparts on the graph of PCCModel.forward_train (pcgcv2_amd/grad.py, csrc/grad.hip).
Sums are accumulated in fp64 in a fixed order on the device (csrc/loss.hip) and rounded once to the fp32 scalar the reference returns;
they are bitwise reproducible run to run.

    python -m pcgcv2_amd.loss --filedir cloud.ply --ckptdir x.pth [--training]
"""
import torch

from . import ops
from .data_utils import isin, isin_mask, istopk              # noqa: F401  (isin: the reference's loss.py imports it too)


def _u8(mask):
    return mask if mask.dtype == torch.uint8 else mask.to(torch.uint8)


@torch.no_grad()
def get_bce(data, groud_truth):
    """loss.py:8-15: BCE-with-logits of data.F against isin(data.C, ground_truth.C), in bits, summed over the rows (mean x rows / ln 2)
    -> 0-dim fp32 device tensor.  Membership probe and sum in two launches; the logits never leave the device."""
    mask = isin_mask(data.C, groud_truth)
    bce, _ = ops.bce_logits(data.F, mask)
    return bce[0].float()


@torch.no_grad()
def get_bits(likelihood):
    """loss.py:17-20: -sum(log2(likelihood)) -> 0-dim fp32 device tensor."""
    lik = likelihood if likelihood.dim() == 2 else likelihood.reshape(likelihood.shape[0], -1)
    if lik.stride(-1) != 1:
        lik = lik.contiguous()
    return ops.neg_log2_sum(lik)[0].float()


def bce(data, groud_truth, scale=1.0):
    """Differentiable get_bce: scale * get_bce(data, groud_truth) as one autograd leaf over data.F (the logits of PCCModel.forward_train).
    `scale` carries alpha / len(out_cls) of trainer.py:127-129 into the fp64 evaluation: value and gradient are each rounded once."""
    from . import grad
    return grad.BCE.apply(data.F, isin_mask(data.C, groud_truth), float(scale))


def bits(likelihood, scale=1.0):
    """Differentiable get_bits: scale * get_bits(likelihood) for the likelihood PCCModel.forward_train returned, differentiated with
    respect to the latent and the bottleneck's 12 parameter tensors as one leaf (fp64 chain, one rounding; elements below the likelihood
    bound contribute no gradient, as Low_bound.backward yields for this loss).  `scale` carries beta / len(x) of trainer.py:132-133."""
    from . import grad
    src = getattr(likelihood, '_rate_of', None)
    if src is None:
        raise ValueError('loss.bits: not the likelihood of PCCModel.forward_train (use get_bits for forward values)')
    y_q, eb = src
    params = [p for lst in (eb._matrices, eb._biases, eb._factors) for p in lst]
    return grad.Bits.apply(y_q, float(scale), eb._likelihood_bound, *params)


def sum_loss(out_set, n_points, alpha=1., beta=1.):
    """trainer.py:127-134: alpha * sum_l get_bce(out_cls_l, truth_l) / len(out_cls_l) + beta * get_bits(likelihood) / len(x)
    -> (sum_loss with a grad_fn, per-scale bce values, bpp)"""
    total, bces = 0, []
    for out_cls, ground_truth in zip(out_set['out_cls_list'], out_set['ground_truth_list']):
        curr = bce(out_cls, ground_truth, scale=1.0 / float(len(out_cls)))
        total = total + alpha * curr
        bces.append(curr)
    bpp = bits(out_set['likelihood'], scale=1.0 / float(n_points))
    return total + beta * bpp, bces, bpp


def _triple(TP, FN, FP):
    precision = TP / (TP + FP + 1e-7)
    recall = TP / (TP + FN + 1e-7)
    IoU = TP / (TP + FP + FN + 1e-7)
    return [round(precision, 4), round(recall, 4), round(IoU, 4)]


@torch.no_grad()
def get_cls_metrics(pred, real):
    """loss.py:30-40: [precision, recall, IoU] of a predicted against a real boolean mask, rounded to 4 places.  Device masks are counted
    on the device (pcgc_bce_logits without logits: TP, FN, FP, TN in one pass, four integers read back); CPU masks on the host."""
    if pred.is_cuda:
        _, counts = ops.bce_logits(None, _u8(real).contiguous(), _u8(pred).contiguous())
        TP, FN, FP, _ = counts.tolist()
    else:
        pred, real = pred.bool(), real.bool()
        TP, FN, FP = int((pred & real).sum()), int((~pred & real).sum()), int((pred & ~real).sum())
    return _triple(TP, FN, FP)


@torch.no_grad()
def get_metrics(data, groud_truth):
    """loss.py:22-28: metrics of "the top-k logits, k = ground-truth rows per batch item" against membership in the ground truth
    -> [precision, recall, IoU].  (The reference's last line hands back element 0 of that list only; the whole triple is what
    Trainer.test's `metrics` record is read for, so the triple is returned.)  Both masks are produced and counted on the device."""
    mask_real = isin_mask(data.C, groud_truth)
    nums = list(groud_truth.cmap.batch_rows)
    mask_pred = _u8(istopk(data, nums, rho=1.0))
    _, counts = ops.bce_logits(None, mask_real, mask_pred.contiguous())
    TP, FN, FP, _ = counts.tolist()
    return _triple(TP, FN, FP)


def kept_masks(out_set):
    """per decoder level, the uint8 mask over the level's candidates (the rows of out_cls_list[l]) of the voxels the general-mask
    pruning of a teacher-forced forward kept"""
    levels = [cls.cmap.origin[1] for cls in out_set['out_cls_list'][1:]] + [out_set['out'].cmap]
    for lvl in levels:
        if lvl.origin is None or lvl.origin[0] != 'pruned':
            raise ValueError('kept_masks: not the output of PCCModel.forward(training=True)')
    return [lvl.origin[2] for lvl in levels]


@torch.no_grad()
def evaluate(model, x, alpha=1., beta=1., training=False, generator=None):
    """What Trainer.test records for one cloud (trainer.py:78-101): run x through model.forward and return
    {'bce', 'bces', 'bpp', 'sum_loss', 'metrics'} — per-scale BCE and the rate estimate divided by len(x), their sum (weighted by alpha / beta; the reference records
    the plain sum, which the defaults give), and
    the metrics of the voxels the decoder keeps at each scale.  With training=False (what Trainer.test runs) the kept voxels are the
    top-k logits, k = ground-truth rows, so the metrics are get_metrics per scale.  `training=True` evaluates the teacher-forced graph
    (noise on the latent, top-k | ground truth pruning): the kept set then contains every true voxel, so recall is exactly 1.0 and
    precision / IoU tell how many extra voxels the top-k adds."""
    out_set = model(x, training=training, generator=generator) if generator is not None else model(x, training=training)
    n = float(len(x))
    bce, bce_list = 0, []
    for out_cls, ground_truth in zip(out_set['out_cls_list'], out_set['ground_truth_list']):
        curr_bce = get_bce(out_cls, ground_truth) / n
        bce = bce + curr_bce
        bce_list.append(curr_bce.item())
    bpp = get_bits(out_set['likelihood']) / n
    if training:
        metrics = [get_cls_metrics(kept, isin_mask(out_cls.C, ground_truth))
                   for kept, out_cls, ground_truth in zip(kept_masks(out_set), out_set['out_cls_list'], out_set['ground_truth_list'])]
    else:
        metrics = [get_metrics(out_cls, ground_truth) for out_cls, ground_truth in zip(out_set['out_cls_list'], out_set['ground_truth_list'])]
    return {'bce': bce.item(), 'bces': bce_list, 'bpp': bpp.item(), 'sum_loss': alpha * bce.item() + beta * bpp.item(), 'metrics': metrics}


def main(argv=None):
    import argparse
    import json
    from .data_utils import load_sparse_tensor
    from .pcc_model import PCCModel
    ap = argparse.ArgumentParser(description='forward losses and metrics of one cloud (what Trainer.test records)')
    ap.add_argument('--filedir', required=True, help='ASCII PLY')
    ap.add_argument('--ckptdir', required=True, help="checkpoint: torch.load(path)['model']")
    ap.add_argument('--training', action='store_true', help='teacher-forced graph: noise on the latent, top-k | ground truth pruning')
    ap.add_argument('--alpha', type=float, default=1.)
    ap.add_argument('--beta', type=float, default=1.)
    args = ap.parse_args(argv)
    device = torch.device('cuda')
    model = PCCModel().to(device)
    model.load_state_dict(torch.load(args.ckptdir, map_location=device)['model'])
    x = load_sparse_tensor(args.filedir, device)
    print(json.dumps(evaluate(model, x, alpha=args.alpha, beta=args.beta, training=args.training)))


if __name__ == '__main__':
    main()
