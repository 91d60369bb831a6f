"""fp64 restatement (numpy) of the forward losses the device kernels of csrc/loss.hip compute: the bottleneck likelihood and its bits
(reference entropy_model.py:82-101,112-140, loss.py:17-20), coordinate membership (data_utils.py:63-75), BCE with logits in bits and
the classification metrics (loss.py:8-15,30-40).  Written from the formulas; shares no code with the package, the oracle or the
reference.  tests/test_eval_loss_cpu.py pins it to the reference's own fp64 answers (tests/golden/eval_loss.npz) to 1e-12 relative
before the GPU is judged by it."""
import numpy as np

FILTERS = (1, 3, 3, 3, 1)
# what the reference divides by: torch.log(torch.tensor(2.0)) is an fp32 tensor even when the logits are fp64 (loss.py:13)
LN2_REFERENCE = float(np.log(np.float32(2.0), dtype=np.float32))


def eb_unpack(params, C=8):
    """packed fp32 parameters (matrices 0..3 | biases 0..3 | factors 0..3) -> three lists of fp64 arrays [C, fo, fi] / [C, fo, 1]"""
    p = np.asarray(params, np.float64)
    out, off = [], 0
    shapes = [(C, FILTERS[i + 1], FILTERS[i]) for i in range(4)] + [(C, FILTERS[i + 1], 1) for i in range(4)] * 2
    for shp in shapes:
        n = int(np.prod(shp))
        out.append(p[off:off + n].reshape(shp))
        off += n
    assert off == len(p)
    return out[0:4], out[4:8], out[8:12]


def _softplus(x):
    return np.logaddexp(0.0, x)


def _sigmoid(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def logits_cumulative(params, v):
    """v: fp64 [n, C] -> logits [n, C]: four layers z <- softplus(M) z + b; z <- z + tanh(f) tanh(z)"""
    mats, biases, factors = eb_unpack(params, v.shape[1])
    z = v.T[:, None, :]                                          # [C, 1, n]
    for M, b, f in zip(mats, biases, factors):
        z = np.matmul(_softplus(M), z) + b
        z = z + np.tanh(f) * np.tanh(z)
    return z[:, 0, :].T


def likelihood(params, y, bound=1e-9):
    """|sigmoid(s up) - sigmoid(s lo)| with s = -sign(lo + up), bounded below -> fp64 [n, C]"""
    y = np.asarray(y, np.float64)
    lo, up = logits_cumulative(params, y - 0.5), logits_cumulative(params, y + 0.5)
    s = -np.sign(lo + up)
    return np.maximum(np.abs(_sigmoid(s * up) - _sigmoid(s * lo)), bound)


def bits(lik):
    return float(-np.sum(np.log2(np.asarray(lik, np.float64))))


def coord_keys(c):
    """[n, 4] (batch, x, y, z), 0 <= x, y, z < 2^20, batch < 16 -> one int64 per row"""
    c = np.asarray(c, np.int64)
    return (c[:, 0] << 60) | (c[:, 3] << 40) | (c[:, 2] << 20) | c[:, 1]


def isin(data, truth):
    """membership by binary search in the sorted keys of `truth`"""
    k = np.sort(coord_keys(truth))
    q = coord_keys(data)
    if len(k) == 0:
        return np.zeros(len(q), bool)
    pos = np.minimum(np.searchsorted(k, q), len(k) - 1)
    return k[pos] == q


def bce_bits(logits, mask, ln2=np.log(2.0)):
    """sum_i max(x, 0) - x y + log1p(exp(-|x|)), in bits"""
    x = np.asarray(logits, np.float64).ravel()
    y = np.asarray(mask, np.float64).ravel()
    return float(np.sum(np.maximum(x, 0.0) - x * y + np.log1p(np.exp(-np.abs(x)))) / ln2)


def counts(pred, real):
    pred, real = np.asarray(pred, bool), np.asarray(real, bool)
    return int((pred & real).sum()), int((~pred & real).sum()), int((pred & ~real).sum()), int((~pred & ~real).sum())


def cls_metrics(pred, real):
    TP, FN, FP, _ = counts(pred, real)
    return [round(TP / (TP + FP + 1e-7), 4), round(TP / (TP + FN + 1e-7), 4), round(TP / (TP + FP + FN + 1e-7), 4)]


def topk_mask(vals, k):
    """the k largest; equal values: the lower row first"""
    v = np.asarray(vals, np.float32).ravel() + np.float32(0)
    mask = np.zeros(len(v), bool)
    mask[np.argsort(-v, kind='stable')[:int(min(len(v), k))]] = True
    return mask
