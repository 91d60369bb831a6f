"""fp64 restatement (numpy) of the forward losses the device kernels of csrc/loss.hip compute: the bottleneck likelihood and its bits
(reference entropy_model.py:82-101,112-140, loss.py:17-20), coordinate membership (data_utils.py:63-75), BCE with logits in bits and
the classification metrics (loss.py:8-15,30-40).  Written from the formulas; shares no code with the package, the oracle or the
reference.  tests/test_eval_loss_cpu.py pins it to the reference's own fp64 answers (tests/golden/eval_loss.npz) to 1e-12 relative
before the GPU is judged by it."""
import math

import numpy as np

import fp64_reference as R

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


def bce_terms(logits, mask):
    """the per-row term max(x, 0) - x y + log1p(exp(-|x|)) in fp64 (natural units: not divided by ln 2); any non-zero mask byte is set"""
    x = np.asarray(logits, np.float64).ravel()
    y = (np.asarray(mask).ravel() != 0).astype(np.float64)
    return np.maximum(x, 0.0) - x * y + np.log1p(np.exp(-np.abs(x)))


def exact_sum(a):
    """the correctly rounded sum (math.fsum) of the flattened array"""
    return math.fsum(np.asarray(a, np.float64).ravel().tolist())


def sum_bound(terms, ulps):
    """how far an fp64 sum of the m terms, added in ANY order, may lie from exact_sum when every term carries `ulps` ulp of its own:
    BOUND_SLACK (m + ulps) 2^-53 sum |terms| (Higham eq. 3.5 to first order, the form fp64_reference uses; the slack covers the rest)"""
    t = np.asarray(terms, np.float64)
    return R.BOUND_SLACK * (t.size + ulps) * 2.0 ** -53 * exact_sum(np.abs(t))


def tile_channels(params, C):
    """packed parameters for C channels taken from a C = 8 packing: channel c <- c % 8, tensor by tensor in packing order"""
    idx = np.arange(C) % 8
    return np.concatenate([t[idx].ravel() for lst in eb_unpack(params, 8) for t in lst]).astype(np.asarray(params).dtype)


# ---- inputs of tests/test_loss_reductions_*.py: the CPU file proves on them that a reduction slip cannot hide inside the bound, the GPU
# file runs the kernels on them.  A case of n rows is the first n rows of ONE seeded draw, so a reference computed on the largest serves all.
BCE_BLOCK_ROWS = 1024                                            # rows one workgroup of the BCE pass covers
LIK_BLOCK = 256                                                  # elements one workgroup of the likelihood / -log2 passes covers
SLOTS = 256                                                      # stride of the second stage: slot s is added by thread s % 256
BCE_SIZES = (0, 1, 3, 4, 5, 1023, 1024, 1025, 262143, 262144, 262145, 263169, 600001)
LIK_ROWS_C8 = (0, 1, 31, 32, 33, 8191, 8192, 8193, 20001)
OTHER_CHANNELS = (1, 3, 5, 16)
# +-0, the smallest denormal, tiny, ordinary, where exp(-|x|) leaves fp32 / falls below 2^-53 / turns denormal / underflows in fp64, huge
BCE_VALUES = np.array([s * v for v in (0.0, 2.0 ** -149, 1e-30, 1.0, 17.0, 40.0, 88.7, 104.0, 745.0, 800.0, 1e6, np.finfo(np.float32).max)
                       for s in (1.0, -1.0)], np.float32)


def lik_rows(C):
    return LIK_ROWS_C8 if C == 8 else (1, 256 // C, 256 // C + 1, 65536 // C, 65536 // C + 1)


def bce_case(n):
    """-> (logits fp32 [n] uniform in [-4, 4] with exact +0 and -0 planted, truth uint8 [n], pred uint8 [n]); the masks hold the byte
    values {0, 1, 2, 255} (non-zero means set) in a pattern without a period"""
    if not hasattr(bce_case, 'full'):
        rng = np.random.default_rng(2024)
        m = max(BCE_SIZES)
        x = rng.uniform(-4.0, 4.0, size=m).astype(np.float32)
        x[0::97] = 0.0
        x[50::97] = -0.0
        vals = np.array([0, 0, 1, 2, 255], np.uint8)
        bce_case.full = (x, vals[rng.integers(0, 5, size=m)], vals[rng.integers(0, 5, size=m)])
    return tuple(a[:n].copy() for a in bce_case.full)


def latent_case(n, C):
    """-> fp32 [n, C]: integers in [-14, 14] plus U(-0.5, 0.5)"""
    cache = latent_case.__dict__.setdefault('full', {})
    if C not in cache:
        rng = np.random.default_rng(3000 + C)
        m = max(lik_rows(C))
        cache[C] = (rng.integers(-14, 15, size=(m, C)) + rng.uniform(-0.5, 0.5, size=(m, C))).astype(np.float32)
    return cache[C][:n].copy()


GRAD_BASE_ROWS = 2049


def grad_rows(C):
    rows = (0, 1, 255, 256, 257, 2049, 20001) if C == 8 else (1, 8 * (256 // C), 8 * (256 // C) + 1, 2049)
    return tuple(dict.fromkeys(rows))


def gradient_case(n, C):
    """-> (y fp32 [n, C], idx int64 [n]): y = base[idx] for ONE seeded base of 2 049 rows per C — latent_case's distribution with every
    seventh row far in the tails, where the likelihood is at its bound; the first n base rows, or (n > 2 049) rows sampled with replacement"""
    cache = gradient_case.__dict__.setdefault('base', {})
    if C not in cache:
        rng = np.random.default_rng(5000 + C)
        m = GRAD_BASE_ROWS
        y = rng.integers(-14, 15, size=(m, C)) + rng.uniform(-0.5, 0.5, size=(m, C))
        tails = np.arange(3, m, 7)
        y[tails] = rng.choice([-1.0, 1.0], size=(len(tails), C)) * rng.uniform(60.0, 400.0, size=(len(tails), C))
        cache[C] = y.astype(np.float32)
    idx = np.arange(n) if n <= GRAD_BASE_ROWS else np.random.default_rng(6000 + C).integers(0, GRAD_BASE_ROWS, size=n)
    return cache[C][idx].copy(), idx


def likelihood_samples():
    """1 000 fp32 likelihoods in [1e-9, 0.1], log-uniform, both ends included"""
    rng = np.random.default_rng(4000)
    v = np.exp(rng.uniform(np.log(1e-9), np.log(0.1), size=1000)).astype(np.float32)
    v[0], v[1] = np.float32(1e-9), np.float32(0.1)
    return np.clip(v, np.float32(1e-9), np.float32(0.1))


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
