"""GPU tests of the forward half of the training graph: isin / likelihood / bits / BCE / metrics on device against the reference's
answers (tests/golden/eval_loss.npz) and the tests' fp64 restatement (tests/eval_reference.py); PCCModel.forward in both modes against a
decoder assembled from the oracle's primitives; loss.evaluate.

Tolerances.  The device evaluates the likelihood and the sums in fp64 and rounds once to fp32, so against the reference's fp64 answer it
may deviate by that one rounding (2^-23 relative covers it) or by what the reference's own fp32 arithmetic deviates (the fixture carries
both columns), whichever is larger — never by more."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import eval_reference as er
from oracle import pcgc_oracle as orc
from pcgcv2_amd import data_utils, loss, ops, synthetic
from pcgcv2_amd.sparse import SparseTensor, sparse_collate

DEV = torch.device('cuda:0')
ONE_ROUNDING = 2.0 ** -23
BOUND32 = np.float32(1e-9)


def _t(a, dt=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(DEV)


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'eval_loss.npz'))


@pytest.fixture(scope='module')
def sd():
    return synthetic.synthetic_state_dict()


@pytest.fixture(scope='module')
def sd_np(sd):
    return synthetic.state_dict_to_numpy(sd)


@pytest.fixture(scope='module')
def model(sd):
    from pcgcv2_amd.pcc_model import PCCModel
    m = PCCModel().to(DEV)
    m.load_state_dict(sd)
    return m


def _cloud(names):
    """one shell, or several collated into a batch (items overlap in space: only the batch index keeps them apart)"""
    clouds = [synthetic.shell(nm) for nm in names]
    coords, feats = sparse_collate(clouds, [torch.ones((len(c), 1)) for c in clouds])
    return SparseTensor(feats, coordinates=coords, tensor_stride=1, device=DEV)


def _rows(c):
    return set(map(tuple, np.asarray(c).tolist()))


# ------------------------------------------------------------------------------------------------ isin
def test_isin_equals_the_reference_mask(golden):
    for i in range(int(golden['n_bce'])):
        c, t = golden[f'e{i}_coords'], golden[f'e{i}_truth']
        got = data_utils.isin(_t(c), _t(t))
        assert got.dtype == torch.bool and got.device.type == 'cuda'
        np.testing.assert_array_equal(got.cpu().numpy(), golden[f'e{i}_isin'])
        # the truth given as a sparse tensor: probed through the level's own table
        gt = SparseTensor(torch.ones((len(t), 1)), coordinates=_t(t), tensor_stride=1, device=DEV)
        np.testing.assert_array_equal(data_utils.isin(_t(c), gt).cpu().numpy(), golden[f'e{i}_isin'])


@pytest.mark.parametrize('n,m,hi,seed', [(1000, 700, 12, 0), (4097, 5000, 40, 1), (63, 1, 4, 2), (130001, 90000, 1 << 20, 3), (257, 0, 9, 4)])
def test_isin_on_random_clouds(n, m, hi, seed):
    """duplicate rows in `data`, the same xyz in two batch items, both ends of the coordinate range, an empty ground truth, row counts
    that are no multiple of a wave"""
    rng = np.random.default_rng(seed)
    data = np.concatenate([rng.integers(0, 16, size=(n, 1)), rng.integers(0, hi, size=(n, 3))], 1).astype(np.int32)
    truth = np.concatenate([rng.integers(0, 16, size=(m, 1)), rng.integers(0, hi, size=(m, 3))], 1).astype(np.int32)
    data[n // 2:n // 2 + n // 8] = data[:n // 8]                                   # duplicates in data
    top = (1 << 20) - 1
    ends = np.array([[0, 0, 0, 0], [0, top, top, top], [15, top, top, 0], [15, 0, 0, 0], [7, top, 0, top]], np.int32)
    data[:5] = ends
    if m >= 5000:
        truth[:3] = ends[[1, 2, 4]]
        same_xyz = data[10:40].copy()                                              # in the truth under ANOTHER batch index only
        same_xyz[:, 0] = (same_xyz[:, 0] + 1) % 16
        truth[10:40] = same_xyz
        truth[50:300] = data[50:300]
    want = np.isin(er.coord_keys(data), er.coord_keys(truth))
    assert np.array_equal(want, er.isin(data, truth))
    got = data_utils.isin(_t(data), _t(truth))
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    # "top-k | truth" in one launch
    other = rng.random(n) < 0.3
    fused = data_utils.isin_mask(_t(data), _t(truth), or_mask=_t(other.astype(np.uint8)))
    np.testing.assert_array_equal(fused.cpu().numpy().astype(bool), want | other)


# ------------------------------------------------------------------------------------------------ likelihood / bits
def _bottleneck(params):
    from pcgcv2_amd.entropy_model import EntropyBottleneck
    eb = EntropyBottleneck(8)
    mats, biases, factors = er.eb_unpack(params)
    with torch.no_grad():
        for lst, vals in ((eb._matrices, mats), (eb._biases, biases), (eb._factors, factors)):
            for p, v in zip(lst, vals):
                p.copy_(torch.from_numpy(v.astype(np.float32)))
    return eb.to(DEV)


def _rel(a, ref):
    return float(np.max(np.abs(np.asarray(a, np.float64) - ref) / ref))


def test_likelihood_and_bits_against_the_reference(golden):
    for i in range(int(golden['n_bottleneck'])):
        kind, params, y = str(golden[f'b{i}_kind']), golden[f'b{i}_params'], golden[f'b{i}_y']
        lik32, lik64 = golden[f'b{i}_lik32'], golden[f'b{i}_lik64']
        bits32, bits64 = float(golden[f'b{i}_bits32']), float(golden[f'b{i}_bits64'])
        eb = _bottleneck(params)
        out, lik_t = eb(_t(y), quantize_mode=None)
        assert out.data_ptr() == _t(y).data_ptr() or torch.equal(out, _t(y))
        lik = lik_t.cpu().numpy()
        assert lik.dtype == np.float32 and lik.shape == y.shape
        allow = max(_rel(lik32, lik64), ONE_ROUNDING)
        dev = _rel(lik, lik64)
        bits = float(loss.get_bits(lik_t).item())
        allow_bits = max(abs(bits32 - bits64) / bits64, ONE_ROUNDING)
        dev_bits = abs(bits - bits64) / bits64
        print(f'case {i} ({kind}): likelihood rel {dev:.3e} (allowed {allow:.3e}); bits rel {dev_bits:.3e} (allowed {allow_bits:.3e})')
        assert dev <= allow
        assert dev_bits <= allow_bits
        # elements at the bound are exactly 1e-9f
        at_bound = lik64 == 1e-9
        assert np.all(lik[at_bound] == BOUND32) and np.all(lik >= BOUND32)
        if kind == 'tails':
            assert at_bound.any()
        # the unbounded form differs exactly where the bound acts
        raw = eb._likelihood(_t(y)).cpu().numpy()
        np.testing.assert_array_equal(np.maximum(raw, BOUND32), lik)
        # the fused rate (likelihood pointer null) is the same double as get_bits of the stored tensor
        _, fused = ops.eb_likelihood(_t(y), eb.packed_params(DEV), want_likelihood=False, want_bits=True)
        assert float(fused.item()) == float(ops.neg_log2_sum(lik_t).item())
        if kind == 'int':
            # the same formula in fp64, one cast: the oracle's table entries, bit for bit
            lo, hi = float(y.min()), float(y.max())
            table = np.maximum(orc.likelihood(params, lo, hi), BOUND32)                 # [L, 8]
            want = table[(y - lo).astype(np.int64), np.arange(8)[None, :]]
            np.testing.assert_array_equal(lik, want)
        # a strided view (columns of a wider tensor) gives the same values
        wide = torch.zeros((len(y), 12), dtype=torch.float32, device=DEV)
        wide[:, 2:10] = _t(y)
        np.testing.assert_array_equal(eb(wide[:, 2:10], quantize_mode=None)[1].cpu().numpy(), lik)


def test_quantize_modes(golden):
    eb = _bottleneck(golden['b1_params'])
    y = _t(golden['b1_y'])
    out, lik = eb(y, quantize_mode='symbols')
    np.testing.assert_array_equal(out.cpu().numpy(), np.rint(golden['b1_y']))
    np.testing.assert_array_equal(lik.cpu().numpy(), eb(torch.round(y), quantize_mode=None)[1].cpu().numpy())
    g = torch.Generator(device=DEV); g.manual_seed(5)
    a, _ = eb(y, quantize_mode='noise', generator=g)
    g.manual_seed(5)
    b, _ = eb(y, generator=g)                                                          # "noise" is the default mode
    assert torch.equal(a, b)
    d = a.double().cpu().numpy() - golden['b1_y'].astype(np.float64)
    assert d.min() >= -0.5 and d.max() < 0.5 and d.std() > 0.2
    with pytest.raises(Exception):
        eb(y, quantize_mode='nearest')


# ------------------------------------------------------------------------------------------------ BCE / metrics
def _bce_case(golden, i):
    c, t, logits = golden[f'e{i}_coords'], golden[f'e{i}_truth'], golden[f'e{i}_logits']
    data = SparseTensor(_t(logits.reshape(-1, 1)), coordinates=_t(c), tensor_stride=1, device=DEV)
    truth = SparseTensor(torch.ones((len(t), 1)), coordinates=_t(t), tensor_stride=1, device=DEV)
    np.testing.assert_array_equal(data.C.cpu().numpy(), c)                             # (unique rows: the constructor keeps them as they are)
    return data, truth


def test_bce_counts_and_metrics_against_the_reference(golden):
    for i in range(int(golden['n_bce'])):
        data, truth = _bce_case(golden, i)
        assert data.cmap.batch_rows == golden[f'e{i}_rows'].tolist() and truth.cmap.batch_rows == golden[f'e{i}_nums'].tolist()
        bce32, bce64 = float(golden[f'e{i}_bce32']), float(golden[f'e{i}_bce64'])
        got = loss.get_bce(data, truth)
        assert got.dim() == 0 and got.device.type == 'cuda' and got.dtype == torch.float32
        allow = max(abs(bce32 - bce64) / bce64, ONE_ROUNDING)
        dev = abs(float(got.item()) - bce64) / bce64
        print(f'case {i}: bce rel {dev:.3e} (allowed {allow:.3e})')
        assert dev <= allow
        mask, pred = golden[f'e{i}_isin'], golden[f'e{i}_pred']
        # the fp64 sum before its one rounding, against the restatement
        bce_d, counts = ops.bce_logits(data.F, _t(mask.astype(np.uint8)), _t(pred.astype(np.uint8)))
        assert abs(float(bce_d.item()) - er.bce_bits(golden[f'e{i}_logits'], mask)) <= 1e-12 * bce64
        assert tuple(counts.tolist()) == er.counts(pred, mask)
        assert loss.get_metrics(data, truth) == golden[f'e{i}_metrics'].tolist()
        assert loss.get_cls_metrics(_t(pred), _t(mask)) == golden[f'e{i}_metrics'].tolist()
        np.testing.assert_array_equal(data_utils.istopk(data, golden[f'e{i}_nums'].tolist()).cpu().numpy(), pred)
        # strided and unaligned logits take the scalar loads: the same partition, the same double
        n = len(mask)
        wide = torch.zeros((n, 3), dtype=torch.float32, device=DEV)
        wide[:, 1] = data.F[:, 0]
        b2, c2 = ops.bce_logits(wide[:, 1:2], _t(mask.astype(np.uint8)), _t(pred.astype(np.uint8)))
        shifted = torch.zeros(n + 1, dtype=torch.float32, device=DEV)
        shifted[1:] = data.F[:, 0]
        b3, c3 = ops.bce_logits(shifted[1:], _t(mask.astype(np.uint8)), _t(pred.astype(np.uint8)))
        assert float(b2.item()) == float(bce_d.item()) == float(b3.item()) and c2.tolist() == counts.tolist() == c3.tolist()


# ------------------------------------------------------------------------------------------------ PCCModel.forward
def _item_slices(rows):
    off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    return [slice(int(a), int(b)) for a, b in zip(off[:-1], off[1:])]


def _oracle_decoder(sd_np, C8, F8, nums_list, truths=None):
    """the decoder (autoencoder.py:251-273) from the oracle's primitives; pruning keeps, per batch item, the top-k logits — and, with
    `truths` (teacher forcing, autoencoder.py:241-244), every candidate that is a ground-truth voxel.  -> (cls levels [(C, F)], kept masks,
    the no-tie-at-a-threshold flag, out coordinates)"""
    C_, x, stride = np.ascontiguousarray(C8, np.int32), F8, 8
    cls_list, masks, no_tie = [], [], True
    for l in range(3):
        x = orc.relu(orc.conv_up2(x, sd_np[f'decoder.up{l}.kernel'], sd_np[f'decoder.up{l}.bias']))
        lvl = orc.Level(orc.children_coords(C_, stride), stride // 2)
        stride //= 2
        x = orc.relu(orc._conv3(sd_np, f'decoder.conv{l}', lvl, x))
        x = orc._block(sd_np, f'decoder.block{l}', lvl, x)
        cls = orc._conv3(sd_np, f'decoder.conv{l}_cls', lvl, x)
        cls_list.append((lvl.C, cls))
        rows = [int((lvl.C[:, 0] == b).sum()) for b in range(len(nums_list[l]))]
        assert np.all(np.diff(lvl.C[:, 0]) >= 0)                                       # items are contiguous
        mask = np.zeros(len(lvl.C), bool)
        for sl, k in zip(_item_slices(rows), nums_list[l]):
            v = cls[sl, 0]
            mask[sl] = orc.topk_mask(v, k)
            s = np.sort(v + np.float32(0))[::-1]
            if 0 < k < len(s) and s[k - 1] == s[k]:
                no_tie = False
        if truths is not None:
            mask |= np.isin(er.coord_keys(lvl.C), er.coord_keys(truths[l]))
        masks.append(mask)
        C_, x = lvl.C[mask], x[mask]
    return cls_list, masks, no_tie, C_


def _np(t):
    return t.cpu().numpy()


@pytest.mark.parametrize('names', [['shell7'], ['shell7', 'shell6', 'shell8']])
def test_forward_inference_equals_oracle_and_coder(model, sd_np, names, tmp_path):
    from pcgcv2_amd.coder import Coder
    x = _cloud(names)
    out = model(x, training=False)
    assert set(out) == {'out', 'out_cls_list', 'prior', 'likelihood', 'ground_truth_list'}
    y_list = model.encoder(x)
    y = y_list[0]
    # ground truths: the encoder's two finer levels and the input
    assert len(out['ground_truth_list']) == 3 and out['ground_truth_list'][2] is x
    for gt, lvl in zip(out['ground_truth_list'][:2], y_list[1:]):
        np.testing.assert_array_equal(_np(gt.C), _np(lvl.C))
        np.testing.assert_array_equal(_np(gt.F), _np(lvl.F))
    np.testing.assert_array_equal(_np(out['prior'].C), _np(y.C))
    np.testing.assert_array_equal(_np(out['prior'].F), np.rint(_np(y.F)))
    np.testing.assert_array_equal(_np(out['likelihood']), _np(model.entropy_bottleneck(torch.round(y.F), quantize_mode=None)[1]))
    nums_list = [gt.cmap.batch_rows for gt in out['ground_truth_list']]
    assert nums_list[2] == [len(synthetic.shell(nm)) for nm in names]
    cls_ref, masks, no_tie, out_C = _oracle_decoder(sd_np, _np(y.C), np.rint(_np(y.F)), nums_list)
    assert no_tie, 'a tie straddles a top-k threshold: the coder (sorted latent) may keep another row'
    for l in range(3):
        np.testing.assert_array_equal(_np(out['out_cls_list'][l].C), cls_ref[l][0])
        np.testing.assert_array_equal(_np(out['out_cls_list'][l].F), cls_ref[l][1])
    np.testing.assert_array_equal(_np(out['out'].C), out_C)
    if len(names) == 1:
        C1, _, cls1 = orc.decoder_forward(sd_np, _np(y.C), np.rint(_np(y.F)), [n[0] for n in nums_list], return_cls=True)
        for l in range(3):
            np.testing.assert_array_equal(_np(out['out_cls_list'][l].C), cls1[l][0])
            np.testing.assert_array_equal(_np(out['out_cls_list'][l].F), cls1[l][1])
        np.testing.assert_array_equal(_np(out['out'].C), C1)
    # the coder's decoded cloud(s), as sets of rows
    coder = Coder(model, str(tmp_path / 'c'))
    got = _np(out['out'].C)
    if len(names) == 1:
        coder.encode(x)
        assert _rows(got) == _rows(_np(coder.decode().C))
    else:
        posts = [f'_i{i}' for i in range(len(names))]
        coder.encode_batch(x, posts)
        for b, dec in enumerate(coder.decode_batch(posts)):
            assert _rows(got[got[:, 0] == b][:, 1:]) == _rows(_np(dec.C)[:, 1:]), b


@pytest.mark.parametrize('names', [['shell7'], ['shell7', 'shell6', 'shell8']])
def test_forward_teacher_forced(model, sd_np, names):
    x = _cloud(names)
    g = torch.Generator(device=DEV); g.manual_seed(11)
    out = model(x, training=True, generator=g)
    y = model.encoder(x)[0]
    d = _np(out['prior'].F).astype(np.float64) - _np(y.F).astype(np.float64)
    assert d.min() >= -0.5 and d.max() < 0.5 and d.std() > 0.2
    # the likelihood at prior.F: one rounding of the fp64 value, bounded
    params = _np(model.entropy_bottleneck.packed_params(DEV))
    lik64 = er.likelihood(params, _np(out['prior'].F))
    lik = _np(out['likelihood'])
    dev = _rel(lik, lik64)
    print(f'{names}: likelihood rel {dev:.3e} against the fp64 restatement')
    assert dev <= ONE_ROUNDING and np.all(lik >= BOUND32)
    truths = [_np(gt.C) for gt in out['ground_truth_list']]
    nums_list = [gt.cmap.batch_rows for gt in out['ground_truth_list']]
    cls_ref, masks, _, out_C = _oracle_decoder(sd_np, _np(y.C), _np(out['prior'].F), nums_list, truths=truths)
    for l in range(3):
        np.testing.assert_array_equal(_np(out['out_cls_list'][l].C), cls_ref[l][0])
        np.testing.assert_array_equal(_np(out['out_cls_list'][l].F), cls_ref[l][1])
        # kept = top-k | truth, recomputed from the DEVICE's logits; rows in candidate order
        cls = out['out_cls_list'][l]
        C, F = _np(cls.C), _np(cls.F)
        keep = np.zeros(len(C), bool)
        for sl, k in zip(_item_slices(cls.cmap.batch_rows), nums_list[l]):
            keep[sl] = orc.topk_mask(F[sl, 0], k)
        keep |= np.isin(er.coord_keys(C), er.coord_keys(truths[l]))
        np.testing.assert_array_equal(keep, masks[l])
        assert _rows(truths[l]) <= _rows(C[keep])                                      # every true voxel of the level is a candidate and survives
    np.testing.assert_array_equal(_np(out['out'].C), out_C)
    assert _rows(_np(x.C)) <= _rows(_np(out['out'].C))
    # inference mode takes the codec's path and is not disturbed by the teacher-forced run
    again = model(x, training=False)
    assert len(again['out']) == sum(nums_list[2])


def test_me_sparse_tensor_on_another_tensors_coordinates(model):
    """pcc_model.py:18-23: ME.SparseTensor(features=, coordinate_map_key=, coordinate_manager=, device=) shares the coordinates (and the
    cached maps) of the tensor the key was taken from"""
    from pcgcv2_amd import ME
    c = synthetic.shell('shell6')
    coords, feats = ME.utils.sparse_collate([c], [torch.ones((len(c), 1))])
    a = ME.SparseTensor(features=feats, coordinates=coords, tensor_stride=1, device=DEV)
    f = torch.arange(len(a), dtype=torch.float32, device=DEV).reshape(-1, 1)
    b = ME.SparseTensor(features=f, coordinate_map_key=a.coordinate_map_key, coordinate_manager=a.coordinate_manager, device=a.device)
    assert b.cmap is a.cmap and b.coordinate_map_key is a.coordinate_map_key and torch.equal(b.F, f) and torch.equal(b.C, a.C)
    assert [len(d) for d in b.decomposed_coordinates] == [len(c)]
    with pytest.raises(ValueError):
        ME.SparseTensor(features=f, coordinates=coords, coordinate_map_key=a.coordinate_map_key)


# ------------------------------------------------------------------------------------------------ evaluate
def test_evaluate_is_the_composition_and_reproducible(model):
    x = _cloud(['shell7', 'shell6'])
    n = float(len(x))
    rec = loss.evaluate(model, x)
    assert set(rec) == {'bce', 'bces', 'bpp', 'sum_loss', 'metrics'}
    out = model(x, training=False)
    bces = [float((loss.get_bce(c, t) / n).item()) for c, t in zip(out['out_cls_list'], out['ground_truth_list'])]
    bce = 0
    for c, t in zip(out['out_cls_list'], out['ground_truth_list']):
        bce = bce + loss.get_bce(c, t) / n
    bpp = float((loss.get_bits(out['likelihood']) / n).item())
    assert rec['bces'] == bces and rec['bce'] == float(bce.item()) and rec['bpp'] == bpp
    assert rec['sum_loss'] == rec['bce'] + rec['bpp']
    assert rec['metrics'] == [loss.get_metrics(c, t) for c, t in zip(out['out_cls_list'], out['ground_truth_list'])]
    # determinism: a second run on a fresh stream gives the same bits
    for _ in range(2):
        s = torch.cuda.Stream(device=DEV)
        s.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(s):
            rec2 = loss.evaluate(model, x)
        s.synchronize()
        assert rec2['bpp'] * n == rec['bpp'] * n and rec2['bces'] == rec['bces'] and rec2 == rec


def test_evaluate_teacher_forced_recall(model):
    """with training=True the recall at every level is exactly 1.0: evaluate scores the voxels the decoder KEEPS (top-k | ground truth
    under teacher forcing; the plain top-k, i.e. get_metrics, in inference mode).  The top-k of the logits alone has a recall of about
    0.44 / 0.34 / 0.28 with the synthetic weights in either mode (oracle, shell7 + shell6) — teacher forcing changes which voxels
    survive, not how the logits rank — so the 1.0 really is the ground-truth half of the mask."""
    x = _cloud(['shell7', 'shell6'])
    g = torch.Generator(device=DEV); g.manual_seed(3)
    rec = loss.evaluate(model, x, training=True, generator=g)
    print('teacher-forced metrics [precision, recall, IoU] per level:', rec['metrics'])
    assert [m[1] for m in rec['metrics']] == [1.0, 1.0, 1.0]
    g.manual_seed(3)
    out = model(x, training=True, generator=g)
    kept = loss.kept_masks(out)
    for l, (cls, gt) in enumerate(zip(out['out_cls_list'], out['ground_truth_list'])):
        real = np.isin(er.coord_keys(_np(cls.C)), er.coord_keys(_np(gt.C)))
        assert int(real.sum()) == len(gt)
        assert rec['metrics'][l] == er.cls_metrics(_np(kept[l]).astype(bool), real)
        assert 0 < rec['metrics'][l][0] < 1 and rec['metrics'][l][0] == rec['metrics'][l][2]      # (recall 1: precision = IoU)
        topk = loss.get_metrics(cls, gt)
        assert topk[1] < 1.0 and topk[0] == topk[1]                                               # k = truth rows: precision = recall
    n = float(len(x))
    assert rec['bces'] == [float((loss.get_bce(c, t) / n).item()) for c, t in zip(out['out_cls_list'], out['ground_truth_list'])]
    assert rec['bpp'] == float((loss.get_bits(out['likelihood']) / n).item())


# ------------------------------------------------------------------------------------------------ full size
def test_full_size_frame(model, tmp_path):
    """the benchmark's vox10 frame (shell10, 786 632 points) through forward(training=False) and evaluate; out.C against the coder's
    decoded cloud as a set.  The no-tie precondition is checked on the device's own logits (bit-equal to the oracle's on the small
    clouds above; the oracle needs minutes for this one)."""
    from pcgcv2_amd.coder import Coder
    x = _cloud(['shell10'])
    assert len(x) == 786632
    out = model(x, training=False)
    for cls, gt in zip(out['out_cls_list'], out['ground_truth_list']):
        v = torch.sort(cls.F[:, 0] + 0.0, descending=True).values
        k = len(gt)
        assert 0 < k < len(v) and bool((v[k - 1] != v[k]).item()), 'a tie straddles a top-k threshold'
    coder = Coder(model, str(tmp_path / 'f'))
    coder.encode(x)
    dec = coder.decode()
    assert len(out['out']) == len(dec) == len(x)
    a = np.sort(er.coord_keys(_np(out['out'].C)))
    b = np.sort(er.coord_keys(_np(dec.C)))
    np.testing.assert_array_equal(a, b)
    rec = loss.evaluate(model, x)
    print('shell10:', rec, ' F.bin bits per input point:', 8 * os.path.getsize(str(tmp_path / 'f_F.bin')) / len(x))
    assert np.isfinite(rec['bpp']) and rec['bpp'] > 0 and all(np.isfinite(b) and b > 0 for b in rec['bces'])
    rec_t = loss.evaluate(model, x, training=True)
    assert np.isfinite(rec_t['sum_loss'])
