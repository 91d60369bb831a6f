"""CPU-side checks of the forward losses (no GPU): the C ABI, the reference's names and argument lists, get_cls_metrics on host masks,
and the tests' own fp64 restatement (tests/eval_reference.py) against the reference's fp64 answers in tests/golden/eval_loss.npz."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import eval_reference as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'eval_loss.npz'))


def test_header_declares_the_loss_primitives():
    header = open(os.path.join(ROOT, 'include', 'pcgc_hip.h')).read()
    declared = set(re.findall(r'\b(pcgc_\w+)\s*\(', re.sub(r'/\*.*?\*/', '', header, flags=re.S)))
    assert {'pcgc_hash_contains', 'pcgc_eb_likelihood', 'pcgc_bce_logits'} <= declared
    from pcgcv2_amd._lib import lib
    for name in ('pcgc_hash_contains', 'pcgc_eb_likelihood', 'pcgc_bce_logits', 'pcgc_neg_log2_sum', 'pcgc_loss_workspace_bytes'):
        assert hasattr(lib(), name)


def _args(fn):
    return list(inspect.signature(fn).parameters)


def test_reference_names_and_argument_lists():
    """the reference's definitions (loss.py:8,17,22,30; pcc_model.py:15,26; entropy_model.py:103,112,132; autoencoder.py:239,251;
    data_utils.py:63): same names, the reference's arguments first and in its order"""
    from pcgcv2_amd import loss, pcc_model, entropy_model, autoencoder, data_utils
    assert _args(loss.get_bce) == ['data', 'groud_truth']
    assert _args(loss.get_bits) == ['likelihood']
    assert _args(loss.get_metrics) == ['data', 'groud_truth']
    assert _args(loss.get_cls_metrics) == ['pred', 'real']
    assert _args(loss.evaluate)[:4] == ['model', 'x', 'alpha', 'beta']
    assert _args(pcc_model.PCCModel.get_likelihood)[:3] == ['self', 'data', 'quantize_mode']
    assert _args(pcc_model.PCCModel.forward)[:3] == ['self', 'x', 'training']
    assert inspect.signature(pcc_model.PCCModel.forward).parameters['training'].default is True
    eb = entropy_model.EntropyBottleneck
    assert _args(eb.forward)[:3] == ['self', 'inputs', 'quantize_mode']
    assert inspect.signature(eb.forward).parameters['quantize_mode'].default == 'noise'
    assert 'generator' in _args(eb.forward)
    assert _args(eb._likelihood) == ['self', 'inputs']
    assert _args(eb._quantize)[:3] == ['self', 'inputs', 'mode']
    assert _args(autoencoder.Decoder.prune_voxel) == ['self', 'data', 'data_cls', 'nums', 'ground_truth', 'training']
    assert _args(autoencoder.Decoder.forward) == ['self', 'x', 'nums_list', 'ground_truth_list', 'training']
    assert _args(data_utils.isin) == ['data', 'ground_truth']


def test_me_sparse_tensor_takes_a_coordinate_map_key():
    from pcgcv2_amd import ME
    assert {'coordinate_map_key', 'coordinate_manager'} <= set(_args(ME.SparseTensor.__init__))
    assert isinstance(ME.SparseTensor.coordinate_map_key, property) and isinstance(ME.SparseTensor.coordinate_manager, property)


def test_get_cls_metrics_equals_the_reference(golden):
    from pcgcv2_amd import loss
    for i in range(int(golden['n_bce'])):
        pred, real = torch.from_numpy(golden[f'e{i}_pred']), torch.from_numpy(golden[f'e{i}_isin'])
        assert loss.get_cls_metrics(pred, real) == golden[f'e{i}_metrics'].tolist()
        assert er.cls_metrics(golden[f'e{i}_pred'], golden[f'e{i}_isin']) == golden[f'e{i}_metrics'].tolist()


def test_host_isin_equals_the_reference(golden):
    from pcgcv2_amd import data_utils
    for i in range(int(golden['n_bce'])):
        c, t = golden[f'e{i}_coords'], golden[f'e{i}_truth']
        assert np.array_equal(data_utils.isin(torch.from_numpy(c), torch.from_numpy(t)).numpy(), golden[f'e{i}_isin'])
        assert np.array_equal(er.isin(c, t), golden[f'e{i}_isin'])


def test_restatement_top_k_equals_the_reference(golden):
    for i in range(int(golden['n_bce'])):
        off, pred = 0, []
        for r, k in zip(golden[f'e{i}_rows'], golden[f'e{i}_nums']):
            pred.append(er.topk_mask(golden[f'e{i}_logits'][off:off + r], k))
            off += r
        assert np.array_equal(np.concatenate(pred), golden[f'e{i}_pred'])


def test_restatement_likelihood_and_bits_match_the_reference_fp64(golden):
    for i in range(int(golden['n_bottleneck'])):
        lik = er.likelihood(golden[f'b{i}_params'], golden[f'b{i}_y'])
        ref = golden[f'b{i}_lik64']
        rel = float(np.max(np.abs(lik - ref) / ref))
        rel_bits = abs(er.bits(lik) - float(golden[f'b{i}_bits64'])) / float(golden[f'b{i}_bits64'])
        print(f'case {i} ({golden[f"b{i}_kind"]}): likelihood {rel:.3e}  bits {rel_bits:.3e}')
        assert rel <= 1e-12 and rel_bits <= 1e-12


def test_restatement_bce_matches_the_reference_fp64(golden):
    for i in range(int(golden['n_bce'])):
        mask = er.isin(golden[f'e{i}_coords'], golden[f'e{i}_truth'])
        ref = float(golden[f'e{i}_bce64'])
        rel = abs(er.bce_bits(golden[f'e{i}_logits'], mask, ln2=er.LN2_REFERENCE) - ref) / ref
        # ... and the true ln 2 moves the value by the rounding of that fp32 constant only
        rel_true = abs(er.bce_bits(golden[f'e{i}_logits'], mask) - ref) / ref
        print(f'case {i}: {rel:.3e} (fp32 ln 2), {rel_true:.3e} (ln 2)')
        assert rel <= 1e-12 and rel_true <= 2.0 ** -27
