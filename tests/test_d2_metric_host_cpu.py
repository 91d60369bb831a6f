"""CPU-side checks of the device D2 metric's plumbing (no GPU): the lattice conversion of PLY coordinates and the sweep's --metric option."""
import numpy as np
import pytest

from pcgcv2_amd import pc_error as pe


def test_lattice_coords_rejects_non_integer_coordinates():
    xyz = np.array([[1.0, 2.0, 3.0], [4.0, 5.5, 6.0]])
    with pytest.raises(ValueError, match='non-integer'):
        pe.lattice_coords(xyz, 'cpu')


def test_lattice_coords_keeps_every_row():
    xyz = np.array([[1.0, 2.0, 3.0], [1.0, 2.0, 3.0], [0.0, 7.0, 9.0]])      # (duplicates stay: the host metric sees the file's rows)
    c = pe.lattice_coords(xyz, 'cpu', batch=2).numpy()
    assert c.dtype == np.int32 and c.tolist() == [[2, 1, 2, 3], [2, 1, 2, 3], [2, 0, 7, 9]]


def test_sweep_metric_option_is_checked_and_defaults_to_host():
    import inspect
    from pcgcv2_amd import test as sweep_mod
    assert inspect.signature(sweep_mod.sweep).parameters['metric'].default == 'host'
    assert inspect.signature(sweep_mod.test).parameters['metric'].default == 'host'
    with pytest.raises(ValueError, match='metric'):
        next(sweep_mod.sweep('unused.ply', [], 'unused', metric='gpu'))
    with pytest.raises(SystemExit):
        sweep_mod.main(['--metric', 'gpu'])
