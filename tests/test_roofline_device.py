"""The roofline records of real launches (one encode + decode of shell8 under three dispatch records, tools/record_roofline.py) against the
fixture recorded before the accounting moved to pcgcv2_amd/roofline.py: keys, kernel strings, launch counts, pair counts, bytes and flops are
integers and strings, so they must be EQUAL."""
import importlib.util
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _recorder():
    spec = importlib.util.spec_from_file_location('record_roofline', os.path.join(ROOT, 'tools', 'record_roofline.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_records_equal_the_fixture_and_every_launcher_fires():
    from pcgcv2_amd import ops
    rec = _recorder()
    with open(os.path.join(ROOT, 'tests', 'golden', 'roofline_records.json')) as f:
        want = json.load(f)
    keep = ops.PATH
    try:
        records, decoded = rec.run(want['cloud'])
    finally:
        ops.configure(keep)
        ops.PROFILE.reset(enabled=False)
    assert rec.missing(records) == []
    assert not ops.PROFILE.enabled and not ops.PROFILE.counting and ops.PATH == keep
    got = json.loads(json.dumps(records))                       # (tuples -> lists, as the fixture went through)
    assert sorted(got) == sorted(want['records'])
    for name, recs in want['records'].items():
        assert [r['key'] for r in got[name]] == [r['key'] for r in recs], name
        for g, w in zip(got[name], recs):
            assert g == w, (name, w['key'])
    first = decoded['every_min_0']
    for name, c in decoded.items():
        np.testing.assert_array_equal(c, first, err_msg=f'decoded coordinates under {name}')
