"""pcgcv2_amd/roofline.py without a GPU: the accounting functions against the recorded fixture (tests/golden/roofline_records.json, written by
tools/record_roofline.py from real launches) and against DESIGN.md §5's formulas written out; the report on records with plain-number timings."""
import json
import os

import pytest

from pcgcv2_amd import ops, roofline

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'roofline_records.json')
FIELDS = ('kernel', 'n_out', 'launches', 'pairs', 'gathered_bytes', 'flops', 'compulsory_bytes', 'mfma_issued_flops')
HBM = 8000.0                     # GB/s: any peak does, the tests below state their fractions against it


class _Ms:
    """stand-in for a HIP event: `start.elapsed_time(end)` -> the milliseconds `end` was given"""

    def __init__(self, ms=None):
        self.ms = ms

    def elapsed_time(self, end):
        return end.ms


def _events(times_ms):
    return [(_Ms(), _Ms(t)) for t in times_ms]


def _profile(*entries):
    """entries: (key, Work, [launch time in ms])"""
    p = roofline._Profile()
    for key, work, times in entries:
        p.records[key] = dict(work._asdict(), events=_events(times))
    return p


def _flat(kernel, n, flops, compulsory=0, issued=None):
    """a record with constant figures and its own pair count"""
    return roofline.Work(kernel, n, lambda P: 0, lambda P: flops, compulsory, issued, 1)


# ------------------------------------------------------------------------------------------------ the fixture
def _ceil(a, b):
    return (a + b - 1) // b


def _work_of(rec):
    """the Work of a fixture record, from its key, its kernel string and the recorded shapes alone"""
    key, kernel, shape = rec['key'], rec['kernel'], rec['shape']
    name = kernel.split(' (')[0]
    if key[0] == 'conv' and key[1] == 1:
        return roofline.unit_conv(kernel, key[2], key[3], mapless='k_conv_unit_coarse' in kernel)
    if key[0] == 'conv':
        Cin, Cout, n = key[1:]
        if name.startswith('k3 gather conv'):           # (the gather ladder takes its MFMA kernels from 8192 rows on, for 16 / 32 / 64 channels)
            mfma = Cin in (16, 32, 64) and Cout in (16, 32, 64) and n >= 8192
            return roofline.k3_conv(kernel, Cin, Cout, n, n_in=shape['n_in'], issued=2 * 27 * _ceil(n, 16) * 16 * Cin * Cout if mfma else None)
        if name.startswith('k_rows_conv'):
            return roofline.k3_conv(kernel, Cin, Cout, n, residual=shape['residual'], issued=2 * 27 * _ceil(n, 16) * 16 * Cin * Cout)
        assert name == 'k_conv_packed64'
        return roofline.k3_conv(kernel, 64, 64, n, issued=lambda P: 2 * (P + 8 * 27 * _ceil(n, 96)) * 64 * 64)
    if key[0] == 'child_conv':
        Cin, Cout, n = key[1:]
        n_p = n // 8
        if name.startswith('k_child_q4'):
            return roofline.child_conv(kernel, Cin, 1, n_p, issued=_ceil(n_p, 64) * 96 * 16 * 512)
        per_tile = 64 * (Cin // 16) * 4 if Cout == 1 else 216 * (Cin // 16) * (Cout // 16) * 4
        return roofline.child_conv(kernel, Cin, Cout, n_p, residual=shape['residual'], issued=_ceil(n_p, 16) * per_tile * 2048)
    if key[0] == 'down':
        return roofline.down_conv(kernel, key[1], key[2], key[3], shape['n_in'])
    if key[0] == 'up2':
        return roofline.up2_conv(kernel, key[1], key[2], key[3] // 8, rows=shape['rows'], mfma=(key[1], key[2]) in ((64, 32), (32, 16)))
    # a fused InceptionResNet pass: key = (kernel name, n)
    n = key[1]
    if name.startswith('k_irn_'):
        C = int(name.split('<')[1].split(',')[0].rstrip('>'))
        return roofline.irn_pass(1 if name.startswith('k_irn_a') else 2, kernel, n, C, n)
    variants = [(v, ps) for v in ops._IRN.values() for ps in (1, 2) if v.names[ps - 1] + v.desc == kernel]
    assert variants, kernel
    v, ps = variants[0]                                  # (k_child_irn_b<16> is pass B of two rows: same figures)
    assert all(w.per_tile[q - 1] == v.per_tile[ps - 1] and w.parent_map == v.parent_map for w, q in variants)
    C = {'k_rows_irn_a64': 64, 'k_rows_irn_b64': 64}.get(name, 16 if '<16>' in name or name.startswith('k_child_q4') else 32)
    m = n // 8 if v.parent_map else n
    return roofline.irn_pass(ps, kernel, n, C, m, _ceil(m, v.tile_rows) * v.per_tile[ps - 1] * v.mfma_flops)


def _fixture():
    with open(GOLDEN) as f:
        return json.load(f)['records']


def test_fixture_covers_every_config_and_family():
    recs = _fixture()
    assert set(recs) == {'every_min_0', 'no_quad_block', 'valu_and_gather'}
    kinds = {r['key'][0] if r['key'][0] in ('conv', 'child_conv', 'down', 'up2') else 'irn' for rs in recs.values() for r in rs}
    assert kinds == {'conv', 'child_conv', 'down', 'up2', 'irn'}


@pytest.mark.parametrize('config', ['every_min_0', 'no_quad_block', 'valu_and_gather'])
def test_accounting_functions_reproduce_the_recorded_launches(config):
    """every record of the fixture: the pure function of its shapes, pushed through detail() with as many (made-up) timings as it had launches
    and the recorded pair count, gives the recorded integers and strings"""
    recs = _fixture()[config]
    prof = roofline._Profile()
    for r in recs:
        work = _work_of(r)
        prof.records[tuple(r['key'])] = dict(work._asdict(), events=_events([0.25] * r['launches']))
        if work.pairs is None:
            assert prof.pairs.setdefault(work.n, r['pairs']) == r['pairs']          # one count per level, whichever launch counted it
    got = {d['key']: d for d in prof.detail()}
    assert len(got) == len(recs)
    for r in recs:
        d = got[tuple(r['key'])]
        assert {f: d[f] for f in FIELDS if f in d} == {f: r[f] for f in FIELDS if f in r}, r['key']


def test_design_formulas_written_out():
    """DESIGN.md §5 / SURVEY §8(d), literally, for one launch of each family"""
    P, n, Cin, Cout = 17_000, 1_000, 32, 64
    w = roofline.k3_conv('k', Cin, Cout, n)
    assert w.flops(P) == 2 * P * Cin * Cout
    assert w.gathered(P) == P * Cin * 4 + P * 8 + n * Cout * 4
    assert w.compulsory == n * Cin * 4 + 27 * n * 4 + n * Cout * 4                   # every input row, map entry and output row once
    assert roofline.k3_conv('k', Cin, Cout, n, residual=True).compulsory == w.compulsory + n * Cout * 4
    n_fine, n_coarse = 7_777, 1_000
    d = roofline.down_conv('k', Cin, Cout, n_coarse, n_fine)
    assert d.pairs == n_fine                                                          # k2 s2: P = N_fine
    assert d.flops(d.pairs) == 2 * n_fine * Cin * Cout
    assert d.gathered(d.pairs) == n_fine * Cin * 4 + n_coarse * Cout * 4
    assert d.compulsory == n_fine * Cin * 4 + 8 * n_coarse * 4 + n_coarse * Cout * 4
    assert d.mfma_issued == 2 * 8 * 1_008 * Cin * Cout                                # 16-row tiles: 1 000 -> 1 008 rows, all 8 offsets
    u = roofline.up2_conv('k', Cin, Cout, n_coarse, rows=True, mfma=False)
    assert (u.n, u.pairs, u.mfma_issued) == (8 * n_coarse, 8 * n_coarse, None)
    assert u.flops(u.pairs) == 2 * (8 * n_coarse) * Cin * Cout
    assert u.gathered(u.pairs) == (8 * n_coarse) * (Cin + Cout) * 4
    assert u.compulsory == n_coarse * Cin * 4 + 8 * n_coarse * Cout * 4 + n_coarse * 4
    # a fused pass is charged the sum of its convs; k1: N (Cin + Cout) 4 bytes, 2 N Cin Cout flops
    C, Q = 32, 8
    k3 = lambda a, b: (P * a * 4 + P * 8 + n * b * 4, 2 * P * a * b)
    k1 = lambda a, b: (n * (a + b) * 4, 2 * n * a * b)
    A, B = roofline.irn_pass(1, 'a', n, C, n), roofline.irn_pass(2, 'b', n, C, n)
    assert (A.gathered(P), A.flops(P)) == tuple(map(sum, zip(k3(C, Q), k1(C, Q))))                        # k3 C -> C/4 + k1 C -> C/4
    assert (B.gathered(P), B.flops(P)) == tuple(map(sum, zip(k3(Q, 2 * Q), k3(Q, Q), k1(Q, 2 * Q))))      # k3 C/4 -> C/2 + k3 C/4 -> C/4 + k1 C/4 -> C/2
    assert A.compulsory == n * C * 4 + 27 * n * 4 + n * 2 * Q * 4                     # x, the map, t
    assert B.compulsory == n * 2 * Q * 4 + 27 * n * 4 + n * C * 4 + n * C * 4         # t, the map, the residual x, out
    assert roofline.irn_pass(1, 'a', 8 * n, C, n).compulsory == 8 * n * C * 4 + 27 * n * 4 + 8 * n * 2 * Q * 4      # a children level: its PARENTS' map


def test_halo_cells_and_reexports():
    assert ops.PROFILE.__class__ is roofline._Profile and ops._halo_cells is roofline._halo_cells
    assert ops.child_pairs is roofline.child_pairs and ops.MFMA_F32_PEAK_TFLOPS == roofline.MFMA_F32_PEAK_TFLOPS
    w = [0] * 27
    for kp, jc, reach in roofline._halo_cells():
        w[kp] += len(reach)
    assert w[13] == 64 and sorted(set(w)) == [1, 4, 16, 64] and sum(w) == 216       # centre, corner / edge / face neighbours


# ------------------------------------------------------------------------------------------------ the report
PEAK_FLOPS_PER_MS = roofline.MFMA_F32_PEAK_TFLOPS * 1e9          # flops in 1 ms at the fp32 MFMA peak


def _fam(p, steps=1):
    return {f['kernel']: f for f in p.families(steps, HBM)}


def test_dominant_is_the_largest_median_time_name():
    p = _profile((('a', 1), _flat('k_a (x)', 1, 0.3 * PEAK_FLOPS_PER_MS), [1.0, 1.0, 1.0]),
                 (('b', 1), _flat('k_b (x)', 1, 0.01 * PEAK_FLOPS_PER_MS), [0.5, 0.5, 0.5]))
    fam = _fam(p)
    assert fam['k_b']['median_us_per_step'] < (1 - p.TIE) * fam['k_a']['median_us_per_step']      # not tied: the lower fraction of k_b must not matter
    assert fam['k_b']['frac'] < fam['k_a']['frac']
    assert p.dominant(1, HBM) == ('k_a', (('a', 1),))


def test_dominant_tie_goes_to_the_lowest_fraction_then_the_name():
    p = _profile((('a', 1), _flat('k_a (x)', 1, 0.30 * PEAK_FLOPS_PER_MS), [1.00]),
                 (('b', 1), _flat('k_b (x)', 1, 0.10 * PEAK_FLOPS_PER_MS), [0.97]),
                 (('c', 1), _flat('k_c (x)', 1, 0.01 * PEAK_FLOPS_PER_MS), [0.90]))
    fam = _fam(p)
    top = fam['k_a']['median_us_per_step']
    assert top == max(f['median_us_per_step'] for f in fam.values())
    assert fam['k_b']['median_us_per_step'] >= (1 - p.TIE) * top > fam['k_c']['median_us_per_step']      # b within 5 % of a, c not
    assert fam['k_c']['frac'] < fam['k_b']['frac'] < fam['k_a']['frac']
    assert p.dominant(1, HBM)[0] == 'k_b'                       # not k_a (the largest time), not k_c (the lowest fraction, but outside the tie)
    q = _profile((('z', 1), _flat('k_z (x)', 1, 0.2 * PEAK_FLOPS_PER_MS), [1.0]), (('y', 1), _flat('k_y (x)', 1, 0.2 * PEAK_FLOPS_PER_MS), [1.0]))
    fq = _fam(q)
    assert fq['k_y']['frac'] == fq['k_z']['frac'] and fq['k_y']['median_us_per_step'] == fq['k_z']['median_us_per_step']
    assert q.dominant(1, HBM) == ('k_y', (('y', 1),))


def test_one_slow_sample_does_not_change_the_pick():
    slow = [0.5, 9.0, 0.5]
    p = _profile((('a', 1), _flat('k_a (x)', 1, 0.3 * PEAK_FLOPS_PER_MS), [1.0, 1.0, 1.0]),
                 (('b', 1), _flat('k_b (x)', 1, 0.01 * PEAK_FLOPS_PER_MS), slow))
    d = {r['name']: r for r in p.detail()}
    assert max(slow) == 9.0 and max(slow) > sum([1.0, 1.0, 1.0])       # the outlier is the largest sample, larger than k_a's whole time
    assert d['k_b']['ms'] > d['k_a']['ms']                                 # by summed (or mean) time k_b would lead
    assert d['k_b']['median_us'] == 500.0
    assert p.dominant(1, HBM)[0] == 'k_a'
    del p.records[('b', 1)]['events'][1]                                   # without the outlier: the same pick
    assert p.dominant(1, HBM)[0] == 'k_a'


def test_families_pool_levels_by_name():
    assert roofline._Profile.name_of('k_x<2, 2> (k3 32->32 on a plain level, LDS)') == 'k_x<2, 2>'
    p = _profile((('x', 300), _flat('k_x (on the large level)', 300, 3e9, compulsory=3e6, issued=6e9), [0.3, 0.3]),
                 (('x', 100), _flat('k_x (described otherwise)', 100, 1e9, compulsory=1e6, issued=2e9), [0.1, 0.1, 0.1, 0.1]),
                 (('y', 100), _flat('k_y (x)', 100, 1e9), [0.2]),
                 (('u', 100), roofline.Work('k_uncounted (no pair count for its level)', 100, lambda P: 0, lambda P: 0), [5.0]))
    fam = p.families(2, HBM)
    assert [f['kernel'] for f in fam] == ['k_x', 'k_y']                     # sorted by name; a record without a pair count is left out
    x = fam[0]
    assert x['levels'] == [100, 300] and x['launches_per_step'] == 3.0
    assert x['us_per_step'] == 500.0 and x['median_us_per_step'] == 500.0   # (2 x 0.3 + 4 x 0.1) ms over 2 steps
    assert x['TFLOPs'] == round((2 * 3e9 + 4 * 1e9) / 1e-3 / 1e12, 2)       # sum of flops / sum of time
    assert x['issued_over_algorithmic'] == 2.0 and fam[1]['issued_over_algorithmic'] is None
    assert x['compulsory_frac_of_hbm'] == round((2 * 3e6 + 4 * 1e6) / 1e-3 / 1e9 / HBM, 4)
    agg = p.aggregate(HBM, 2)
    assert agg['launches_per_step'] == 3.5 and agg['GFLOP_per_step'] == round((2 * 3e9 + 4 * 1e9 + 1e9) / 2 / 1e9, 2)


@pytest.mark.parametrize('mfma_frac,issued_frac,hbm_frac,bound', [
    (0.10, 0.20, 0.15, 'mfma'),        # the pipe utilisation (issued flops) is the larger fraction
    (0.30, 0.30, 0.15, 'mfma'),
    (0.10, 0.20, 0.50, 'hbm'),         # an MFMA kernel whose compulsory traffic is closer to ITS peak than either flop rate
    (0.10, None, 0.01, 'hbm'),         # no MFMA issued: priced against HBM whatever the fractions
])
def test_summary_names_the_closer_roofline(mfma_frac, issued_frac, hbm_frac, bound):
    ms = 2.0
    work = _flat('k_a (described)', 64, mfma_frac * PEAK_FLOPS_PER_MS * ms, compulsory=hbm_frac * HBM * 1e9 * ms * 1e-3,
                 issued=None if issued_frac is None else issued_frac * PEAK_FLOPS_PER_MS * ms)
    p = _profile((('a', 64), work, [ms, ms]), (('b', 64), _flat('k_b (x)', 64, 1.0), [0.1]))
    roof = p.summary(HBM, 2, name='k_a')
    assert roof['algorithmic']['frac_of_fp32_mfma_peak'] == pytest.approx(mfma_frac, abs=1e-4)
    assert roof['algorithmic']['frac_of_hbm_peak'] == pytest.approx(hbm_frac, abs=1e-4)
    if issued_frac is None:
        assert 'mfma_issued' not in roof
    else:
        assert roof['mfma_issued']['pipe_utilisation'] == pytest.approx(issued_frac, abs=1e-4)
        assert (max(mfma_frac, issued_frac) >= hbm_frac) == (bound == 'mfma')
    assert roof['bound'] == bound
    assert roof['unit'] == ('TFLOP/s' if bound == 'mfma' else 'GB/s') and roof['frac'] == pytest.approx(mfma_frac if bound == 'mfma' else hbm_frac, abs=1e-4)
    assert (roof['kernel'], roof['description'], roof['launches_timed'], roof['launches_per_step']) == ('k_a', 'k_a (described)', 2, 1.0)
    assert roof['all_launches'] == p.aggregate(HBM, 2)
    assert p.summary(HBM, 2)['kernel'] == p.dominant(2, HBM)[0] == 'k_a'    # default: the dominant name
    assert p.summary(HBM, 2, name='k_none') is None
