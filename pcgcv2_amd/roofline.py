"""Roofline accounting of the sparse-conv launches: what one launch is charged, as pure functions of its shapes, and the
report bench.py prints.  Host-only: nothing here calls the native library; torch supplies the HIP events and the pair counts.

Per launch, with P = (in,out) pairs of the level's k3 map (counted, not assumed), n rows:
    gathered bytes      k3 conv: P*Cin*4 + P*8 + n*Cout*4 ;  k1 conv: n*(Cin+Cout)*4 — every (in,out) pair
                     charged: the re-use of a row by its ~18 outputs is served by L2 / LDS, so this rate can exceed the HBM peak
    compulsory bytes                   every input row, kernel-map entry and output row once: what HBM has to move
    flops                              2*P*Cin*Cout (+ 2*n*Cin*Cout for k1 parts);  k2 s2 down / generative up: P = fine rows
    mfma_issued                        fp32 MFMA flops the kernel issues (zero-padded columns and absent rows included)
A fused InceptionResNet pass is charged the sum of the convs it computes:
    pass A: k3 C->C/4 + k1 C->C/4          pass B: k3 C/4->C/2 + k3 C/4->C/4 + k1 C/4->C/2.
"""
from collections import namedtuple

import numpy as np
import torch

MFMA_F32_PEAK_TFLOPS = 157.3      # MI355X_MICROARCH.md: dense fp32 MFMA peak

# what one launch is charged: the kernel string ('name (description)'), the output rows, gathered bytes and flops as functions of P,
# compulsory bytes, issued MFMA flops (a number, a function of P, or None: no MFMA) and P itself where the launch knows it (k2 s2)
Work = namedtuple('Work', 'kernel n gathered flops compulsory mfma_issued pairs', defaults=(None, None, None))


def dense_issued(K, rows, Cin, Cout):
    """fp32 MFMA flops of a kernel that walks all K offsets of every 16-row tile"""
    return 2 * K * ((rows + 15) // 16 * 16) * Cin * Cout


def k3_conv(kernel, Cin, Cout, n, n_in=None, map_rows=None, residual=False, issued=None):
    """k3 s1 conv on n rows (n_in input rows, default n) through a [27][map_rows] map: the level's own (default) or its parents'"""
    n_in = n if n_in is None else n_in
    map_rows = n if map_rows is None else map_rows
    return Work(kernel, n, lambda P: P * Cin * 4 + P * 8 + n * Cout * 4, lambda P: 2 * P * Cin * Cout,
                n_in * Cin * 4 + 27 * map_rows * 4 + n * Cout * 4 + (n * Cout * 4 if residual else 0), issued)


def child_conv(kernel, Cin, Cout, n_p, residual=False, issued=None):
    """k3 s1 conv on the 8 n_p rows of a children level, gathered through the parent level's map"""
    return k3_conv(kernel, Cin, Cout, 8 * n_p, map_rows=n_p, residual=residual, issued=issued)


def unit_conv(kernel, Cout, n, mapless=False):
    """k3 conv 1 -> Cout on the all-ones input: no feature rows; mapless reads coordinates and parent rows instead of a map of its own"""
    return Work(kernel, n, lambda P: P * 4 + P * 8 + n * Cout * 4, lambda P: 2 * P * Cout,
                (n * 16 + n * 4 if mapless else 27 * n * 4) + n * Cout * 4)


def down_conv(kernel, Cin, Cout, n_c, n_in):
    """k2 s2: every fine row is one (in,out) pair (bytes = N_fine Cin 4 + N_coarse Cout 4, flops = 2 N_fine Cin Cout)"""
    return Work(kernel, n_c, lambda P: P * Cin * 4 + n_c * Cout * 4, lambda P: 2 * P * Cin * Cout,
                n_in * Cin * 4 + 8 * n_c * 4 + n_c * Cout * 4, dense_issued(8, n_c, Cin, Cout), n_in)


def up2_conv(kernel, Cin, Cout, n_in, rows=False, mfma=False):
    """generative transpose k2 s2: P = fine rows (bytes = N_fine (Cin + Cout) 4, flops = 2 N_fine Cin Cout); rows: a row gather"""
    return Work(kernel, 8 * n_in, lambda P: P * (Cin + Cout) * 4, lambda P: 2 * P * Cin * Cout,
                n_in * Cin * 4 + 8 * n_in * Cout * 4 + (n_in * 4 if rows else 0), dense_issued(8, n_in, Cin, Cout) if mfma else None, 8 * n_in)


def irn_pass(ps, kernel, n, C, map_rows, issued=None):
    """pass ps (1 = A, 2 = B) of the fused InceptionResNet block on n rows of C channels through a [27][map_rows] map"""
    Q = C // 4
    map_bytes = 27 * map_rows * 4
    if ps == 1:
        return Work(kernel, n, lambda P: (P * C * 4 + P * 8 + n * Q * 4) + n * (C + Q) * 4, lambda P: 2 * P * C * Q + 2 * n * C * Q,
                    n * C * 4 + map_bytes + n * 2 * Q * 4, issued)
    return Work(kernel, n, lambda P: (P * Q * 4 + P * 8 + n * 2 * Q * 4) + (P * Q * 4 + P * 8 + n * Q * 4) + n * 3 * Q * 4,
                lambda P: 2 * P * Q * 2 * Q + 2 * P * Q * Q + 2 * n * Q * 2 * Q, n * 2 * Q * 4 + map_bytes + n * C * 4 + n * C * 4, issued)


def _halo_cells():
    """The 64 cells of a parent's 4x4x4 halo in ascending (cz, cy, cx) order -> list of (kp, j', reach) where kp = index of the
    neighbour parent in the PARENT level's k3 map, j' = which of its children the cell is, and reach = [(j, k)]: the children j
    of the centre parent whose 3x3x3 window contains the cell, with the kernel offset k they see it through."""
    P1 = (0, 1, 1, 2)                  # floor(c / 2) + 1 for c = -1, 0, 1, 2
    B = (1, 0, 1, 0)                   # c & 1
    cells = []
    for cz in range(4):
        for cy in range(4):
            for cx in range(4):
                kp = P1[cz] * 9 + P1[cy] * 3 + P1[cx]
                jc = B[cx] + 2 * B[cy] + 4 * B[cz]
                reach = []
                for j in range(8):
                    kx, ky, kz = cx - (j & 1), cy - ((j >> 1) & 1), cz - (j >> 2)          # = (c - j) + 1 per axis
                    if 0 <= kx <= 2 and 0 <= ky <= 2 and 0 <= kz <= 2:
                        reach.append((j, kz * 9 + ky * 3 + kx))
                cells.append((kp, jc, reach))
    assert sum(len(r) for _, _, r in cells) == 216
    return cells


_CHILD_WEIGHT = None


def child_pairs(parent_nbr):
    """(in,out) pairs of the CHILDREN level's k3 map, counted from the parent map (the children map is never built): a present
    parent neighbour at offset kp contributes as many (child row, offset) pairs as halo cells of that parent are reached:
    64 for the centre, 16 per face, 4 per edge, 1 per corner neighbour."""
    global _CHILD_WEIGHT
    if _CHILD_WEIGHT is None or _CHILD_WEIGHT.device != parent_nbr.device:
        w = np.zeros(27, np.int64)
        for kp, jc, reach in _halo_cells():
            w[kp] += len(reach)
        _CHILD_WEIGHT = torch.from_numpy(w).to(parent_nbr.device)
    return int(((parent_nbr >= 0).sum(1) * _CHILD_WEIGHT).sum().item())


class _Profile:
    """Brackets the sparse-conv launches with HIP events on the stream they are launched on, and turns the timings into the
    `roofline` object of bench.py.  Records are per (kernel, level) key; the report groups them by kernel NAME (the text of `kernel`
    before ' (': what a rocprofv3 --stats line pools too), so that `roofline.kernel` is a statistic of one compiled kernel over every
    level it serves.  The report half reads the timings through `e0.elapsed_time(e1)` alone."""

    TIE = 0.05                     # kernel names whose per-step time is within 5 % of the largest are tied: the lower fraction of peak wins

    def __init__(self):
        self.reset(False)

    def reset(self, enabled=False, only=None):
        self.enabled = enabled
        self.only = None if only is None else frozenset(only)      # bracket just these (kernel, level) keys: keeps the event overhead out of a timed region
        self.counting = False
        self.records = {}          # key -> dict(the fields of Work, events=[(e0,e1)])
        self.pairs = {}            # n_out -> P of the level's k3 map

    def want(self, key):
        return self.enabled and (self.only is None or key in self.only)

    @staticmethod
    def name_of(kernel):
        return kernel.split(' (')[0]

    def launch(self, wanted, own, parent, call, *args):
        """call(*args) -> its result.  wanted: False, or (key, Work) — written `PROFILE.want(key) and (key, roofline.<family>(...))` at the
        launch, so that an unwanted launch builds no string and no record: then events are recorded on the current stream around the call
        (closed on whatever way the call ends).  Otherwise, while `counting`, the pairs of the level are counted from its own map `own` or
        its parents' map `parent` (None: nothing to count)."""
        if wanted:
            key, work = wanted
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            self.records.setdefault(key, dict(work._asdict(), events=[]))['events'].append((e0, e1))
            e0.record()
            try:
                return call(*args)
            finally:
                e1.record()
        out = call(*args)
        if self.counting:
            if own is not None:
                self.count(own)
            elif parent is not None:
                self.count_children(parent)
        return out

    def count(self, nbr):
        n = nbr.shape[1]
        if n not in self.pairs:
            self.pairs[n] = int((nbr >= 0).sum().item())

    def count_children(self, parent_nbr):
        n = 8 * parent_nbr.shape[1]
        if n not in self.pairs:
            self.pairs[n] = child_pairs(parent_nbr)

    def detail(self):
        """one entry per (kernel, level): mean AND median launch time (a first-touch allocation or a preempted launch must not decide a ranking)"""
        out = []
        for key, r in self.records.items():
            ts = sorted(e0.elapsed_time(e1) for e0, e1 in r['events'])
            ms = sum(ts)
            us = ms / len(ts) * 1e3
            med = (ts[len(ts) // 2] if len(ts) % 2 else 0.5 * (ts[len(ts) // 2 - 1] + ts[len(ts) // 2])) * 1e3
            d = {'key': key, 'name': self.name_of(r['kernel']), 'kernel': r['kernel'], 'n_out': r['n'], 'launches': len(ts), 'ms': ms, 'avg_us': us, 'median_us': med}
            P = r['pairs'] if r['pairs'] is not None else self.pairs.get(r['n'])     # (k2 s2 convs carry their own P = fine rows)
            if P is not None:
                d['pairs'] = P
                d['gathered_bytes'] = r['gathered'](P)
                d['flops'] = r['flops'](P)
                d['gathered_GBps'] = d['gathered_bytes'] / (us * 1e-6) / 1e9
                d['TFLOPs'] = d['flops'] / (us * 1e-6) / 1e12
                if r['compulsory'] is not None:
                    d['compulsory_bytes'] = r['compulsory']
                    d['compulsory_GBps'] = r['compulsory'] / (us * 1e-6) / 1e9
                if r['mfma_issued'] is not None:
                    issued = r['mfma_issued'](P) if callable(r['mfma_issued']) else r['mfma_issued']      # (a packed kernel issues per present pair)
                    d['mfma_issued_flops'] = issued
                    d['mfma_issued_TFLOPs'] = issued / (us * 1e-6) / 1e12
            out.append(d)
        return sorted(out, key=lambda d: -d['ms'])

    def families(self, steps, peak_gbs):
        """the fixed report: one entry per kernel NAME, its levels pooled (sum of flops / sum of time): us per step, launches per step, fraction
        of the fp32 MFMA peak (algorithmic flops), issued / algorithmic, compulsory-traffic fraction of the HBM peak; sorted by name"""
        groups = {}
        for d in self.detail():
            if 'pairs' in d:
                groups.setdefault(d['name'], []).append(d)
        fam = []
        for name, ds in groups.items():
            ms = sum(d['ms'] for d in ds)
            med_ms = sum(d['median_us'] * d['launches'] for d in ds) * 1e-3
            fl = sum(d['flops'] * d['launches'] for d in ds)
            comp = sum(d.get('compulsory_bytes', 0) * d['launches'] for d in ds)
            issued = sum(d.get('mfma_issued_flops', 0) * d['launches'] for d in ds)
            f = {'kernel': name, 'levels': sorted({d['n_out'] for d in ds}), 'launches_per_step': round(sum(d['launches'] for d in ds) / steps, 2),
                 'us_per_step': round(ms * 1e3 / steps, 1), 'median_us_per_step': round(med_ms * 1e3 / steps, 1),
                 'TFLOPs': round(fl / (ms * 1e-3) / 1e12, 2), 'frac': round(fl / (ms * 1e-3) / 1e12 / MFMA_F32_PEAK_TFLOPS, 4),
                 'issued_over_algorithmic': round(issued / fl, 2) if issued and fl else None,
                 'compulsory_frac_of_hbm': round(comp / (ms * 1e-3) / 1e9 / peak_gbs, 4)}
            fam.append(f)
        return sorted(fam, key=lambda f: f['kernel'])

    def dominant(self, steps, peak_gbs):
        """(kernel name, its keys): the name with the largest per-step time (median launch time x launches, so one slow sample cannot decide);
        names within TIE of it are tied and the LOWEST fraction of the fp32 MFMA peak wins — a rule that returns the same kernel on every box
        as long as the ranking of the fractions holds, where "largest time" alone flipped between four groups 3 % apart."""
        fam = self.families(steps, peak_gbs)
        if not fam:
            return None, ()
        top = max(f['median_us_per_step'] for f in fam)
        tied = [f for f in fam if f['median_us_per_step'] >= (1.0 - self.TIE) * top]
        best = min(tied, key=lambda f: (f['frac'], f['kernel']))
        keys = tuple(k for k, r in self.records.items() if self.name_of(r['kernel']) == best['kernel'])
        return best['kernel'], keys

    def summary(self, peak_gbs, steps, name=None):
        """roofline of one kernel name (default: `dominant`), its levels pooled: achieved = sum of algorithmic flops / sum of launch time.
        `bound` is the roofline the kernel sits closer to: "mfma" (algorithmic fp32 flops against the dense fp32 MFMA peak) or
        "hbm" (compulsory bytes against the HBM peak).  `aggregate` = every bracketed launch; `families` = the per-name table."""
        d_all = [r for r in self.detail() if 'pairs' in r]
        if not d_all:
            return None
        if name is None:
            name, _ = self.dominant(steps, peak_gbs)
        d = [r for r in d_all if r['name'] == name]
        if not d:
            return None
        t_s = sum(r['ms'] for r in d) * 1e-3
        launches = sum(r['launches'] for r in d)
        fl = sum(r['flops'] * r['launches'] for r in d)
        comp = sum(r.get('compulsory_bytes', 0) * r['launches'] for r in d)
        gath = sum(r['gathered_bytes'] * r['launches'] for r in d)
        issued = sum(r.get('mfma_issued_flops', 0) * r['launches'] for r in d)
        tf, cg = fl / t_s / 1e12, comp / t_s / 1e9
        hbm_frac, mfma_frac = cg / peak_gbs, tf / MFMA_F32_PEAK_TFLOPS
        # an MFMA kernel is priced against the matrix peak unless its compulsory traffic rate is the larger fraction of ITS peak even
        # compared with the pipe utilisation (issued flops), i.e. unless it really is the memory side that is closer to its limit
        is_mfma = issued > 0 and max(mfma_frac, issued / t_s / 1e12 / MFMA_F32_PEAK_TFLOPS) >= hbm_frac
        roof = {'bound': 'mfma' if is_mfma else 'hbm'}
        if is_mfma:
            roof.update(achieved=round(tf, 2), peak=MFMA_F32_PEAK_TFLOPS, unit='TFLOP/s', frac=round(mfma_frac, 4))
        else:
            roof.update(achieved=round(cg, 2), peak=peak_gbs, unit='GB/s', frac=round(hbm_frac, 4))
        roof.update(traffic=None, kernel=name, description=d[0]['kernel'], avg_launch_us=round(t_s * 1e6 / launches, 2), launches_timed=launches,
                    launches_per_step=round(launches / steps, 2),
                    selection=f'kernel NAME with the largest per-step time (median launch time x launches, levels pooled); names within {int(self.TIE * 100)} % '
                              'are tied and the lowest fraction of peak wins',
                    levels=[{'n_out': r['n_out'], 'pairs': r['pairs'], 'launches': r['launches'], 'avg_launch_us': round(r['avg_us'], 2),
                             'flops_per_launch': r['flops'], 'frac_of_fp32_mfma_peak': round(r['TFLOPs'] / MFMA_F32_PEAK_TFLOPS, 4),
                             'compulsory_bytes_per_launch': r.get('compulsory_bytes'),
                             'mfma_issued_flops_per_launch': r.get('mfma_issued_flops')} for r in sorted(d, key=lambda r: -r['n_out'])],
                    algorithmic={'flops_per_launch': fl / launches, 'TFLOPs': round(tf, 2), 'frac_of_fp32_mfma_peak': round(mfma_frac, 4),
                                 'compulsory_bytes_per_launch': comp / launches, 'compulsory_GBps': round(cg, 1), 'frac_of_hbm_peak': round(hbm_frac, 4),
                                 'gathered_bytes_per_launch': gath / launches, 'gathered_GBps': round(gath / t_s / 1e9, 1),
                                 'note': 'per-launch figures are means over the launches of this kernel name (levels pooled: see `levels`); gathered = SURVEY 8d '
                                         'formula, every (in,out) pair charged — the row re-use is served by L2/LDS, not HBM'})
        if issued:
            roof['mfma_issued'] = {'flops_per_launch': issued / launches, 'TFLOPs': round(issued / t_s / 1e12, 2),
                                   'pipe_utilisation': round(issued / t_s / 1e12 / MFMA_F32_PEAK_TFLOPS, 4), 'issued_over_algorithmic': round(issued / fl, 2),
                                   'note': 'fp32 MFMA flops issued (zero-padded columns and absent rows included) / time'}
        roof['all_launches'] = self.aggregate(peak_gbs, steps)
        return roof

    def aggregate(self, peak_gbs, steps):
        d = [r for r in self.detail() if 'pairs' in r]
        tot_g = sum(r['gathered_bytes'] * r['launches'] for r in d)
        tot_c = sum(r.get('compulsory_bytes', 0) * r['launches'] for r in d)
        tot_f = sum(r['flops'] * r['launches'] for r in d)
        tot_ms = sum(r['ms'] for r in d)
        return {'ms_per_step': round(tot_ms / steps, 3), 'launches_per_step': round(sum(r['launches'] for r in d) / steps, 2),
                'GFLOP_per_step': round(tot_f / steps / 1e9, 2),
                'TFLOPs': round(tot_f / (tot_ms * 1e-3) / 1e12, 2), 'frac_of_fp32_mfma_peak': round(tot_f / (tot_ms * 1e-3) / 1e12 / MFMA_F32_PEAK_TFLOPS, 4),
                'compulsory_GBps': round(tot_c / (tot_ms * 1e-3) / 1e9, 1), 'frac_of_hbm_peak': round(tot_c / (tot_ms * 1e-3) / 1e9 / peak_gbs, 4),
                'gathered_GBps': round(tot_g / (tot_ms * 1e-3) / 1e9, 1)}
