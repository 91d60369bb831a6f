"""Record the time-independent half of the roofline report as a fixture: tests/golden/roofline_records.json.

One Coder.encode + decode of a small shell with synthetic weights under three dispatch records, chosen so that every bracketed launcher of
pcgcv2_amd/ops.py fires; one step with every launch bracketed, one that counts the kernel-map pairs (what bench.py does).  Of each
PROFILE.detail() entry the integers and strings are kept (FIELDS), plus the shapes of the launch that the key does not carry (`shape`:
input rows, residual, row gather), noted by wrappers around the public launchers.  tests/test_roofline_device.py makes the same runs and
demands equality; tests/test_roofline_cpu.py feeds the shapes to the pure accounting functions.

    python tools/record_roofline.py [--out tests/golden/roofline_records.json] [--cloud shell8]
"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIELDS = ('key', 'kernel', 'n_out', 'launches', 'pairs', 'gathered_bytes', 'flops', 'compulsory_bytes', 'mfma_issued_flops')

# a piece of the kernel string of every bracketed launcher (and of every kernel name one launcher can carry): a record that misses one
# of them is not written
EXPECTED = (
    'k3 gather conv Cin=', '(k_conv_unit: kernel map only', '(k_conv_unit_coarse: presence from',
    'k_irn_a<64, 16> (per-row gather, VALU)', 'k_irn_b<64, 16> (', 'k_irn_a_split<32> (', 'k_irn_b_split<32> (', 'k_irn_a_split<16> (', 'k_irn_b_split<16> (',
    'k_rows_irn_a64 (', 'k_rows_irn_b64 (', 'k_rows_irn_a32 (', 'k_rows_irn_b32 (', 'k_rows_q4_a32 (', 'k_rows_q4_b32 (',
    'k_child_q4<1, 8, 2> (', 'k_child_q4<0, 8, 2> (', 'k_child_irn_a<16> (', 'k_child_irn_b<16> (', 'k_child_irn_a<32> (', 'k_child_irn_b<32> (',
    'k_child_cls<1> (', 'k_child_cls<2> (', 'k_child_conv<1, 1> (', 'k_child_conv<2, 2> (',
    'k_rows_conv<2, 2> (', 'k_conv_packed64 (', 'k_rows_down<1, 2> (', 'k_rows_down<2, 4> (', 'k_rows_down<4, 2> (',
    'k_conv_up2<64, 32> (generative transpose k2 s2, eight GEMMs', 'k_conv_up2<32, 16> (', 'k_conv_up2<8, 64> (generative transpose k2 s2, one thread per',
)


def configs():
    """name -> PathConfig changes (pcgcv2_amd/pathconfig.py): quad-block + rows + packed + mapless kernels on every level; the same with the
    packed-N kernels in place of the quad-block ones; the VALU passes, the gather ladder and the unit conv through its own map"""
    from pcgcv2_amd.pathconfig import FIELDS as PATH_FIELDS
    every = {f: 0 for f in sorted(PATH_FIELDS) if '_MIN' in f}
    off = ('ROWS_IRN64', 'ROWS_IRN32', 'CHILD_MFMA', 'ROWS_CONV', 'PACKED_CONV64', 'ROWS_DOWN', 'UNIT_CONV_MAPLESS')
    return {'every_min_0': every, 'no_quad_block': dict(every, ROWS_Q4=False, CHILD_Q4=False), 'valu_and_gather': {f: False for f in off}}


class _Watch:
    """wraps the launchers whose accounting needs more than their key: notes, per key, the shapes a pure function has to be told"""

    def __init__(self, ops):
        self.ops, self.seen, self.saved = ops, {}, {}

    def __enter__(self):
        ops, seen = self.ops, self.seen

        def wrap(name, note):
            fn = self.saved[name] = getattr(ops, name)

            def wrapped(*a, **kw):
                key, shape = note(*a, **kw)
                if key is not None:
                    seen.setdefault(key, shape)
                return fn(*a, **kw)
            setattr(ops, name, wrapped)

        def gather(nbr, x, W, bias, out=None, residual=None, relu=False, n_out=None):
            if W.dim() != 3 or W.shape[0] != 27:
                return None, None
            return ('conv', W.shape[1], W.shape[2], nbr.shape[1]), {'n_in': x.shape[0]}
        wrap('conv_gather', gather)
        wrap('conv_child', lambda nbr, x, table, bias, Cout, out=None, residual=None, relu=False:
             (('child_conv', x.shape[1], Cout, x.shape[0]), {'residual': residual is not None}))
        wrap('conv_rows', lambda nbr, x, table, bias, Cout, out=None, residual=None, relu=False:
             (('conv', x.shape[1], Cout, x.shape[0]), {'residual': residual is not None}))
        wrap('conv_down_rows', lambda down, x, table, bias, Cout, relu=False: (('down', x.shape[1], Cout, down.shape[1]), {'n_in': x.shape[0]}))
        wrap('conv_up2', lambda x, W, bias, relu=False, rows=None:
             (('up2', W.shape[1], W.shape[2], 8 * (x.shape[0] if rows is None else rows.shape[0])), {'rows': rows is not None}))
        return self

    def __exit__(self, *exc):
        for name, fn in self.saved.items():
            setattr(self.ops, name, fn)
        return False


def run(cloud='shell8'):
    """-> ({config: [record]}, {config: decoded coordinates as a numpy array}); records sorted by key, FIELDS + `shape` each"""
    import numpy as np
    import torch
    from pcgcv2_amd import ops, synthetic
    from pcgcv2_amd.coder import Coder
    from pcgcv2_amd.pcc_model import PCCModel
    from pcgcv2_amd.sparse import SparseTensor
    dev = torch.device('cuda:0')
    c = synthetic.shell(cloud).numpy()
    c4 = torch.from_numpy(np.concatenate([np.zeros((len(c), 1), np.int32), c], 1)).to(dev)
    model = PCCModel().to(dev)
    model.load_state_dict(synthetic.synthetic_state_dict())
    records, decoded = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        coder = Coder(model, os.path.join(tmp, 'f'))
        for name, changes in configs().items():
            x = SparseTensor(torch.ones((len(c4), 1)), coordinates=c4, tensor_stride=1, device=dev)
            with ops.path(**changes), _Watch(ops) as watch:
                try:
                    ops.PROFILE.reset(enabled=True)
                    coder.encode(x, postfix='_' + name)
                    out = coder.decode(postfix='_' + name)
                    ops.PROFILE.enabled = False
                    ops.PROFILE.counting = True
                    x.cmap.drop_caches()
                    coder.encode(x, postfix='_' + name)
                    coder.decode(postfix='_' + name)
                    ops.PROFILE.counting = False
                    torch.cuda.synchronize()
                    detail = ops.PROFILE.detail()
                finally:
                    ops.PROFILE.reset(enabled=False)
            recs = []
            for d in detail:
                r = {f: d[f] for f in FIELDS if f in d}
                r['key'] = list(d['key'])
                r['shape'] = watch.seen.get(d['key'], {})
                recs.append(r)
            records[name] = sorted(recs, key=lambda r: json.dumps(r['key']))
            decoded[name] = out.C.cpu().numpy()
    return records, decoded


def missing(records):
    kernels = {r['kernel'] for recs in records.values() for r in recs}
    return [e for e in EXPECTED if not any(e in k for k in kernels)]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'roofline_records.json'))
    ap.add_argument('--cloud', default='shell8')
    args = ap.parse_args()
    records, decoded = run(args.cloud)
    for name, recs in records.items():
        print(name, len(recs), 'records')
        for r in recs:
            print('   ', r['key'], r['kernel'].split(' (')[0], 'pairs' in r)
    miss = missing(records)
    unpaired = [(n, r['key']) for n, recs in records.items() for r in recs if 'pairs' not in r]
    assert not miss, f'no launch of: {miss}'
    assert not unpaired, f'records without a pair count: {unpaired}'
    first = next(iter(decoded.values()))
    assert all((d == first).all() for d in decoded.values()), 'decoded coordinates differ between the dispatch records'
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    one = lambda v: json.dumps(v, sort_keys=True)
    with open(args.out, 'w') as f:                       # one record per line
        f.write('{"cloud": %s,\n "configs": %s,\n "records": {\n' % (one(args.cloud), one(configs())))
        f.write(',\n'.join('  %s: [\n%s\n  ]' % (one(name), ',\n'.join('   ' + one(r) for r in recs)) for name, recs in sorted(records.items())))
        f.write('\n }}\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
