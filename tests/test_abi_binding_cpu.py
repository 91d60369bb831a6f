"""The ctypes binding is read from include/pcgc_hip.h (pcgcv2_amd/_lib.py): the reader on a small header, rows of the real header stated by
hand (one per type rule), the loaded libraries against the derived table, and the struct and constants the Python side takes from the header."""
import ctypes as C

import pytest

from pcgcv2_amd import _lib, ops
from pcgcv2_amd._lib import CONSTANTS, SIGNATURES, PcgcError, parse_header

vp, cp, ci, i32, i64, u32, u64, sz, f32, f64 = (C.c_void_p, C.c_char_p, C.c_int, C.c_int32, C.c_int64, C.c_uint32, C.c_uint64, C.c_size_t,
                                                 C.c_float, C.c_double)

SMALL = r'''
/* a header in the style of pcgc_hip.h; int pcgc_in_a_comment(int x); */
#ifndef SMALL_H
#define SMALL_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
const char* pcgc_text(void);
int pcgc_nothing();
// int pcgc_in_a_line_comment(int x);
#define SMALL_WORDS 6
#define SMALL_TEXT "6"
#define SMALL_MACRO(x) ((x) + 1)
int pcgc_many(const int32_t* coords /*[dev n,4] (batch, x, y, z)*/, int64_t n, int32_t stride,
              uint64_t* keys /*[dev cap], (pow2)*/,
              float factor, double scale, uint64_t seed, uint32_t colour, size_t bytes,
              void* stream);            /* vals[slot] = smallest row, (see above) */
int pcgc_array(int64_t out[3]);
int pcgc_names(const char* stem, const char* const* stems, char** out, const char text[16]);
typedef int (*small_fn)(const float* params, int C, uint16_t* table);
int pcgc_callback(small_fn fn, int C);
double pcgc_seconds(void);
uint64_t pcgc_seed(int);
uint32_t pcgc_crc(uint32_t crc, const void* bytes, int64_t n);
size_t pcgc_bytes(int64_t n);
enum { SMALL_A, SMALL_B, SMALL_C = 8, SMALL_D, SMALL_E = -2,
       SMALL_F };
typedef struct small_item {
    int64_t offset;
    int32_t first_row, rows,
            width;
    float weight;
} small_item;
int pcgc_items(const small_item* items /*[host n]*/, int n);
#ifdef __cplusplus
}
#endif
#endif
'''


def test_reader_on_a_small_header():
    sig, constants, structs = parse_header(SMALL)
    assert sig == {
        'pcgc_text': (cp, []),
        'pcgc_nothing': (ci, []),
        'pcgc_many': (ci, [vp, i64, i32, vp, f32, f64, u64, u32, sz, vp]),
        'pcgc_array': (ci, [vp]),
        'pcgc_names': (ci, [cp, vp, vp, vp]),
        'pcgc_callback': (ci, [vp, ci]),
        'pcgc_seconds': (f64, []),
        'pcgc_seed': (u64, [ci]),
        'pcgc_crc': (u32, [u32, vp, i64]),
        'pcgc_bytes': (sz, [i64]),
        'pcgc_items': (ci, [vp, ci]),
    }
    assert list(sig) == ['pcgc_text', 'pcgc_nothing', 'pcgc_many', 'pcgc_array', 'pcgc_names', 'pcgc_callback', 'pcgc_seconds', 'pcgc_seed',
                         'pcgc_crc', 'pcgc_bytes', 'pcgc_items']
    assert constants == {'SMALL_WORDS': 6, 'SMALL_A': 0, 'SMALL_B': 1, 'SMALL_C': 8, 'SMALL_D': 9, 'SMALL_E': -2, 'SMALL_F': -1}
    assert structs == {'small_item': [('offset', i64), ('first_row', i32), ('rows', i32), ('width', i32), ('weight', f32)]}


@pytest.mark.parametrize('declaration, name', [
    ('int pcgc_bad_argument(int a, unsigned int b);', 'pcgc_bad_argument'),
    ('int pcgc_bad_scalar(int a, long b);', 'pcgc_bad_scalar'),
    ('int pcgc_bad_small(uint8_t flag);', 'pcgc_bad_small'),
    ('long pcgc_bad_return(int a);', 'pcgc_bad_return'),
    ('void pcgc_bad_void(int a);', 'pcgc_bad_void'),
    ('int pcgc_bad_unnamed(some_t);', 'pcgc_bad_unnamed'),
    ('int pcgc_bad_inline_callback(int (*fn)(int), int n);', 'pcgc_bad_inline_callback'),
])
def test_reader_refuses_what_it_does_not_know_and_names_the_function(declaration, name):
    with pytest.raises(PcgcError, match=name):
        parse_header('int pcgc_good(int a);\n' + declaration + '\nint pcgc_after(void);\n', 'small.h')


def test_reader_refuses_unknown_struct_fields_and_enumerators():
    with pytest.raises(PcgcError, match='small_item'):
        parse_header('typedef struct small_item { int64_t offset; uint8_t* rows; } small_item;')
    with pytest.raises(PcgcError, match='SMALL_B'):
        parse_header('enum { SMALL_A, SMALL_B = SMALL_A + 1 };')


def test_missing_header_is_an_error_that_names_the_path():
    with pytest.raises(PcgcError, match='no_such_header.h'):
        _lib._read('no_such_header.h')


def test_real_header_rows_one_per_rule():
    assert len(SIGNATURES) == 208
    assert SIGNATURES['pcgc_last_error'] == (cp, [])
    assert SIGNATURES['pcgc_hash_capacity'] == (i64, [i64])
    assert SIGNATURES['pcgc_coords_scale'] == (ci, [vp, i64, f32, vp, vp])
    assert SIGNATURES['pcgc_bce_logits_bwd'] == (ci, [vp, i64, i64, vp, f64, vp, vp])
    res, args = SIGNATURES['pcgc_mesh_sample']
    assert res is ci and len(args) == 11 and args[5] is u64 and args[6] is u64 and [a for a in args if a is u64] == [u64, u64]
    assert SIGNATURES['pcgc_crc32'] == (u32, [u32, vp, i64])
    assert SIGNATURES['pcgc_scan_workspace_bytes'] == (sz, [i64])
    assert SIGNATURES['pcgc_occ_rans_batch_workspace_bytes'] == (i64, [i64, i64])
    assert SIGNATURES['pcgc_last_sched'] == (ci, [vp])
    res, args = SIGNATURES['pcgc_items_encode']
    assert res is ci and len(args) == 13 and args[0] is ci and args[1] is vp and cp not in args
    assert args[6] is ci and args[7] is vp and args[8] is vp and args[9] is vp                      # C, counts, eb_params, the pcgc_table_fn
    assert SIGNATURES['pcgc_ply_read_ascii_geo'] == (i64, [cp, vp, i64])
    assert len(SIGNATURES['pcgc_normals_estimate'][1]) == 24
    assert SIGNATURES['pcgc_partition'] == (ci, [vp, i64, i32, i64, i32, vp, vp, vp, vp, vp, vp, sz, vp])
    for name, (res, args) in SIGNATURES.items():                                                    # the classes themselves, never look-alikes
        assert any(res is t for t in (ci, i64, sz, u32, cp)), name
        assert all(any(a is t for t in (vp, cp, ci, i32, i64, u32, u64, sz, f32, f64)) for a in args), name


def test_loaded_libraries_carry_the_derived_rows():
    L = _lib.lib()
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(L, name)
        assert fn.restype is res and len(fn.argtypes) == len(args) and all(a is b for a, b in zip(fn.argtypes, args)), name
    R = _lib.reftable_lib()
    assert _lib.REFTABLE_SIGNATURES == {'pcgc_reference_table': (ci, [vp, ci, f32, f32, vp, vp]), 'pcgc_reference_table_clear': (ci, [])}
    for name, (res, args) in _lib.REFTABLE_SIGNATURES.items():
        fn = getattr(R, name)
        assert fn.restype is res and len(fn.argtypes) == len(args) and all(a is b for a, b in zip(fn.argtypes, args)), name


def test_collate_item_and_constants_follow_the_header():
    item = _lib.CollateItem
    assert item.__name__ == 'CollateItem' and C.sizeof(item) == 32
    assert item._fields_ == [('offset', i64), ('first_row', i32), ('rows', i32), ('width', i32), ('symmetry', i32), ('extent', i32), ('reserved', i32)]
    assert [getattr(item, name).offset for name, _ in item._fields_] == [0, 8, 12, 16, 20, 24, 28]
    one = item(1 << 40, 2, 3, 4, 5, 6, 0)                                                          # the order ops.collate_rows constructs it in
    assert (one.offset, one.first_row, one.rows, one.width, one.symmetry, one.extent, one.reserved) == (1 << 40, 2, 3, 4, 5, 6, 0)
    assert CONSTANTS['PCGC_RC_CKPT_WORDS'] == 6 == ops.RC_CKPT_WORDS
    assert CONSTANTS['PCGC_COLLATE_MAX_ITEMS'] == 16 == ops.COLLATE_MAX_ITEMS
    assert CONSTANTS['PARTITION_MAX_BLOCKS'] == 1024 == ops.PARTITION_MAX_BLOCKS
    assert CONSTANTS['PARTITION_INFO_WORDS'] == CONSTANTS['PARTITION_PHASE_WORDS'] == 8
    assert [CONSTANTS['PARTITION_INFO_' + w] for w in ('ROUNDS', 'BLOCKS', 'OVERSIZE', 'BAD_RANGE', 'BAD_BATCH', 'WOULD_BE')] == [0, 1, 2, 3, 4, 5]
    assert CONSTANTS['PARTITION_INFO_BAD_BATCH'] == 4
    assert len(ops.PARTITION_PHASES) == CONSTANTS['PARTITION_PHASE_COPIES'] + 1
    assert [CONSTANTS['PARTITION_PHASE_' + p.upper()] for p in ops.PARTITION_PHASES] == list(range(len(ops.PARTITION_PHASES)))
    assert 'PCGC_HIP_H' not in CONSTANTS                                                            # the include guard defines no integer
