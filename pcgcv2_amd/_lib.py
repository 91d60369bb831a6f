"""ctypes binding of libpcgc_hip.so, READ from include/pcgc_hip.h: the header is the only statement of the C ABI.  At import
`parse_header` turns every prototype into a row of SIGNATURES, `typedef struct pcgc_collate_item` into CollateItem's fields and the integer
`#define`s and anonymous enums into CONSTANTS; a new entry point needs its declaration in the header and nothing here.  Type rules: a
parameter with `*` or `[` is c_void_p, except a `char` with exactly one `*` (c_char_p); a function-pointer typedef is c_void_p; the scalars
are those of _SCALARS.  Anything else raises, naming the function.  There is NO fallback: if the HIP library is missing or a call fails,
the product raises."""
import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('PCGC_LIB') or os.path.join(_HERE, 'libpcgc_hip.so')       # (PCGC_LIB: an experiment build, pcgcv2_amd/_build.py)


class PcgcError(RuntimeError):
    pass


_SCALARS = {'int': C.c_int, 'int32_t': C.c_int32, 'int64_t': C.c_int64, 'size_t': C.c_size_t, 'float': C.c_float, 'double': C.c_double,
            'uint32_t': C.c_uint32, 'uint64_t': C.c_uint64}


def _ctype(decl, callbacks, what):
    """the ctypes class of one return type or parameter declaration (comments already stripped)"""
    words = [w for w in re.findall(r'\w+', decl) if w != 'const']
    if '*' in decl or '[' in decl:
        return C.c_char_p if words[:1] == ['char'] and decl.count('*') == 1 and '[' not in decl else C.c_void_p
    if words and words[0] in callbacks and len(words) <= 2:
        return C.c_void_p
    if not words or words[0] not in _SCALARS or len(words) > 2:                 # (two words: a type and the parameter's name)
        raise PcgcError(f'{what}: `{" ".join(decl.split())}` is no type the binding knows ({", ".join(_SCALARS)}, pointers, arrays)')
    return _SCALARS[words[0]]


def parse_header(text, where='header'):
    """C header text -> (signatures {name: (restype, argtypes)}, constants {name: int}, structs {name: _fields_})"""
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    text = re.sub(r'//[^\n]*', ' ', text)
    constants = {m[1]: int(m[2]) for m in re.finditer(r'^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(-?\d+)[ \t]*$', text, re.M)}
    text = re.sub(r'^[ \t]*#.*$', ' ', text, flags=re.M)

    def enum(m):
        value = 0
        for item in filter(None, (s.strip() for s in m[1].split(','))):
            name, _, explicit = (s.strip() for s in item.partition('='))
            if explicit:
                if not re.fullmatch(r'-?\d+', explicit):
                    raise PcgcError(f'{where}: enumerator {name} = {explicit} is no integer the binding can read')
                value = int(explicit)
            constants[name] = value
            value += 1
        return ' '
    text = re.sub(r'\benum\s*\{([^}]*)\}\s*;', enum, text)

    structs = {}

    def struct(m):
        fields = []
        for decl in filter(None, (s.strip() for s in m[2].split(';'))):
            base, names = (decl.split(None, 1) + [''])[:2]
            for name in (s.strip() for s in names.split(',')):
                if base not in _SCALARS or not re.fullmatch(r'\w+', name):
                    raise PcgcError(f'{where}: struct {m[1]}: `{decl}` is no field the binding knows')
                fields.append((name, _SCALARS[base]))
        structs[m[1]] = fields
        return ' '
    text = re.sub(r'\btypedef\s+struct\s+(\w+)\s*\{([^}]*)\}\s*\w+\s*;', struct, text)

    callbacks = set()
    text = re.sub(r'\btypedef\b[^;{}()]*\(\s*\*\s*(\w+)\s*\)\s*\([^()]*\)\s*;', lambda m: callbacks.add(m[1]) or ' ', text)

    signatures = {}
    for ret, name, args in re.findall(r'([\w\s*]+?)\s*\b(pcgc_\w+)\s*\(([^()]*)\)\s*;', text):
        args = [] if args.strip() in ('', 'void') else args.split(',')
        signatures[name] = (_ctype(ret, callbacks, f'{where}: return of {name}'),
                            [_ctype(a, callbacks, f'{where}: argument {k} of {name}') for k, a in enumerate(args)])
    unread = set(re.findall(r'\b(pcgc_\w+)\s*\(', text)) - set(signatures)
    if unread:
        raise PcgcError(f'{where}: the binding cannot read the declaration of {", ".join(sorted(unread))}')
    return signatures, constants, structs


def _read(header):
    path = os.path.join(_HERE, '..', 'include', header)
    if not os.path.exists(path):
        raise PcgcError(f'{path} not found: the ctypes binding is read from it')
    with open(path) as f:
        return parse_header(f.read(), path)


# name -> (restype, argtypes), {name: int} of the #defines and enums, {name: _fields_}: include/pcgc_hip.h as the compiler reads it
SIGNATURES, CONSTANTS, _STRUCTS = _read('pcgc_hip.h')
REFTABLE_SIGNATURES = _read('pcgc_reftable.h')[0]


class CollateItem(C.Structure):
    """pcgc_collate_item of include/pcgc_hip.h"""
    _fields_ = _STRUCTS['pcgc_collate_item']


def _bind(l, signatures):
    for name, (res, args) in signatures.items():
        fn = getattr(l, name)
        fn.restype, fn.argtypes = res, args
    return l


_lib = None


def lib():
    """Load (once) and return the bound library.  Raises if it is not built: there is no CPU / eager fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise PcgcError(f'{LIB_PATH} not found: run `python -c "import __graft_entry__ as g; g.build()"` '
                            '(hipcc --offload-arch=gfx950). The HIP library is mandatory; there is no fallback path.')
        _lib = _bind(C.CDLL(LIB_PATH), SIGNATURES)
    return _lib


REFTABLE_PATH = os.path.join(_HERE, 'libpcgc_reftable.so')
_reftable = None


def reftable_lib():
    """libpcgc_reftable.so (csrc/reftable.cpp), bound from include/pcgc_reftable.h"""
    global _reftable
    if _reftable is None:
        if not os.path.exists(REFTABLE_PATH):
            raise PcgcError(f'{REFTABLE_PATH} not found: run `python -c "import __graft_entry__ as g; g.build()"`')
        import torch  # noqa: F401  (libtorch_cpu must be loaded first)
        _reftable = _bind(C.CDLL(REFTABLE_PATH), REFTABLE_SIGNATURES)
    return _reftable


def check(rc, what=''):
    if rc != 0:
        raise PcgcError(f'{what or "pcgc call"} failed ({rc}): {lib().pcgc_last_error().decode()}')
