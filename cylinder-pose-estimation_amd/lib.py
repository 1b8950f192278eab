"""ctypes loader for libcpe_hip.so (C ABI: include/cpe.h).

include/cpe.h is the one declaration of the boundary; nothing of it is typed again here.  At import the header is parsed
(no library and no GPU needed) into
  _SIGS        name -> (restype, argtypes) of every `CPE_API` prototype,
  Cpe...       a ctypes.Structure per `typedef struct { ... } CpeX;`, published under the header's name,
  const        every numeric `#define CPE_X`, named without the prefix: const.MAXP, const.FIT_LM, const.ST_OVERFLOW.
load() refuses a library whose cpe_version() is not the header's CPE_VERSION.
There is NO CPU fallback: if the HIP library is missing or a call fails, this raises."""
import ctypes as C
import os
import re
import subprocess
import types

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.path.join(_HERE, 'libcpe_hip.so')
HEADER_PATH = os.path.normpath(os.path.join(_HERE, '..', 'include', 'cpe.h'))
_lib = None


class CpeError(RuntimeError):
    pass


def build(verbose=False):
    """compile every HIP source for gfx950 (hipcc cross-compiles without a GPU)."""
    cmd = ['make', '-C', os.path.join(_HERE, 'csrc'), '-j4']
    if not verbose:
        cmd.insert(1, '-s')
    subprocess.check_call(cmd)
    return SO_PATH


# by value: parameters, returns and structure fields; a pointer may point at any of _POINTEES or at a structure of the header
_VALUES = {'int32_t': C.c_int32, 'int64_t': C.c_int64, 'uint64_t': C.c_uint64, 'size_t': C.c_size_t, 'double': C.c_double}
_POINTEES = set(_VALUES) | {'void', 'char', 'uint8_t', 'int16_t', 'uint16_t', 'uint32_t', 'float'}


def _ctype(decl, structs, where):
    """ctypes type of a parameter or return declaration: char * -> c_char_p, any other known pointer -> c_void_p (callers
    pass data_ptr() ints, addressof, byref), known values -> theirs, void -> None; anything else raises"""
    words = [t for t in re.findall(r'\w+|\*', decl) if t != 'const']
    base, stars = (words or [''])[0], words.count('*')
    if stars == 1 and (base in _POINTEES or base in structs):
        return C.c_char_p if base == 'char' else C.c_void_p
    if stars == 0 and base in _VALUES:
        return _VALUES[base]
    if words == ['void']:
        return None
    raise CpeError(f'{where}: no ctypes type for "{" ".join(decl.split())}"')


def _number(text):
    """value of an int or float literal, optionally signed and parenthesised; None for anything else"""
    text = re.sub(r'^\(\s*(.*?)\s*\)$', r'\1', text.strip())
    for convert in (lambda t: int(t, 0), float):
        try:
            return convert(text)
        except ValueError:
            pass
    return None


def parse_header(text):
    """-> (sigs, structs, consts) of a header written like include/cpe.h"""
    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)     # comments first: they hold commas, parentheses and names
    structs = {}
    for body, name in re.findall(r'typedef\s+struct\s*\w*\s*\{(.*?)\}\s*(\w+)\s*;', text, flags=re.S):
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(';'))):
            one = r'\w+\s*(?:\[\d+\])?'                             # a value type and its declarators: `int32_t a, win[2]`
            m = re.fullmatch(rf'(\w+)\s+({one}(?:\s*,\s*{one})*)', decl)
            if not m or m.group(1) not in _VALUES:
                raise CpeError(f'struct {name}: no ctypes type for "{decl}"')
            ctype = _VALUES[m.group(1)]
            for field, dim in re.findall(r'(\w+)\s*(?:\[(\d+)\])?', m.group(2)):
                fields.append((field, ctype * int(dim) if dim else ctype))
        structs[name] = type(name, (C.Structure,), {'_fields_': fields})
    sigs = {}
    for ret, name, params in re.findall(r'^CPE_API\s+([^;()]*?)(cpe_\w+)\s*\(([^;()]*)\)\s*;', text, flags=re.M):
        args = [] if params.strip() == 'void' else [_ctype(p, structs, name) for p in params.split(',')]
        if None in args:
            raise CpeError(f'{name}: a parameter of type void')
        sigs[name] = (_ctype(ret, structs, name), args)
    defines = re.findall(r'^[ \t]*#[ \t]*define[ \t]+CPE_(\w+)[ \t]+(\S.*)$', text, flags=re.M)
    consts = {name: _number(value) for name, value in defines}
    return sigs, structs, types.SimpleNamespace(**{k: v for k, v in consts.items() if v is not None})


def _parse_own_header():
    try:
        with open(HEADER_PATH) as f:
            return parse_header(f.read())
    except OSError as e:
        raise CpeError(f'{HEADER_PATH}: the C header this binding is derived from cannot be read ({e})') from e


_SIGS, _STRUCTS, const = _parse_own_header()
globals().update(_STRUCTS)      # CpeDetectParams, CpeDetectConstants, CpeFitParams, ...: the header's typedef names

MAXP, MAXL, PRED_MAXN = const.MAXP, const.MAXL, const.PRED_MAXN
DETECT_SKIP_DEBUG_PLANES = const.DETECT_SKIP_DEBUG_PLANES                   # CpeDetectParams.flags
CONSENSUS_MAX_HYP = const.CONSENSUS_MAX_HYP
CONSENSUS_CONVERGED, CONSENSUS_SHRUNK = const.CONSENSUS_CONVERGED, const.CONSENSUS_SHRUNK   # flags of cpe_multi_frame_consensus_batch


def const_group(prefix):
    """{'binary': 0, 'hmask': 1, ...} for 'PLANE_': the header's CPE_<prefix>* constants by their lower-case remainder"""
    return {k[len(prefix):].lower(): v for k, v in vars(const).items() if k.startswith(prefix)}


TARGETS = const_group('TARGET_')


def detect_constants(target='cylinder'):
    """dict of the reference's inline constants as the kernels use them (cpe_detect_constants: a report, not a setter)"""
    c = _STRUCTS['CpeDetectConstants']()
    check(load().cpe_detect_constants(TARGETS[target], C.byref(c)), 'cpe_detect_constants')
    return {k: getattr(c, k) for k, _ in c._fields_}


def load():
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise CpeError(f'{SO_PATH} not found: run `python -c "import __graft_entry__ as g; g.build()"` '
                           '(the product path has no CPU fallback)')
        lib = C.CDLL(SO_PATH)
        built = lib.cpe_version()       # int32_t (void): ctypes' defaults fit
        if built != const.VERSION:      # the one way left for argtypes and code to disagree: refuse it
            raise CpeError(f'{SO_PATH} is version {built}, {HEADER_PATH} declares {const.VERSION}: rebuild the library')
        for name, (res, args) in _SIGS.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def check(rc, what):
    if rc != 0:
        msg = load().cpe_last_error_string().decode()
        raise CpeError(f'{what} failed (rc={rc}): {msg}')


def profile(on):
    load().cpe_profile_enable(1 if on else 0)


def profile_report():
    """-> list of (kernel, calls, total_ms) sorted by total time (descending); clears the timers"""
    buf = C.create_string_buffer(1 << 16)
    load().cpe_profile_report(buf, len(buf))
    out = []
    for line in buf.value.decode().splitlines():
        name, calls, ms = line.rsplit(',', 2)
        out.append((name, int(calls), float(ms)))
    return out


def declared_symbols():
    """names declared with CPE_API in include/cpe.h"""
    return sorted(_SIGS)
