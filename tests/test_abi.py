"""The Python binding is derived from include/cpe.h: every prototype is bound and exported, the structures lie as the C
compiler lays them out, the constants keep the values and names callers know, and a stale library is refused (no compute calls)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'cpe.h')

# the package's constants as callers import them: frozen here, whatever the header calls them
LIB_NAMES = dict(MAXP=2048, MAXL=256, PRED_MAXN=4096, CONSENSUS_MAX_HYP=4096, CONSENSUS_CONVERGED=1, CONSENSUS_SHRUNK=2,
                 DETECT_SKIP_DEBUG_PLANES=1)
FIT_NAMES = dict(MAXP=2048, SEL_CHOOSE_IDX=0, SEL_THRESHOLD=1, SEL_JOIN=2, FIT_NELDER_MEAD=0, FIT_LM=1,
                 FLAG_FALLBACK=1, FLAG_OVERFLOW=2, ST_OK=0, ST_FEW_POINTS=5, ST_OVERFLOW=6, FIT_MIN_POINTS=5, MATCH_MAX_WIN=8,
                 MATCH_SHIFTED=1, MATCH_WEAK=2, MATCH_EDGE=4, MATCH_OVERFLOW=8, PLANE_NO_GRID=1, PLANE_ORIGIN_POINT=2,
                 RELABEL_NO_CENTRE=1, RELABEL_OVERFLOW=2, RELABEL_FEW_LINES=4, LINE_KEPT=0, LINE_UNSUPPORTED=1, LINE_PHANTOM=2,
                 FUSED_TRUNCATED=4, PRED_MAXN=4096, PRED_OK=0, PRED_NO_FRAME=1, PRED_NO_PLANE=2, PRED_PARALLEL=3, PRED_MISS=4,
                 PRED_GRAZING=5, SHIFT_MAX_WIN=8, SHIFT_SHIFTED=1, SHIFT_WEAK=2, SHIFT_EDGE=4)
PLANES = dict(binary=0, hmask=1, vmask=2, mask_contour=3, roi_h=4, roi_v=5, exp_h=6, exp_v=7, joints=8, state=9,
              clahe=10, blur19=11, blur7=12, labels=13, sweep=14)


def test_exports(cpe):
    so = cpe.lib.SO_PATH
    assert os.path.exists(so), 'libcpe_hip.so missing: run __graft_entry__.build()'
    lib = ctypes.CDLL(so)
    names = cpe.lib.declared_symbols()
    assert 'cpe_preprocess_batch' in names
    for n in names:
        assert hasattr(lib, n), f'{n} declared in include/cpe.h but not exported'
    assert cpe.lib.load().cpe_version() >= 100
    # every prototype is bound: the header's `CPE_API ...` lines (the two `#define CPE_API` lines begin with `#`)
    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', open(HEADER).read(), flags=re.S)
    declared = sum(line.startswith('CPE_API ') for line in text.splitlines())
    assert declared == len(cpe.lib._SIGS) == len(names) and declared >= 60


def test_structures_lie_as_the_c_compiler_lays_them_out(cpe, tmp_path):
    structs = cpe.lib._STRUCTS
    assert len(structs) == 14 and all(getattr(cpe.lib, k) is v for k, v in structs.items())
    src = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(void) {']
    want = []
    for name, cls in structs.items():
        src.append(f'printf("{name} %zu\\n", sizeof({name}));')
        want.append(f'{name} {ctypes.sizeof(cls)}')
        for field, _ in cls._fields_:
            src.append(f'printf("{name}.{field} %zu %zu\\n", offsetof({name}, {field}), sizeof((({name} *)0)->{field}));')
            want.append(f'{name}.{field} {getattr(cls, field).offset} {getattr(cls, field).size}')
    src += ['return 0; }', '']
    (tmp_path / 'layout.c').write_text('\n'.join(src))
    subprocess.run([os.environ.get('CC', 'cc'), '-o', str(tmp_path / 'layout'), str(tmp_path / 'layout.c')], check=True)
    got = subprocess.run([str(tmp_path / 'layout')], check=True, capture_output=True, text=True).stdout.splitlines()
    assert got == want
    assert 'CpeRansacParams.seed 16 8' in got and 'CpeRansacParams 40' in got and 'CpeDetectConstants 176' in got
    assert 'CpeIndexShiftParams.win 0 8' in got and sum('CpeDetectConstants.' in g for g in got) == 34


def test_an_unknown_type_is_refused_by_name(cpe):
    P = cpe.lib.parse_header
    with pytest.raises(cpe.lib.CpeError, match='cpe_x'):
        P('CPE_API int32_t cpe_x(const __fp16 *p);')
    with pytest.raises(cpe.lib.CpeError, match='cpe_y'):
        P('CPE_API int32_t cpe_y(int32_t n, unsigned m);')
    with pytest.raises(cpe.lib.CpeError, match='cpe_z'):
        P('CPE_API float cpe_z(void);')
    with pytest.raises(cpe.lib.CpeError, match='CpeQ'):
        P('typedef struct CpeQ { int32_t a; float *b; } CpeQ;')
    for field in ('int32_t *p', 'int32_t v[CPE_N]', 'const double d', 'int32_t'):
        with pytest.raises(cpe.lib.CpeError, match='CpeR'):
            P('typedef struct { %s; } CpeR;' % field)
    sigs, structs, const = P('/* a, b */ typedef struct { int32_t a, w[2]; uint64_t s; } CpeP;  // c\n'
                             '#define CPE_A (-3)\n#define CPE_B 1e-6 /* x */\n#define CPE_C CPE_A << 1\n'
                             'CPE_API const char *cpe_u(const CpeP *p, /* x, y */ char *s,\n   const double *d, size_t n);\n'
                             'CPE_API void cpe_v(void);\n')
    c = ctypes
    assert sigs == {'cpe_u': (c.c_char_p, [c.c_void_p, c.c_char_p, c.c_void_p, c.c_size_t]), 'cpe_v': (None, [])}
    assert [(k, t) for k, t in structs['CpeP']._fields_][0::2] == [('a', c.c_int32), ('s', c.c_uint64)]
    assert structs['CpeP'].w.offset == 4 and structs['CpeP'].w.size == 8 and structs['CpeP'].s.offset == 16
    assert vars(const) == dict(A=-3, B=1e-6)


def test_a_missing_header_is_named(cpe, monkeypatch):
    monkeypatch.setattr(cpe.lib, 'HEADER_PATH', os.path.join(ROOT, 'include', 'no_such_cpe.h'))
    with pytest.raises(cpe.lib.CpeError, match='no_such_cpe.h'):
        cpe.lib._parse_own_header()


@pytest.mark.parametrize('module,name,value', [('lib', k, v) for k, v in LIB_NAMES.items()] +
                         [('fit', k, v) for k, v in FIT_NAMES.items()])
def test_public_names_keep_their_values(cpe, module, name, value):
    got = getattr(getattr(cpe, module), name)
    assert got == value and type(got) is int


def test_tables_of_names_keep_their_values(cpe):
    import torch
    assert cpe.api.PLANES == PLANES
    assert cpe.api.TARGETS == dict(cylinder=0, plane=1) == cpe.lib.TARGETS
    assert sorted(cpe.api.STATUS_TEXT) == list(range(8)) and cpe.api.STATUS_TEXT[6] == 'workspace capacity exceeded'
    pix = {torch.uint8: 0, torch.int16: 1, torch.float32: 2, torch.float64: 3}
    if hasattr(torch, 'uint16'):
        pix[torch.uint16] = 1
    assert cpe.iotool._PIX == pix
    assert cpe.lib.const.FIT_LM == 1 and cpe.lib.const.VERSION >= 126 and cpe.lib.const.ERR_ARG == -1


def test_a_stale_library_is_refused(cpe, monkeypatch):
    built = cpe.lib.load().cpe_version()
    assert built == cpe.lib.const.VERSION
    monkeypatch.setattr(cpe.lib, '_lib', None)
    monkeypatch.setattr(cpe.lib.const, 'VERSION', built + 1)
    with pytest.raises(cpe.lib.CpeError, match=rf'{built}\b.*\b{built + 1}\b.*rebuild'):
        cpe.lib.load()
    assert cpe.lib._lib is None
