"""cpe_grid_relabel_batch (csrc/fit.hip k_grid_relabel) against the numpy reference of tests/relabel_cases.py.

Every case's margin is > 1e-6 and its tolerance <= 1e-6 px (tests/test_relabel_cases_cpu.py), so id_out, cnt_out, src, the line
table's labels, indices, points and states, counts and flags are compared exactly; p at the case's tol and pitch at twice
that.  The C entry point is called with every output filled with poison first: what the call leaves untouched shows."""
import ctypes as C

import numpy as np
import pytest
import torch

import relabel_cases as RC

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A
FPOISON = 1e300
INT_KEYS = ('id', 'cnt', 'src', 'lines', 'counts', 'flags')
F64_KEYS = ('xy', 'line_p', 'pitch')


def _raw(cpe, gpu, xy, ids, cnt, center, swap=0, min_pts=3, merge_frac=0.65, dir=(1, 1), alias=None):
    """the C call on poisoned outputs -> rc, dict of numpy arrays"""
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(gpu)
    n = len(cnt)
    i = dict(xy=t(xy, np.float64), id=t(ids, np.int32), cnt=t(cnt, np.int32), center=t(center, np.float64))
    full = lambda *shape: torch.full(shape, POISON, dtype=torch.int32, device=gpu)
    ffull = lambda *shape: torch.full(shape, FPOISON, dtype=torch.float64, device=gpu)
    o = dict(xy=ffull(n, RC.MAXP, 2), id=full(n, RC.MAXP, 2), cnt=full(n), src=full(n, RC.MAXP), lines=full(n, 2, RC.MAXL, 4),
             line_p=ffull(n, 2, RC.MAXL), pitch=ffull(n, 2), counts=full(n, 2, 4), flags=full(n))
    ptr = lambda a: None if a.numel() == 0 else a.data_ptr()
    po = {k: ptr(v) for k, v in o.items()}
    if alias == 'xy':
        po['xy'] = ptr(i['xy'])
    elif alias == 'id':
        po['id'] = ptr(i['id'])
    elif alias == 'tail':                               # src starts inside id_out
        po['src'] = po['id'] + 4 * (o['id'].numel() - 1)
    prm = cpe.lib.CpeRelabelParams(swap, min_pts, merge_frac, (C.c_int32 * 2)(*dir))
    rc = cpe.lib.load().cpe_grid_relabel_batch(ptr(i['xy']), ptr(i['id']), ptr(i['cnt']), ptr(i['center']), n, C.addressof(prm), po['xy'],
                                               po['id'], po['cnt'], po['src'], po['lines'], po['line_p'], po['pitch'], po['counts'],
                                               po['flags'], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in o.items()}


def _call(cpe, gpu, case, poison=None):
    rc, out = _raw(cpe, gpu, *RC.arrays(case, poison), **case['params'])
    assert rc == 0, cpe.lib.load().cpe_last_error_string()
    return out


def _untouched_i(a):
    return (np.ascontiguousarray(a).view(np.uint32) == POISON).all()


def _compare(name, g, ref):
    assert np.array_equal(g['cnt'], ref['cnt']), f'{name}: cnt_out\n{g["cnt"]}\n{ref["cnt"]}'
    assert np.array_equal(g['flags'], ref['flags']), f'{name}: flags\n{g["flags"]}\n{ref["flags"]}'
    assert np.array_equal(g['counts'], ref['counts']), f'{name}: counts\n{g["counts"]}\n{ref["counts"]}'
    worst = 0.0
    for f, m in enumerate(ref['cnt']):
        assert np.array_equal(g['id'][f, :m], ref['id'][f, :m]), f'{name}: id_out of image {f}'
        assert np.array_equal(g['src'][f, :m], ref['src'][f, :m]), f'{name}: src of image {f}'
        assert g['xy'][f, :m].tobytes() == ref['xy'][f, :m].tobytes(), f'{name}: xy_out of image {f}'
        assert _untouched_i(g['id'][f, m:]) and _untouched_i(g['src'][f, m:]) and (g['xy'][f, m:] == FPOISON).all(), \
            f'{name}: image {f}: slots from cnt_out on were written'
        for c in range(2):
            nl = ref['counts'][f, c, 0]
            for j, k in enumerate(('label', 'index', 'points', 'state')):
                assert np.array_equal(g['lines'][f, c, :nl, j], ref[k][f, c, :nl]), f'{name}: image {f} component {c}: line {k}'
            assert _untouched_i(g['lines'][f, c, nl:]) and (g['line_p'][f, c, nl:] == FPOISON).all(), \
                f'{name}: image {f} component {c}: line slots past the labels seen were written'
            tol = ref['tol'][f, c]
            d = max(np.abs(g['line_p'][f, c, :nl] - ref['p'][f, c, :nl]).max() if nl else 0.0, abs(g['pitch'][f, c] - ref['pitch'][f, c]) / 2)
            worst = max(worst, d)
            assert d <= tol, f'{name}: image {f} component {c}: p / pitch off by {d:.3e} > {tol:.3e}'
    print(f'{name}: p / pitch off by at most {worst:.2e} (tol up to {ref["tol"].max():.2e}), margin {ref["margin"]:.2e}')


@pytest.mark.parametrize('name', list(RC.cases()))
def test_case(cpe, gpu, name):
    """boards behind every measured label pattern; batches of 1, 3 and 65 images; counts -1, 0, 1, 2, 63, 64, 65, 2048, 3000; 1,
    2, 3, 64, 65 and 256 lines per component; a label span of 255 and of 256 (OVERFLOW, either component); labels at both ends of
    int32; NaN / Inf pixels, a NaN / Inf centre; min_pts 2 and 5; dir -1; swap 1 on transposed tables.  Poison in the inputs past
    every count changes no bit"""
    case = RC.cases()[name]
    a = _call(cpe, gpu, case, poison=41)
    b = _call(cpe, gpu, case)
    for k in INT_KEYS + F64_KEYS:
        assert a[k].tobytes() == b[k].tobytes(), f'{name}: {k} depends on slots past the count'
    _compare(name, a, RC.reference(name))


def test_three_calls_give_equal_bits(cpe, gpu):
    for name in ('measured pattern', '256 lines', '65 images'):
        outs = [_call(cpe, gpu, RC.cases()[name], poison=3) for _ in range(3)]
        for o in outs[1:]:
            for k in INT_KEYS + F64_KEYS:
                assert o[k].tobytes() == outs[0][k].tobytes(), f'{name}: {k} does not repeat'


def test_refused_arguments(cpe, gpu):
    """min_pts 1, merge_frac 0, 1 and NaN, dir 0 and 2, swap 2 and -1, an output that is an input, two outputs that share
    bytes: CPE_ERR_ARG and nothing written"""
    case = RC.cases()['identity']
    arr = RC.arrays(case)
    for what, kw in (('min_pts 1', dict(min_pts=1)), ('min_pts 0', dict(min_pts=0)), ('merge_frac 0', dict(merge_frac=0.0)),
                     ('merge_frac 1', dict(merge_frac=1.0)), ('merge_frac nan', dict(merge_frac=float('nan'))),
                     ('dir 0', dict(dir=(0, 1))), ('dir 2', dict(dir=(1, 2))), ('swap 2', dict(swap=2)), ('swap -1', dict(swap=-1)),
                     ('xy_out = xy', dict(alias='xy')), ('id_out = id', dict(alias='id')), ('src inside id_out', dict(alias='tail'))):
        rc, g = _raw(cpe, gpu, *arr, **kw)
        assert rc == -1, what
        for k in INT_KEYS:
            assert _untouched_i(g[k]), f'{what}: {k} written'
        for k in F64_KEYS:
            assert (g[k] == FPOISON).all(), f'{what}: {k} written'
    dev = [torch.from_numpy(a).to(gpu) for a in arr]
    tabs = cpe.fit.GridTables(*dev[:3])
    for kw in (dict(min_pts=1), dict(merge_frac=0.0), dict(merge_frac=1.5), dict(dir=(0, 1)), dict(dir=(1,)), dict(swap=2)):
        with pytest.raises(ValueError):
            cpe.fit.grid_relabel_batch(tabs, dev[3], **kw)
    with pytest.raises(TypeError):
        cpe.fit.grid_relabel_batch(tabs, dev[3][:, :1])


def test_n_zero(cpe, gpu):
    rc, g = _raw(cpe, gpu, np.zeros((0, RC.MAXP, 2)), np.zeros((0, RC.MAXP, 2), np.int32), np.zeros(0, np.int32), np.zeros((0, 2)))
    assert rc == 0
    z = lambda *s, dt=torch.float64: torch.zeros(s, dtype=dt, device=gpu)
    out = cpe.fit.grid_relabel_batch(cpe.fit.GridTables(z(0, RC.MAXP, 2), z(0, RC.MAXP, 2, dt=torch.int32), z(0, dt=torch.int32)), z(0, 2))
    assert tuple(out['tables'].xy.shape) == (0, RC.MAXP, 2) and tuple(out['lines']['p'].shape) == (0, 2, RC.MAXL)
    assert tuple(out['counts'].shape) == (0, 2, 4) and tuple(out['flags'].shape) == (0,)


def test_python_layer_equals_the_c_call(cpe, gpu):
    """fit.grid_relabel_batch: the same bits as the C call where it writes, zeros elsewhere"""
    for name in ('measured pattern', 'swap 1 transposed', 'dir -1', 'min_pts 5', 'span 256', 'nan centre', 'counts'):
        case = RC.cases()[name]
        raw = _call(cpe, gpu, case)
        xy, ids, cnt, ctr = (torch.from_numpy(a).to(gpu) for a in RC.arrays(case))
        out = cpe.fit.grid_relabel_batch(cpe.fit.GridTables(xy, ids, cnt), ctr, **case['params'])
        torch.cuda.synchronize()
        assert set(out) == {'tables', 'src', 'lines', 'pitch', 'counts', 'flags'}
        assert set(out['lines']) == {'label', 'index', 'points', 'state', 'p'}
        h = lambda t: t.cpu().numpy()
        for k, t in (('cnt', out['tables'].cnt), ('counts', out['counts']), ('flags', out['flags']), ('pitch', out['pitch'])):
            assert h(t).tobytes() == raw[k].tobytes(), f'{name}: {k}'
        got = dict(xy=h(out['tables'].xy), id=h(out['tables'].id), src=h(out['src']))
        lines = np.stack([h(out['lines'][k]) for k in ('label', 'index', 'points', 'state')], -1)
        for f, m in enumerate(raw['cnt']):
            for k in ('xy', 'id', 'src'):
                assert got[k][f, :m].tobytes() == raw[k][f, :m].tobytes() and not got[k][f, m:].any(), f'{name}: {k} of image {f}'
            for c in range(2):
                nl = raw['counts'][f, c, 0]
                assert np.array_equal(lines[f, c, :nl], raw['lines'][f, c, :nl]) and not lines[f, c, nl:].any()
                p = h(out['lines']['p'])[f, c]
                assert p[:nl].tobytes() == raw['line_p'][f, c, :nl].tobytes() and not p[nl:].any()
