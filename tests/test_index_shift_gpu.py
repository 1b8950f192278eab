"""cpe_index_shift_batch (csrc/fit.hip k_index_shift) against the numpy reference of tests/index_shift_cases.py.

Every case's margin is > 1e-6 (tests/test_index_shift_cases_cpu.py), so shift, score, scores, flags and idx_out are compared
exactly; rms at the case's rms_tol.  The C entry point is called with every output filled with poison first: what the call
leaves untouched shows."""
import ctypes as C

import numpy as np
import pytest
import torch

import index_shift_cases as SC
import table_tri_cases as TC

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A
INT_KEYS = ('shift', 'score', 'scores', 'flags', 'idx')


def _raw(cpe, gpu, X, I, cnt, use, table, win=(4, 4), tau=1.0, min_score=8, swap=0, scores=True, idx_out=None, lo=None, hi=None):
    """the C call on poisoned outputs -> rc, dict of numpy arrays"""
    t = lambda a, dt=None: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(gpu)
    n = len(cnt)
    dX, dI, dc, du = t(X), t(I), t(cnt), t(use)
    P, st = t(table['P'], np.float64), t(table['status'], np.int32)
    ncand = 2 * abs(win[0]) + 2 * abs(win[1]) + 2             # (a refused window still gets buffers that would hold it)
    full = lambda *shape: torch.full(shape, POISON, dtype=torch.int32, device=gpu)
    o = dict(shift=full(n, 2), score=full(n, 2, 4), scores=full(n, max(ncand, 1)), flags=full(n, 2), idx=full(n, SC.MAXP, 2),
             rms=torch.full((n, 2, 2), 1e300, dtype=torch.float64, device=gpu))
    prm = cpe.lib.CpeIndexShiftParams((C.c_int32 * 2)(*win), tau, min_score, swap)
    ptr = lambda a: None if a is None or a.numel() == 0 else a.data_ptr()
    rc = cpe.lib.load().cpe_index_shift_batch(ptr(dX), ptr(dI), ptr(dc), n, ptr(du), P.data_ptr(), st.data_ptr(),
                                              table['lo'] if lo is None else lo, table['hi'] if hi is None else hi, C.addressof(prm),
                                              ptr(o['shift']), ptr(o['score']), ptr(o['scores']) if scores else None, ptr(o['rms']),
                                              ptr(o['flags']), ptr(dI) if idx_out == 'alias' else ptr(o['idx']),
                                              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in o.items()}


def _call(cpe, gpu, case, poison=None, **kw):
    X, I, cnt, use = SC.arrays(case, poison)
    rc, out = _raw(cpe, gpu, X, I, cnt, use, case['table'], **dict(SC.params(case), **kw))
    assert rc == 0, cpe.lib.load().cpe_last_error_string()
    return out


def _compare(name, g, ref, scores=True):
    for k in ('shift', 'score', 'flags') + (('scores',) if scores else ()):
        assert np.array_equal(g[k], ref[k]), f'{name}: {k}\n{g[k]}\n{ref[k]}'
    d = np.abs(g['rms'] - ref['rms']).max() if g['rms'].size else 0.0
    print(f'{name}: rms off by {d:.2e} (tol {ref["rms_tol"]:.2e}), margin {ref["margin"]:.2e}')
    assert d <= ref['rms_tol'], f'{name}: rms {d:.3e} > {ref["rms_tol"]:.3e}'
    for f, c in enumerate(ref['count']):
        assert np.array_equal(g['idx'][f, :c], ref['idx'][f, :c]), f'{name}: idx_out of frame {f}'
        assert (g['idx'][f, c:].view(np.uint32) == POISON).all(), f'{name}: frame {f}: slots past the count were written'


@pytest.mark.parametrize('name', list(SC.cases()))
def test_case(cpe, gpu, name):
    """batches of 1, 2, 3, 5, 6, 8, 12 and 65 frames; counts -1 .. 3000; windows 0, 1, 2, 4, 5, 8; L 1, 25, 33, 65, 256; shifts of
    +-1, +-2, +-3 in either or both families, on the border of the window (EDGE) and outside it; NaN / Inf; use; garbage indices;
    refused lines; swap; WEAK by min_score, by the lead rule and by ties.  Poison in the inputs past every count changes no bit"""
    case = SC.cases()[name]
    a = _call(cpe, gpu, case, poison=41)
    b = _call(cpe, gpu, case)
    for k in INT_KEYS + ('rms',):
        assert a[k].tobytes() == b[k].tobytes(), f'{name}: {k} depends on slots past the count'
    _compare(name, a, SC.reference(name))


def test_scores_null_and_repeat(cpe, gpu):
    case = SC.cases()['eight shifts']
    ref = SC.reference('eight shifts')
    outs = [_call(cpe, gpu, case) for _ in range(3)]
    for o in outs[1:]:
        for k in INT_KEYS + ('rms',):
            assert o[k].tobytes() == outs[0][k].tobytes(), f'{k} does not repeat'
    g = _call(cpe, gpu, case, scores=False)
    _compare('scores NULL', g, ref, scores=False)
    for k in ('shift', 'score', 'flags', 'idx', 'rms'):
        assert g[k].tobytes() == outs[0][k].tobytes()


def test_refused_arguments(cpe, gpu):
    """a window of 9, L = 257, tau = 0 or NaN, a negative min_score, swap 2, idx_out = idx: CPE_ERR_ARG and nothing written"""
    case = SC.cases()['three frames']
    X, I, cnt, use = SC.arrays(case)
    rig = case['table']
    big = dict(P=np.zeros((2, 257, 4)), status=np.zeros((2, 257), np.int32), lo=0, hi=256)
    for what, kw, tab in (('win 9', dict(win=(9, 0)), rig), ('win 9', dict(win=(0, 9)), rig), ('win -1', dict(win=(-1, 4)), rig),
                          ('tau 0', dict(tau=0.0), rig), ('tau nan', dict(tau=float('nan')), rig), ('tau < 0', dict(tau=-1.0), rig),
                          ('min_score', dict(min_score=-1), rig), ('swap', dict(swap=2), rig), ('alias', dict(idx_out='alias'), rig),
                          ('L 257', {}, big), ('L 0', dict(lo=3, hi=2), rig)):
        rc, g = _raw(cpe, gpu, X, I, cnt, use, tab, **kw)
        assert rc == -1, what
        for k in INT_KEYS:
            assert (g[k].view(np.uint32) == POISON).all(), f'{what}: {k} written'
        assert (g['rms'] == 1e300).all()
    tab = cpe.fit.LaserTable(*(torch.from_numpy(rig[k]).to(gpu) for k in ('P', 'status')), rig['lo'], rig['hi'],
                             torch.zeros(4, dtype=torch.float64, device=gpu), torch.zeros(1, dtype=torch.int32, device=gpu))
    dX, dI, dc = (torch.from_numpy(a).to(gpu) for a in (X, I, cnt))
    for kw in (dict(win=(9, 4)), dict(win=(4, 9)), dict(tau=0.0), dict(tau=float('nan'))):
        with pytest.raises(ValueError):
            cpe.fit.index_shift_batch(dX, dI, dc, tab, **kw)
    with pytest.raises(ValueError):
        cpe.fit.LaserTable(torch.zeros((2, 257, 4)), torch.zeros((2, 257), dtype=torch.int32), 0, 256, torch.zeros(4), torch.zeros(1))


def test_n_zero(cpe, gpu):
    rig = TC.rig_table(-16, 16)
    rc, g = _raw(cpe, gpu, np.zeros((0, SC.MAXP, 3)), np.zeros((0, SC.MAXP, 2), np.int32), np.zeros(0, np.int32), None, rig)
    assert rc == 0
    tab = cpe.fit.LaserTable(*(torch.from_numpy(rig[k]).to(gpu) for k in ('P', 'status')), -16, 16,
                             torch.zeros(4, dtype=torch.float64, device=gpu), torch.zeros(1, dtype=torch.int32, device=gpu))
    out = cpe.fit.index_shift_batch(torch.zeros((0, SC.MAXP, 3), dtype=torch.float64, device=gpu),
                                    torch.zeros((0, SC.MAXP, 2), dtype=torch.int32, device=gpu),
                                    torch.zeros(0, dtype=torch.int32, device=gpu), tab)
    assert tuple(out['shift'].shape) == (0, 2) and tuple(out['scores'].shape) == (0, 18) and tuple(out['idx'].shape) == (0, SC.MAXP, 2)


def test_python_layer_equals_the_c_call(cpe, gpu):
    """fit.index_shift_batch: the same bits as the C call, zeros past the count, and swap from the table's family0"""
    for name, family0, ids, transposed in (('three frames', 'col', 'col_row', False), ('transposed swap 1', 'row', 'col_row', True),
                                           ('transposed swap 1', 'col', 'row_col', True), ('use', 'col', 'col_row', False),
                                           ('window 2 5', 'row', 'row_col', False)):
        case = SC.cases()[name]
        X, I, cnt, use = SC.arrays(case)
        raw = _call(cpe, gpu, case)
        t = case['table']
        tab = cpe.fit.LaserTable(torch.from_numpy(t['P']).to(gpu), torch.from_numpy(t['status']).to(gpu), t['lo'], t['hi'],
                                 torch.zeros(4, dtype=torch.float64, device=gpu), torch.zeros(1, dtype=torch.int32, device=gpu), family0)
        assert tab.swap_for(ids) == SC.params(case)['swap'] == int(transposed)
        p = SC.params(case)
        out = cpe.fit.index_shift_batch(*(torch.from_numpy(a).to(gpu) for a in (X, I, cnt)), tab,
                                        use=None if use is None else torch.from_numpy(use).to(gpu), win=p['win'], tau=p['tau'],
                                        min_score=p['min_score'], ids=ids)
        torch.cuda.synchronize()
        assert set(out) == {'shift', 'score', 'scores', 'rms', 'flags', 'idx'}
        for k in ('shift', 'score', 'scores', 'flags', 'rms'):
            assert out[k].cpu().numpy().tobytes() == raw[k].tobytes(), f'{name}: {k}'
        got = out['idx'].cpu().numpy()
        for f, c in enumerate(SC.reference(name)['count']):
            assert np.array_equal(got[f, :c], raw['idx'][f, :c]) and not got[f, c:].any()
