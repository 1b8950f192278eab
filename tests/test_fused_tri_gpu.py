"""cpe_fused_triangulate_batch (csrc/fit.hip k_fused_triangulate) against the numpy reference of tests/fused_tri_cases.py: points,
residuals and stats at the tolerances derived there; m, counts, flags, idx, src and the order exactly; a frame with an empty table
against cpe_table_triangulate_batch bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import fused_tri_cases as FC
import table_tri_cases as TC

pytestmark = pytest.mark.gpu

KEYS = ('pts3', 'idx', 'res', 'src', 'm', 'counts', 'stats', 'flags')
SENTINEL_F, SENTINEL_I = -7.25, -77


def _table(cpe, gpu, t, family0='col'):
    return cpe.fit.LaserTable(torch.from_numpy(t['P']).to(gpu), torch.from_numpy(t['status'].astype(np.int32)).to(gpu), t['lo'], t['hi'],
                              torch.zeros(4, dtype=torch.float64, device=gpu), torch.zeros(1, dtype=torch.int32, device=gpu), family0)


def _tables(cpe, gpu, frames, poison=None):
    return [cpe.fit.GridTables(*(torch.from_numpy(a).to(gpu) for a in t)) for t in FC.pack2(frames, poison)]


def _fuse(cpe, gpu, frames, table, poison=None, family0='col', **kw):
    K1, K2, T21 = FC.rig_cams()
    kw.pop('swap', None)                      # the wrapper derives it from family0
    g1, g2 = _tables(cpe, gpu, frames, poison)
    out = cpe.fit.fused_triangulate_batch(g1, g2, K1, K2, T21, _table(cpe, gpu, table, family0), **kw)
    torch.cuda.synchronize()
    return {k: out[k].cpu().numpy() for k in KEYS}


def _frame(out, i):
    return {k: out[k][i] for k in KEYS}


def _report(name, g, ref):
    if ref['m']:
        m = ref['m']
        print(f'{name}: m {m} counts {ref["counts"]}  X {np.abs(g["pts3"][:m] - ref["X"]).max():.2e} / {ref["tol_X"].min():.2e}  '
              f'res {np.abs(g["res"][:m] - ref["res"]).max(0)} / {ref["tol_res"].max(0)}')


@pytest.mark.parametrize('need_both', [0, 1])
def test_batches_of_1_3_65(cpe, gpu, need_both):
    seen = set()
    for names, frames in FC.batches():
        a = _fuse(cpe, gpu, frames, TC.main_table(), poison=41, need_both=need_both)     # NaN, infinities, garbage indices past every count
        b = _fuse(cpe, gpu, frames, TC.main_table(), need_both=need_both)                # zeros there
        for k in KEYS:
            assert a[k].tobytes() == b[k].tobytes(), f'{k} depends on slots past the count'
        for i, name in enumerate(names):
            ref = FC.frame_reference(name, need_both)
            g = _frame(a, i)
            if name not in seen:
                _report(name, g, ref)
            FC.compare_frame(g, ref, f'{name} (frame {i} of {len(names)}, need_both {need_both})')
            assert not g['pts3'][ref['m']:].any() and not g['src'][ref['m']:].any()      # the wrapper's zeros past m
            seen.add(name)
    assert seen == set(FC.frame_cases())


@pytest.mark.parametrize('name', list(FC.call_cases()))
def test_calls_with_their_own_table_and_parameters(cpe, gpu, name):
    """every line refused, L = 1 and 256, swap through a transposed table, need_both, other sigmas, the max_res and max_px gates,
    truncation (2048 + 100 disjoint points: m = 2048, counts[5] = 100, the flag)"""
    case = FC.call_cases()[name]
    family0 = 'row' if case['params'].get('swap') else 'col'
    got = _fuse(cpe, gpu, case['frames'], case['table'], poison=9, family0=family0, **case['params'])
    for i, ref in enumerate(FC.call_reference(name)):
        _report(f'{name} [{i}]', _frame(got, i), ref)
        FC.compare_frame(_frame(got, i), ref, f'{name} frame {i}')
    if name == 'truncation':
        assert int(got['m'][0]) == FC.MAXP and int(got['counts'][0, 5]) == 100 and int(got['flags'][0]) == FC.FLAG_TRUNCATED


@pytest.mark.parametrize('cam', [1, 2])
def test_an_empty_table_gives_the_one_camera_call_bit_for_bit(cpe, gpu, cam):
    """the same device function: X, idx and the plane residuals of cpe_table_triangulate_batch, also for indices of any size
    (the frames hold camera 1's pixels; read as camera 2's they give other points, fewer of them, which serves as well)"""
    names = ('count 129', 'one component out of range', 'nan pixels', 'count 2048', 'refused across rounds')
    one = [TC.frame_cases()[k] for k in names]
    empty = dict(xy=np.zeros((3, 2)), id=np.zeros((3, 2), np.int32), cnt=0)
    frames = [(f, empty) if cam == 1 else (empty, f) for f in one]
    K, Tc = TC.camera(cam)
    for need_both in (0, 1):
        a = _fuse(cpe, gpu, frames, TC.main_table(), poison=3, need_both=need_both)
        gp = cpe.fit.GridTables(*(torch.from_numpy(x).to(gpu) for x in TC.pack(one, 5)))
        b = cpe.fit.table_triangulate_batch(gp, K, Tc, _table(cpe, gpu, TC.main_table()), need_both=need_both)
        b = {k: v.cpu().numpy() for k, v in b.items()}
        assert np.array_equal(a['m'], b['m']) and a['m'].sum() > 300 and not a['flags'].any()
        assert a['pts3'].tobytes() == b['pts3'].tobytes() and a['idx'].tobytes() == b['idx'].tobytes()
        assert a['res'][:, :, 2:].tobytes() == b['res'].tobytes() and not a['res'][:, :, :2].any()
        assert a['stats'][:, 2:].tobytes() == b['stats'].tobytes() and not a['stats'][:, :2].any()
        for i in range(len(one)):
            m = int(a['m'][i])
            assert np.array_equal(a['src'][i, :m, 0], (1 << (cam - 1)) | (b['src'][i, :m, 0] << 2))
            assert np.array_equal(a['src'][i, :m, cam], b['src'][i, :m, 1]) and (a['src'][i, :m, 3 - cam] == -1).all()
            assert a['counts'][i].tolist() == [m, 0, m if cam == 1 else 0, m if cam == 2 else 0, int(b['counts'][i, 2] + b['counts'][i, 3]), 0]


def _raw(cpe, gpu, frames, t, prm, fill=None):
    """the C call itself -> rc, the outputs (pre-filled with the sentinels where fill is set)"""
    K1, K2, T21 = FC.rig_cams()
    n = len(frames)
    g1, g2 = _tables(cpe, gpu, frames) if n else [cpe.fit.GridTables(torch.zeros((0, TC.MAXP, 2), dtype=torch.float64, device=gpu),
                                                                    torch.zeros((0, TC.MAXP, 2), dtype=torch.int32, device=gpu),
                                                                    torch.zeros(0, dtype=torch.int32, device=gpu))] * 2
    dv = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64).reshape(-1)).to(gpu)
    Kd1, Kd2, Td, P = dv(K1), dv(K2), dv(T21), dv(t['P'])
    st = torch.from_numpy(np.ascontiguousarray(t['status'], np.int32)).to(gpu)
    mk = lambda shape, dt, v: torch.full((max(n, 1),) + shape, v if fill else 0, dtype=dt, device=gpu)
    o = dict(pts3=mk((TC.MAXP, 3), torch.float64, SENTINEL_F), idx=mk((TC.MAXP, 2), torch.int32, SENTINEL_I),
             res=mk((TC.MAXP, 4), torch.float64, SENTINEL_F), src=mk((TC.MAXP, 3), torch.int32, SENTINEL_I), m=mk((), torch.int32, SENTINEL_I),
             counts=mk((6,), torch.int32, SENTINEL_I), stats=mk((4,), torch.float64, SENTINEL_F), flags=mk((), torch.int32, SENTINEL_I))
    rc = cpe.lib.load().cpe_fused_triangulate_batch(g1.xy.data_ptr(), g1.id.data_ptr(), g1.cnt.data_ptr(), g2.xy.data_ptr(), g2.id.data_ptr(),
                                                    g2.cnt.data_ptr(), n, Kd1.data_ptr(), Kd2.data_ptr(), Td.data_ptr(), P.data_ptr(),
                                                    st.data_ptr(), t['lo'], t['hi'], None if prm is None else C.addressof(prm),
                                                    *(o[k].data_ptr() for k in KEYS), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in o.items()}


def test_null_params_sentinels_and_equal_bits(cpe, gpu):
    """NULL params are the defaults; slots from m on, of every per-point output, keep what they held; two calls, the same bits"""
    names = ('counts 200 / 130', 'duplicates', 'nan pixels', 'index span overflow', 'both empty', 'thirds')
    frames = [FC.frame_cases()[k] for k in names]
    t = TC.main_table()
    rc, a = _raw(cpe, gpu, frames, t, None, fill=True)
    assert rc == 0
    rc, b = _raw(cpe, gpu, frames, t, cpe.lib.CpeFusedTriParams(0, 0, 0.01, 0.25, 0.02, 0.0, 0.0), fill=True)
    assert rc == 0
    for k in KEYS:
        assert a[k].tobytes() == b[k].tobytes(), k
    for i, name in enumerate(names):
        ref = FC.frame_reference(name)
        FC.compare_frame(_frame(a, i), ref, name)
        m = ref['m']
        assert (a['pts3'][i, m:] == SENTINEL_F).all() and (a['res'][i, m:] == SENTINEL_F).all(), f'{name}: a slot from m on was written'
        assert (a['idx'][i, m:] == SENTINEL_I).all() and (a['src'][i, m:] == SENTINEL_I).all(), f'{name}: a slot from m on was written'
    assert a['flags'][3] == FC.FLAG_OVERFLOW and a['m'][3] == 0 and not a['counts'][3].any() and not a['stats'][3].any()


def test_arguments(cpe, gpu):
    t = TC.main_table()
    fr = [FC.frame_cases()['counts 65 / all']]
    P = cpe.lib.CpeFusedTriParams
    rc, _ = _raw(cpe, gpu, fr, dict(TC.rig_table(-128, 127), hi=128), None)      # L = 257
    assert rc == -1
    rc, _ = _raw(cpe, gpu, fr, dict(t, hi=t['lo'] - 1), None)                      # L = 0
    assert rc == -1
    for bad in (P(2, 0, 0.01, 0.25, 0.02, 0, 0), P(0, 2, 0.01, 0.25, 0.02, 0, 0), P(0, 0, -1.0, 0.25, 0.02, 0, 0), P(0, 0, 0.01, 0.0, 0.02, 0, 0),
                P(0, 0, 0.01, 0.25, -0.02, 0, 0), P(0, 0, 0.01, float('nan'), 0.02, 0, 0), P(0, 0, 0.01, 0.25, float('inf'), 0, 0),
                P(0, 0, 0.01, 0.25, 0.02, float('nan'), 0), P(0, 0, 0.01, 0.25, 0.02, 0, float('nan'))):
        rc, _ = _raw(cpe, gpu, fr, t, bad)
        assert rc == -1
    rc, o = _raw(cpe, gpu, [], t, None, fill=True)                                 # n = 0: a no-op
    assert rc == 0 and (o['m'] == SENTINEL_I).all() and (o['pts3'] == SENTINEL_F).all()
    g1, g2 = _tables(cpe, gpu, fr)
    K1, K2, T21 = FC.rig_cams()
    with pytest.raises(TypeError):
        cpe.fit.fused_triangulate_batch(cpe.fit.GridTables(g1.xy.float(), g1.id, g1.cnt), g2, K1, K2, T21, _table(cpe, gpu, t))
    with pytest.raises(ValueError):
        cpe.fit.fused_triangulate_batch(g1, g2, K1, K2, T21, _table(cpe, gpu, t), sigma_mm=0.0)
    z = cpe.fit.GridTables(g1.xy[:0], g1.id[:0], g1.cnt[:0])
    assert cpe.fit.fused_triangulate_batch(z, z, K1, K2, T21, _table(cpe, gpu, t))['pts3'].shape == (0, TC.MAXP, 3)


def test_fit_on_fused_points(cpe, gpu):
    """fit_single_cylinder_fused_batch = the fused call, then the fit on its points; mean_err is the rms ray residual; an
    overflowing frame is reported as ST_OVERFLOW"""
    fit = cpe.fit
    case = FC.noisy_case(0, 'noisy', True)
    frames = [case['frame'], FC.frame_cases()['index span overflow']]
    K1, K2, T21 = FC.rig_cams()
    g1, g2 = _tables(cpe, gpu, frames)
    tab = _table(cpe, gpu, case['table'])
    out = fit.fit_single_cylinder_fused_batch(g1, g2, K1, K2, T21, tab, TC.RADIUS, mode=fit.FIT_LM)
    tri = fit.fused_triangulate_batch(g1, g2, K1, K2, T21, tab)
    ref = fit.fit_cylinder_batch(tri['pts3'], tri['m'], TC.RADIUS, mode=fit.FIT_LM)
    torch.cuda.synchronize()
    for k in ('pts3', 'idx', 'res', 'src', 'm', 'counts', 'stats', 'flags'):
        assert torch.equal(out[k], tri[k]), k
    assert torch.equal(out['cyl'][0], ref['cyl'][0]) and torch.equal(out['mean_err'], tri['stats'][:, 0])
    assert out['status'].tolist() == [fit.ST_OK, fit.ST_OVERFLOW] and int(out['m'][0]) == case['n_points']
    deg, mm = TC.axis_errors(out['cyl'][0, 1].cpu().numpy())
    print(f'fused fit on a frame with thirds missing: axis {deg:.4f} deg, {mm:.4f} mm off the true axis')
    b = TC.NOISY_TRI_BOUNDS[1]
    assert deg <= b['axis_deg'] and mm <= b['axis_mm']
