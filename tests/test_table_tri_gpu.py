"""cpe_table_triangulate_batch (csrc/fit.hip k_table_triangulate) against the numpy reference of tests/table_tri_cases.py: points,
residuals and stats at the tolerances derived there; m, counts, idx, src and the order exactly."""
import ctypes as C

import numpy as np
import pytest
import torch

import plane_fit_cases as PC
import table_tri_cases as TC

pytestmark = pytest.mark.gpu

KEYS = ('pts3', 'idx', 'res', 'src', 'm', 'counts', 'stats')
SENTINEL_F, SENTINEL_I = -7.25, -77


def _table(cpe, gpu, t, family0='col'):
    return cpe.fit.LaserTable(torch.from_numpy(t['P']).to(gpu), torch.from_numpy(t['status'].astype(np.int32)).to(gpu), t['lo'], t['hi'],
                              torch.zeros(4, dtype=torch.float64, device=gpu), torch.zeros(1, dtype=torch.int32, device=gpu), family0)


def _tables(cpe, gpu, frames, poison=None):
    xy, I, cnt = (torch.from_numpy(a).to(gpu) for a in TC.pack(frames, poison))
    return cpe.fit.GridTables(xy, I, cnt)


def _tri(cpe, gpu, frames, table, cam=1, poison=None, family0='col', **kw):
    K, Tc = TC.camera(cam)
    out = cpe.fit.table_triangulate_batch(_tables(cpe, gpu, frames, poison), K, Tc, _table(cpe, gpu, table, family0), **kw)
    torch.cuda.synchronize()
    return {k: out[k].cpu().numpy() for k in KEYS}


def _frame(out, i):
    return {k: out[k][i] for k in KEYS}


def _report(name, g, ref):
    if ref['m']:
        m = ref['m']
        print(f'{name}: m {m}  X {np.abs(g["pts3"][:m] - ref["X"]).max():.2e} / {ref["tol_X"].min():.2e}  '
              f'res {np.abs(g["res"][:m] - ref["res"]).max():.2e} / {ref["tol_res"][ref["tol_res"] > 0].min():.2e}')


@pytest.mark.parametrize('need_both', [0, 1])
def test_batches_of_1_3_65(cpe, gpu, need_both):
    seen = set()
    for names, frames in TC.batches():
        a = _tri(cpe, gpu, frames, TC.main_table(), poison=41, need_both=need_both)      # NaN, infinities, garbage indices past every count
        b = _tri(cpe, gpu, frames, TC.main_table(), need_both=need_both)                 # zeros there
        for k in KEYS:
            assert a[k].tobytes() == b[k].tobytes(), f'{k} depends on slots past the count'
        for i, name in enumerate(names):
            ref = TC.frame_reference(name, need_both)
            g = _frame(a, i)
            if name not in seen:
                _report(name, g, ref)
            TC.compare_frame(g, ref, f'{name} (frame {i} of {len(names)}, need_both {need_both})')
            assert not g['pts3'][ref['m']:].any() and not g['src'][ref['m']:].any()      # the wrapper's zeros past m
            seen.add(name)
    assert seen == set(TC.frame_cases())


@pytest.mark.parametrize('name', list(TC.call_cases()))
def test_calls_with_their_own_table_and_parameters(cpe, gpu, name):
    case = TC.call_cases()[name]
    got = _tri(cpe, gpu, case['frames'], case['table'], case['cam'], poison=9, **case['params'])
    for i, ref in enumerate(TC.call_reference(name)):
        _report(f'{name} [{i}]', _frame(got, i), ref)
        TC.compare_frame(_frame(got, i), ref, f'{name} frame {i}')


def test_family0_names_the_swap(cpe, gpu):
    """the same planes with the families exchanged and family0='row' said so: the same bits; unsaid: other points"""
    frames = [TC.frame_cases()[k] for k in ('count 129', 'one component out of range', 'count 2048')]
    a = _tri(cpe, gpu, frames, TC.main_table())
    b = _tri(cpe, gpu, frames, TC.transposed(TC.main_table()), family0='row')
    for k in KEYS:
        assert a[k].tobytes() == b[k].tobytes(), k
    c = _tri(cpe, gpu, frames, TC.transposed(TC.main_table()))
    assert c['stats'][0, 1] > 1.0 > a['stats'][0, 1]
    # tables whose id is (row, col), as the planar detector writes them: the components exchanged, the same points
    sw = [dict(f, id=np.ascontiguousarray(f['id'][:, ::-1])) for f in frames]
    K, Tc = TC.camera(1)
    d = cpe.fit.table_triangulate_batch(_tables(cpe, gpu, sw), K, Tc, _table(cpe, gpu, TC.main_table()), ids='row_col')
    torch.cuda.synchronize()
    assert d['pts3'].cpu().numpy().tobytes() == a['pts3'].tobytes() and np.array_equal(d['m'].cpu().numpy(), a['m'])
    assert np.array_equal(d['idx'].cpu().numpy()[..., ::-1], a['idx']) and np.array_equal(d['res'].cpu().numpy()[..., ::-1], a['res'])


def _raw(cpe, gpu, gp, K, Tc, t, prm, lo=None, hi=None):
    """the C entry with every output pre-filled with a sentinel -> rc, dict of numpy outputs"""
    n = gp.cnt.shape[0]
    f = lambda *s: torch.full(s, SENTINEL_F, dtype=torch.float64, device=gpu)
    i = lambda *s: torch.full(s, SENTINEL_I, dtype=torch.int32, device=gpu)
    o = dict(pts3=f(n, TC.MAXP, 3), idx=i(n, TC.MAXP, 2), res=f(n, TC.MAXP, 2), src=i(n, TC.MAXP, 2), m=i(n), counts=i(n, 4), stats=f(n, 2))
    Kd = torch.as_tensor(np.asarray(K, np.float64).reshape(9)).to(gpu)
    Td = None if Tc is None else torch.as_tensor(np.asarray(Tc, np.float64).reshape(16)).to(gpu)
    P, st = torch.from_numpy(t['P']).to(gpu), torch.from_numpy(t['status'].astype(np.int32)).to(gpu)
    rc = cpe.lib.load().cpe_table_triangulate_batch(gp.xy.data_ptr(), gp.id.data_ptr(), gp.cnt.data_ptr(), n, Kd.data_ptr(),
                                                    None if Td is None else Td.data_ptr(), P.data_ptr(), st.data_ptr(),
                                                    t['lo'] if lo is None else lo, t['hi'] if hi is None else hi,
                                                    None if prm is None else C.addressof(prm), *(o[k].data_ptr() for k in KEYS),
                                                    torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in o.items()}


def test_null_params_null_pose_and_untouched_slots(cpe, gpu):
    """NULL params are the defaults, a NULL pose is the identity bit for bit, and slots from m on keep what they held"""
    frames = [TC.frame_cases()[k] for k in ('refused across rounds', 'all refused', 'count 65', 'nan pixels', 'count 0')]
    gp = _tables(cpe, gpu, frames, poison=3)
    K = PC.rig()[0]
    t = TC.main_table()
    rc, a = _raw(cpe, gpu, gp, K, None, t, None)
    assert rc == 0
    rc, b = _raw(cpe, gpu, gp, K, np.eye(4), t, cpe.lib.CpeTableTriParams(0, 0, 0.01, 0.0))
    assert rc == 0
    for k in KEYS:
        assert a[k].tobytes() == b[k].tobytes(), k
    want = _tri(cpe, gpu, frames, t, poison=3)
    for i, fr in enumerate(frames):
        m = int(a['m'][i])
        assert m == want['m'][i] and np.array_equal(a['counts'][i], want['counts'][i]) and a['stats'][i].tobytes() == want['stats'][i].tobytes()
        for k in ('pts3', 'idx', 'res', 'src'):
            assert a[k][i, :m].tobytes() == want[k][i, :m].tobytes(), k
        assert (a['pts3'][i, m:] == SENTINEL_F).all() and (a['res'][i, m:] == SENTINEL_F).all()
        assert (a['idx'][i, m:] == SENTINEL_I).all() and (a['src'][i, m:] == SENTINEL_I).all()
    assert a['m'].tolist() == [190, 0, want['m'][2], want['m'][3], 0] and not a['stats'][1].any() and not a['stats'][4].any()


def test_bad_arguments_are_refused(cpe, gpu):
    gp = _tables(cpe, gpu, [TC.frame_cases()['count 65']])
    K = PC.rig()[0]
    big = dict(P=np.zeros((2, 257, 4)), status=np.zeros((2, 257), np.int32), lo=-128, hi=128)
    assert _raw(cpe, gpu, gp, K, None, big, None)[0] == -1                                  # L = 257
    t = TC.main_table()
    assert _raw(cpe, gpu, gp, K, None, t, None, lo=3, hi=2)[0] == -1 and _raw(cpe, gpu, gp, K, None, t, None, lo=-2 ** 31, hi=2 ** 31 - 1)[0] == -1
    P = cpe.lib.CpeTableTriParams
    for bad in (P(2, 0, 0.01, 0.0), P(0, -1, 0.01, 0.0), P(0, 0, -0.5, 0.0), P(0, 0, float('nan'), 0.0), P(0, 0, 0.01, float('nan'))):
        rc, o = _raw(cpe, gpu, gp, K, None, t, bad)
        assert rc == -1 and (o['m'] == SENTINEL_I).all()
    assert _raw(cpe, gpu, gp, K, None, TC.rig_table(-128, 127), None)[0] == 0               # L = 256
    with pytest.raises(ValueError):
        _table(cpe, gpu, big)
    with pytest.raises(TypeError):
        cpe.fit.table_triangulate_batch(cpe.fit.GridTables(gp.xy.float(), gp.id, gp.cnt), K, None, _table(cpe, gpu, t))
    z = cpe.fit.GridTables(gp.xy[:0], gp.id[:0], gp.cnt[:0])
    assert cpe.fit.table_triangulate_batch(z, K, None, _table(cpe, gpu, t))['pts3'].shape == (0, TC.MAXP, 3)


@pytest.mark.parametrize('ransac', [None, dict(hypotheses=16, sample=12, tau=0.5, seed=3)], ids=['fit', 'ransac'])
def test_mono_fit_equals_its_layers(cpe, gpu, ransac):
    idx, _, uv1, uv2 = TC.cylinder_frame()
    K2, T21 = TC.camera(2)
    frames = [dict(xy=uv2, id=idx), dict(xy=uv2[:3], id=idx[:3]), dict(xy=uv2[::4], id=idx[::4])]
    gp, tab = _tables(cpe, gpu, frames, poison=1), _table(cpe, gpu, TC.noisy_table(0))
    kw = dict(need_both=True, max_res=0.4)
    out = cpe.fit.fit_single_cylinder_mono_batch(gp, K2, T21, tab, TC.RADIUS, ransac=ransac, mode=cpe.fit.FIT_LM, **kw)
    tri = cpe.fit.table_triangulate_batch(gp, K2, T21, tab, **kw)
    if ransac is None:
        fit = cpe.fit.fit_cylinder_batch(tri['pts3'], tri['m'], TC.RADIUS, mode=cpe.fit.FIT_LM)
    else:
        fit = cpe.fit.fit_cylinder_ransac_batch(tri['pts3'], tri['m'], TC.RADIUS, mode=cpe.fit.FIT_LM, **ransac)
    torch.cuda.synchronize()
    for k in KEYS:
        assert out[k].cpu().numpy().tobytes() == tri[k].cpu().numpy().tobytes(), k
    for k in fit:
        assert out[k].cpu().numpy().tobytes() == fit[k].cpu().numpy().tobytes(), k
    assert torch.equal(out['mean_err'], tri['stats'][:, 0]) and out['status'].tolist() == [0, 5, 0] and out['m'].tolist()[1] == 3
    assert set(out) == set(tri) | set(fit) | {'mean_err'}


@pytest.mark.parametrize('cam', [1, 2])
def test_noisy_table_and_pixels_against_truth(cpe, gpu, cam):
    """the 12-pose noisy tables and 0.25 px pixels of the five seeds in one batch: points and fitted axis within the bounds
    measured on the reference (tests/table_tri_cases.py), and the points equal to the reference's at the derived tolerances"""
    K, Tc = TC.camera(cam)
    worst = dict(mean_mm=0.0, worst_mm=0.0, axis_deg=0.0, axis_mm=0.0)
    for seed in TC.NOISY_SEEDS:
        case = TC.noisy_case(seed, cam)
        out = cpe.fit.fit_single_cylinder_mono_batch(_tables(cpe, gpu, [case['frame']]), K, Tc, _table(cpe, gpu, case['table']), TC.RADIUS,
                                                     mode=cpe.fit.FIT_LM)
        torch.cuda.synchronize()
        TC.compare_frame({k: out[k][0].cpu().numpy() for k in KEYS}, case['ref'], f'seed {seed}')
        m = int(out['m'][0])
        assert int(out['status'][0]) == 0 and m >= 400
        e = TC.noisy_errors(out['pts3'][0, :m].cpu().numpy(), case['Xtrue'], out['cyl_raw'][0, 1].cpu().numpy())
        worst = {k: max(worst[k], e[k]) for k in worst}
    print(f'camera {cam}: ' + '  '.join(f'{k} {v:.4f} / {TC.NOISY_TRI_BOUNDS[cam][k]:.4f}' for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= TC.NOISY_TRI_BOUNDS[cam][k], (k, v)
