"""cpe_grid_predict_batch and cpe_grid_assign_batch (csrc/fit.hip k_grid_predict, k_grid_assign) against the numpy references of
tests/grid_predict_cases.py: points, pixels and distances at the tolerances derived there; states, visibility, counts, indices,
src, node_slot and the order exactly; equal bits over three calls; sentinels untouched from m on; every refusal with nothing
written; the Python layer against the C calls."""
import ctypes as C

import numpy as np
import pytest
import torch

import grid_predict_cases as G
import plane_fit_cases as PC
import table_tri_cases as TC

pytestmark = pytest.mark.gpu

SENTINEL_F, SENTINEL_I = -7.25, -77
PKEYS = ('X', 'px', 'state', 'vis', 'counts')
AKEYS = ('xy', 'id', 'src', 'dist', 'm', 'counts', 'stats', 'node_slot')


def _dv(gpu, a, dt=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dt).reshape(-1)).to(gpu)


def _ltable(cpe, gpu, t, family0='col', centre_status=0):
    centre = torch.from_numpy(np.concatenate([PC.rig()[5], [0.0]])).to(gpu)
    return cpe.fit.LaserTable(torch.from_numpy(t['P']).to(gpu), torch.from_numpy(t['status'].astype(np.int32)).to(gpu), t['lo'], t['hi'],
                              centre, torch.full((1,), centre_status, dtype=torch.int32, device=gpu), family0)


def _predict_raw(cpe, gpu, cyl, use, t, prm, N, radius=G.RADIUS):
    """the C call on sentinel-filled outputs -> rc, outputs"""
    K1, K2, T21 = PC.rig()[:3]
    n = len(cyl)
    d = dict(cyl=_dv(gpu, cyl), K1=_dv(gpu, K1), K2=_dv(gpu, K2), T21=_dv(gpu, T21), P=_dv(gpu, t['P']), st=_dv(gpu, t['status'], np.int32),
             centre=_dv(gpu, PC.rig()[5]))
    used = None if use is None else _dv(gpu, use, np.uint8)
    mk = lambda shape, dt, v: torch.full((max(n, 1),) + shape, v, dtype=dt, device=gpu)
    o = dict(X=mk((N, 3), torch.float64, SENTINEL_F), px=mk((2, N, 2), torch.float64, SENTINEL_F), state=mk((N,), torch.int32, SENTINEL_I),
             vis=mk((N,), torch.int32, SENTINEL_I), counts=mk((4,), torch.int32, SENTINEL_I))
    rc = cpe.lib.load().cpe_grid_predict_batch(d['cyl'].data_ptr() if n else None, None if used is None else used.data_ptr(), n, radius,
                                               d['K1'].data_ptr(), d['K2'].data_ptr(), d['T21'].data_ptr(), d['P'].data_ptr(),
                                               d['st'].data_ptr(), t['lo'], t['hi'], d['centre'].data_ptr(),
                                               None if prm is None else C.addressof(prm), *(o[k].data_ptr() for k in PKEYS),
                                               torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in o.items()}


def _params(cpe, a):
    I2 = C.c_int32 * 2
    return cpe.lib.CpeGridPredictParams(I2(*a['win_lo']), I2(*a['win_hi']), a['min_cos'], a['img_w'], a['img_h'])


def _untouched(o):
    return all((v == (SENTINEL_F if v.dtype == np.float64 else SENTINEL_I)).all() for v in o.values())


@pytest.mark.parametrize('name', list(G.predict_cases()))
def test_predict_cases(cpe, gpu, name):
    case = G.predict_cases()[name]
    a = G.predict_call_arrays(case)
    refs = G.predict_reference(name)
    N = refs[0]['Nu'] * refs[0]['Nv']
    runs = [_predict_raw(cpe, gpu, case['cyl'], case['use'], case['table'], _params(cpe, a), N) for _ in range(3)]
    assert all(rc == 0 for rc, _ in runs)
    got = runs[0][1]
    for k in PKEYS:
        assert got[k].tobytes() == runs[1][1][k].tobytes() == runs[2][1][k].tobytes(), f'{k}: three calls, other bits'
    worst_x = worst_p = 0.0
    for f, ref in enumerate(refs):
        G.compare_predict({k: got[k][f] for k in PKEYS}, ref, f'{name} frame {f}')
        worst_x, worst_p = max(worst_x, np.abs(got['X'][f] - ref['X']).max()), max(worst_p, np.abs(got['px'][f] - ref['px']).max())
    print(f'{name}: {len(refs)} frames x {N} nodes, X off by {worst_x:.2e} (tolerance >= {min(r["tol_X"][r["state"] == 0].min(initial=1) for r in refs):.2e}), '
          f'px by {worst_p:.2e}')
    # the Python layer makes the same call
    t = _ltable(cpe, gpu, case['table'])
    img = None if a['img_w'] <= 0 else (a['img_h'], a['img_w'])
    out = cpe.fit.grid_predict_batch(torch.from_numpy(case['cyl']).to(gpu), G.RADIUS, *PC.rig()[:3], t,
                                     use=None if case['use'] is None else torch.from_numpy(case['use']).to(gpu), window=case['window'],
                                     min_cos=a['min_cos'], image_size=img)
    for k in PKEYS:
        assert out[k].cpu().numpy().tobytes() == got[k].tobytes(), f'{k}: the Python layer differs from the C call'
    assert (out['Nu'], out['Nv']) == (refs[0]['Nu'], refs[0]['Nv'])


def test_predict_null_arguments_and_refusals(cpe, gpu):
    """NULL params = the whole table, min_cos 0.1, no bound; NULL use = every frame; n = 0 and every refusal write nothing"""
    case = G.predict_cases()['rig table, three poses']
    a = G.predict_call_arrays(case)
    N = (G.HI - G.LO + 1) ** 2
    rc, d = _predict_raw(cpe, gpu, case['cyl'], None, case['table'], None, N)
    rc2, e = _predict_raw(cpe, gpu, case['cyl'], np.ones(3, np.uint8), case['table'], _params(cpe, a), N)
    assert rc == 0 and rc2 == 0 and all(d[k].tobytes() == e[k].tobytes() for k in PKEYS)
    rc, o = _predict_raw(cpe, gpu, case['cyl'][:0], None, case['table'], None, N)
    assert rc == 0 and _untouched(o)
    for name, ((lo, hi), win, prm) in G.REFUSED_CALLS.items():
        t = TC.rig_table(lo, hi)
        p = dict(dict(min_cos=0.1, img_w=0, img_h=0), **prm)
        I2 = C.c_int32 * 2
        rc, o = _predict_raw(cpe, gpu, case['cyl'], None, t, cpe.lib.CpeGridPredictParams(I2(win[0][0], win[1][0]), I2(win[0][1], win[1][1]),
                                                                                         p['min_cos'], 0, 0), 16)
        assert rc == -1 and _untouched(o), name
    big = TC.rig_table(-120, 120)
    rc, o = _predict_raw(cpe, gpu, case['cyl'], None, big, None, 16)                         # NULL params on 241 x 241 nodes
    assert rc == -1 and _untouched(o)
    for radius in (0.0, -1.0, float('nan'), float('inf')):
        rc, o = _predict_raw(cpe, gpu, case['cyl'], None, case['table'], None, N, radius=radius)
        assert rc == -1 and _untouched(o)
    rc, o = _predict_raw(cpe, gpu, case['cyl'], None, dict(TC.rig_table(-128, 127), hi=128), None, 16)   # L = 257
    assert rc == -1 and _untouched(o)
    fit, K = cpe.fit, PC.rig()[:3]
    cyl = torch.from_numpy(case['cyl']).to(gpu)
    with pytest.raises(ValueError):
        fit.grid_predict_batch(cyl, G.RADIUS, *K, _ltable(cpe, gpu, big))                      # no window, more than 4096 nodes
    with pytest.raises(ValueError):
        fit.grid_predict_batch(cyl, G.RADIUS, *K, _ltable(cpe, gpu, case['table'], centre_status=5))
    with pytest.raises(ValueError):
        fit.grid_predict_batch(cyl, G.RADIUS, *K, _ltable(cpe, gpu, case['table']), window=((G.LO - 1, 0), (0, 0)))
    with pytest.raises(TypeError):
        fit.grid_predict_batch(cyl.float(), G.RADIUS, *K, _ltable(cpe, gpu, case['table']))
    assert fit.grid_predict_batch(cyl[:0], G.RADIUS, *K, _ltable(cpe, gpu, case['table']))['X'].shape == (0, N, 3)


# ------------------------------------------------------------------------------------------------------ assign
def _assign_raw(cpe, gpu, call, poison=None, prm=None, node_slot=True, alias=None, px_stride=None, cam_bit=None, Nu=None):
    """the C call on sentinel-filled outputs -> rc, outputs.  alias: the name of an output that is given the input xy instead"""
    xy, I, cnt = (torch.from_numpy(a).to(gpu) for a in TC.pack(call['frames'], poison))
    n, N = len(call['frames']), call['Nu'] * call['Nv']
    px, vis = _dv(gpu, call['px']), _dv(gpu, call['vis'], np.int32)
    mk = lambda shape, dt, v: torch.full((max(n, 1),) + shape, v, dtype=dt, device=gpu)
    o = dict(xy=mk((TC.MAXP, 2), torch.float64, SENTINEL_F), id=mk((TC.MAXP, 2), torch.int32, SENTINEL_I), src=mk((TC.MAXP,), torch.int32, SENTINEL_I),
             dist=mk((TC.MAXP,), torch.float64, SENTINEL_F), m=mk((), torch.int32, SENTINEL_I), counts=mk((8,), torch.int32, SENTINEL_I),
             stats=mk((2,), torch.float64, SENTINEL_F), node_slot=mk((N,), torch.int32, SENTINEL_I))
    ptr = {k: v.data_ptr() for k, v in o.items()}
    if not node_slot:
        ptr['node_slot'] = None
    if alias:
        ptr[alias] = xy.data_ptr()
    rc = cpe.lib.load().cpe_grid_assign_batch(xy.data_ptr(), I.data_ptr(), cnt.data_ptr(), n, px.data_ptr(), 2 * N if px_stride is None else px_stride,
                                              vis.data_ptr(), call['cam_bit'] if cam_bit is None else cam_bit, call['win_lo'][0], call['win_lo'][1],
                                              call['Nu'] if Nu is None else Nu, call['Nv'], None if prm is None else C.addressof(prm),
                                              *(ptr[k] for k in AKEYS), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in o.items()}


def _assign_params(cpe, params):
    p = dict(dict(tau_px=4.0, ratio=0.5, swap=0), **params)
    return cpe.lib.CpeGridAssignParams(p['tau_px'], p['ratio'], p['swap'], 0)


def _check_call(cpe, gpu, call, what):
    """poisoned and zero-filled inputs past the counts give the same bits, three calls the same bits, every image the reference,
    and nothing from m on is written"""
    prm = _assign_params(cpe, call['params'])
    rc, a = _assign_raw(cpe, gpu, call, poison=41, prm=prm)
    assert rc == 0
    for poison in (None, 41):
        rc, b = _assign_raw(cpe, gpu, call, poison=poison, prm=prm)
        assert rc == 0
        for k in AKEYS:
            assert a[k].tobytes() == b[k].tobytes(), f'{what}: {k} differs between calls (inputs past the count: {poison})'
    for i, ref in enumerate(G.assign_reference(call)):
        G.compare_assign({k: a[k][i] for k in AKEYS}, ref, f'{what} image {i}')
        m = ref['m']
        assert (a['xy'][i, m:] == SENTINEL_F).all() and (a['dist'][i, m:] == SENTINEL_F).all(), f'{what} image {i}: a slot from m on was written'
        assert (a['id'][i, m:] == SENTINEL_I).all() and (a['src'][i, m:] == SENTINEL_I).all(), f'{what} image {i}: a slot from m on was written'
    return a


def test_assign_batches_of_1_3_65_on_reference_pixels(cpe, gpu):
    """every batch is one call of one camera: 1 and 65 images of camera 1, 3 and 65 of camera 2"""
    px, vis = G.main_pixels()
    seen, sizes = set(), []
    for names in G.main_batches():
        calls = G.main_group_calls(names, px, vis)
        assert len(calls) == 1 and len(calls[0]['frames']) == len(names) == calls[0]['px'].shape[0]
        call = calls[0]
        _check_call(cpe, gpu, call, f'batch of {len(names)}, camera {call["cam_bit"] + 1}')
        seen |= set(call['names'])
        sizes.append((call['cam_bit'], len(call['frames'])))
    assert sizes == [(0, 1), (1, 3), (0, 65), (1, 65)] and seen == set(G.main_frames())


def test_python_layer_with_a_row_first_table(cpe, gpu):
    """family0='row': the table's family 0 holds the rows.  ids='col_row' tables then address it with swap 1, ids='row_col' tables
    (the planar detector's order) with swap 0; either way the kept points and their indices are those of the column-first table"""
    fit, K = cpe.fit, PC.rig()[:3]
    fr = G.main_frames()
    names = ['indices one off', 'camera 2, near pose', 'camera 2, far pose']
    cyl = torch.from_numpy(np.stack([G.POSES['near'], G.POSES['near'], G.POSES['far']])).to(gpu)
    t = TC.rig_table(G.LO, G.HI)
    xy, I, cnt = (torch.from_numpy(a).to(gpu) for a in TC.pack([fr[k] for k in names], 5))
    base = fit.grid_assign_batch(fit.GridTables(xy, I, cnt), fit.grid_predict_batch(cyl, G.RADIUS, *K, _ltable(cpe, gpu, t)), 2)
    pred = fit.grid_predict_batch(cyl, G.RADIUS, *K, _ltable(cpe, gpu, TC.transposed(t), family0='row'))
    assert pred['family0'] == 'row'
    a = fit.grid_assign_batch(fit.GridTables(xy, I, cnt), pred, 2, ids='col_row')
    b = fit.grid_assign_batch(fit.GridTables(xy, I.flip(2).contiguous(), cnt), pred, 2, ids='row_col')
    torch.cuda.synchronize()
    px, vis = pred['px'].cpu().numpy(), pred['vis'].cpu().numpy()
    for out, swap, ids in ((a, 1, I), (b, 0, I.flip(2))):
        got = dict(xy=out['tables'].xy, id=out['tables'].id, src=out['src'], dist=out['dist'], m=out['m'], counts=out['counts'], stats=out['stats'],
                   node_slot=out['node_slot'])
        got = {k: v.cpu().numpy() for k, v in got.items()}
        for i, k in enumerate(names):
            ref = G.ref_grid_assign(fr[k]['xy'], ids[i].cpu().numpy(), len(fr[k]['xy']), px[i, 1], vis[i], 1, (G.LO, G.LO), pred['Nu'], pred['Nv'], swap=swap)
            assert ref['margin'] > 1e-6 and ref['m'] > 200
            G.compare_assign({kk: got[kk][i] for kk in AKEYS}, ref, f'{k}, swap {swap}')
    assert torch.equal(a['m'], base['m']) and torch.equal(a['src'], base['src']) and torch.equal(a['counts'], base['counts'])
    assert torch.equal(a['tables'].id, base['tables'].id) and torch.equal(b['tables'].id, base['tables'].id.flip(2)) and torch.equal(b['src'], base['src'])
    assert int(base['counts'][0, 2]) > 50                  # the re-numbered points of 'indices one off'


@pytest.mark.parametrize('name', list(G.special_calls()))
def test_assign_calls_with_their_own_tables(cpe, gpu, name):
    call = G.special_calls()[name]
    a = _check_call(cpe, gpu, call, name)
    print(f'{name}: counts {a["counts"].tolist()}')


def test_assign_on_the_gpus_own_prediction(cpe, gpu):
    """predict on the GPU, assign through the Python layer, and the reference of the assignment on those very pixels"""
    fit, K = cpe.fit, PC.rig()[:3]
    fr = G.main_frames()
    poses = np.stack([G.predict_cases()['rig table, three poses']['cyl'][p] for p in range(3)])
    tab = _ltable(cpe, gpu, TC.rig_table(G.LO, G.HI))
    for cam in (0, 1):
        names = [k for k in fr if fr[k]['cam'] == cam]
        pred = fit.grid_predict_batch(torch.from_numpy(poses[[fr[k]['pose'] for k in names]]).to(gpu), G.RADIUS, *K, tab)
        gp = fit.GridTables(*(torch.from_numpy(x).to(gpu) for x in TC.pack([fr[k] for k in names], 13)))
        out = fit.grid_assign_batch(gp, pred, cam + 1)
        torch.cuda.synchronize()
        px, vis = pred['px'].cpu().numpy(), pred['vis'].cpu().numpy()
        call = dict(frames=[fr[k] for k in names], px=px[:, cam], vis=vis, cam_bit=cam, win_lo=(G.LO, G.LO), Nu=pred['Nu'], Nv=pred['Nv'], params={})
        got = dict(xy=out['tables'].xy, id=out['tables'].id, src=out['src'], dist=out['dist'], m=out['m'], counts=out['counts'],
                   stats=out['stats'], node_slot=out['node_slot'])
        got = {k: v.cpu().numpy() for k, v in got.items()}
        assert np.array_equal(got['m'], out['tables'].cnt.cpu().numpy())
        for i, ref in enumerate(G.assign_reference(call)):
            assert ref['margin'] > 1e-6
            G.compare_assign({k: got[k][i] for k in AKEYS}, ref, f'{names[i]} on the GPU prediction')
            assert not got['xy'][i, ref['m']:].any() and not got['src'][i, ref['m']:].any()      # the wrapper's zeros past m
        if cam == 0:       # the C call on the whole px with the stride of two cameras gives the layer's bits
            rc, raw = _assign_raw(cpe, gpu, dict(call, px=px), poison=13, px_stride=4 * pred['Nu'] * pred['Nv'])
            assert rc == 0 and all(np.array_equal(raw[k][i, :int(got['m'][i])], got[k][i, :int(got['m'][i])]) for k in ('id', 'src', 'dist')
                                   for i in range(len(names)))


def test_assign_null_arguments_and_refusals(cpe, gpu):
    call = G.special_calls()['mirrored ties']
    rc, a = _assign_raw(cpe, gpu, call, prm=None)
    rc2, b = _assign_raw(cpe, gpu, call, prm=_assign_params(cpe, {}), node_slot=False)
    assert rc == 0 and rc2 == 0
    for k in AKEYS[:-1]:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert (b['node_slot'] == SENTINEL_I).all() and (a['node_slot'] != SENTINEL_I).all()
    rc, o = _assign_raw(cpe, gpu, dict(call, frames=[], px=call['px'][:0], vis=call['vis'][:0]))
    assert rc == 0 and _untouched(o)
    P = cpe.lib.CpeGridAssignParams
    for bad in (P(0.0, 0.5, 0, 0), P(-1.0, 0.5, 0, 0), P(float('nan'), 0.5, 0, 0), P(float('inf'), 0.5, 0, 0), P(4.0, 0.0, 0, 0),
                P(4.0, 1.5, 0, 0), P(4.0, float('nan'), 0, 0), P(4.0, 0.5, 2, 0)):
        rc, o = _assign_raw(cpe, gpu, call, prm=bad)
        assert rc == -1 and _untouched(o)
    for kw in (dict(cam_bit=2), dict(cam_bit=-1), dict(px_stride=49), dict(Nu=0), dict(Nu=1000), dict(alias='xy'), dict(alias='dist')):
        rc, o = _assign_raw(cpe, gpu, call, **kw)
        assert rc == -1 and _untouched(o), kw
    fit, K = cpe.fit, PC.rig()[:3]
    pred = fit.grid_predict_batch(torch.from_numpy(G.POSES['true'][None]).to(gpu), G.RADIUS, *K, _ltable(cpe, gpu, TC.rig_table(G.LO, G.HI)))
    gp = fit.GridTables(*(torch.from_numpy(x).to(gpu) for x in TC.pack([G.main_frames()['count 65']])))
    for kw in (dict(cam=3), dict(cam=1, tau_px=0.0), dict(cam=1, ratio=1.5), dict(cam=1, ids='x')):
        with pytest.raises(ValueError):
            fit.grid_assign_batch(gp, pred, **kw)
    with pytest.raises(TypeError):
        fit.grid_assign_batch(fit.GridTables(gp.xy.float(), gp.id, gp.cnt), pred, 1)
    with pytest.raises(TypeError):
        fit.grid_assign_batch(fit.GridTables(gp.xy.repeat(2, 1, 1), gp.id.repeat(2, 1, 1), gp.cnt.repeat(2)), pred, 1)    # two images, one frame
