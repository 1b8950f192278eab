"""cpe_fit_projector_model and cpe_projector_model_table (csrc/fit.hip k_pm_moments, k_pm_solve, k_pm_finish, k_pm_table) against
the numpy / scipy reference of tests/proj_model_cases.py, which works on the points where the kernels work on moments.

At the case's tolerance (derived there): the model against the reference's optimum, and the reference's own Gauss-Newton step
at the returned model, a stationarity check that does not lean on scipy's path.  Moments: N exactly; the centroid to 64 eps |X|;
the scatter to 64 N eps |X|^2 (centred sums of N terms); the line rms to 2 tol (every residual moves by at most |dC| + |X| dn).
Exactly: masks, counts, frames, frame_counts and info's status, refits, kept residuals and flags.  The LM's iteration and
evaluation counts (info[2], info[3]) depend on the solver's path, which the reference does not share: they are checked to be
positive and to repeat."""
import ctypes as C

import numpy as np
import pytest
import torch

import plane_fit_cases as PC
import proj_model_cases as M
import table_tri_cases as TC

pytestmark = pytest.mark.gpu

KEYS = ('model', 'info', 'moments', 'count', 'frames', 'inlier_mask', 'frame_counts')


def _call(cpe, gpu, case, poison=None):
    X, I, cnt, use, ok = M.arrays(case, poison)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    out = cpe.fit.fit_projector_model(t(X), t(I), t(cnt), case['lo'], case['hi'], use=t(use), frame_ok=t(ok), x0=case.get('x0'),
                                      **M.params(case))
    torch.cuda.synchronize()
    return out, {k: out[k].cpu().numpy() for k in KEYS}


def _compare(name, g, ref):
    L = ref['count'].shape[1]
    info = g['info']
    print(f'{name}: info {info.tolist()}')
    assert info[0] == ref['status'] and info[1] == ref['rounds'], f'{name}: status, refits {info[:2]} != {ref["status"]}, {ref["rounds"]}'
    assert info[4] == ref['kept'][0] and info[5] == ref['kept'][1] and info[6] == 0 and info[7] == 0, f'{name}: info {info}'
    for k, r in (('inlier_mask', 'mask'), ('count', 'count'), ('frames', 'frames'), ('frame_counts', 'frame_counts')):
        assert np.array_equal(g[k], ref[r]), f'{name}: {k} differs'
    assert np.isfinite(g['model']).all() and np.isfinite(g['moments']).all()
    mom, rm = g['moments'], ref['moments']
    assert np.array_equal(mom[..., 0], rm[..., 0]) and not mom[..., 11].any()
    xmax = max((float(np.linalg.norm(ref['R'].P[k], axis=1).max()) for k in range(2) if len(ref['R'].P[k])), default=0.0)
    assert np.abs(mom[..., 1:4] - rm[..., 1:4]).max() <= 64 * M.EPS * xmax, f'{name}: centroids'
    assert (np.abs(mom[..., 4:10] - rm[..., 4:10]).max(-1) <= 64 * np.maximum(rm[..., 0], 1) * M.EPS * xmax ** 2).all(), f'{name}: scatter'
    if ref['status'] != M.ST_OK:
        assert not g['model'].any() and not mom[..., 10].any(), f'{name}: a failed fit has a model'
        assert info[2] == 0 and info[3] == 0
        return
    assert info[2] > 0 and info[3] > info[2], f'{name}: LM counts {info[2:4]}'
    x, tol = g['model'][:15], ref['tol']
    f = float((ref['R'].res(x, ref['keep']) ** 2).sum())
    assert abs(g['model'][15] - f) <= 1e-9 * (1 + f), f'{name}: the objective from moments {g["model"][15]} is not the points\' {f}'
    assert abs(g['model'][15] - ref['f']) <= 1e-9 * (1 + ref['f']), f'{name}: objective {g["model"][15]} != {ref["f"]}'
    for k in range(2):
        assert abs(np.linalg.norm(x[3 + 6 * k:6 + 6 * k]) - 1) <= 64 * M.EPS, f'{name}: a_{k} not unit'
    if name in M.GAUGE:
        return
    step, _ = M.gn_step(ref['R'], ref['keep'], x)
    print(f'{name}: |x - ref| {np.abs(x - ref["x"]).max():.2e}  |gn step| {np.abs(step).max():.2e}  tol {tol:.2e}')
    assert np.abs(x - ref['x']).max() <= tol, f'{name}: model {np.abs(x - ref["x"]).max():.3e} > {tol:.3e}'
    assert np.abs(step).max() <= tol, f'{name}: not stationary, Gauss-Newton step {np.abs(step).max():.3e} > {tol:.3e}'
    assert np.abs(mom[..., 10] - rm[..., 10]).max() <= 2 * tol, f'{name}: line rms'


@pytest.mark.parametrize('name', list(M.cases()))
def test_case(cpe, gpu, name):
    """batches of 0, 1, 2, 3, 4, 6, 10, 12 and 65 frames; counts -1 .. 3000; NaN / Inf; use; frame_ok; L 2, 5, 11, 25, 56, 256; the
    FEW_POINTS endings; max_rounds 0 / 1 / 4; x0.  Poison past every count changes no bit, and a second call repeats every bit"""
    case = M.cases()[name]
    _, a = _call(cpe, gpu, case, poison=41)
    _, b = _call(cpe, gpu, case)
    for k in KEYS:
        assert a[k].tobytes() == b[k].tobytes(), f'{name}: {k} depends on slots past the count, or does not repeat'
    _compare(name, a, M.reference(name))


def test_one_frame_and_repeat(cpe, gpu):
    """a batch of 1 is the 'one pose' case; here two more calls of the trimmed case on the same tensors: equal bits"""
    case = M.cases()['shifted']
    outs = [_call(cpe, gpu, case)[1] for _ in range(3)]
    for o in outs[1:]:
        for k in KEYS:
            assert o[k].tobytes() == outs[0][k].tobytes(), f'{k} does not repeat'
    ref = M.reference('shifted')
    trimmed = outs[0]['frame_counts'][:, 1]
    assert np.array_equal(np.nonzero(trimmed)[0], M.SHIFTED) and (trimmed[list(M.SHIFTED)] == 225).all()
    assert not outs[0]['frame_counts'][:, 3].any() and ref['rounds'] == 2


def test_L_257_is_refused(cpe, gpu):
    X, I, cnt, _, _ = M.arrays(M.cases()['boards 3'])
    X, I, cnt = (torch.from_numpy(a).to(gpu) for a in (X, I, cnt))
    with pytest.raises(ValueError):
        cpe.fit.fit_projector_model(X, I, cnt, 0, 256)
    L = cpe.lib.load()
    o = torch.zeros(64, dtype=torch.float64, device=gpu)
    rc = L.cpe_fit_projector_model(X.data_ptr(), I.data_ptr(), cnt.data_ptr(), 3, None, None, 0, 256, None, None, o.data_ptr(),
                                   o.data_ptr(), o.data_ptr(), o.data_ptr(), o.data_ptr(), o.data_ptr(), o.data_ptr(), None)
    assert rc == -1
    assert L.cpe_projector_model_table(o.data_ptr(), o.data_ptr(), 0, 256, o.data_ptr(), o.data_ptr(), o.data_ptr(), o.data_ptr(),
                                       None) == -1
    torch.cuda.synchronize()
    assert not o.cpu().numpy().any()


@pytest.mark.parametrize('name', ['cylinder 12', 'one pose'])
def test_table(cpe, gpu, name):
    """the table of a model: the planes follow the model and the sign rule; the columns -12..-1 that no cylinder frame showed lie
    within the noisy bound of true_line_planes; a failed model gives a refused table; and the table drives
    table_triangulate_batch as ref_table_triangulate says"""
    out, g = _call(cpe, gpu, M.cases()[name])
    pm = cpe.fit.ProjectorModel.from_fit(out)
    tab = pm.table(-12, 12)
    torch.cuda.synchronize()
    P, st, ctr = tab.P.cpu().numpy(), tab.status.cpu().numpy(), tab.centre.cpu().numpy()
    if name == 'one pose':
        assert (st == M.ST_FEW_POINTS).all() and not P.any() and not ctr.any() and int(tab.centre_status[0]) == M.ST_FEW_POINTS
        assert pm.status == M.ST_FEW_POINTS and pm.rms == 0.0
        return
    x = g['model'][:15]
    assert (st == M.ST_OK).all() and int(tab.centre_status[0]) == M.ST_OK
    kept = int(g['info'][4] + g['info'][5])
    assert np.array_equal(ctr[:3], x[:3]) and abs(ctr[3] - np.sqrt(g['model'][15] / kept)) <= 64 * M.EPS and abs(pm.rms - ctr[3]) <= 64 * M.EPS
    tl, bound = PC.true_line_planes(-12, 12), M.NOISY_BOUNDS['cyl']
    for k in range(2):
        nh, _ = M.normals(x, k, np.arange(-12, 13))
        for j in range(25):
            want = PC._orient_big(nh[j])
            assert np.abs(P[k, j, :3] - want).max() <= 64 * M.EPS and abs(P[k, j, 3] + want @ x[:3]) <= 64 * M.EPS * 400
            a = np.degrees(PC.angle(P[k, j, :3], tl[k, j]))
            assert min(a, 180 - a) <= bound['normal_deg'], f'family {k} line {j - 12}: {min(a, 180 - a):.4f} deg'
            assert abs(P[k, j, :3] @ PC.rig()[5] + P[k, j, 3]) <= bound['offset_mm']
    # any range, also one the fit never saw
    far = pm.table(100, 355)
    assert tuple(far.P.shape) == (2, 256, 4) and bool((far.status == 0).all())
    # the table in use
    idx, Xt, uv1, uv2 = TC.cylinder_frame(0.25, 0)
    xy, ids, cnt = TC.pack([dict(xy=uv1, id=idx)])
    gp = cpe.fit.GridTables(*(torch.from_numpy(a).to(gpu) for a in (xy, ids, cnt)))
    K, Tc = TC.camera(1)
    tri = cpe.fit.table_triangulate_batch(gp, K, Tc, tab)
    torch.cuda.synchronize()
    ref = TC.ref_table_triangulate(uv1, idx, len(idx), K, Tc, P, st, -12, 12)
    got = {k: tri[k][0].cpu().numpy() for k in ('pts3', 'idx', 'res', 'src', 'm', 'counts', 'stats')}
    TC.compare_frame(got, ref, 'model table')
    assert ref['m'] == len(idx)
    assert np.linalg.norm(got['pts3'][:ref['m']] - Xt, axis=1).mean() <= TC.NOISY_TRI_BOUNDS[1]['mean_mm']


def test_save_load(cpe, gpu, tmp_path):
    out, g = _call(cpe, gpu, M.cases()['boards 3'])
    pm = cpe.fit.ProjectorModel.from_fit(out, family0='row')
    pm.save(tmp_path / 'pm')
    back = cpe.fit.ProjectorModel.load(tmp_path / 'pm.npz', gpu)
    assert back.family0 == 'row' and torch.equal(back.model, pm.model) and torch.equal(back.info, pm.info)
    a, b = pm.table(-3, 3), back.table(-3, 3)
    assert torch.equal(a.P, b.P) and a.family0 == 'row'
    assert torch.equal(pm.C, pm.model[:3]) and torch.equal(pm.a[1], pm.model[9:12]) and torch.equal(pm.b[0], pm.model[6:9])
