"""cpe_fit_cylinder_pixels_batch (csrc/fit.hip k_fit_cylinder_pixels) against the numpy reference of tests/pixel_fit_cases.py: counts,
pt_state and status exactly; residuals and points at the returned pose at the prediction's own tolerances; fvals and stats against
the sums of the call's residuals; the pose and f against scipy's optimum within the recorded bounds; equal bits over three calls;
sentinels overwritten everywhere; optional outputs NULL; every refusal with nothing written; the Python layer against the C call."""
import numpy as np
import pytest
import torch

import pixel_fit_cases as X
import plane_fit_cases as PC
import table_tri_cases as TC

pytestmark = pytest.mark.gpu

SENTINEL_F, SENTINEL_I = -7.25, -77
KEYS = ('cyl', 'fvals', 'iters', 'counts', 'stats', 'status', 'res', 'pt_state', 'X')
EPS = X.EPS


def _dv(gpu, a, dt=np.float64):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dt).reshape(-1)).to(gpu)


def _ltable(cpe, gpu, t, family0='col', centre_status=0):
    centre = torch.from_numpy(np.concatenate([PC.rig()[5], [0.0]])).to(gpu)
    return cpe.fit.LaserTable(torch.from_numpy(t['P']).to(gpu), torch.from_numpy(t['status'].astype(np.int32)).to(gpu), t['lo'], t['hi'],
                              centre, torch.full((1,), centre_status, dtype=torch.int32, device=gpu), family0)


def _inputs(gpu, case):
    a = X.call_arrays(case)
    K1, K2, T21 = PC.rig()[:3]
    t = case['table']
    d = {k: _dv(gpu, a[k], np.float64 if k.startswith('xy') else np.int32) for k in ('xy1', 'id1', 'cnt1', 'xy2', 'id2', 'cnt2')}
    d.update(cyl0=_dv(gpu, case['cyl0']), use=_dv(gpu, case['use'], np.uint8), K1=_dv(gpu, K1), K2=_dv(gpu, K2), T21=_dv(gpu, T21),
             P=_dv(gpu, t['P']), st=_dv(gpu, t['status'], np.int32), centre=_dv(gpu, PC.rig()[5]), n=a['n'])
    return d


def _raw(cpe, gpu, case, d=None, optional=True, alias=None, null=(), **over):
    """the C call on sentinel-filled outputs -> rc, outputs.  alias: (output, input) names: the output is given the input's address;
    null: inputs passed as NULL; over: scalar arguments other than the case's"""
    d = _inputs(gpu, case) if d is None else d
    n, t = d['n'], case['table']
    mk = lambda shape, dt, v: torch.full((max(n, 1),) + shape, v, dtype=dt, device=gpu)
    F, I = torch.float64, torch.int32
    o = dict(cyl=mk((6,), F, SENTINEL_F), fvals=mk((2,), F, SENTINEL_F), iters=mk((2,), I, SENTINEL_I), counts=mk((4,), I, SENTINEL_I),
             stats=mk((4,), F, SENTINEL_F), status=mk((), I, SENTINEL_I), res=mk((2, X.MAXP, 2), F, SENTINEL_F),
             pt_state=mk((2, X.MAXP), I, SENTINEL_I), X=mk((2, X.MAXP, 3), F, SENTINEL_F))
    p = lambda k: None if d[k] is None or k in null else d[k].data_ptr()
    op = {k: v.data_ptr() for k, v in o.items()}
    if not optional:
        op.update(res=None, pt_state=None, X=None)
    if alias:
        op[alias[0]] = d[alias[1]].data_ptr()
    s = dict(radius=X.RADIUS, lo=t['lo'], hi=t['hi'], swap=case['swap'], min_cos=case['min_cos'], gate_px=case['gate_px'], tol_x=1e-9, tol_f=1e-9,
             max_iter=100, n=n)
    s.update(over)
    rc = cpe.lib.load().cpe_fit_cylinder_pixels_batch(p('xy1'), p('id1'), p('cnt1'), p('xy2'), p('id2'), p('cnt2'), p('cyl0'), p('use'), s['n'],
                                                      s['radius'], p('K1'), p('K2'), p('T21'), p('P'), p('st'), s['lo'], s['hi'], p('centre'),
                                                      s['swap'], s['min_cos'], s['gate_px'], s['tol_x'], s['tol_f'], s['max_iter'],
                                                      *(op[k] for k in KEYS), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in o.items()}


def _untouched(o):
    return all((v == (SENTINEL_F if v.dtype == np.float64 else SENTINEL_I)).all() for v in o.values())


def _compare_frame(got, ref, cyl0, what):
    assert int(got['status']) == ref['status'], f'{what}: status {int(got["status"])} != {ref["status"]}'
    assert np.array_equal(got['counts'], ref['counts']), f'{what}: counts {got["counts"]} != {ref["counts"]}'
    assert np.array_equal(got['pt_state'], ref['pt_state']), f'{what}: pt_state differs'
    for k in KEYS:
        assert np.isfinite(got[k]).all(), f'{what}: {k} is not finite'
    if ref['status'] != X.ST_OK:
        for k in ('cyl', 'fvals', 'iters', 'stats', 'res', 'X'):
            assert not got[k].any(), f'{what}: {k} of a frame without a fit is not zero'
        return None
    ev = X.evaluate_at(ref, got['cyl'])
    assert ev['ok'], f'{what}: a member of S has no node at the returned pose'
    used = ref['pt_state'] == 0
    assert not got['res'][~used].any() and not got['X'][~used].any(), f'{what}: res or X outside S is not zero'
    er, ex = np.abs(got['res'] - ev['res']).max(2), np.abs(got['X'] - ev['X']).max(2)
    assert (er <= ev['tol_res']).all(), f'{what}: res off by {er.max():.3e}, tolerance {ev["tol_res"][used].min():.3e}'
    assert (ex <= ev['tol_X']).all(), f'{what}: X off by {ex.max():.3e}, tolerance {ev["tol_X"][used].min():.3e}'
    # fvals[1] and stats: the sums of the call's own residuals, m squares
    r2 = (got['res'] ** 2).sum(2)
    m = 2 * int(used.sum())
    rel = (2 * m + 18) * EPS
    n1, n2 = int(used[0].sum()), int(used[1].sum())
    want = np.array([np.sqrt(r2[0].sum() / n1) if n1 else 0.0, np.sqrt(r2[1].sum() / n2) if n2 else 0.0, np.sqrt(r2.sum() / (n1 + n2)),
                     np.sqrt(r2.max())])
    assert abs(got['fvals'][1] - r2.sum()) <= rel * r2.sum(), f'{what}: fvals[1] {got["fvals"][1]!r} != {r2.sum()!r}'
    assert (np.abs(got['stats'] - want) <= rel * want).all(), f'{what}: stats {got["stats"]} != {want}'
    # fvals[0]: the reference at the same start pose, through the residuals' tolerances
    e0 = X.evaluate_at(ref, cyl0)
    t0 = e0['tol_res'][used]
    r0 = np.abs(e0['res'][used]).sum(1)
    assert abs(got['fvals'][0] - ref['fvals'][0]) <= (2 * r0 * t0 + 2 * t0 * t0).sum() + rel * ref['fvals'][0], f'{what}: fvals[0]'
    assert got['fvals'][1] <= got['fvals'][0]
    assert 1 <= got['iters'][0] <= 3 * ref['iters'][0] and got['iters'][0] < got['iters'][1], f'{what}: iters {got["iters"]}, reference {ref["iters"]}'
    dp = df = None
    if ref['opt'] is not None and ref['nan_trials'] == 0:
        dp, df = X.against_scipy(got['cyl'], got['fvals'][1], ref['opt'], cyl0)
        assert abs(df) <= X.PIXFIT_F_BOUND, f'{what}: f / f_ls - 1 = {df:.3e}, bound {X.PIXFIT_F_BOUND:.3e}'
        if ref['opt']['well_posed']:
            assert dp <= X.PIXFIT_POSE_BOUND, f'{what}: gauge-fixed pose {dp:.3e} off scipy\'s optimum, bound {X.PIXFIT_POSE_BOUND:.3e}'
        else:
            dp = None
    return er.max(), ex.max(), dp, df


@pytest.mark.parametrize('name', list(X.cases()))
def test_cases(cpe, gpu, name):
    case = X.cases()[name]
    refs = X.reference(name)
    d = _inputs(gpu, case)
    runs = [_raw(cpe, gpu, case, d) for _ in range(3)]
    assert all(rc == 0 for rc, _ in runs)
    got = runs[0][1]
    for k in KEYS:
        assert got[k].tobytes() == runs[1][1][k].tobytes() == runs[2][1][k].tobytes(), f'{k}: three calls, other bits'
        assert not (got[k] == (SENTINEL_F if got[k].dtype == np.float64 else SENTINEL_I)).any(), f'{k}: a slot was not written'
    worst = [0.0, 0.0, 0.0, 0.0]
    for f, ref in enumerate(refs):
        out = _compare_frame({k: got[k][f] for k in KEYS}, ref, case['cyl0'][f], f'{name} frame {f}')
        if out:
            worst = [max(w, abs(v)) if v is not None else w for w, v in zip(worst, out)]
    print(f'{name}: {len(refs)} frames, res off by {worst[0]:.2e} px, X by {worst[1]:.2e} mm; against scipy: pose {worst[2]:.2e}, '
          f'f / f_ls - 1 {worst[3]:.2e}; iterations {got["iters"][:, 0].max()}')
    # the optional outputs NULL: the others keep their bits
    rc, b = _raw(cpe, gpu, case, d, optional=False)
    assert rc == 0 and all(b[k].tobytes() == got[k].tobytes() for k in KEYS[:6])
    assert all((b[k] == (SENTINEL_F if b[k].dtype == np.float64 else SENTINEL_I)).all() for k in KEYS[6:])
    # the Python layer makes the same call
    fit = cpe.fit
    tb = lambda c: None if d[f'xy{c}'] is None else fit.GridTables(d[f'xy{c}'].view(-1, X.MAXP, 2), d[f'id{c}'].view(-1, X.MAXP, 2), d[f'cnt{c}'])
    family0, ids = ('row', 'col_row') if case['swap'] else ('col', 'col_row')
    out = fit.fit_cylinder_pixels_batch(tb(1), tb(2), d['cyl0'].view(-1, 6), X.RADIUS, *PC.rig()[:3], _ltable(cpe, gpu, case['table'], family0),
                                        use=d['use'], gate_px=case['gate_px'], min_cos=case['min_cos'], ids=ids, want=('res', 'pt_state', 'X'))
    for k in KEYS:
        assert out[k].cpu().numpy().tobytes() == got[k].tobytes(), f'{k}: the Python layer differs from the C call'


def test_a_frame_does_not_depend_on_its_place_or_on_what_lies_past_the_counts(cpe, gpu):
    case = X.cases()['counts']
    _, a = _raw(cpe, gpu, case)
    _, b = _raw(cpe, gpu, dict(case, poison=None))
    order = np.arange(len(case['cyl0']))[::-1]
    rev = dict(case, fr1=[case['fr1'][i] for i in order], fr2=[case['fr2'][i] for i in order], cyl0=case['cyl0'][order], poison=5)
    _, c = _raw(cpe, gpu, rev)
    for k in KEYS:
        assert a[k].tobytes() == b[k].tobytes(), f'{k}: depends on the slots past the counts'
        assert a[k][order].tobytes() == c[k].tobytes(), f'{k}: depends on the frame\'s place in the batch'


def test_null_arguments_and_refusals(cpe, gpu):
    case = X.cases()['gate 4 px']
    d = _inputs(gpu, case)
    rc, good = _raw(cpe, gpu, case, d)
    assert rc == 0
    rc, a = _raw(cpe, gpu, case, d, null=('use',))                                    # NULL use = every frame
    rc2, b = _raw(cpe, gpu, dict(case, use=np.ones(2, np.uint8)))
    assert rc == 0 and rc2 == 0 and all(a[k].tobytes() == b[k].tobytes() == good[k].tobytes() for k in KEYS)
    for gate in (0.0, -1.0, float('nan')):                                            # <= 0 (or NaN): no gate
        rc, a = _raw(cpe, gpu, case, d, gate_px=gate)
        assert rc == 0 and not a['counts'][:, 3].any() and (a['counts'][:, :2].sum(1) == good['counts'][:, [0, 1, 3]].sum(1)).all()
    rc, o = _raw(cpe, gpu, case, d, n=0)
    assert rc == 0 and _untouched(o)
    nan, inf = float('nan'), float('inf')
    refused = [dict(radius=0.0), dict(radius=-1.0), dict(radius=nan), dict(radius=inf), dict(hi=case['table']['lo'] - 1),
               dict(lo=-128, hi=128), dict(min_cos=0.0), dict(min_cos=1.0), dict(min_cos=nan), dict(swap=2), dict(swap=-1), dict(tol_x=0.0),
               dict(tol_x=nan), dict(tol_f=0.0), dict(tol_f=-1e-9), dict(max_iter=0), dict(n=-1)]
    for kw in refused:
        rc, o = _raw(cpe, gpu, case, d, **kw)
        assert rc == -1 and _untouched(o), kw
    for null in (('xy1',), ('id2',), ('cnt1',), ('xy1', 'id1', 'cnt1', 'xy2', 'id2', 'cnt2'), ('cyl0',), ('K1',), ('K2',), ('T21',), ('P',),
                 ('st',), ('centre',)):
        rc, o = _raw(cpe, gpu, case, d, null=null)
        assert rc == -1 and _untouched(o), null
    for alias in (('cyl', 'cyl0'), ('res', 'xy1'), ('X', 'xy2'), ('pt_state', 'id1'), ('fvals', 'K1'), ('stats', 'P'), ('status', 'cnt2'),
                  ('counts', 'st'), ('iters', 'centre')):
        rc, o = _raw(cpe, gpu, case, d, alias=alias)
        o.pop(alias[0])
        assert rc == -1 and _untouched(o), alias
    assert cpe.lib.load().cpe_last_error_string().decode().startswith('cpe_fit_cylinder_pixels_batch')


def test_python_layer_arguments(cpe, gpu):
    fit, K = cpe.fit, PC.rig()[:3]
    case = X.cases()['one frame']
    d = _inputs(gpu, case)
    gp1 = fit.GridTables(d['xy1'].view(-1, X.MAXP, 2), d['id1'].view(-1, X.MAXP, 2), d['cnt1'])
    gp2 = fit.GridTables(d['xy2'].view(-1, X.MAXP, 2), d['id2'].view(-1, X.MAXP, 2), d['cnt2'])
    cyl0, tab = d['cyl0'].view(-1, 6), _ltable(cpe, gpu, case['table'])
    out = fit.fit_cylinder_pixels_batch(gp1, gp2, cyl0, X.RADIUS, *K, tab)
    assert out['res'] is not None and out['pt_state'] is None and out['X'] is None and int(out['status'][0]) == 0
    # a row-first table read through ids='row_col' tables is the same problem
    flip = lambda g: fit.GridTables(g.xy, g.id.flip(2).contiguous(), g.cnt)
    alt = fit.fit_cylinder_pixels_batch(flip(gp1), flip(gp2), cyl0, X.RADIUS, *K, tab, ids='row_col')
    assert torch.equal(alt['cyl'], out['cyl']) and torch.equal(alt['res'], out['res'])
    for kw in (dict(min_cos=0.0), dict(tol_x=0.0), dict(max_iter=0), dict(want=('res', 'nope')), dict(ids='x')):
        with pytest.raises(ValueError):
            fit.fit_cylinder_pixels_batch(gp1, gp2, cyl0, X.RADIUS, *K, tab, **kw)
    with pytest.raises(ValueError):
        fit.fit_cylinder_pixels_batch(None, None, cyl0, X.RADIUS, *K, tab)
    with pytest.raises(ValueError):
        fit.fit_cylinder_pixels_batch(gp1, gp2, cyl0, X.RADIUS, *K, _ltable(cpe, gpu, case['table'], centre_status=5))
    with pytest.raises(TypeError):
        fit.fit_cylinder_pixels_batch(gp1, gp2, cyl0.float(), X.RADIUS, *K, tab)
    with pytest.raises(TypeError):
        fit.fit_cylinder_pixels_batch(gp1, gp2, cyl0.repeat(2, 1), X.RADIUS, *K, tab)
    empty = fit.fit_cylinder_pixels_batch(fit.GridTables(gp1.xy[:0], gp1.id[:0], gp1.cnt[:0]), None, cyl0[:0], X.RADIUS, *K, tab)
    assert empty['cyl'].shape == (0, 6) and empty['res'].shape == (0, 2, X.MAXP, 2)
