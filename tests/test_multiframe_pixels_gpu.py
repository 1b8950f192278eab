"""cpe_multi_frame_fit_pixels_batch (csrc/fit.hip k_multi_frame_pixels) against the numpy reference of
tests/multiframe_pixel_cases.py: counts, pt_state, n_used and status exactly; residuals, frame and group statistics at the returned
frame poses within the reference's own tolerances; the pose and F against scipy within the recorded bounds; frame_cyl against
T * TAGVcyl; N against the reference J'J; the iteration count; equal bits on a second call; groups permuted; every refusal with
nothing written."""
import numpy as np
import pytest
import torch

import multiframe_pixel_cases as M
import plane_fit_cases as PC

pytestmark = pytest.mark.gpu

SENTINEL_F, SENTINEL_I = -7.25, -77
GROUP_KEYS = ('x', 'T', 'fvals', 'iters', 'n_used', 'counts', 'stats', 'status', 'N')
FRAME_KEYS = ('pt_state', 'frame_cyl', 'frame_stats', 'res')
KEYS = GROUP_KEYS + FRAME_KEYS
EPS = M.EPS


def _dv(gpu, a, dt=np.float64):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dt).reshape(-1)).to(gpu)


def _inputs(gpu, case):
    a = M.call_arrays(case)
    K1, K2, T21 = PC.rig()[:3]
    t = case['table']
    d = {k: _dv(gpu, a[k], np.float64 if k.startswith('xy') else np.int32) for k in ('xy1', 'id1', 'cnt1', 'xy2', 'id2', 'cnt2')}
    d.update(TAGV=_dv(gpu, case['TAGV']), frame_ok=_dv(gpu, case['frame_ok'], np.int32), gs=_dv(gpu, case['group_start'], np.int32),
             x0=_dv(gpu, case['x0']), K1=_dv(gpu, K1), K2=_dv(gpu, K2), T21=_dv(gpu, T21), P=_dv(gpu, t['P']), st=_dv(gpu, t['status'], np.int32),
             centre=_dv(gpu, PC.rig()[5]), n=a['n'], G=len(case['group_start']) - 1)
    return d


def _raw(cpe, gpu, case, d=None, optional=True, alias=None, null=(), **over):
    """the C call on sentinel-filled outputs -> rc, outputs"""
    d = _inputs(gpu, case) if d is None else d
    n, G, t = d['n'], d['G'], case['table']
    F, I = torch.float64, torch.int32
    mk = lambda k, shape, dt: torch.full((max(k, 1),) + shape, SENTINEL_F if dt is F else SENTINEL_I, dtype=dt, device=gpu)
    o = dict(x=mk(G, (6,), F), T=mk(G, (16,), F), fvals=mk(G, (2,), F), iters=mk(G, (2,), I), n_used=mk(G, (), I), counts=mk(G, (4,), I),
             stats=mk(G, (4,), F), status=mk(G, (), I), N=mk(G, (21,), F), pt_state=mk(n, (2, M.MAXP), I), frame_cyl=mk(n, (6,), F),
             frame_stats=mk(n, (4,), F), res=mk(n, (2, M.MAXP, 2), F))
    p = lambda k: None if d[k] is None or k in null else d[k].data_ptr()
    op = {k: (None if k in null else v.data_ptr()) for k, v in o.items()}
    if not optional:
        op.update(N=None, res=None)
    if alias:
        op[alias[0]] = d[alias[1]].data_ptr()
    s = dict(radius=M.RADIUS, lo=t['lo'], hi=t['hi'], swap=case['swap'], min_cos=case['min_cos'], sel_cos=case['sel_cos'], gate_px=case['gate_px'],
             tol_x=1e-9, tol_f=1e-9, max_iter=100, n=n, G=G)
    s.update(over)
    rc = cpe.lib.load().cpe_multi_frame_fit_pixels_batch(
        p('xy1'), p('id1'), p('cnt1'), p('xy2'), p('id2'), p('cnt2'), p('TAGV'), p('frame_ok'), p('gs'), s['G'], s['n'], p('x0'), s['radius'],
        p('K1'), p('K2'), p('T21'), p('P'), p('st'), s['lo'], s['hi'], p('centre'), s['swap'], s['min_cos'], s['sel_cos'], s['gate_px'],
        s['tol_x'], s['tol_f'], s['max_iter'], *(op[k] for k in KEYS), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in o.items()}


def _sentinel(v):
    return v == (SENTINEL_F if v.dtype == np.float64 else SENTINEL_I)


def _untouched(o):
    return all(_sentinel(v).all() for v in o.values())


def _compare_group(got, g, ref, what):
    """-> (res off, pose off scipy, f / f_ls - 1, N off) of a fitted group, None otherwise"""
    assert int(got['status'][g]) == ref['status'], f'{what}: status {int(got["status"][g])} != {ref["status"]}'
    assert int(got['n_used'][g]) == ref['n_used'], f'{what}: n_used'
    assert np.array_equal(got['counts'][g], ref['counts']), f'{what}: counts {got["counts"][g]} != {ref["counts"]}'
    if ref['status'] != M.ST_OK:
        for k in GROUP_KEYS:
            if k != 'status':
                assert not got[k][g].any(), f'{what}: {k} of a group without a fit is not zero'
        for f in ref['kept']:
            for k in ('frame_cyl', 'frame_stats', 'res'):
                assert _sentinel(got[k][f]).all(), f'{what}: {k} of frame {f} was written'
        return None
    for k in GROUP_KEYS:
        assert np.isfinite(got[k][g]).all(), f'{what}: {k} is not finite'
    kept, grp = ref['kept'], ref['grp']
    T = got['T'][g].reshape(4, 4)
    assert np.abs(T - M.LM.vec2T(got['x'][g])).max() <= 8 * EPS, f'{what}: T is not vec2T(x)'   # (the device library's sin / cos)
    # frame_cyl against T * TAGVcyl of the returned T
    for i, f in enumerate(kept):
        want, tol = M.frame_cyl(T, grp.A[i]), M.frame_cyl_tol(T, grp.A[i])
        assert (np.abs(got['frame_cyl'][f] - want) <= tol).all(), f'{what}: frame_cyl of frame {f} off by {np.abs(got["frame_cyl"][f] - want).max():.2e}'
    # residuals and statistics: the reference at the frame poses the call returned
    ev = M.evaluate_at(ref, T, [got['frame_cyl'][f] for f in kept])
    assert ev['ok'], f'{what}: a member of S has no node at the returned pose'
    worst_r = 0.0
    sq, m1, m2, s1, s2, rmax = 0.0, 0, 0, 0.0, 0.0, 0.0
    for i, f in enumerate(kept):
        used = np.zeros((2, M.MAXP), bool)
        n1 = ref['n1'][i]
        st = ref['states'][i]
        used[0, :n1], used[1, :len(st) - n1] = st[:n1] == 0, st[n1:] == 0
        assert not got['res'][f][~used].any(), f'{what}: res of frame {f} outside S is not zero'
        er = np.abs(got['res'][f] - ev['res'][i]).max(2)
        assert (er <= ev['tol_res'][i]).all(), f'{what}: res of frame {f} off by {er.max():.3e}'
        worst_r = max(worst_r, float(er.max()))
        r2 = (got['res'][f] ** 2).sum(2)
        a, b = int(used[0].sum()), int(used[1].sum())
        rel = (2 * 2 * (a + b) + 18) * EPS
        want = np.array([np.sqrt(r2[0].sum() / a) if a else 0.0, np.sqrt(r2[1].sum() / b) if b else 0.0,
                         np.sqrt(r2.sum() / (a + b)) if a + b else 0.0, np.sqrt(r2.max())])
        assert (np.abs(got['frame_stats'][f] - want) <= rel * want).all(), f'{what}: frame_stats of frame {f} {got["frame_stats"][f]} != {want}'
        sq, m1, m2, s1, s2, rmax = sq + r2.sum(), m1 + a, m2 + b, s1 + r2[0].sum(), s2 + r2[1].sum(), max(rmax, float(np.sqrt(r2.max())))
    rel = (2 * 2 * (m1 + m2) + 18) * EPS
    want = np.array([np.sqrt(s1 / m1) if m1 else 0.0, np.sqrt(s2 / m2) if m2 else 0.0, np.sqrt(sq / (m1 + m2)), rmax])
    assert abs(got['fvals'][g, 1] - sq) <= rel * sq, f'{what}: fvals[1] {got["fvals"][g, 1]!r} != {sq!r}'
    assert (np.abs(got['stats'][g] - want) <= rel * want).all(), f'{what}: stats {got["stats"][g]} != {want}'
    # fvals[0]: the reference at the start, through the residuals' tolerances
    e0 = M.evaluate_at(ref, M.LM.vec2T(ref['grp_x0']))
    t0 = np.concatenate([t[t > 0] for t in e0['tol_res']])
    r0 = np.concatenate([np.abs(r).sum(2)[t > 0] for r, t in zip(e0['res'], e0['tol_res'])])
    assert abs(got['fvals'][g, 0] - ref['fvals'][0]) <= (2 * r0 * t0 + 2 * t0 * t0).sum() + rel * ref['fvals'][0], f'{what}: fvals[0]'
    assert got['fvals'][g, 1] <= got['fvals'][g, 0]
    it = got['iters'][g]
    assert 1 <= it[0] <= 3 * ref['iters'][0] and it[0] < it[1], f'{what}: iters {it}, reference {ref["iters"]}'
    # N against the reference J'J at the returned pose
    Nr = np.zeros((6, 6)); Nr[np.triu_indices(6)] = ev['N']
    Ng = np.zeros((6, 6)); Ng[np.triu_indices(6)] = got['N'][g]
    dg = np.sqrt(np.diag(Nr))
    dn = float((np.abs(Ng - Nr) / (dg[:, None] * dg[None, :]))[np.triu_indices(6)].max())
    assert dn <= M.PIXMF_N_BOUND, f'{what}: N off by {dn:.3e} of sqrt(N_aa N_bb), bound {M.PIXMF_N_BOUND:.3e}'
    dp = df = None
    if ref['nan_trials'] == 0:
        dp, df = M.pose_difference(T, ref['opt']['T']), got['fvals'][g, 1] / ref['opt']['f'] - 1
        assert dp <= M.PIXMF_POSE_BOUND, f'{what}: pose {dp:.3e} off scipy\'s optimum, bound {M.PIXMF_POSE_BOUND:.3e}'
        assert abs(df) <= M.PIXMF_F_BOUND, f'{what}: f / f_ls - 1 = {df:.3e}, bound {M.PIXMF_F_BOUND:.3e}'
    return worst_r, dp, df, dn


def _check_call(cpe, gpu, name, case, refs):
    d = _inputs(gpu, case)
    runs = [_raw(cpe, gpu, case, d) for _ in range(2)]
    assert all(rc == 0 for rc, _ in runs)
    got = runs[0][1]
    for k in KEYS:
        assert got[k].tobytes() == runs[1][1][k].tobytes(), f'{k}: a second call gave other bits'
    for k in GROUP_KEYS:
        assert not _sentinel(got[k]).any(), f'{k}: a slot was not written'
    assert np.array_equal(got['pt_state'][:d['n']], M.expected_pt_state(case, refs)), f'{name}: pt_state differs'
    worst = [0.0, 0.0, 0.0, 0.0]
    for g, ref in enumerate(refs):
        ref['grp_x0'] = case['x0'][g]
        out = _compare_group(got, g, ref, f'{name} group {g}')
        if out:
            worst = [max(w, abs(v)) if v is not None else w for w, v in zip(worst, out)]
    print(f'{name}: res off by {worst[0]:.2e} px; against scipy: pose {worst[1]:.2e}, f / f_ls - 1 {worst[2]:.2e}; N {worst[3]:.2e}; '
          f'iterations {got["iters"][:, 0].max()}')
    # the optional outputs NULL: the others keep their bits
    rc, b = _raw(cpe, gpu, case, d, optional=False)
    assert rc == 0 and all(b[k].tobytes() == got[k].tobytes() for k in KEYS if k not in ('N', 'res'))
    assert _sentinel(b['N']).all() and _sentinel(b['res']).all()
    return d, got


@pytest.mark.parametrize('name', list(M.cases()))
def test_cases(cpe, gpu, name):
    case = M.cases()[name]
    d, got = _check_call(cpe, gpu, name, case, M.reference(name))
    # the Python layer makes the same call
    v = lambda k, *s: None if d[k] is None else d[k].view(-1, *s)
    centre = torch.from_numpy(np.concatenate([PC.rig()[5], [0.0]])).to(gpu)
    t = case['table']
    tab = cpe.fit.LaserTable(torch.from_numpy(t['P']).to(gpu), torch.from_numpy(t['status'].astype(np.int32)).to(gpu), t['lo'], t['hi'], centre,
                             torch.zeros(1, dtype=torch.int32, device=gpu), 'row' if case['swap'] else 'col')
    out = cpe.multiframe.fit_multi_frame_pixels_gpu(v('xy1', M.MAXP, 2), v('id1', M.MAXP, 2), d['cnt1'], v('xy2', M.MAXP, 2), v('id2', M.MAXP, 2),
                                                    d['cnt2'], d['TAGV'].view(-1, 16), d['x0'].view(-1, 6), M.RADIUS, *PC.rig()[:3], tab,
                                                    frame_ok=d['frame_ok'], group_start=d['gs'], sel_cos=case['sel_cos'], min_cos=case['min_cos'],
                                                    gate_px=case['gate_px'], want_res=True)
    for k in GROUP_KEYS + ('pt_state',):
        assert out[k].cpu().numpy().tobytes() == got[k][:out[k].shape[0]].tobytes(), f'{k}: the Python layer differs from the C call'
    for g, ref in enumerate(M.reference(name)):
        cov = out['cov'][g].cpu().numpy()
        if ref['status'] != M.ST_OK:
            assert np.isnan(cov).all()
            continue
        Nf = np.zeros((6, 6)); Nf[np.triu_indices(6)] = got['N'][g]; Nf = Nf + np.triu(Nf, 1).T
        want = got['fvals'][g, 1] / (2 * got['counts'][g, :2].sum() - 6) * np.linalg.inv(Nf)
        assert np.allclose(cov, want, rtol=1e-6, atol=0) and np.allclose(cov, cov.T)
        for f in ref['kept']:
            assert out['frame_cyl'][f].cpu().numpy().tobytes() == got['frame_cyl'][f].tobytes()
            assert out['res'][f].cpu().numpy().tobytes() == got['res'][f].tobytes()
    others = sorted(set(range(d['n'])) - {f for r in M.reference(name) if r['status'] == M.ST_OK for f in r['kept']})
    assert torch.isnan(out['frame_cyl'][others]).all() and not out['res'][others].any()


def test_a_frame_at_the_capacity(cpe, gpu):
    _check_call(cpe, gpu, 'full tables', M.full_table_case(), M.reference('full tables'))


def test_a_group_does_not_depend_on_its_place_or_on_what_lies_past_the_counts(cpe, gpu):
    case = M.cases()['three groups']
    _, a = _raw(cpe, gpu, case)
    _, b = _raw(cpe, gpu, dict(case, poison=None))
    for k in KEYS:
        assert a[k].tobytes() == b[k].tobytes(), f'{k}: depends on the slots past the counts'
    gs = case['group_start']
    order = [3, 1, 0, 2]
    frames = np.concatenate([np.arange(gs[g], gs[g + 1]) for g in order]).astype(int)
    perm = dict(case, fr1=[case['fr1'][f] for f in frames], fr2=[case['fr2'][f] for f in frames], TAGV=case['TAGV'][frames],
                frame_ok=case['frame_ok'][frames], group_start=np.cumsum([0] + [gs[g + 1] - gs[g] for g in order]).astype(np.int32),
                x0=case['x0'][order], poison=5)
    _, c = _raw(cpe, gpu, perm)
    for k in GROUP_KEYS:
        assert a[k][:4][order].tobytes() == c[k][:4].tobytes(), f'{k}: depends on the group\'s place in the batch'
    for k in FRAME_KEYS:
        assert a[k][frames].tobytes() == c[k][:len(frames)].tobytes(), f'{k}: depends on the group\'s place in the batch'


def test_more_kept_frames_than_the_capacity(cpe, gpu):
    """CPE_MULTI_MAXF + 1 frames without detections, then a group that is fitted: OVERFLOW for the first alone"""
    base = M.cases()['two frames']
    nf = M.MAXF + 1
    empty = dict(xy=np.zeros((0, 2)), id=np.zeros((0, 2), np.int32))
    case = dict(base, fr1=[empty] * nf + base['fr1'], fr2=[empty] * nf + base['fr2'], TAGV=np.concatenate([np.tile(base['TAGV'][:1], (nf, 1, 1)), base['TAGV']]),
                group_start=np.array([0, nf, nf + 2], np.int32), x0=np.concatenate([base['x0'], base['x0']]), poison=None)
    rc, got = _raw(cpe, gpu, case)
    assert rc == 0 and got['status'][0] == M.ST_OVERFLOW and got['status'][1] == M.ST_OK
    for k in GROUP_KEYS:
        if k != 'status':
            assert not got[k][0].any(), f'{k} of the overflowing group is not zero'
    assert (got['pt_state'][:nf] == -1).all()
    _, alone = _raw(cpe, gpu, base)
    for k in GROUP_KEYS:
        assert got[k][1].tobytes() == alone[k][0].tobytes(), k
    # a range outside [0, n]: OVERFLOW, no frame touched
    rc, got = _raw(cpe, gpu, dict(base, group_start=np.array([0, 3], np.int32)))
    assert rc == 0 and got['status'][0] == M.ST_OVERFLOW and _sentinel(got['pt_state']).all()


def test_refusals_write_nothing(cpe, gpu):
    case = M.cases()['gate 4 px']
    d = _inputs(gpu, case)
    rc, good = _raw(cpe, gpu, case, d)
    assert rc == 0
    rc, o = _raw(cpe, gpu, case, d, G=0)
    assert rc == 0 and _untouched(o)
    nan, inf = float('nan'), float('inf')
    refused = [dict(radius=0.0), dict(radius=-1.0), dict(radius=nan), dict(radius=inf), dict(hi=case['table']['lo'] - 1), dict(lo=-128, hi=128),
               dict(min_cos=0.0), dict(min_cos=1.0), dict(min_cos=nan), dict(sel_cos=0.05), dict(sel_cos=1.0), dict(sel_cos=nan), dict(swap=2),
               dict(swap=-1), dict(tol_x=0.0), dict(tol_x=nan), dict(tol_f=0.0), dict(tol_f=-1e-9), dict(max_iter=0), dict(n=-1), dict(G=-1)]
    for kw in refused:
        rc, o = _raw(cpe, gpu, case, d, **kw)
        assert rc == -1 and _untouched(o), kw
    for null in (('xy1',), ('id2',), ('cnt1',), ('xy1', 'id1', 'cnt1', 'xy2', 'id2', 'cnt2'), ('TAGV',), ('gs',), ('x0',), ('K1',), ('K2',), ('T21',),
                 ('P',), ('st',), ('centre',), ('pt_state',), ('frame_cyl',), ('frame_stats',), ('x',), ('status',)):
        rc, o = _raw(cpe, gpu, case, d, null=null)
        assert rc == -1 and _untouched(o), null
    for alias in (('x', 'x0'), ('res', 'xy1'), ('pt_state', 'id1'), ('fvals', 'K1'), ('stats', 'P'), ('status', 'cnt2'), ('counts', 'st'),
                  ('iters', 'centre'), ('frame_cyl', 'TAGV'), ('n_used', 'gs')):
        rc, o = _raw(cpe, gpu, case, d, alias=alias)
        o.pop(alias[0])
        assert rc == -1 and _untouched(o), alias
    assert cpe.lib.load().cpe_last_error_string().decode().startswith('cpe_multi_frame_fit_pixels_batch')
    # sel_cos = min_cos is allowed; a NULL frame_ok keeps every frame
    rc, a = _raw(cpe, gpu, case, d, sel_cos=case['min_cos'])
    assert rc == 0 and a['status'][0] == M.ST_OK
    rc, a = _raw(cpe, gpu, dict(case, frame_ok=np.ones(3, np.int32)))
    assert rc == 0 and all(a[k].tobytes() == good[k].tobytes() for k in KEYS)


def test_python_layer_arguments(cpe, gpu):
    case = M.cases()['two frames']
    d = _inputs(gpu, case)
    t = case['table']
    centre = torch.from_numpy(np.concatenate([PC.rig()[5], [0.0]])).to(gpu)
    tab = lambda st=0: cpe.fit.LaserTable(torch.from_numpy(t['P']).to(gpu), torch.from_numpy(t['status'].astype(np.int32)).to(gpu), t['lo'], t['hi'],
                                          centre, torch.full((1,), st, dtype=torch.int32, device=gpu))
    tabs = [d['xy1'].view(-1, M.MAXP, 2), d['id1'].view(-1, M.MAXP, 2), d['cnt1'], d['xy2'].view(-1, M.MAXP, 2), d['id2'].view(-1, M.MAXP, 2), d['cnt2']]
    call = lambda tb=tabs, x0=case['x0'], table=None, **kw: cpe.multiframe.fit_multi_frame_pixels_gpu(
        *tb, torch.from_numpy(np.ascontiguousarray(case['TAGV'].reshape(-1, 16))), x0, M.RADIUS, *PC.rig()[:3], table or tab(), **kw)
    out = call()
    assert int(out['status'][0]) == 0 and out['res'] is None and out['cov'].shape == (1, 6, 6)
    for kw in (dict(min_cos=0.0), dict(sel_cos=0.05), dict(sel_cos=1.0), dict(tol_x=0.0), dict(max_iter=0)):
        with pytest.raises(ValueError):
            call(**kw)
    with pytest.raises(ValueError):
        call(x0=None)
    with pytest.raises(ValueError):
        call(tb=[None] * 6)
    with pytest.raises(ValueError):
        call(tb=tabs[:2] + [None] + tabs[3:])
    with pytest.raises(ValueError):
        call(table=tab(5))
    with pytest.raises(TypeError):
        call(tb=[tabs[0].float()] + tabs[1:])
