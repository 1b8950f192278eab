"""cpe_multi_frame_fit_pixels_angles_batch (csrc/fit.hip k_multi_frame_pixels_angles) against the numpy reference of
tests/multiframe_joint_cases.py: counts, pt_state, n_used and status exactly; residuals and statistics at the returned frame poses
within the reference's own tolerances; the pose, the angles and F against scipy within twice the recorded bounds; N and frame_N
against the reference's blocks at the returned point; a memberless frame keeps the bits of its nominal angles; the capacity and one
frame more; equal bits on a second call; groups permuted; every refusal with nothing written."""
import numpy as np
import pytest
import torch

import multiframe_joint_cases as J
import multiframe_pixel_cases as M
import plane_fit_cases as PC

pytestmark = pytest.mark.gpu

SENTINEL_F, SENTINEL_I = -7.25, -77
GROUP_KEYS = ('x', 'T', 'fvals', 'iters', 'n_used', 'counts', 'stats', 'status', 'N')
FRAME_KEYS = ('pt_state', 'frame_cyl', 'frame_stats', 'res', 'angles', 'frame_N')
KEYS = GROUP_KEYS + FRAME_KEYS
EPS = J.EPS


def _dv(gpu, a, dt=np.float64):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dt).reshape(-1)).to(gpu)


def _inputs(gpu, case):
    a = J.call_arrays(case)
    K1, K2, T21 = PC.rig()[:3]
    t = case['table']
    d = {k: _dv(gpu, a[k], np.float64 if k.startswith('xy') else np.int32) for k in ('xy1', 'id1', 'cnt1', 'xy2', 'id2', 'cnt2')}
    d.update(angles0=_dv(gpu, case['angles']), frame_ok=_dv(gpu, case['frame_ok'], np.int32), gs=_dv(gpu, case['group_start'], np.int32),
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
             stats=mk(G, (4,), F), status=mk(G, (), I), N=mk(G, (21,), F), pt_state=mk(n, (2, J.MAXP), I), frame_cyl=mk(n, (6,), F),
             frame_stats=mk(n, (4,), F), res=mk(n, (2, J.MAXP, 2), F), angles=mk(n, (2,), F), frame_N=mk(n, (17,), F))
    p = lambda k: None if d[k] is None or k in null else d[k].data_ptr()
    op = {k: (None if k in null else v.data_ptr()) for k, v in o.items()}
    if not optional:
        op.update(N=None, res=None, frame_N=None)
    if alias:
        op[alias[0]] = d[alias[1]].data_ptr()
    s = dict(radius=J.RADIUS, lo=t['lo'], hi=t['hi'], swap=case['swap'], min_cos=case['min_cos'], sel_cos=case['sel_cos'], gate_px=case['gate_px'],
             tol_x=1e-9, tol_f=1e-9, max_iter=100, n=n, G=G, w_pan=case['w_pan'], w_tilt=case['w_tilt'])
    s.update(over)
    rc = cpe.lib.load().cpe_multi_frame_fit_pixels_angles_batch(
        p('xy1'), p('id1'), p('cnt1'), p('xy2'), p('id2'), p('cnt2'), p('angles0'), p('frame_ok'), p('gs'), s['G'], s['n'], p('x0'), s['w_pan'],
        s['w_tilt'], s['radius'], p('K1'), p('K2'), p('T21'), p('P'), p('st'), s['lo'], s['hi'], p('centre'), s['swap'], s['min_cos'], s['sel_cos'],
        s['gate_px'], s['tol_x'], s['tol_f'], s['max_iter'], *(op[k] for k in KEYS), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in o.items()}


def _sentinel(v):
    return v == (SENTINEL_F if v.dtype == np.float64 else SENTINEL_I)


def _untouched(o):
    return all(_sentinel(v).all() for v in o.values())


def _rel_blocks(got, want):
    """the largest difference of two sets of blocks (U or N (6,6), V (F,2,2), W (F,6,2)), each entry relative to the square root of
    the product of its two diagonal entries"""
    (Ng, Vg, Wg), (Nw, Vw, Ww) = got, want
    dn = np.sqrt(np.diag(Nw))
    worst = float((np.abs(Ng - Nw) / (dn[:, None] * dn[None, :])).max())
    for vg, wg, vw, ww in zip(Vg, Wg, Vw, Ww):
        dv = np.sqrt(np.diag(vw))
        worst = max(worst, float((np.abs(vg - vw) / (dv[:, None] * dv[None, :])).max()), float((np.abs(wg - ww) / (dn[:, None] * dv[None, :])).max()))
    return worst


def _compare_group(got, g, ref, what, chains, scipy=True):
    """-> (res off, pose off scipy, angles off scipy, F / F_ls - 1, blocks off) of a fitted group, None otherwise"""
    assert int(got['status'][g]) == ref['status'], f'{what}: status {int(got["status"][g])} != {ref["status"]}'
    assert int(got['n_used'][g]) == ref['n_used'], f'{what}: n_used'
    assert np.array_equal(got['counts'][g], ref['counts']), f'{what}: counts {got["counts"][g]} != {ref["counts"]}'
    if ref['status'] != J.ST_OK:
        for k in GROUP_KEYS:
            if k != 'status':
                assert not got[k][g].any(), f'{what}: {k} of a group without a fit is not zero'
        for f in ref['kept']:
            for k in ('frame_cyl', 'frame_stats', 'res', 'angles', 'frame_N'):
                assert _sentinel(got[k][f]).all(), f'{what}: {k} of frame {f} was written'
        return None
    for k in GROUP_KEYS:
        assert np.isfinite(got[k][g]).all(), f'{what}: {k} is not finite'
    kept, grp = ref['kept'], ref['grp']
    T = got['T'][g].reshape(4, 4)
    q = got['angles'][kept]
    assert np.abs(T - M.LM.vec2T(got['x'][g])).max() <= 8 * EPS, f'{what}: T is not vec2T(x)'
    # a frame without a member keeps the bits of its nominal angles
    for i, f in enumerate(kept):
        if len(ref['S'][i]) == 0:
            assert q[i].tobytes() == grp.q0[i].tobytes(), f'{what}: the memberless frame {f} moved: {q[i]!r} from {grp.q0[i]!r}'
    # frame_cyl against T * chain(q) of the returned T and angles, the chain with the bits the header names: cpe_agv_chain_batch's
    for i, f in enumerate(kept):
        want, tol = M.frame_cyl(T, chains[i]), M.frame_cyl_tol(T, chains[i])
        assert (np.abs(got['frame_cyl'][f] - want) <= tol).all(), f'{what}: frame_cyl of frame {f} off by {np.abs(got["frame_cyl"][f] - want).max():.2e}'
    # residuals and statistics: the reference at the frame poses the call returned
    cyls = [got['frame_cyl'][f] for f in kept]
    ev = J.evaluate_at(ref, T, q, cyls)
    assert ev['ok'], f'{what}: a member of S has no node at the returned point'
    worst_r = 0.0
    sq, m1, m2, s1, s2, rmax = 0.0, 0, 0, 0.0, 0.0, 0.0
    for i, f in enumerate(kept):
        used = np.zeros((2, J.MAXP), bool)
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
    rel = (2 * 2 * (m1 + m2) + 2 * len(kept) + 18) * EPS
    want = np.array([np.sqrt(s1 / m1) if m1 else 0.0, np.sqrt(s2 / m2) if m2 else 0.0, np.sqrt(sq / (m1 + m2)), rmax])
    full = sq + grp.prior(q)
    assert abs(got['fvals'][g, 1] - full) <= rel * full, f'{what}: fvals[1] {got["fvals"][g, 1]!r} != {full!r}'
    assert (np.abs(got['stats'][g] - want) <= rel * want).all(), f'{what}: stats {got["stats"][g]} != {want}'
    # fvals[0]: the reference at the start (the prior's part is zero there), through the residuals' tolerances
    e0 = J.evaluate_at(ref, M.LM.vec2T(ref['grp_x0']), grp.q0)
    t0 = np.concatenate([t[t > 0] for t in e0['tol_res']])
    r0 = np.concatenate([np.abs(r).sum(2)[t > 0] for r, t in zip(e0['res'], e0['tol_res'])])
    assert abs(got['fvals'][g, 0] - ref['fvals'][0]) <= (2 * r0 * t0 + 2 * t0 * t0).sum() + rel * ref['fvals'][0], f'{what}: fvals[0]'
    assert got['fvals'][g, 1] <= got['fvals'][g, 0]
    it = got['iters'][g]
    assert 1 <= it[0] <= 3 * ref['iters'][0] and it[0] < it[1], f'{what}: iters {it}, reference {ref["iters"]}'
    # N and frame_N against the reference's blocks at the returned point
    U, gx, V, W, gq = ev['blocks']
    Ng = np.zeros((6, 6)); Ng[np.triu_indices(6)] = got['N'][g]; Ng = Ng + np.triu(Ng, 1).T
    fN = got['frame_N'][kept]
    Vg = np.stack([fN[:, [0, 1]], fN[:, [1, 2]]], 1)
    db = _rel_blocks((Ng, Vg, fN[:, 3:15].reshape(-1, 6, 2)), (J.reduced(U, V, W), V, W))
    assert db <= J.JOINT_N_BOUND, f'{what}: N / frame_N off by {db:.3e}, bound {J.JOINT_N_BOUND:.3e}'
    # the gradient of a frame's block, g = J'r + the prior's: by Cauchy-Schwarz a change dr of the residuals moves g_k by at most
    # sqrt(V_kk) |dr|, with |dr|^2 <= 2 sum tol_res^2; the sums themselves are held as the blocks are, at the level sqrt(V_kk F)
    dr = np.array([np.sqrt(2 * (t * t).sum()) for t in ev['tol_res']])
    gtol = np.sqrt(np.stack([V[:, 0, 0], V[:, 1, 1]], 1)) * (dr[:, None] + J.JOINT_N_BOUND * np.sqrt(full))
    assert (np.abs(fN[:, 15:] - gq) <= gtol).all(), f'{what}: the gradients of frame_N are off by {(np.abs(fN[:, 15:] - gq) / gtol).max():.2e} of the bound'
    dp = da = df = None
    if ref['nan_trials'] == 0:
        # against scipy's optimum within twice the bounds; where scipy is not run (the capacity case, see the cases file) against the
        # restated loop's result within three times: the loop lies within the bounds of the optimum and the kernel within twice
        o, k, name = (ref['opt'], 2, 'scipy\'s optimum') if scipy else (dict(T=ref['T'], q=ref['angles'], f=ref['fvals'][1]), 3, 'the restated loop')
        dp, da, df = M.pose_difference(T, o['T']), float(np.abs(q - o['q']).max()), got['fvals'][g, 1] / o['f'] - 1
        assert dp <= k * J.JOINT_POSE_BOUND, f'{what}: pose {dp:.3e} off {name}, bound {k * J.JOINT_POSE_BOUND:.3e}'
        assert da <= k * J.JOINT_ANGLE_BOUND, f'{what}: angles {da:.3e} off {name}, bound {k * J.JOINT_ANGLE_BOUND:.3e}'
        assert abs(df) <= k * J.JOINT_F_BOUND, f'{what}: F / F_ref - 1 = {df:.3e}, bound {k * J.JOINT_F_BOUND:.3e}'
    return worst_r, dp, da, df, db


def _check_call(cpe, gpu, name, case, refs, scipy=True):
    d = _inputs(gpu, case)
    runs = [_raw(cpe, gpu, case, d) for _ in range(2)]
    assert all(rc == 0 for rc, _ in runs)
    got = runs[0][1]
    for k in KEYS:
        assert got[k].tobytes() == runs[1][1][k].tobytes(), f'{k}: a second call gave other bits'
    for k in GROUP_KEYS:
        assert not _sentinel(got[k]).any(), f'{k}: a slot was not written'
    assert np.array_equal(got['pt_state'][:d['n']], J.expected_pt_state(case, refs)), f'{name}: pt_state differs'
    worst = [0.0] * 5
    A = cpe.multiframe.agv_chain_batch(torch.from_numpy(got['angles'][:d['n']].copy()).to(gpu)).cpu().numpy().reshape(-1, 4, 4)
    for g, ref in enumerate(refs):
        ref['grp_x0'] = case['x0'][g]
        out = _compare_group(got, g, ref, f'{name} group {g}', A[ref['kept']], scipy)
        if out:
            worst = [max(w, abs(v)) if v is not None else w for w, v in zip(worst, out)]
    print(f'{name}: res off by {worst[0]:.2e} px; against {"scipy" if scipy else "the restated loop"}: pose {worst[1]:.2e}, angles {worst[2]:.2e}, F / F_ls - 1 {worst[3]:.2e}; '
          f'blocks {worst[4]:.2e}; iterations {got["iters"][:, 0].max()}')
    # the optional outputs NULL: the others keep their bits
    rc, b = _raw(cpe, gpu, case, d, optional=False)
    opt = ('N', 'res', 'frame_N')
    assert rc == 0 and all(b[k].tobytes() == got[k].tobytes() for k in KEYS if k not in opt)
    assert all(_sentinel(b[k]).all() for k in opt)
    return d, got


@pytest.mark.parametrize('name', list(J.cases()))
def test_cases(cpe, gpu, name):
    _check_call(cpe, gpu, name, J.cases()[name], J.reference(name))


def test_the_capacity_and_one_frame_more(cpe, gpu):
    """CPE_MFJOINT_MAXF kept frames of 3 + 3 detections are fitted; one frame more is OVERFLOW for that group alone"""
    case = J.capacity_case()
    _, got = _check_call(cpe, gpu, 'capacity', case, J.reference('capacity'), scipy=False)
    assert got['status'][0] == J.ST_OK and got['n_used'][0] == J.MAXF
    over = J.capacity_case(1)
    rc, o = _raw(cpe, gpu, over)
    assert rc == 0 and o['status'][0] == J.ST_OVERFLOW and o['status'][1] == J.ST_OK
    for k in GROUP_KEYS:
        if k != 'status':
            assert not o[k][0].any(), f'{k} of the overflowing group is not zero'
        assert o[k][1].tobytes() == got[k][1].tobytes(), f'{k}: the group after the overflowing one differs'
    nf = J.MAXF + 1
    assert (o['pt_state'][:nf, :, :3] == 1).all() and (o['pt_state'][:nf, :, 3:] == -1).all()
    for k in ('frame_cyl', 'frame_stats', 'res', 'angles', 'frame_N'):
        assert _sentinel(o[k][:nf]).all(), f'{k} of the overflowing group was written'
    # a range outside [0, n]: OVERFLOW, no frame touched
    base = J.cases()['two frames']
    rc, o = _raw(cpe, gpu, dict(base, group_start=np.array([0, 3], np.int32)))
    assert rc == 0 and o['status'][0] == J.ST_OVERFLOW and _sentinel(o['pt_state']).all()


def test_a_group_does_not_depend_on_its_place_or_on_what_lies_past_the_counts(cpe, gpu):
    case = J.cases()['three groups']
    _, a = _raw(cpe, gpu, case)
    _, b = _raw(cpe, gpu, dict(case, poison=None))
    for k in KEYS:
        assert a[k].tobytes() == b[k].tobytes(), f'{k}: depends on the slots past the counts'
    gs = case['group_start']
    order = [3, 1, 0, 2]
    frames = np.concatenate([np.arange(gs[g], gs[g + 1]) for g in order]).astype(int)
    perm = dict(case, fr1=[case['fr1'][f] for f in frames], fr2=[case['fr2'][f] for f in frames], angles=case['angles'][frames],
                TAGV=case['TAGV'][frames], frame_ok=case['frame_ok'][frames],
                group_start=np.cumsum([0] + [gs[g + 1] - gs[g] for g in order]).astype(np.int32), x0=case['x0'][order], poison=5)
    _, c = _raw(cpe, gpu, perm)
    for k in GROUP_KEYS:
        assert a[k][:4][order].tobytes() == c[k][:4].tobytes(), f'{k}: depends on the group\'s place in the batch'
    for k in FRAME_KEYS:
        assert a[k][frames].tobytes() == c[k][:len(frames)].tobytes(), f'{k}: depends on the group\'s place in the batch'


def test_refusals_write_nothing(cpe, gpu):
    case = J.cases()['gate 4 px']
    d = _inputs(gpu, case)
    rc, good = _raw(cpe, gpu, case, d)
    assert rc == 0
    rc, o = _raw(cpe, gpu, case, d, G=0)
    assert rc == 0 and _untouched(o)
    nan, inf = float('nan'), float('inf')
    refused = [dict(radius=0.0), dict(radius=-1.0), dict(radius=nan), dict(radius=inf), dict(hi=case['table']['lo'] - 1), dict(lo=-128, hi=128),
               dict(min_cos=0.0), dict(min_cos=1.0), dict(min_cos=nan), dict(sel_cos=0.05), dict(sel_cos=1.0), dict(sel_cos=nan), dict(swap=2),
               dict(swap=-1), dict(tol_x=0.0), dict(tol_x=nan), dict(tol_f=0.0), dict(tol_f=-1e-9), dict(max_iter=0), dict(n=-1), dict(G=-1),
               dict(w_pan=0.0), dict(w_pan=-1.0), dict(w_pan=nan), dict(w_pan=inf), dict(w_tilt=0.0), dict(w_tilt=-125.0), dict(w_tilt=nan),
               dict(w_tilt=inf)]
    for kw in refused:
        rc, o = _raw(cpe, gpu, case, d, **kw)
        assert rc == -1 and _untouched(o), kw
    for null in (('xy1',), ('id2',), ('cnt1',), ('xy1', 'id1', 'cnt1', 'xy2', 'id2', 'cnt2'), ('angles0',), ('gs',), ('x0',), ('K1',), ('K2',),
                 ('T21',), ('P',), ('st',), ('centre',), ('pt_state',), ('frame_cyl',), ('frame_stats',), ('x',), ('status',), ('angles',)):
        rc, o = _raw(cpe, gpu, case, d, null=null)
        assert rc == -1 and _untouched(o), null
    for alias in (('x', 'x0'), ('res', 'xy1'), ('pt_state', 'id1'), ('fvals', 'K1'), ('stats', 'P'), ('status', 'cnt2'), ('counts', 'st'),
                  ('iters', 'centre'), ('angles', 'angles0'), ('n_used', 'gs'), ('frame_N', 'xy2')):
        rc, o = _raw(cpe, gpu, case, d, alias=alias)
        o.pop(alias[0])
        assert rc == -1 and _untouched(o), alias
    assert cpe.lib.load().cpe_last_error_string().decode().startswith('cpe_multi_frame_fit_pixels_angles_batch')
    # sel_cos = min_cos is allowed; a NULL frame_ok keeps every frame
    rc, a = _raw(cpe, gpu, case, d, sel_cos=case['min_cos'])
    assert rc == 0 and a['status'][0] == J.ST_OK
    rc, a = _raw(cpe, gpu, dict(case, frame_ok=np.ones(3, np.int32)))
    assert rc == 0 and all(a[k].tobytes() == good[k].tobytes() for k in KEYS)


def test_the_acceptance_comparisons_hold_on_the_gpu(cpe, gpu):
    """the five perturbed scenes as five groups of one call, each from its fixed-angle fit: the joint fit's frame axes are nearer
    than the fixed-angle fit's in angle and in distance and its pixel rms is below 0.40, as on the reference"""
    runs = [J.accuracy_run(F, seed) for F, seed in J.ACCURACY_RUNS]
    cat = lambda k: [f for r in runs for f in r['scene'][k]]
    gs = np.cumsum([0] + [F for F, _ in J.ACCURACY_RUNS]).astype(np.int32)
    ang = np.concatenate([r['scene']['angles'] for r in runs])
    case = dict(J.cases()['two frames'], fr1=cat('fr1'), fr2=cat('fr2'), angles=ang, TAGV=J.JointGroup.chains(ang), group_start=gs,
                x0=np.stack([r['fixed']['x'] for r in runs]), poison=None)
    rc, got = _raw(cpe, gpu, case)
    assert rc == 0 and (got['status'][:len(runs)] == J.ST_OK).all()
    for g, ((F, seed), run) in enumerate(zip(J.ACCURACY_RUNS, runs)):
        err = J.axis_rms(got['T'][g].reshape(4, 4), got['angles'][gs[g]:gs[g + 1]], run['scene'])
        print(f'F = {F:2d} seed {seed}: fixed {run["err_fixed"][0]:.4f} deg {run["err_fixed"][1]:.4f} mm; joint on the GPU {err[0]:.4f} deg {err[1]:.4f} mm, '
              f'{got["stats"][g, 2]:.4f} px; reference {run["err_joint"][0]:.4f} {run["err_joint"][1]:.4f}')
        assert err[0] < run['err_fixed'][0] and err[1] < run['err_fixed'][1] and got['stats'][g, 2] < 0.40
