"""The build-defined frame-angle solver on the GPU: cpe_agv_chain_batch, cpe_frame_angles_lm_batch /
multiframe.agv_chain_batch, multiframe.estimate_frame_angles_gpu / experiment.run_experiment(frame_angles=True).

Scenes: frame_angles_cases.gpu_scene -- F = 1, 2, 13, 65 frames at noise 0 and 0.05, point counts 5, 63, 64, 65, 160, 2048 in
turn (lane tails, several rounds, a full table).  Yardsticks:
  chain    oracle.get_TAGVcyl on n = 1, 64, 65, 1000 angle pairs: rotation entries within 16 * 2^-53, column 4 within 1e-12 mm
           (trig values 4 ulp off over link lengths summing to 574.2)
  A        tolerance 0: TAGV against cpe_agv_chain_batch(angles), fvals against cpe_multi_frame_terms at that table, Tcyl against
           the product restated in numpy, a second call, a batch in reversed frame order, several poses against single-pose calls
  B        scipy's least_squares(method='lm', xtol = ftol = 1e-14) from the true angles: angles within 1e-5 rad,
           f <= f_ls (1 + 1e-6) (<= tol_f 1e-3 = 1e-8 on the noise-free scenes, where f is rounding residue), iterations <= 3 x
           the numpy restatement's, the noise-free scenes within 1e-5 rad of the truth, the start within 1e-12 of the
           restatement's from the same cyl_raw
Measured on one MI355X (run with -s): chain rotation entries 2 x 2^-53, column 4 1.14e-13 mm; angles within 2.8e-9 rad of
scipy's optimum, 3.3e-10 rad from the truth without noise, the start 8.3e-17 rad from the restatement's; iterations <= 4 as the
restatement's, evaluations <= 11 (restatement 13)."""
import ctypes as C
import json
import math

import numpy as np
import pytest

import frame_angles_cases as fc
import multiframe_cases as mc

R = mc.RADIUS
ST_OK, ST_FEW, ST_OVERFLOW = 0, 5, 6
KEYS = ('angles0', 'angles', 'fvals', 'iters', 'TAGV', 'Tcyl', 'status')
SCENES = [(F, noise) for F in fc.GPU_FRAMES for noise in fc.GPU_NOISES]
IDS = [f'F{F}_noise{noise}' for F, noise in SCENES]


def host(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def frames_equal(a, ia, b, ib, keys=KEYS):
    return all(np.array_equal(bits(a[k][ia]), bits(b[k][ib])) for k in keys)


def assert_failed_frame(r, f, status):
    assert r['status'][f] == status
    for k in KEYS[:-1]:
        assert not r[k][f].any(), f'{k} of a frame with status {status} must be zero'


@pytest.fixture(scope='module')
def scenes(cpe, gpu):
    """(F, noise) -> the scene on the host and the device, its per-frame fits (on the GPU), and per frame the restatement's
    start and fit and scipy's optimum: computed once"""
    import torch
    from cpe_amd import fit
    out = {}
    for F, noise in SCENES:
        P, cnt, angles, Ttrue = fc.gpu_scene(F, noise)
        Pd, cd = torch.from_numpy(P).to(gpu), torch.from_numpy(cnt).to(gpu)
        per = fit.fit_cylinder_batch(Pd, cd, R)
        assert not per['status'].any()
        raw = per['cyl_raw'].cpu().numpy()
        ref = []
        for i in range(F):
            prob = fc.FrameProblem(P[i, :cnt[i]], Ttrue)
            assert fc.usable(cnt[i], raw[i, 1])
            start = fc.start_from_direction(Ttrue, raw[i, 1, 3:6])
            q, f, iters, evals = fc.lm(prob, start)
            q_ls, f_ls = fc.scipy_optimum(prob, angles[i])
            ref.append(dict(start=start, q=q, f=f, iters=iters, evals=evals, q_ls=q_ls, f_ls=f_ls))
        out[(F, noise)] = dict(P=P, cnt=cnt, angles=angles, Ttrue=Ttrue, raw=raw, Pd=Pd, cd=cd, rawd=per['cyl_raw'].contiguous(),
                               Td=torch.from_numpy(Ttrue.reshape(1, 16)).to(gpu), ref=ref, noise=noise)
    return out


def estimate(s, **kw):
    from cpe_amd import multiframe
    args = dict(pts3=s['Pd'], cnt=s['cd'], cyl_raw=s['rawd'], T=s['Td'], radius=R)
    args.update(kw)
    return host(multiframe.estimate_frame_angles_gpu(**args))


@pytest.fixture(scope='module')
def single(scenes):
    return {key: estimate(scenes[key]) for key in SCENES}


def frame_terms(cpe, s, TAGV, T16, X=None, cnt=None):
    import torch
    X, cnt = (s['Pd'], s['cd']) if X is None else (X, cnt)
    dev = X.device
    n = cnt.shape[0]
    terms = torch.zeros(n, dtype=torch.float64, device=dev)
    A = torch.from_numpy(np.ascontiguousarray(TAGV)).to(dev)
    T = torch.from_numpy(np.ascontiguousarray(T16, dtype=np.float64)).to(dev)
    rc = cpe.lib.load().cpe_multi_frame_terms(X.data_ptr(), cnt.data_ptr(), n, A.data_ptr(), T.data_ptr(), R, terms.data_ptr(),
                                              torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    return terms.cpu().numpy()


def chain(cpe, angles, dev):
    import torch
    return cpe.multiframe.agv_chain_batch(torch.from_numpy(np.ascontiguousarray(angles, dtype=np.float64)).to(dev)).cpu().numpy()


# -------------------------------------------------------------------------------------------------------------- the chain
@pytest.mark.gpu
@pytest.mark.parametrize('n', [1, 64, 65, 1000])
def test_chain_against_the_oracle(cpe, orc, gpu, n):
    rng = np.random.default_rng(n)
    q = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1.2, 1.2, n)], 1)
    special = np.array([[0, 0], [1e-300, -1e-300], [-1e-9, 1e-9], [0.3, 1.0], [-0.3, -1.0], [0.0, 1e-17], [-0.0, -0.0], [1.5, 1.2]])
    if n == 1:
        q[0] = [0.3, 1.0]
    else:
        q[-len(special):] = special
    got = chain(cpe, q, gpu).reshape(n, 4, 4)
    ref = np.stack([orc.get_TAGVcyl(float(a), float(b)) for a, b in q]).reshape(n, 4, 4)
    rot, col4 = np.abs(got[:, :3, :3] - ref[:, :3, :3]).max(), np.abs(got[:, :3, 3] - ref[:, :3, 3]).max()
    print(f'n = {n}: rotation entries {rot / 2.0 ** -53:.2f} x 2^-53, column 4 {col4:.3g} mm')
    assert rot <= 16 * 2.0 ** -53
    assert col4 <= 1e-12
    assert np.array_equal(got[:, 3], np.tile([0.0, 0, 0, 1], (n, 1)))
    if n == 64:                                            # n = 0 is a no-op, also with NULL pointers
        assert cpe.lib.load().cpe_agv_chain_batch(None, 0, None, None) == 0
        assert cpe.lib.load().cpe_agv_chain_batch(None, -1, None, None) == -1


# ------------------------------------------------------------------------------------------------------------ yardstick A
@pytest.mark.gpu
@pytest.mark.parametrize('key', SCENES, ids=IDS)
def test_outputs_equal_the_exported_pieces(cpe, gpu, scenes, single, key):
    s, got = scenes[key], single[key]
    assert (got['status'] == ST_OK).all()
    T16 = s['Ttrue'].ravel()
    A = chain(cpe, got['angles'], gpu)
    assert np.array_equal(bits(got['TAGV']), bits(A))
    assert np.array_equal(bits(got['fvals'][:, 1]), bits(frame_terms(cpe, s, A, T16)))
    assert np.array_equal(bits(got['fvals'][:, 0]), bits(frame_terms(cpe, s, chain(cpe, got['angles0'], gpu), T16)))
    for i in range(len(s['cnt'])):
        assert np.array_equal(bits(got['Tcyl'][i]), bits(fc.tcyl_product(T16, got['TAGV'][i]))), f'Tcyl of frame {i}'
    again = estimate(s)
    assert all(np.array_equal(bits(again[k]), bits(got[k])) for k in KEYS)
    import torch
    rev = estimate(s, pts3=torch.flip(s['Pd'], [0]).contiguous(), cnt=torch.flip(s['cd'], [0]).contiguous(),
                   cyl_raw=torch.flip(s['rawd'], [0]).contiguous())
    assert all(np.array_equal(bits(rev[k][::-1]), bits(got[k])) for k in KEYS)


# ------------------------------------------------------------------------------------------------------------ yardstick B
@pytest.mark.gpu
@pytest.mark.parametrize('key', SCENES, ids=IDS)
def test_reaches_the_optimum(scenes, single, key):
    s, got = scenes[key], single[key]
    F = len(s['cnt'])
    assert (got['status'] == ST_OK).all()
    dq = max(fc.angle_distance(got['angles'][i], s['ref'][i]['q_ls']) for i in range(F))
    d0 = max(fc.angle_distance(got['angles0'][i], s['ref'][i]['start']) for i in range(F))
    dt = max(fc.angle_distance(got['angles'][i], s['angles'][i]) for i in range(F))
    off = max(fc.angle_distance(got['angles0'][i], s['angles'][i]) for i in range(F))
    print(f'{key}: to scipy {dq:.3g} rad, start to the restatement {d0:.3g} rad, start {off:.3g} rad / result {dt:.3g} rad from the truth; '
          f'iterations <= {got["iters"][:, 0].max()} (restatement {max(r["iters"] for r in s["ref"])}), evaluations <= {got["iters"][:, 1].max()} '
          f'(restatement {max(r["evals"] for r in s["ref"])})')
    for i in range(F):
        ref = s['ref'][i]
        assert fc.angle_distance(got['angles'][i], ref['q_ls']) <= 1e-5
        if s['noise'] == 0:
            assert got['fvals'][i, 1] <= 1e-8
            assert fc.angle_distance(got['angles'][i], s['angles'][i]) <= 1e-5
        else:
            assert got['fvals'][i, 1] <= ref['f_ls'] * (1 + 1e-6)
        assert got['iters'][i, 0] <= 3 * ref['iters']
        assert got['iters'][i, 1] >= got['iters'][i, 0] + 1
        assert fc.angle_distance(got['angles0'][i], ref['start']) <= 1e-12
        assert got['fvals'][i, 1] <= got['fvals'][i, 0]


# ---------------------------------------------------------------------------------------------------------- several poses
@pytest.mark.gpu
def test_several_poses(scenes, gpu):
    import torch
    s = scenes[(13, 0.05)]
    F = 13
    T1, T2 = s['Ttrue'].copy(), s['Ttrue'].copy()
    T1[:3, 3] += [1.0, -2.0, 3.0]
    c, sn = math.cos(0.01), math.sin(0.01)
    T2[:3, :3] = np.array([[c, -sn, 0], [sn, c, 0], [0, 0, 1.0]]) @ T2[:3, :3]
    Ts = np.stack([s['Ttrue'].ravel(), T1.ravel(), T2.ravel()])
    idx = np.array([i % 3 for i in range(F)], np.int32)
    idx[:3] = [2, 2, 0]
    mixed = estimate(s, T=torch.from_numpy(Ts).to(gpu), pose_index=torch.from_numpy(idx).to(gpu))
    assert (mixed['status'] == ST_OK).all()
    alone = [estimate(s, T=torch.from_numpy(Ts[g:g + 1].copy()).to(gpu)) for g in range(3)]
    for i in range(F):
        assert frames_equal(mixed, i, alone[idx[i]], i), f'frame {i} with pose {idx[i]} differs from the single-pose call'
    assert not frames_equal(alone[0], 0, alone[1], 0)
    zeros = estimate(s, T=torch.from_numpy(Ts).to(gpu), pose_index=torch.zeros(F, dtype=torch.int32, device=gpu))
    null = estimate(s, T=torch.from_numpy(Ts).to(gpu))
    assert all(np.array_equal(bits(zeros[k]), bits(null[k])) and np.array_equal(bits(null[k]), bits(alone[0][k])) for k in KEYS)


# ------------------------------------------------------------------------------------------------------------------ a0_in
@pytest.mark.gpu
def test_given_start(cpe, scenes, single, gpu):
    import torch
    s, got = scenes[(13, 0.05)], single[(13, 0.05)]
    nominal = np.deg2rad(np.round(np.rad2deg(s['angles'])))
    a0 = torch.from_numpy(nominal).to(gpu)
    given = estimate(s, a0=a0)
    assert (given['status'] == ST_OK).all() and np.array_equal(given['angles0'], nominal)
    print(f'from the nominal angles: {np.abs(given["angles"] - got["angles"]).max():.3g} rad from the closed-form start\'s result')
    for i in range(13):
        assert fc.angle_distance(given['angles'][i], s['ref'][i]['q_ls']) <= 1e-5
    without_raw = estimate(s, a0=a0, cyl_raw=None)                                  # cyl_raw NULL beside a0_in
    assert all(np.array_equal(bits(without_raw[k]), bits(given[k])) for k in KEYS)
    L = cpe.lib.load()
    out = {k: torch.full((13, w), 7.25 if dt == torch.float64 else 77, dtype=dt, device=gpu)
           for k, w, dt in (('a0', 2, torch.float64), ('a', 2, torch.float64), ('fv', 2, torch.float64), ('it', 2, torch.int32),
                            ('st', 1, torch.int32))}
    rc = L.cpe_frame_angles_lm_batch(s['Pd'].data_ptr(), s['cd'].data_ptr(), None, s['Td'].data_ptr(), None, 1, 13, R, None, None,
                                     out['a0'].data_ptr(), out['a'].data_ptr(), out['fv'].data_ptr(), out['it'].data_ptr(), None, None,
                                     out['st'].data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == -1 and b'cpe_frame_angles_lm_batch' in L.cpe_last_error_string()
    torch.cuda.synchronize()
    assert all((t == (7.25 if t.dtype == torch.float64 else 77)).all() for t in out.values())
    # NULL TAGVcyl / Tcyl are accepted: the other outputs are those of the full call
    rc = L.cpe_frame_angles_lm_batch(s['Pd'].data_ptr(), s['cd'].data_ptr(), s['rawd'].data_ptr(), s['Td'].data_ptr(), None, 1, 13, R, None, None,
                                     out['a0'].data_ptr(), out['a'].data_ptr(), out['fv'].data_ptr(), out['it'].data_ptr(), None, None,
                                     out['st'].data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    assert np.array_equal(bits(out['a'].cpu().numpy()), bits(got['angles'])) and np.array_equal(out['it'].cpu().numpy(), got['iters'])


# --------------------------------------------------------------------------------------------------------------- statuses
@pytest.mark.gpu
def test_statuses(cpe, scenes, single, gpu):
    import torch
    s, good = scenes[(13, 0.05)], single[(13, 0.05)]
    F = 13
    assert s['cnt'][:8].tolist() == [5, 63, 64, 65, 160, 2048, 5, 63]
    cnt = s['cd'].clone()
    cnt[0], cnt[1], cnt[5] = 0, 4, mc.MAXP + 100                     # frame 6 keeps its 5 points, frame 5 is a full table
    raw = s['rawd'].clone()
    raw[4, 1, 4] = float('nan')
    raw[3, 1, 3:6] = 0
    P = s['Pd'].clone()
    P[7, 3, 1] = float('nan')
    idx = torch.zeros(F, dtype=torch.int32, device=gpu)
    idx[8], idx[9] = -1, 2
    T2 = torch.cat([s['Td'], s['Td']])
    got = estimate(s, pts3=P, cnt=cnt, cyl_raw=raw, T=T2, pose_index=idx)
    expect = {0: ST_FEW, 1: ST_FEW, 3: ST_FEW, 4: ST_FEW, 7: ST_FEW, 8: ST_OVERFLOW, 9: ST_OVERFLOW}
    for f in range(F):
        if f in expect:
            assert_failed_frame(got, f, expect[f])
        else:                                               # the neighbours are undisturbed; cnt above CPE_MAXP is clamped
            assert frames_equal(got, f, good, f), f'frame {f} beside failed frames differs from the clean call'
    assert all(np.isfinite(got[k]).all() for k in KEYS)
    # with a given start the fitted rows are not read
    a0 = torch.from_numpy(s['angles']).to(gpu)
    given = estimate(s, cyl_raw=raw, a0=a0)
    assert (given['status'] == ST_OK).all()
    # a start that is not finite
    a0[2, 0] = float('inf')
    assert_failed_frame(estimate(s, a0=a0), 2, ST_FEW)
    # arguments
    from cpe_amd import lib
    with pytest.raises(lib.CpeError, match='cpe_frame_angles_lm_batch'):
        from cpe_amd import multiframe
        p = multiframe._tol_params()                       # mode CPE_FIT_NELDER_MEAD
        out = [torch.empty((F, 2), dtype=torch.float64, device=gpu) for _ in range(3)]
        it, st = torch.empty((F, 2), dtype=torch.int32, device=gpu), torch.empty(F, dtype=torch.int32, device=gpu)
        lib.check(lib.load().cpe_frame_angles_lm_batch(s['Pd'].data_ptr(), s['cd'].data_ptr(), s['rawd'].data_ptr(), s['Td'].data_ptr(), None, 1, F,
                                                       R, C.addressof(p), None, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                                       it.data_ptr(), None, None, st.data_ptr(), torch.cuda.current_stream().cuda_stream),
                  'cpe_frame_angles_lm_batch')
    # n = 0 is a no-op
    empty = estimate(s, pts3=s['Pd'][:0], cnt=s['cd'][:0], cyl_raw=s['rawd'][:0])
    assert all(empty[k].shape[0] == 0 for k in KEYS)
    assert lib.load().cpe_frame_angles_lm_batch(*([None] * 5), 1, 0, R, None, *([None] * 9)) == 0


@pytest.mark.gpu
def test_iteration_cap_and_far_start_end_within_the_caps(scenes, gpu):
    """max_iter is honoured, and a start near the pole of tan(tilt) ends within 200 iterations of 12 trials with a finite result
    or status 5"""
    import torch
    s = scenes[(13, 0.05)]
    capped = estimate(s, a0=torch.zeros((13, 2), dtype=torch.float64, device=gpu), max_iter=1)
    assert (capped['iters'][:, 0] <= 1).all() and (capped['status'] == ST_OK).all()
    a0 = torch.tensor([[1.2, 1.5], [-3.0, -1.56], [0.0, math.pi / 2], [1e6, 0.0]] * 4, dtype=torch.float64, device=gpu)[:13]
    far = estimate(s, a0=a0)
    assert (far['iters'][:, 0] <= 200).all() and (far['iters'][:, 1] <= 1 + 12 * 200).all()
    for f in range(13):
        if far['status'][f] == ST_OK:
            assert all(np.isfinite(far[k][f]).all() for k in KEYS) and far['fvals'][f, 1] <= far['fvals'][f, 0]
        else:
            assert_failed_frame(far, f, ST_FEW)


# ------------------------------------------------------------------------------------------------------------- experiment
H, W, NF = 480, 640, 6


@pytest.mark.gpu
def test_run_experiment_frame_angles(cpe, gpu, tmp_path):
    """the folder of test_multiframe_lm_gpu.py::test_run_experiment_lm_mode"""
    from PIL import Image
    from cpe_amd import experiment, multiframe, synth
    b = synth.render_batch(NF, H, W, seed=0, with_gt=False)
    stems = ['-10', '-21', '00', '1-2', '11', '2-1']
    L, Rr = b['left'].numpy(), b['right'].numpy()
    for i, st in enumerate(stems):
        Image.fromarray(L[i]).save(tmp_path / f'{st}L.png')
        Image.fromarray(Rr[i]).save(tmp_path / f'{st}R.png')
    for side in 'LR':
        Image.fromarray(np.zeros((H, W), np.uint8)).save(tmp_path / f'3-3{side}.png')
    lens = lambda K: dict(IntrinsicMatrix=np.asarray(K, dtype=np.float64).tolist(), RadialDistortion=[0.012, -0.004],
                          TangentialDistortion=[0.0002, -0.0001])
    (tmp_path / 'cam.json').write_text(json.dumps(dict(LeftCamera=lens(b['K1']), RightCamera=lens(b['K2']))))
    args = (str(tmp_path), str(tmp_path / 'cam.json'), b['K1'], b['K2'], b['T21'], b['radius'])
    plain = experiment.run_experiment(*args, chunk=4, multi_frame='lm')
    res = experiment.run_experiment(*args, chunk=4, multi_frame='lm', frame_angles=True)
    assert set(plain) == {'names', 'angles', 'records', 'pts3', 'cnt', 'cyl_raw', 'skipped', 'T_cam_agv', 'fval'}
    assert set(res) == set(plain) | {'angles_est', 'angles_status', 'angles_delta_deg'}
    assert res['T_cam_agv'] == plain['T_cam_agv'] and res['fval'] == plain['fval']
    F = len(res['names'])
    bad = {s['index'] for s in res['skipped']}
    good = [i for i in range(F) if i not in bad]
    assert len(bad) >= 1 and len(good) >= 2
    import torch
    g = torch.tensor(good, device=res['pts3'].device)
    direct = host(multiframe.estimate_frame_angles_gpu(res['pts3'][g], res['cnt'][g], res['cyl_raw'][g], res['T_cam_agv'], b['radius']))
    assert res['angles_est'].shape == (F, 2) and res['angles_status'].shape == (F,) and res['angles_delta_deg'].shape == (F, 2)
    for k, i in enumerate(good):
        assert res['angles_status'][i] == direct['status'][k]
        if direct['status'][k] == ST_OK:
            assert np.array_equal(bits(res['angles_est'][i]), bits(direct['angles'][k]))
            assert np.array_equal(res['angles_delta_deg'][i], np.rad2deg(res['angles_est'][i] - res['angles'][i]))
        else:
            assert np.isnan(res['angles_est'][i]).all()
    for i in bad:
        assert res['angles_status'][i] == -1 and np.isnan(res['angles_est'][i]).all() and np.isnan(res['angles_delta_deg'][i]).all()
    print('status', res['angles_status'].tolist(), 'delta (deg)', np.round(res['angles_delta_deg'], 3).tolist())
