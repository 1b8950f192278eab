"""The joint pose-and-angles fit in the Python layers: multiframe.fit_multi_frame_pixels_angles_gpu against the numpy reference of
tests/multiframe_joint_cases.py on one perturbed 8-frame scene, its cov and angle_sigma against numpy, its argument checks; and
experiment.run_experiment(multi_frame_joint=) on a rendered 640 x 480 folder: the new dict, every other entry bit for bit as without
the keyword."""
import json

import numpy as np
import pytest
import torch

import multiframe_joint_cases as J
import multiframe_pixel_cases as M
import plane_fit_cases as PC
import table_tri_cases as TC

pytestmark = pytest.mark.gpu

H, W = 480, 640


def _ltable(cpe, gpu, t, centre, family0='col'):
    return cpe.fit.LaserTable(torch.from_numpy(t['P']).to(gpu), torch.from_numpy(t['status'].astype(np.int32)).to(gpu), t['lo'], t['hi'],
                              torch.from_numpy(np.concatenate([centre, [0.0]])).to(gpu), torch.zeros(1, dtype=torch.int32, device=gpu), family0)


def _tables(cpe, gpu, sc):
    GT = cpe.fit.GridTables
    mats = lambda k: [np.concatenate([f['xy'], f['id']], 1) for f in sc[k]]
    return GT.from_lists(mats('fr1'), gpu), GT.from_lists(mats('fr2'), gpu)


def test_the_python_layer_against_the_reference(cpe, gpu):
    run = J.accuracy_run(8, 0)
    sc, ref = run['scene'], run['joint']
    tab = _ltable(cpe, gpu, TC.rig_table(TC.LO, TC.HI), PC.rig()[5])
    gp1, gp2 = _tables(cpe, gpu, sc)
    call = lambda **kw: cpe.multiframe.fit_multi_frame_pixels_angles_gpu(gp1.xy, gp1.id, gp1.cnt, gp2.xy, gp2.id, gp2.cnt, sc['angles'],
                                                                         run['fixed']['x'][None], J.RADIUS, *PC.rig()[:3], tab, **kw)
    out = call()
    got = {k: v.cpu().numpy() for k, v in out.items() if v is not None}
    assert out['res'] is None and got['status'].tolist() == [0] and got['counts'][0].tolist() == ref['counts'].tolist()
    o = J.scipy_optimum(ref, run['fixed']['x'])
    dp, da, df = M.pose_difference(got['T'][0], o['T']), float(np.abs(got['angles'] - o['q']).max()), got['fvals'][0, 1] / o['f'] - 1
    err = J.axis_rms(got['T'][0].reshape(4, 4), got['angles'], sc)
    print(f'against scipy: pose {dp:.2e}, angles {da:.2e}, F / F_ls - 1 {df:.2e}; frame axes {err[0]:.4f} deg {err[1]:.4f} mm, {got["stats"][0, 2]:.4f} px')
    assert dp <= 2 * J.JOINT_POSE_BOUND and da <= 2 * J.JOINT_ANGLE_BOUND and abs(df) <= 2 * J.JOINT_F_BOUND
    assert err[0] < run['err_fixed'][0] and err[1] < run['err_fixed'][1] and got['stats'][0, 2] < 0.40
    assert got['angles0'].tobytes() == sc['angles'].tobytes() and got['TAGV'].shape == (8, 16)
    # explicit weights override the sigmas; the default is sigma_px / sigma_angle
    same = call(sigma_px=0.5, sigma_angle=0.004)
    other = call(w_pan=80.0, w_tilt=200.0, sigma_angle=1.0)
    assert same['x'].cpu().numpy().tobytes() == got['x'].tobytes() and other['x'].cpu().numpy().tobytes() != got['x'].tobytes()
    # cov and angle_sigma against numpy
    Nf = np.zeros((6, 6)); Nf[np.triu_indices(6)] = got['N'][0]; Nf = Nf + np.triu(Nf, 1).T
    s2 = got['fvals'][0, 1] / (2 * got['counts'][0, :2].sum() - 6)
    cov = s2 * np.linalg.inv(Nf)
    assert np.allclose(got['cov'][0], cov, rtol=1e-6, atol=0)
    for f in range(8):
        fN = got['frame_N'][f]
        V, Wt = np.array([[fN[0], fN[1]], [fN[1], fN[2]]]), fN[3:15].reshape(6, 2).T
        B = np.linalg.solve(V, Wt)
        want = np.sqrt(np.diag(s2 * np.linalg.inv(V) + B @ cov @ B.T))
        assert np.allclose(got['angle_sigma'][f], want, rtol=1e-6, atol=0), f'angle_sigma of frame {f}: {got["angle_sigma"][f]} != {want}'
    # (printed, not asserted: the prior counts as data in the covariance, so a pan offset common to the frames is not covered by it)
    z = np.abs(got['angles'] - sc['true_angles']) / got['angle_sigma']
    print(f'angle errors in sigmas: {np.sort(z.reshape(-1))[::-1][:4]}; sigma {got["angle_sigma"].mean(0)} rad')
    # a frame that is not kept: NaN in the per-frame outputs, its detections refused
    ok = torch.ones(8, dtype=torch.int32, device=gpu); ok[3] = 0
    part = call(frame_ok=ok, want_res=True)
    for k in ('angles', 'frame_N', 'angle_sigma', 'frame_cyl'):
        v = part[k].cpu().numpy()
        assert np.isnan(v[3]).all() and np.isfinite(np.delete(v, 3, 0)).all(), k
    assert not part['res'][3].any() and int(part['n_used'][0]) == 7
    for kw in (dict(w_pan=0.0), dict(w_tilt=float('inf')), dict(sigma_px=-1.0), dict(sel_cos=0.05), dict(max_iter=0)):
        with pytest.raises(ValueError):
            call(**kw)


def test_run_experiment_multi_frame_joint(cpe, gpu, tmp_path):
    """the folder of test_multiframe_pixels_pipeline_gpu.py::test_run_experiment_multi_frame_pixels"""
    from PIL import Image
    from cpe_amd import experiment, synth
    b = synth.render_batch(6, H, W, seed=0, with_gt=False)
    stems = ['-10', '-21', '00', '1-2', '11', '2-1']
    L, Rr = b['left'].numpy(), b['right'].numpy()
    for i, st in enumerate(stems):
        Image.fromarray(L[i]).save(tmp_path / f'{st}L.png')
        Image.fromarray(Rr[i]).save(tmp_path / f'{st}R.png')
    lens = lambda K: dict(IntrinsicMatrix=np.asarray(K, dtype=np.float64).tolist(), RadialDistortion=[0.0, 0.0], TangentialDistortion=[0.0, 0.0])
    (tmp_path / 'cam.json').write_text(json.dumps(dict(LeftCamera=lens(b['K1']), RightCamera=lens(b['K2']))))
    args = (str(tmp_path), str(tmp_path / 'cam.json'), b['K1'], b['K2'], b['T21'], b['radius'])
    Tp = synth.make_rig(b['scene'])[3]
    tab = _ltable(cpe, gpu, TC.true_table(b['scene']), -Tp[:3, :3].T @ Tp[:3, 3])
    kw = dict(device=gpu, chunk=4, laser_table=tab, multi_frame='lm', source='fused')

    def same(a, c, what):
        if torch.is_tensor(a):
            assert torch.is_tensor(c) and a.cpu().numpy().tobytes() == c.cpu().numpy().tobytes(), f'{what} changed'
        elif isinstance(a, np.ndarray):
            assert a.tobytes() == c.tobytes(), f'{what} changed'
        elif isinstance(a, dict):
            assert set(a) == set(c)
            for k in a:
                same(a[k], c[k], f'{what}[{k}]')
        else:
            assert a == c, f'{what} changed'

    plain = experiment.run_experiment(*args, multi_frame_pixels={}, **kw)
    res = experiment.run_experiment(*args, multi_frame_pixels={}, multi_frame_joint={}, **kw)
    assert set(res) == set(plain) | {'multi_frame_joint'}
    for k in plain:
        same(plain[k], res[k], k)
    jt = res['multi_frame_joint']
    assert set(jt) == {'T_cam_agv', 'x', 'fvals', 'px_rms', 'counts', 'status', 'cov', 'frame_cyl', 'frame_stats', 'angles', 'angle_sigma'}
    F = len(res['names'])
    assert jt['angles'].shape == (F, 2) and jt['angle_sigma'].shape == (F, 2) and jt['frame_cyl'].shape == (F, 6) and jt['cov'].shape == (6, 6)
    print(f'status {jt["status"]}, counts {jt["counts"].tolist()}, px rms {float(jt["px_rms"]):.3f} (fixed angles '
          f'{float(res["multi_frame_pixels"]["px_rms"]):.3f}), fvals {jt["fvals"].tolist()}')
    assert jt['status'] == 0 and len(jt['T_cam_agv']) == 16 and float(jt['fvals'][1]) <= float(jt['fvals'][0])
    # (the folder's cylinders do not follow the file names' angles, so the fitted angles are printed, not held to the nominal ones)
    used = ~torch.isnan(jt['angles'][:, 0]).cpu().numpy()
    print(f'fitted - nominal angles of the {used.sum()} used frames: {(jt["angles"].cpu().numpy()[used] - res["angles"][used]).round(4).tolist()}')
    assert used.sum() >= 2 and torch.isfinite(jt['angle_sigma'][torch.from_numpy(used)]).all()
    # without multi_frame_pixels= it starts from the resident mode's pose
    bare = experiment.run_experiment(*args, **kw)
    alone = experiment.run_experiment(*args, multi_frame_joint=dict(sigma_angle=0.001), **kw)
    assert set(alone) == set(bare) | {'multi_frame_joint'} and alone['multi_frame_joint']['status'] == 0
    for k in bare:
        same(bare[k], alone[k], f'without multi_frame_pixels=: {k}')
    for bad in (dict(source='stereo', multi_frame='lm'), dict(source='fused', multi_frame=True, laser_table=tab),
                dict(source='left', multi_frame='nm', laser_table=tab)):
        with pytest.raises(ValueError):
            experiment.run_experiment(*args, device=gpu, multi_frame_joint={}, **bad)
