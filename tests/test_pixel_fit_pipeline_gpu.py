"""The pixel fit in the Python layers: fit.fit_single_cylinder_pixels_batch against its layers bit for bit; the pixels= keyword of
the refined and the one-camera calls, of FramePipeline (chunks of one and two rendered 480 x 640 frames with the scene's true
table) and of experiment.run_experiment against their layers; the refusals; and every path without the keyword as it was."""
import json

import numpy as np
import pytest
import torch

import grid_predict_cases as G
import pixel_fit_cases as X
import plane_fit_cases as PC
import table_tri_cases as TC

pytestmark = pytest.mark.gpu

H, W = 480, 640
POSE_KEYS = ('cyl_raw', 'cyl', 'T')
PIX_KEYS = ('cyl', 'fvals', 'iters', 'counts', 'stats', 'status', 'res', 'pt_state', 'X')
FLAT = ('pixels_taken', 'pixels_fvals', 'pixels_stats', 'pixels_counts', 'pixels_status')


def _ltable(cpe, gpu, t, centre, family0='col'):
    return cpe.fit.LaserTable(torch.from_numpy(t['P']).to(gpu), torch.from_numpy(t['status'].astype(np.int32)).to(gpu), t['lo'], t['hi'],
                              torch.from_numpy(np.concatenate([centre, [0.0]])).to(gpu), torch.zeros(1, dtype=torch.int32, device=gpu), family0)


def _same(a, b, keys, what):
    for k in keys:
        assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), f'{what}: {k} differs'


def _tables(cpe, gpu):
    """four frames: three seeds of the cylinder frame (the last with a third of each image missing) and one without detections"""
    mats1, mats2 = [], []
    for s in range(3):
        idx, _, uv1, uv2 = TC.cylinder_frame(0.25, s)
        g1, g2 = np.concatenate([uv1, idx], 1), np.concatenate([uv2, idx], 1)
        if s == 2:
            g1, g2 = X.third_missing(g1, 0, 0), X.third_missing(g2, 0, 1)
        mats1.append(g1); mats2.append(g2)
    mats1.append(np.zeros((0, 4))); mats2.append(np.zeros((0, 4)))
    GT = cpe.fit.GridTables
    return GT.from_lists(mats1, gpu), GT.from_lists(mats2, gpu)


def test_single_cylinder_pixels_equals_its_layers(cpe, gpu):
    fit, K = cpe.fit, PC.rig()[:3]
    gp1, gp2 = _tables(cpe, gpu)
    tab = _ltable(cpe, gpu, TC.rig_table(G.LO, G.HI), PC.rig()[5])
    out = fit.fit_single_cylinder_pixels_batch(gp1, gp2, *K, tab, X.RADIUS)
    start = fit.fit_single_cylinder_fused_batch(gp1, gp2, *K, tab, X.RADIUS, mode=fit.FIT_LM)
    px = fit.fit_cylinder_pixels_batch(gp1, gp2, start['cyl'][:, 1].contiguous(), X.RADIUS, *K, tab, use=start['status'] == 0,
                                       want=('res', 'pt_state', 'X'))
    torch.cuda.synchronize()
    _same(out['start'], start, ('cyl_raw', 'cyl', 'T', 'fvals', 'iters', 'status', 'pts3', 'm'), 'the start')
    _same(out['pixels'], px, PIX_KEYS, 'the pixel fit')
    assert out['status'].tolist() == [0, 0, 0, 5] and px['status'].tolist() == [0, 0, 0, 5] and out['taken'].tolist() == [True, True, True, False]
    raw, cyl, T = (out[k].cpu().numpy() for k in POSE_KEYS)
    Xn, used = px['X'].cpu().numpy().reshape(4, -1, 3), px['pt_state'].cpu().numpy().reshape(4, -1) == 0
    for f in range(3):
        assert np.array_equal(raw[f, 0], start['cyl'][f, 1].cpu().numpy()) and np.array_equal(raw[f, 1], px['cyl'][f].cpu().numpy())
        ymin = Xn[f][used[f]][:, 1].min()
        for r in range(2):                                          # applyCylParamsPrior with the nodes' points
            o, d = raw[f, r, :3], raw[f, r, 3:] * (1 if raw[f, r, 4] >= 0 else -1)
            want = np.concatenate([o + (ymin - o[1]) / d[1] * d, d])
            assert np.abs(cyl[f, r] - want).max() <= 8 * X.EPS * np.abs(want).max(), f'frame {f} row {r}: the prior'
        assert abs(cyl[f, 1, 1] - ymin) <= 8 * X.EPS * abs(ymin) + 1e-12 and cyl[f, 1, 4] > 0
        y = cyl[f, 1, 3:] / np.linalg.norm(cyl[f, 1, 3:])
        assert np.abs(T[f, :3, 1] - y).max() < 1e-15 and np.abs(T[f, :3, 3] - cyl[f, 1, :3]).max() == 0 and T[f, 3].tolist() == [0, 0, 0, 1]
        assert np.abs(T[f, :3, :3] @ T[f, :3, :3].T - np.eye(3)).max() < 1e-14 and abs(T[f, 0, 2]) < 1e-15       # z = (1, 0, 0) x y
        deg0, mm0 = TC.axis_errors(start['cyl'][f, 1].cpu().numpy())
        deg, mm = TC.axis_errors(cyl[f, 1])
        print(f'frame {f}: start {deg0:.4f} deg {mm0:.4f} mm, pixel fit {deg:.4f} deg {mm:.4f} mm, {px["iters"][f].tolist()} iterations, '
              f'{px["stats"][f, 2]:.3f} px rms')
        bd, bm = X.ACCURACY_BOUNDS['rig']['third' if f == 2 else 'all']          # (recorded for the oracle chain's start; the fused start is no worse)
        assert deg <= bd and mm <= bm
    _same({k: out[k][3:] for k in POSE_KEYS}, {k: start[k][3:] for k in POSE_KEYS}, POSE_KEYS, 'the frame without a fit')
    # a pixel fit that is not ST_OK (everything gated) leaves the start's result, bit for bit
    none = fit.fit_single_cylinder_pixels_batch(gp1, gp2, *K, tab, X.RADIUS, start=start, gate_px=1e-9)
    torch.cuda.synchronize()
    assert not none['taken'].any() and none['pixels']['status'].tolist() == [5] * 4 and (none['pixels']['counts'][:3, 3] > 250).all()
    _same(none, start, POSE_KEYS, 'nothing taken')
    with pytest.raises(ValueError):
        fit.fit_single_cylinder_pixels_batch(gp1, None, *K, tab, X.RADIUS)                      # the default start needs both cameras
    with pytest.raises(ValueError):
        fit.fit_single_cylinder_pixels_batch(gp1, gp2, *K, tab, X.RADIUS, want=('res',))


def test_pixels_keyword_of_the_refined_and_the_mono_calls(cpe, gpu):
    fit, K = cpe.fit, PC.rig()[:3]
    sc = [G.scenario(name, 0) for name in ('off_by_one', 'column_shift')]
    GT = fit.GridTables
    gp1, gp2 = GT.from_lists([s['gp1'] for s in sc], gpu), GT.from_lists([s['gp2'] for s in sc], gpu)
    tab = _ltable(cpe, gpu, TC.rig_table(G.LO, G.HI), PC.rig()[5])
    plain = fit.fit_single_cylinder_refined_batch(gp1, gp2, *K, tab, X.RADIUS)
    none = fit.fit_single_cylinder_refined_batch(gp1, gp2, *K, tab, X.RADIUS, pixels=None)
    pol = fit.fit_single_cylinder_refined_batch(gp1, gp2, *K, tab, X.RADIUS, pixels=dict(gate_px=4.0))
    hand = fit.polish_with_pixels(plain, plain['tables1'], plain['tables2'], *K, tab, X.RADIUS, dict(gate_px=4.0))
    torch.cuda.synchronize()
    keys = ('cyl_raw', 'cyl', 'T', 'fvals', 'iters', 'status', 'pts3', 'idx', 'm', 'mean_err', 'round_taken', 'renumbered')
    _same(plain, none, keys, 'pixels=None')
    assert 'pixels' not in plain and 'pixels' not in none
    _same(pol, hand, keys + FLAT, 'refined, pixels=')
    _same(pol['pixels'], hand['pixels'], PIX_KEYS, 'refined, pixels=')
    _same(pol, plain, tuple(k for k in keys if k not in POSE_KEYS), 'what the polish leaves alone')
    assert pol['pixels_taken'].all() and pol['round_taken'].tolist() == [2, 2]
    for f, name in enumerate(('off_by_one', 'column_shift')):
        deg, mm = TC.axis_errors(pol['cyl'][f, 1].cpu().numpy())
        print(f'{name}: refined {TC.axis_errors(plain["cyl"][f, 1].cpu().numpy())}, polished {(deg, mm)}, counts {pol["pixels_counts"][f].tolist()}')
        assert deg <= G.REFINE_BOUNDS[name]['axis_deg'] and mm <= G.REFINE_BOUNDS[name]['axis_mm']
    # one camera: either camera's tables, the other camera absent
    idx, _, uv1, uv2 = TC.cylinder_frame(0.25, 1)
    for cam, uv in ((1, uv1), (2, uv2)):
        g = GT.from_lists([np.concatenate([uv, idx], 1)], gpu)
        Kc, Tc = TC.camera(cam)
        plain = fit.fit_single_cylinder_mono_batch(g, Kc, Tc, tab, X.RADIUS, mode=fit.FIT_LM)
        pol = fit.fit_single_cylinder_mono_batch(g, Kc, Tc, tab, X.RADIUS, mode=fit.FIT_LM, pixels={})
        px = fit.fit_cylinder_pixels_batch(g if cam == 1 else None, g if cam == 2 else None, plain['cyl'][:, 1].contiguous(), X.RADIUS, *K, tab,
                                           use=plain['status'] == 0, want=('res', 'pt_state', 'X'))
        torch.cuda.synchronize()
        mk = ('fvals', 'iters', 'status', 'pts3', 'idx', 'm', 'counts', 'res', 'src', 'stats', 'mean_err')
        _same(pol, plain, mk, f'camera {cam}: what the polish leaves alone')
        _same(pol['pixels'], px, PIX_KEYS, f'camera {cam}: the pixel fit')
        assert pol['pixels_taken'].all() and pol['pixels_counts'][0, cam - 1] > 400 and pol['pixels_counts'][0, 2 - cam] == 0
        assert torch.equal(pol['cyl_raw'][:, 1], px['cyl']) and 'pixels' not in plain


def _scene():
    from cpe_amd import synth
    b = synth.render_batch(8, H, W, seed=3)
    Tp = synth.make_rig(b['scene'])[3]
    return b, TC.true_table(b['scene']), -Tp[:3, :3].T @ Tp[:3, 3]


def _folder(tmp_path, b, stems):
    from PIL import Image
    L, R = b['left'].numpy(), b['right'].numpy()
    for i, st in enumerate(stems):
        Image.fromarray(L[i]).save(tmp_path / f'{st}L.png')
        Image.fromarray(R[i]).save(tmp_path / f'{st}R.png')
    lens = lambda K: dict(IntrinsicMatrix=np.asarray(K, dtype=np.float64).tolist(), RadialDistortion=[0.0, 0.0], TangentialDistortion=[0.0, 0.0])
    (tmp_path / 'cam.json').write_text(json.dumps(dict(LeftCamera=lens(b['K1']), RightCamera=lens(b['K2']))))
    return str(tmp_path), str(tmp_path / 'cam.json'), b['K1'], b['K2'], b['T21'], b['radius']


def test_pipeline_and_experiment_with_pixels(cpe, gpu, tmp_path):
    from cpe_amd import experiment, iotool, pipeline
    fit = cpe.fit
    b, t, centre = _scene()
    tab = _ltable(cpe, gpu, t, centre)
    args = (H, W, b['K1'], b['K2'], b['T21'], b['radius'])
    left, right = b['left'][:4].to(gpu), b['right'][:4].to(gpu)
    for kw in (dict(source='fused'), dict(source='fused', refine={}), dict(source='left'), dict(source='right')):
        kw = dict(kw, laser_table=tab, fit_mode=fit.FIT_LM)
        plain = pipeline.FramePipeline(*args, chunk=2, device=gpu, **kw)
        pol = pipeline.FramePipeline(*args, chunk=2, device=gpu, pixels={}, **kw)
        assert pol.mode == plain.mode                                    # a step after the mode's fit, no mode of its own
        r0, _, o0 = plain.run_chunk(left[:2], right[:2])
        r1, _, o1 = pol.run_chunk(left[:2], right[:2])
        if kw['source'] == 'fused':
            hand = fit.polish_with_pixels(o0, o0.get('tables1'), o0.get('tables2'), *args[2:5], tab, args[5], {}) if 'refine' in kw else None
        one = pipeline.FramePipeline(*args, chunk=1, device=gpu, pixels={}, **kw).run(left, right)
        two = pol.run(left, right)
        torch.cuda.synchronize()
        assert 'pixels' not in o0 and torch.equal(r0[:, 12:].view(torch.int64), r1[:, 12:].view(torch.int64))
        assert torch.equal(r1[:, 0:12].reshape(2, 2, 6), o1['cyl']) and torch.equal(one.view(torch.int64), two.view(torch.int64))
        assert torch.equal(two[:2].view(torch.int64), r1.view(torch.int64))
        if kw['source'] == 'fused' and 'refine' in kw:
            _same(o1, hand, POSE_KEYS + FLAT, 'the pipeline against polish_with_pixels')
        ok = o1['status'] == 0
        assert ok.any() and torch.equal(o1['pixels_taken'], ok & (o1['pixels_status'] == 0))
        _same({k: o1[k][~o1['pixels_taken']] for k in POSE_KEYS}, {k: o0[k][~o1['pixels_taken']] for k in POSE_KEYS}, POSE_KEYS, 'not taken')
        print(f'{kw["source"]}{" refined" if "refine" in kw else ""}: status {o1["status"].tolist()}, taken {o1["pixels_taken"].tolist()}, '
              f'px rms {o1["pixels_stats"][:, 2].tolist()}, counts {o1["pixels_counts"].tolist()}')
    for kw in (dict(pixels={}), dict(pixels={}, target='plane'), dict(pixels=dict(want=('X',)), source='fused', laser_table=tab)):
        with pytest.raises(ValueError):
            pipeline.FramePipeline(*args, device=gpu, **kw)
    # run_experiment against its layers
    stems = ['-10', '01']
    fargs = _folder(tmp_path, b, stems)
    with pytest.raises(ValueError):
        experiment.run_experiment(*fargs, device=gpu, multi_frame=False, pixels={})
    res = experiment.run_experiment(*fargs, device=gpu, chunk=1, multi_frame=False, laser_table=tab, source='fused', pixels={})
    base = experiment.run_experiment(*fargs, device=gpu, chunk=1, multi_frame=False, laser_table=tab, source='fused')
    cam_l, cam_r = iotool.load_camera_data(fargs[1])
    raw = [torch.from_numpy(np.stack([experiment.read_raw_image(f'{fargs[0]}/{s}{side}.png') for s in sorted(stems)])).to(gpu) for side in 'LR']
    pre = iotool.StereoPrestep(cam_l, cam_r, H, W, gpu)
    fits = pipeline.alloc_fits(2, gpu, source='fused')
    fits.update({k: torch.zeros((2,) + shape, dtype=dt, device=gpu) for k, (shape, dt) in pipeline.PIXELS_OUTPUTS.items()})
    recs = pipeline.FramePipeline(H, W, *fargs[2:], chunk=2, device=gpu, source='fused', laser_table=tab, pixels={}).run_raw(raw[0], raw[1], pre, fits)
    torch.cuda.synchronize()
    assert torch.equal(res['records'].view(torch.int64), recs.view(torch.int64)) and 'pixels' not in base
    assert torch.equal(res['cyl_raw'], fits['cyl_raw']) and torch.equal(res['pts3'], base['pts3']) and torch.equal(res['cnt'], base['cnt'])
    assert torch.equal(res['records'][:, 12:].view(torch.int64), base['records'][:, 12:].view(torch.int64))
    want = dict(cyl=fits['cyl'][:, 1], T=fits['T'], fvals=fits['pixels_fvals'], px_rms=fits['pixels_stats'][:, 2], counts=fits['pixels_counts'],
                status=fits['pixels_status'])
    assert set(res['pixels']) == set(want)
    _same(res['pixels'], want, tuple(want), 'run_experiment(pixels={})')
    assert set(pipeline.alloc_fits(2, gpu, source='fused')) == set(pipeline.FUSED_FIT_OUTPUTS)
