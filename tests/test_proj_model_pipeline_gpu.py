"""experiment.run_experiment(projector=...): the projector model fitted to the cylinder experiment's own stereo points, against
its layers called by hand, against the oracle chain of tests/proj_model_cases.py, and against the scene's true laser planes.

Measured on the oracle chain (oracle detect, match_offset_cases.reference, chooseIdx, triangulate, ref_projector_model with
tau = 1 mm) for synth.render_batch(8, 480, 640, seed=3): 592 residuals on the lines -4..6, no refit, model rms 0.0461 mm; the
table for the lines -6..6 is 0.0741 deg and 0.1196 mm (the true centre's distance from a plane) off TC.true_table(scene) at the
worst.  TABLE_BOUND is twice that.  Without the index search the oracle chain leaves 9 pairs in frame 1, whose left image is
numbered one column off; two refits trim all 9 residuals of either family and no other."""
import functools
import json

import numpy as np
import pytest
import torch

import proj_model_cases as M
import table_tri_cases as TC

pytestmark = pytest.mark.gpu

H, W, SEED, F = 480, 640, 3, 8
TAU = 1.0
TABLE_BOUND = dict(normal_deg=2 * 0.0741, offset_mm=2 * 0.1196)
STEMS = [f'0{i}' for i in range(F)]


@functools.lru_cache(maxsize=None)
def _scene():
    from cpe_amd import synth
    return synth.render_batch(F, H, W, seed=SEED)


def _folder(tmp_path, b):
    from PIL import Image
    L, R = b['left'].numpy(), b['right'].numpy()
    for i, st in enumerate(STEMS):
        Image.fromarray(L[i]).save(tmp_path / f'{st}L.png')
        Image.fromarray(R[i]).save(tmp_path / f'{st}R.png')
    lens = lambda K: dict(IntrinsicMatrix=np.asarray(K, dtype=np.float64).tolist(), RadialDistortion=[0.0, 0.0], TangentialDistortion=[0.0, 0.0])
    (tmp_path / 'cam.json').write_text(json.dumps(dict(LeftCamera=lens(b['K1']), RightCamera=lens(b['K2']))))
    return str(tmp_path), str(tmp_path / 'cam.json'), b['K1'], b['K2'], b['T21'], b['radius']


def _by_hand(cpe, gpu, args, match):
    """the layers under run_experiment: read, pre-step, FramePipeline.run_raw -> records, the fits with the points' indices"""
    from cpe_amd import experiment, iotool, pipeline
    cam_l, cam_r = iotool.load_camera_data(args[1])
    raw = [torch.from_numpy(np.stack([experiment.read_raw_image(f'{args[0]}/{s}{side}.png') for s in STEMS])).to(gpu) for side in 'LR']
    pre = iotool.StereoPrestep(cam_l, cam_r, H, W, gpu)
    fits = pipeline.alloc_fits(F, gpu)
    fits['idx'] = torch.zeros((F, cpe.fit.MAXP, 2), dtype=torch.int32, device=gpu)
    pipe = pipeline.FramePipeline(H, W, *args[2:], chunk=F, device=gpu, match=match)
    rec = pipe.run_raw(raw[0], raw[1], pre, fits)
    torch.cuda.synchronize()
    return rec, fits


def test_run_experiment_projector_equals_its_layers_and_the_oracle_chain(cpe, orc, gpu, tmp_path):
    from cpe_amd import experiment
    b = _scene()
    args = _folder(tmp_path, b)
    path = str(tmp_path / 'model_table.npz')
    res = experiment.run_experiment(*args, device=gpu, chunk=3, multi_frame=False, match_offset={}, projector=dict(tau=TAU), table_path=path)
    plain = experiment.run_experiment(*args, device=gpu, chunk=3, multi_frame=False, match_offset={})
    torch.cuda.synchronize()
    # the option adds two keys and changes nothing else
    assert set(res) == set(plain) | {'projector', 'projector_shifted'}
    for k in plain:
        if isinstance(plain[k], torch.Tensor):
            assert res[k].cpu().numpy().tobytes() == plain[k].cpu().numpy().tobytes(), k
    assert res['skipped'] == [] and res['projector_shifted'] == []
    assert res['offset'][:, 0].tolist() == [0, -1, 0, 0, 0, 0, 0, 0]        # the index search re-numbers frame 1
    # its layers by hand
    rec, out = _by_hand(cpe, gpu, args, {})
    assert torch.equal(res['records'].view(torch.int64), rec.view(torch.int64))
    pm = res['projector']
    ok = torch.ones(F, dtype=torch.int32, device=gpu)
    lo, hi = pm['fit']['lo'], pm['fit']['hi']
    ids = torch.cat([out['idx'][i, :int(out['m'][i])] for i in range(F)])
    assert (lo, hi) == (int(ids.min()), int(ids.max()))
    hand = cpe.fit.fit_projector_model(out['pts3'], out['idx'], out['m'], lo, hi, frame_ok=ok, tau=TAU)
    for k in ('model', 'info', 'moments', 'count', 'frames', 'inlier_mask', 'frame_counts'):
        assert pm['fit'][k].cpu().numpy().tobytes() == hand[k].cpu().numpy().tobytes(), k
    n = max(abs(lo), abs(hi))
    tab = cpe.fit.ProjectorModel.from_fit(hand).table(-n, n)
    saved = cpe.fit.LaserTable.load(path, gpu)
    for t in (pm['laser_table'], saved):
        assert (t.lo, t.hi, t.family0) == (-n, n, 'col') and torch.equal(t.P, tab.P) and torch.equal(t.status, tab.status)
    # the oracle chain: the same counts exactly, the same model at the reference's tolerance
    ref = M.oracle_chain(orc, b, match=True, tau=TAU)
    assert (ref['lo'], ref['hi']) == (lo, hi) and ref['status'] == 0 and ref['margin'] > 1e-6 and ref['tol'] <= 1e-6
    info = hand['info'].cpu().numpy()
    assert info[0] == 0 and info[1] == ref['rounds'] and info[4:6].tolist() == ref['kept'].tolist()
    assert np.array_equal(hand['frame_counts'].cpu().numpy(), ref['frame_counts'])
    x = hand['model'].cpu().numpy()[:15]
    # (the pipeline's points are the oracle's to ~1e-10 mm, TC's pipeline test; the optimum moves by about as much)
    assert np.abs(x - ref['x']).max() <= ref['tol'] + 1e-8, f'model {np.abs(x - ref["x"]).max():.3e} > {ref["tol"] + 1e-8:.3e}'
    # truth
    deg, mm = M.table_errors(tab.P.cpu().numpy(), -n, TC.true_table(b['scene']))
    print(f'lines {lo}..{hi}, table -{n}..{n}: {deg:.4f} deg, {mm:.4f} mm off the true planes; model rms {pm["model"].rms:.4f} mm')
    assert deg <= TABLE_BOUND['normal_deg'] and mm <= TABLE_BOUND['offset_mm']


def test_projector_off_changes_nothing(cpe, gpu, tmp_path):
    from cpe_amd import experiment
    b = _scene()
    args = _folder(tmp_path, b)
    a = experiment.run_experiment(*args, device=gpu, chunk=4, multi_frame=False)
    c = experiment.run_experiment(*args, device=gpu, chunk=4, multi_frame=False, projector=None, table_path=None)
    assert set(a) == set(c) == {'names', 'angles', 'records', 'pts3', 'cnt', 'cyl_raw', 'skipped', 'T_cam_agv', 'fval'}
    for k in ('records', 'pts3', 'cnt', 'cyl_raw'):
        assert a[k].cpu().numpy().tobytes() == c[k].cpu().numpy().tobytes(), k
    _, out = _by_hand(cpe, gpu, args, None)
    assert a['pts3'].cpu().numpy().tobytes() == out['pts3'].cpu().numpy().tobytes()
    with pytest.raises(ValueError):
        experiment.run_experiment(*args, device=gpu, projector={}, source='left')


def test_without_the_index_search_the_shifted_frame_is_named(cpe, gpu, tmp_path):
    from cpe_amd import experiment
    b = _scene()
    args = _folder(tmp_path, b)
    res = experiment.run_experiment(*args, device=gpu, chunk=8, multi_frame=False, projector=dict(tau=TAU))
    assert res['projector_shifted'] == [1]
    fc = res['projector']['fit']['frame_counts'].cpu().numpy()
    assert not fc[1, [0, 2]].any() and (fc[1, [1, 3]] > 0).all() and not np.delete(fc, 1, 0)[:, [1, 3]].any()
    assert res['projector']['model'].status == 0
    deg, mm = M.table_errors(res['projector']['laser_table'].P.cpu().numpy(), res['projector']['laser_table'].lo, TC.true_table(b['scene']))
    print(f'frame 1 trimmed: {deg:.4f} deg, {mm:.4f} mm')
    # without the band the same frame spoils the model: the band is what protects it
    bad = experiment.run_experiment(*args, device=gpu, chunk=8, multi_frame=False, projector={})
    assert bad['projector_shifted'] == [] and bad['projector']['model'].rms > 10 * res['projector']['model'].rms


def test_run_plane_experiment_projector(cpe, gpu, tmp_path):
    """rendered boards (whose two images the planar detector numbers differently): the option adds its two
    keys and nothing else changes; the model is the layers' by hand; `consistent` follows the model's rms"""
    import warnings
    from PIL import Image
    from cpe_amd import experiment, pipeline, synth
    b = synth.render_batch(4, H, W, seed=2, scene=synth.Scene(h=H, w=W, target='plane', tilt_deg=4.0), with_gt=False)
    for i in range(4):
        Image.fromarray(b['left'][i].numpy()).save(tmp_path / f'b{i}L.png')
        Image.fromarray(b['right'][i].numpy()).save(tmp_path / f'b{i}R.png')
    lens = lambda K: dict(IntrinsicMatrix=np.asarray(K, dtype=np.float64).tolist(), RadialDistortion=[0.0, 0.0], TangentialDistortion=[0.0, 0.0])
    (tmp_path / 'cam.json').write_text(json.dumps(dict(LeftCamera=lens(b['K1']), RightCamera=lens(b['K2']))))
    args = (str(tmp_path), str(tmp_path / 'cam.json'), b['K1'], b['K2'], b['T21'])
    path = str(tmp_path / 'pm_table.npz')
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        plain = experiment.run_plane_experiment(*args, device=gpu)
        res = experiment.run_plane_experiment(*args, device=gpu, projector=dict(tau=TAU), table_path=path)
    assert set(res) == set(plain) | {'projector', 'projector_shifted'}
    for k in ('records', 'P', 'T', 'pts3', 'idx', 'cnt', 'inlier_mask'):
        assert res[k].cpu().numpy().tobytes() == plain[k].cpu().numpy().tobytes(), k
    assert plain['table'] is not None and res['table']['P'].cpu().numpy().tobytes() == plain['table']['P'].cpu().numpy().tobytes()
    pm = res['projector']
    assert pm is not None and isinstance(res['projector_shifted'], list)
    F4 = len(res['names'])
    _, _, d_fit, d_l, d_r = pipeline.unpack_counters(res['records'][:, 15])
    ok = ((d_fit == 0) & (d_l == 0) & (d_r == 0)).to(torch.int32)
    hand = cpe.fit.fit_projector_model(res['pts3'], res['idx'], res['cnt'], pm['fit']['lo'], pm['fit']['hi'], use=res['inlier_mask'],
                                       frame_ok=ok, tau=TAU)
    for k in ('model', 'info', 'inlier_mask', 'frame_counts'):
        assert pm['fit'][k].cpu().numpy().tobytes() == hand[k].cpu().numpy().tobytes(), k
    assert F4 == 4 and pm['model'].family0 == 'row' and res['laser_table'] is pm['laser_table']
    saved = cpe.fit.LaserTable.load(path, gpu)
    assert saved.family0 == 'row' and torch.equal(saved.P, pm['laser_table'].P)
    assert res['consistent'] == (pm['model'].status == 0 and pm['model'].rms <= experiment.PLANE_CENTRE_RMS_WARN)
    print(f'boards: model status {pm["model"].status} rms {pm["model"].rms:.3f} mm, consistent {res["consistent"]}, shifted {res["projector_shifted"]}')
