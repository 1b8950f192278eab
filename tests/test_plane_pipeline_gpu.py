"""The planar target end to end: FramePipeline(target='plane') against oracle planar detect -> oracle.choose_idx ->
oracle.triangulate -> the numpy fit of tests/plane_fit_cases.py; experiment.run_plane_experiment against its layers called by
hand; and the default target of both against the code paths they had before the planar target existed."""
import functools
import json

import numpy as np
import pytest
import torch

import plane_fit_cases as PC

pytestmark = pytest.mark.gpu

H, W = 480, 640
# The planar detector numbers the columns of the two images of these boards in opposite directions (tests/test_plane_gpu.py pins it
# to the oracle, not to truth), so equal indices are not the same grid point and the triangulated points lie millimetres off any
# plane: the band is wide.  What is compared here is the chain, not the board.
TAU = 12.0


@functools.lru_cache(maxsize=None)
def _boards(n=2, seed=2):
    """true-plane stereo frames on which the oracle's planar detector ends in status 0 for every image (asserted where used)"""
    from cpe_amd import synth
    return synth.render_batch(n, H, W, seed=seed, scene=synth.Scene(h=H, w=W, target='plane', tilt_deg=4.0), with_gt=False)


@functools.lru_cache(maxsize=None)
def _cylinders():
    from cpe_amd import synth
    return synth.render_batch(2, H, W, seed=0, with_gt=False)


def test_plane_pipeline_against_the_oracle_chain(cpe, orc, gpu):
    from oracle import stages as S
    from cpe_amd import pipeline
    b = _boards()
    pipe = pipeline.FramePipeline(H, W, b['K1'], b['K2'], b['T21'], 0.0, chunk=2, device=gpu, target='plane', plane=dict(tau=TAU))
    rec, det, out = pipe.run_chunk(b['left'].to(gpu), b['right'].to(gpu))
    torch.cuda.synchronize()
    rec = rec.cpu().numpy()
    got = {k: out[k].cpu().numpy() for k in ('P', 'T', 'grid', 'stats', 'n_inliers', 'inlier_mask', 'plane_flags', 'status', 'm', 'pts3',
                                             'idx', 'mean_err')}
    L, R = b['left'].numpy(), b['right'].numpy()
    for i in range(2):
        a, c = S.detect_grid_plane(L[i]), S.detect_grid_plane(R[i])
        assert a['status'] == 0 and c['status'] == 0
        assert int(det['status'][i]) == 0 and int(det['status'][2 + i]) == 0
        c1, c2, idx, _ = orc.choose_idx(np.concatenate([a['xy'], a['id']], 1), np.concatenate([c['xy'], c['id']], 1), b['K1'], b['K2'], b['T21'])
        X, err = orc.triangulate(c1, c2, b['K1'], b['K2'], b['T21'])
        m = int(got['m'][i])
        assert m == len(X) and m >= 20
        assert np.array_equal(got['idx'][i, :m], idx) and np.array_equal(got['pts3'][i, :m], X)
        ref = PC.ref_fit_plane(X, idx, m, TAU, 4)
        print(f'frame {i}: m {m} inliers {ref["n_inliers"]} refits {ref["stats"][6]:.0f} rms {ref["stats"][0]:.3f} margin {ref["margin"]:.2e} '
              f'tol {ref["tol_angle"]:.2e} {ref["tol_off"]:.2e} {ref["tol_grid"]:.2e}')
        assert ref['status'] == 0 and ref['margin'] > 1e-6 and ref['spread_margin'] > 1e-6
        g = dict(P=got['P'][i], T=got['T'][i], grid=got['grid'][i], stats=got['stats'][i], n_inliers=got['n_inliers'][i],
                 mask=got['inlier_mask'][i], flags=got['plane_flags'][i], status=got['status'][i])
        PC.compare_fit(g, ref, f'frame {i}')
        # the record is the fit's outputs in the layout stated beside pipeline.REC
        want = np.concatenate([g['P'], g['T'][:3, 3], g['T'][:3, 0], [np.linalg.norm(g['grid'][1]), np.linalg.norm(g['grid'][2])],
                               g['stats'][:2], [got['mean_err'][i]]])
        assert np.array_equal(rec[i, :10], want[:10]) and np.allclose(rec[i, 10:12], want[10:12], rtol=8 * PC.EPS, atol=0)      # (a norm of three terms: a few ulp between two libraries)
        assert np.array_equal(rec[i, 12:15], want[12:15])
        assert abs(got['mean_err'][i] - err.sum() / m) <= m * PC.EPS * err.max()               # (two summation orders of m terms)
    n_pts, refits, st, st_l, st_r = (t.cpu().tolist() for t in pipeline.unpack_counters(torch.from_numpy(rec[:, 15])))
    assert n_pts == got['m'].tolist() and refits == got['stats'][:, 6].astype(int).tolist() and st == [0, 0] and st_l == [0, 0] and st_r == [0, 0]


def test_plane_pipeline_refuses_the_cylinder_s_options(cpe, gpu):
    from cpe_amd import pipeline
    b = _boards()
    args = (H, W, b['K1'], b['K2'], b['T21'], 45.0)
    for kw in (dict(target='plane', match={}), dict(target='plane', ransac={}), dict(target='sphere'), dict(plane=dict(tau=1.0))):
        with pytest.raises(ValueError):
            pipeline.FramePipeline(*args, device=gpu, **kw)
    fits = pipeline.alloc_fits(3, gpu, 'plane')
    assert fits['P'].shape == (3, 4) and fits['inlier_mask'].shape == (3, PC.MAXP) and fits['idx'].dtype == torch.int32
    assert set(pipeline.alloc_fits(3, gpu)) == set(pipeline.FIT_OUTPUTS) and 'cyl' not in fits


def test_default_target_records_are_bit_identical(cpe, gpu):
    from cpe_amd import pipeline
    b = _cylinders()
    args = (H, W, b['K1'], b['K2'], b['T21'], b['radius'])
    left, right = b['left'].to(gpu), b['right'].to(gpu)
    plain = pipeline.FramePipeline(*args, chunk=2, device=gpu).run(left, right)
    named = pipeline.FramePipeline(*args, chunk=2, device=gpu, target='cylinder', plane=None).run(left, right)
    torch.cuda.synchronize()
    assert torch.equal(plain.view(torch.int64), named.view(torch.int64))
    _, _, st, st_l, st_r = pipeline.unpack_counters(plain[:, 15])
    assert st.tolist() == [0, 0] and st_l.tolist() == [0, 0] and st_r.tolist() == [0, 0]
    # and they are the layers called by hand: detect, fit_single_cylinder_batch
    det = cpe.api.detect_grid_batch(torch.cat([left, right]))
    g1 = cpe.fit.GridTables(det['xy'][:2], det['id'][:2], det['n'][:2]); g2 = cpe.fit.GridTables(det['xy'][2:], det['id'][2:], det['n'][2:])
    out = cpe.fit.fit_single_cylinder_batch(g1, g2, b['K1'], b['K2'], b['T21'], b['radius'])
    assert torch.equal(plain[:, 0:12].reshape(2, 2, 6), out['cyl']) and torch.equal(plain[:, 12:14], out['fvals'])


def _folder(tmp_path, b, stems):
    from PIL import Image
    L, R = b['left'].numpy(), b['right'].numpy()
    for i, st in enumerate(stems):
        Image.fromarray(L[i]).save(tmp_path / f'{st}L.png')
        Image.fromarray(R[i]).save(tmp_path / f'{st}R.png')
    lens = lambda K: dict(IntrinsicMatrix=np.asarray(K, dtype=np.float64).tolist(), RadialDistortion=[0.0, 0.0], TangentialDistortion=[0.0, 0.0])
    (tmp_path / 'cam.json').write_text(json.dumps(dict(LeftCamera=lens(b['K1']), RightCamera=lens(b['K2']))))
    return str(tmp_path), str(tmp_path / 'cam.json'), b['K1'], b['K2'], b['T21']


def _by_hand(cpe, gpu, args, stems, fits, **pipe_kw):
    """the read / upload loop as run_experiment had it before the helper, for one chunk of one image kind"""
    from cpe_amd import experiment, iotool, pipeline
    folder, cam = args[:2]
    cam_l, cam_r = iotool.load_camera_data(cam)
    names = sorted(stems)
    imgs = [(experiment.read_raw_image(f'{folder}/{s}L.png'), experiment.read_raw_image(f'{folder}/{s}R.png')) for s in names]
    pre = iotool.StereoPrestep(cam_l, cam_r, H, W, gpu)
    pipe = pipeline.FramePipeline(H, W, *args[2:], chunk=len(names), device=gpu, **pipe_kw)
    left = torch.from_numpy(np.stack([p[0] for p in imgs])).to(gpu)
    right = torch.from_numpy(np.stack([p[1] for p in imgs])).to(gpu)
    return names, pipe.run_raw(left, right, pre, fits)


def test_run_plane_experiment_equals_its_layers(cpe, gpu, tmp_path):
    from PIL import Image
    from cpe_amd import experiment, pipeline
    stems = ['b0', 'b1', 'b2', 'b3']
    args = _folder(tmp_path, _boards(4, 2), stems)
    for side in 'LR':
        Image.fromarray(np.zeros((H, W), np.uint8)).save(tmp_path / f'zz{side}.png')            # a black pair: skipped
    # these boards are the case the entry point warns about: the planes miss their common point by centimetres
    with pytest.warns(UserWarning, match='grid numbering of the two images probably disagrees'):
        res = experiment.run_plane_experiment(*args, tau=TAU, device=gpu, chunk=3)
    assert res['consistent'] is False and float(res['table']['centre'][3]) > experiment.PLANE_CENTRE_RMS_WARN
    fits = pipeline.alloc_fits(5, gpu, 'plane')
    names, recs = _by_hand(cpe, gpu, args + (0.0,), stems + ['zz'], fits, target='plane', plane=dict(tau=TAU, max_rounds=4))
    torch.cuda.synchronize()
    assert res['names'] == names and torch.equal(res['records'].view(torch.int64), recs.view(torch.int64))
    for k, f in (('P', 'P'), ('T', 'T'), ('grid', 'grid'), ('stats', 'stats'), ('pts3', 'pts3'), ('idx', 'idx'), ('cnt', 'm'),
                 ('n_inliers', 'n_inliers'), ('inlier_mask', 'inlier_mask'), ('plane_flags', 'plane_flags')):
        assert res[k].cpu().numpy().tobytes() == fits[f].cpu().numpy().tobytes(), k
    assert [s['index'] for s in res['skipped']] == [4] and res['skipped'][0]['name'] == 'zz' and fits['status'].tolist()[:4] == [0] * 4
    ok = torch.tensor([1, 1, 1, 1, 0], dtype=torch.int32, device=gpu)
    used = (fits['inlier_mask'][:4] != 0).cpu().numpy()
    ids = fits['idx'][:4].cpu().numpy()[used]
    tab = res['table']
    assert (tab['lo'], tab['hi']) == (int(ids.min()), int(ids.max()))
    hand = cpe.fit.index_planes_batch(fits['pts3'], fits['idx'], fits['m'], tab['lo'], tab['hi'], use=fits['inlier_mask'], frame_ok=ok)
    for k in ('P', 'stats', 'count', 'frames', 'status', 'centre', 'centre_status'):
        assert tab[k].cpu().numpy().tobytes() == hand[k].cpu().numpy().tobytes(), k
    X, I, cnt, use = (fits[k].cpu().numpy() for k in ('pts3', 'idx', 'm', 'inlier_mask'))
    ref = PC.ref_index_planes(X, I, cnt, tab['lo'], tab['hi'], use, ok.cpu().numpy())
    assert ref['spread_margin'] > 1e-6 and (ref['status'] == 0).sum() >= 4
    PC.compare_index_planes({k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in tab.items()}, ref, 'table')


def test_run_plane_experiment_without_a_good_frame(cpe, gpu, tmp_path):
    from PIL import Image
    from cpe_amd import experiment
    b = _boards()
    args = _folder(tmp_path, b, [])
    for side in 'LR':
        Image.fromarray(np.zeros((H, W), np.uint8)).save(tmp_path / f'zz{side}.png')
    with pytest.warns(UserWarning, match='no fitted frame'):
        res = experiment.run_plane_experiment(*args, device=gpu)
    assert res['table'] is None and res['consistent'] is False and [s['index'] for s in res['skipped']] == [0] and not res['P'].any()


def test_run_experiment_is_unchanged_by_the_shared_loop(cpe, gpu, tmp_path):
    from cpe_amd import experiment, pipeline
    stems = ['-10', '01']
    b = _cylinders()
    args = _folder(tmp_path, b, stems) + (b['radius'],)
    res = experiment.run_experiment(*args, device=gpu, chunk=1, multi_frame=False)
    assert set(res) == {'names', 'angles', 'records', 'pts3', 'cnt', 'cyl_raw', 'skipped', 'T_cam_agv', 'fval'}
    fits = pipeline.alloc_fits(2, gpu)
    names, recs = _by_hand(cpe, gpu, args, stems, fits)
    torch.cuda.synchronize()
    assert res['names'] == names == ['-10', '01'] and res['skipped'] == [] and res['T_cam_agv'] is None
    assert np.array_equal(res['angles'], np.deg2rad([[-1.0, 0.0], [0.0, 1.0]]))
    assert torch.equal(res['records'].view(torch.int64), recs.view(torch.int64))
    for k, f in (('pts3', 'pts3'), ('cnt', 'm'), ('cyl_raw', 'cyl_raw')):
        assert res[k].cpu().numpy().tobytes() == fits[f].cpu().numpy().tobytes(), k
