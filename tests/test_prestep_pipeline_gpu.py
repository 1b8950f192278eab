"""Raw frames through the whole path: FramePipeline.run_raw (fused pre-step into the lane's staging pairs, detect in place,
fit) against FramePipeline.run on the frames the separate Undistorter(cubic) produces, and experiment.run_experiment on a
folder of <pan><tilt>L.png / R.png files against the direct calls.  Records are compared bit for bit."""
import json

import numpy as np
import pytest

H, W, F = 480, 640, 6
STRONG = dict(RadialDistortion=[0.21, 0.05], TangentialDistortion=[-0.0011, 0.0009],
              IntrinsicMatrix=[[0.8 * W, 0.3, W / 2 + 1.3], [0, 0.81 * W, H / 2 + 0.9], [0, 0, 1.0]])
# fx = fy = 512 and half-integer principal points: distortPoints is exact, the map is the identity to the last bit
IDENT = dict(RadialDistortion=[0.0, 0.0], TangentialDistortion=[0.0, 0.0], IntrinsicMatrix=[[512.0, 0, 320.5], [0, 512.0, 240.5], [0, 0, 1.0]])


def mild(K):
    """a lens the detector still works behind (as in test_undistort.py::test_gpu_undistort_feeds_detect)"""
    return dict(IntrinsicMatrix=np.asarray(K, dtype=np.float64).tolist(), RadialDistortion=[0.012, -0.004], TangentialDistortion=[0.0002, -0.0001])


@pytest.fixture(scope='module')
def scene(gpu):
    import torch
    from cpe_amd import synth
    b = synth.render_batch(F, H, W, seed=0, with_gt=False)
    b['left'], b['right'] = b['left'].to(gpu).contiguous(), b['right'].to(gpu).contiguous()
    torch.cuda.synchronize()
    return b


def make_pipe(b, **kw):
    from cpe_amd import pipeline
    return pipeline.FramePipeline(H, W, b['K1'], b['K2'], b['T21'], b['radius'], device='cuda:0', **dict(dict(chunk=4), **kw))


def undistorted(cam_l, cam_r, left, right):
    from cpe_amd import iotool
    return (iotool.Undistorter(cam_l, H, W, 'cuda:0', interp='cubic')(left), iotool.Undistorter(cam_r, H, W, 'cuda:0', interp='cubic')(right))


@pytest.fixture(scope='module')
def strong_ref(scene):
    """records of run() on the separately undistorted frames: the reference of every run_raw variant, computed once"""
    import torch
    cam_r = dict(STRONG, RadialDistortion=[0.19, 0.04])
    ul, ur = undistorted(STRONG, cam_r, scene['left'], scene['right'])
    rec = make_pipe(scene).run(ul, ur).cpu().numpy()
    torch.cuda.synchronize()
    return cam_r, rec


def eq(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))      # bit for bit (NaN included)


@pytest.mark.gpu
def test_run_raw_equals_run_on_undistorted_frames(scene, strong_ref):
    import torch
    from cpe_amd import iotool
    cam_r, want = strong_ref
    pre = iotool.StereoPrestep(STRONG, cam_r, H, W, 'cuda:0')
    L, R = scene['left'], scene['right']
    pipe = make_pipe(scene)
    assert eq(pipe.run_raw(L, R, pre).cpu().numpy(), want)
    assert pipe._stage[0].shape == (4, 2, H, W)                                              # one staging tensor per lane, reused
    u16 = lambda t: (t.to(torch.int32) * 257).to(torch.int16)                                # the uint16 bit pattern of 257 v
    assert eq(pipe.run_raw(u16(L), u16(R), pre).cpu().numpy(), want)
    rgb = lambda t: t[..., None].expand(-1, -1, -1, 3).contiguous()
    assert eq(pipe.run_raw(rgb(L), R.to(torch.float32) / 255, pre).cpu().numpy(), want)      # the cameras may differ
    assert eq(make_pipe(scene, lanes=2, chunk=2).run_raw(L, R, pre).cpu().numpy(), want)
    assert eq(make_pipe(scene, chunk=F).run_raw(L, R, pre).cpu().numpy(), want)


@pytest.mark.gpu
def test_zero_distortion_run_raw_equals_run(scene):
    import torch
    from cpe_amd import iotool, pipeline
    pre = iotool.StereoPrestep(IDENT, IDENT, H, W, 'cuda:0')
    yy, xx = np.mgrid[0:H, 0:W]
    assert np.array_equal(pre.maps[0].cpu().numpy(), np.stack([xx, yy], -1).astype(np.float32))
    L, R = scene['left'], scene['right']
    want = make_pipe(scene).run(L, R).cpu().numpy()
    _, _, st_fit, st_l, st_r = (t.tolist() for t in pipeline.unpack_counters(torch.from_numpy(want[:, 15])))
    assert sum(1 for a, b, c in zip(st_fit, st_l, st_r) if a == b == c == 0) >= 2, 'the scene must hold frames that are fitted'
    assert eq(make_pipe(scene).run_raw(L, R, pre).cpu().numpy(), want)


@pytest.fixture(scope='module')
def folder(scene, tmp_path_factory):
    """the frames as <pan><tilt>L.png / R.png; sorted stems: -10 -21 00 1-2 11 2-1 3-3.  '00' is a 16-bit pair (257 v), '11' an
    RGB pair with equal channels, '3-3' all black."""
    from PIL import Image
    d = tmp_path_factory.mktemp('laser_cylinder')
    stems = ['-10', '-21', '00', '1-2', '11', '2-1']
    L, R = scene['left'].cpu().numpy(), scene['right'].cpu().numpy()
    for i, s in enumerate(stems):
        for side, a in (('L', L[i]), ('R', R[i])):
            if s == '00':
                a = a.astype(np.uint16) * 257
            elif s == '11':
                a = np.repeat(a[..., None], 3, -1)
            Image.fromarray(a).save(d / f'{s}{side}.png')
    for side in 'LR':
        Image.fromarray(np.zeros((H, W), np.uint8)).save(d / f'3-3{side}.png')
    (d / 'notes.txt').write_text('not an image')
    cams = dict(LeftCamera=mild(scene['K1']), RightCamera=mild(scene['K2']))
    (d / 'cam.json').write_text(json.dumps(cams))
    return d, stems + ['3-3'], cams


@pytest.mark.gpu
def test_run_experiment(scene, folder, tmp_path):
    import torch
    from scipy.io import loadmat
    from cpe_amd import experiment, iotool, multiframe, pipeline
    d, stems, cams = folder
    b = scene
    mat = tmp_path / 'frames.mat'
    res = experiment.run_experiment(str(d), str(d / 'cam.json'), b['K1'], b['K2'], b['T21'], b['radius'], chunk=4, mat_path=str(mat))
    # the direct calls: separate undistortion, one chunk, the fit tables of run_chunk
    black = torch.zeros((1, H, W), dtype=torch.uint8, device='cuda')
    ul, ur = undistorted(cams['LeftCamera'], cams['RightCamera'], torch.cat([b['left'], black]), torch.cat([b['right'], black]))
    rec, det, out = make_pipe(b, chunk=F + 1).run_chunk(ul, ur)
    assert res['names'] == stems == experiment.unique_names(str(d))
    assert np.array_equal(res['angles'], np.deg2rad([[-1, 0], [-2, 1], [0, 0], [1, -2], [1, 1], [2, -1], [3, -3]]))
    assert eq(res['records'].cpu().numpy(), rec.cpu().numpy())
    assert torch.equal(res['pts3'], out['pts3']) and torch.equal(res['cnt'], out['m'])
    # the black pair is skipped with its statuses, and only it and the frames that failed
    n_pts, _, st_fit, st_l, st_r = (t.cpu().tolist() for t in pipeline.unpack_counters(rec[:, 15]))
    want_skipped = [dict(index=i, name=stems[i], det_left=st_l[i], det_right=st_r[i], fit=st_fit[i]) for i in range(F + 1) if st_l[i] or st_r[i] or st_fit[i]]
    assert res['skipped'] == want_skipped and res['skipped'][-1]['index'] == F and res['skipped'][-1]['det_left'] != 0
    good = [i for i in range(F + 1) if i not in {s['index'] for s in want_skipped}]
    assert len(good) >= 2, 'the scene must hold frames that are fitted'
    g = torch.tensor(good, device='cuda')
    mf = multiframe.fit_multi_frame(out['pts3'][g], out['m'][g], out['cyl_raw'][g], res['angles'][good], b['radius'])
    assert res['T_cam_agv'] == mf['T'] and res['fval'] == mf['fvals'][1] and len(res['T_cam_agv']) == 16
    m = loadmat(str(mat))
    assert [str(x[0][0]) for x in m['names']] == stems and m['frames'].shape == (1, F + 1)
    cyl = out['cyl'].cpu().numpy()
    for i in range(F + 1):
        assert np.array_equal(m['frames'][0, i]['cylParams'], cyl[i].reshape(2, 6)) and m['frames'][0, i]['pts3'].shape == (3, n_pts[i])
    # without the multi-frame fit
    res2 = experiment.run_experiment(str(d), str(d / 'cam.json'), b['K1'], b['K2'], b['T21'], b['radius'], chunk=3, multi_frame=False)
    assert res2['T_cam_agv'] is None and res2['fval'] is None and eq(res2['records'].cpu().numpy(), rec.cpu().numpy())


@pytest.mark.gpu
def test_run_experiment_missing_partner(scene, folder):
    """a left image without its right one: the reference fails in imread, here FileNotFoundError names the file"""
    from PIL import Image
    from cpe_amd import experiment
    d, _, _ = folder
    p = d / 'xxL.png'
    Image.fromarray(np.zeros((H, W), np.uint8)).save(p)
    try:
        with pytest.raises(FileNotFoundError, match='xxR.png'):
            experiment.run_experiment(str(d), str(d / 'cam.json'), scene['K1'], scene['K2'], scene['T21'], scene['radius'])
    finally:
        p.unlink()
