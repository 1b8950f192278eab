"""Planar target (python_grid_detection_plane.py, row f-2) on true-colour frames, GPU vs the oracle composition of
tests/plane_colour_oracle.py.  The reference reads the colour planes twice on this path: get_convex_hull thresholds every
channel (util_plane.py:2590-2689) and indexing_data blurs every channel 7x7 (util_plane.py:1334-1336); the rest works on
BGR2GRAY of the frame.  Where each part is checked:
    mask_contour / rect           == S.get_convex_hull(255 * (max(B,G,R) > 127), 127, 5)        test_colour_hull_plane
    blur7 plane (tiles written)   == S.bgr2gray(S.blur7 per channel)                             test_colour_blur_plane
    status, centre, ids, xy       == PC.detect_grid_plane_bgr (the oracle's planar chain, stage by stage, on the grey image,
                                     with the two colour steps above swapped in)                  test_colour_end_to_end"""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plane_colour_oracle as PC  # noqa: E402

SIZES = [(600, 800, 3), (483, 650, 9), (1200, 1920, 5)]


def _tinted(h, w, seed, n=2):
    """n frames per view, left views then right views, tinted red with white spots"""
    rng = np.random.default_rng(seed + 100)
    return np.stack([PC.tint(g, rng) for g in PC.plane_frames(h, w, n, seed)])


@pytest.mark.gpu
@pytest.mark.parametrize('h,w,seed', SIZES)
def test_colour_hull_plane(cpe, orc, gpu, h, w, seed):
    """the region stage thresholds the any-channel mask, not the luma: mask_contour and rect equal the reference's colour hull,
    which on these frames differs from the luma hull on a real share of the pixels"""
    from oracle import stages as S
    frames = _tinted(h, w, seed)
    det = cpe.api.detect_grid_batch(torch.from_numpy(frames).to(gpu), target='plane')
    torch.cuda.synchronize()
    mc = det['ws'].plane('mask_contour').cpu().numpy()
    state = det['ws'].state()
    for i, bgr in enumerate(frames):
        st, want, rect = PC.colour_hull(bgr)
        assert st == 0
        assert np.array_equal(mc[i], want), (i, int((mc[i] != want).sum()))
        assert (state[i]['rect0'], state[i]['rect1'], state[i]['rect2'], state[i]['rect3']) == rect, i
        _, luma, _ = S.get_convex_hull(S.bgr2gray(bgr))
        assert (luma != want).mean() > 0.05, (i, (luma != want).mean())


@pytest.mark.gpu
@pytest.mark.parametrize('h,w,seed', SIZES)
def test_colour_blur_plane(cpe, orc, gpu, h, w, seed):
    """the 7x7 blur of indexing_data is taken per channel, then converted: on every tile the call writes (the skip rule of
    the grey blur: tiles within the largest indexing window of the region rectangle)"""
    frames = _tinted(h, w, seed)
    det = cpe.api.detect_grid_batch(torch.from_numpy(frames).to(gpu), target='plane')
    torch.cuda.synchronize()
    g7 = det['ws'].plane('blur7').cpu().numpy()
    state = det['ws'].state()
    checked = 0
    for i, bgr in enumerate(frames):
        if int(det['status'][i]) != 0:
            continue
        s = state[i]
        m = PC.blur7_written(h, w, (s['rect0'], s['rect1'], s['rect2'], s['rect3']), s['r0'])
        want = PC.colour_gauss7(bgr)
        assert np.array_equal(g7[i][m], want[m]), (i, int((g7[i][m] != want[m]).sum()))
        assert m.mean() > 0.2
        checked += 1
    assert checked >= 2


def _assert_matches(det, i, ref, tag):
    assert int(det['status'][i]) == ref['status'], (tag, int(det['status'][i]), ref['status'])
    if ref['status'] != 0:
        return
    m = int(det['n'][i])
    assert m == len(ref['xy']), (tag, m, len(ref['xy']))
    assert np.array_equal(det['id'][i, :m].cpu().numpy(), ref['id']), tag
    assert np.array_equal(det['center'][i].cpu().numpy(), ref['center']), tag
    got = det['xy'][i, :m].cpu().numpy()
    assert np.array_equal(got, ref['xy']), (tag, np.abs(got - ref['xy']).max())


@pytest.mark.gpu
@pytest.mark.parametrize('h,w,seed', SIZES)
def test_colour_end_to_end(cpe, orc, gpu, h, w, seed):
    frames = _tinted(h, w, seed)
    det = cpe.api.detect_grid_batch(torch.from_numpy(frames).to(gpu), target='plane')
    torch.cuda.synchronize()
    state = det['ws'].state()
    n_ok = 0
    for i, bgr in enumerate(frames):
        ref = PC.detect_grid_plane_bgr(bgr)
        _assert_matches(det, i, ref, f'frame {i}')
        if ref['status'] == 0:
            assert (state[i]['n_rows'], state[i]['n_cols']) == (ref['n_rows'], ref['n_cols'])
            assert state[i]['r0'] == ref['r0']
            n_ok += 1
            assert len(ref['xy']) >= 60
    assert n_ok >= 3


@pytest.mark.gpu
def test_red_laser_rig(cpe, orc, gpu):
    """a red-only laser (G, B <= 10) with a white spot: the colour entry finds the grid; converting to luma first (the
    behaviour before the planar target took colour frames) leaves only the spot above 127, so the hull is the spot's and the
    grid small or absent"""
    from oracle import stages as S
    rng = np.random.default_rng(21)
    frames = np.stack([PC.red_laser(g, rng) for g in PC.plane_frames(600, 800, 1, 3)])
    assert frames[..., :2][frames[..., 2] < 255].max() <= 10
    dev = torch.from_numpy(frames).to(gpu)
    det = cpe.api.detect_grid_batch(dev, target='plane')
    grey = cpe.api.bgr_to_gray(dev)
    old = cpe.api.detect_grid_batch(grey, target='plane')
    torch.cuda.synchronize()
    for i, bgr in enumerate(frames):
        ref = PC.detect_grid_plane_bgr(bgr)
        assert ref['status'] == 0 and len(ref['xy']) >= 60
        _assert_matches(det, i, ref, f'colour {i}')
        lum = S.detect_grid_plane(S.bgr2gray(bgr))
        _assert_matches(old, i, lum, f'luma {i}')
        assert int(old['status'][i]) != 0 or int(old['n'][i]) < len(ref['xy']) // 4, (int(old['status'][i]), int(old['n'][i]))


@pytest.mark.gpu
@pytest.mark.parametrize('h,w,seed', [(600, 800, 3), (483, 650, 9)])
def test_grey_replicated_colour_is_the_grey_path(cpe, orc, gpu, h, w, seed):
    g = PC.plane_frames(h, w, 1, seed)
    a = cpe.api.detect_grid_batch(torch.from_numpy(np.repeat(g[..., None], 3, 3)).to(gpu), target='plane')
    pa = {k: a['ws'].plane(k).cpu().numpy() for k in ('binary', 'hmask', 'vmask', 'mask_contour', 'roi_h', 'roi_v', 'exp_h', 'exp_v')}
    sa = a['ws'].state()
    b = cpe.api.detect_grid_batch(torch.from_numpy(g).to(gpu), target='plane')
    torch.cuda.synchronize()
    sb = b['ws'].state()
    for k, v in pa.items():
        assert np.array_equal(v, b['ws'].plane(k).cpu().numpy()), k
    assert sa == sb
    assert (a['status'] == 0).all() and torch.equal(a['status'], b['status']) and torch.equal(a['n'], b['n'])
    assert torch.equal(a['xy'], b['xy']) and torch.equal(a['id'], b['id']) and torch.equal(a['center'], b['center'])


@pytest.mark.gpu
def test_colour_planar_argument_checks(cpe, orc, gpu):
    import ctypes as C
    L = cpe.lib.load()
    frames = torch.from_numpy(_tinted(483, 650, 9, n=1)).to(gpu)
    with pytest.raises(Exception):
        cpe.api.detect_grid_batch(frames, target='plane', subpixel=True)
    n, h, w = 1, 128, 128
    ws = cpe.api.DetectWorkspace(n, h, w, gpu)
    buf = torch.zeros(n * h * w * 3 + 4, dtype=torch.uint8, device=gpu)
    outs = [torch.zeros((n, 4096, 2), dtype=torch.float64, device=gpu), torch.zeros((n, 4096, 2), dtype=torch.int32, device=gpu),
            torch.zeros(n, dtype=torch.int32, device=gpu), torch.zeros((n, 2), dtype=torch.float64, device=gpu),
            torch.zeros(n, dtype=torch.int32, device=gpu)]
    for prm, off in ((cpe.lib.CpeDetectParams(0, 7, 1.0, 1, 0), 1), (cpe.lib.CpeDetectParams(1, 7, 1.0, 1, 0), 0)):
        rc = L.cpe_detect_grid_bgr_batch_ex(buf.data_ptr() + off, n, h, w, C.addressof(prm), ws.view.data_ptr(), ws.bytes,
                                            *[t.data_ptr() for t in outs], torch.cuda.current_stream().cuda_stream)
        assert rc != 0, (off, prm.subpixel)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_plane_folder_colour(cpe, orc, gpu, tmp_path):
    """process_images_in_folder on tinted 3-channel PNGs: camera JSON -> per-channel undistortion -> colour planar detect_grid;
    the JSON equals the oracle composition on the undistorted BGR frame"""
    import importlib
    from PIL import Image
    import oracle
    frames = _tinted(600, 800, 3, n=1)
    K = [[1240.0, 0, 400.0], [0, 1240.0, 300.0], [0, 0, 1]]
    dist = [0.01, -0.003, 0.0002, -0.0001]
    cam = dict(IntrinsicMatrix=K, RadialDistortion=dist[:2], TangentialDistortion=dist[2:])
    (tmp_path / 'cam.json').write_text(json.dumps(dict(LeftCamera=cam, RightCamera=cam)))
    src = tmp_path / 'in'; src.mkdir()
    Image.fromarray(np.ascontiguousarray(frames[0][..., ::-1])).save(src / 'img_L_000.png')       # PNG holds RGB
    Image.fromarray(np.ascontiguousarray(frames[1][..., ::-1])).save(src / 'img_R_000.png')
    mod = importlib.import_module('python_grid_detection_plane')
    res = json.loads(mod.process_images_in_folder(str(tmp_path / 'cam.json'), str(src), str(tmp_path / 'out')))
    assert set(res) == {'img_L_000', 'img_R_000'}
    for name, bgr in (('img_L_000', frames[0]), ('img_R_000', frames[1])):
        und = np.stack([oracle.undistort(np.ascontiguousarray(bgr[..., c]), np.array(K), np.array(dist)) for c in range(3)], 2)
        ref = PC.detect_grid_plane_bgr(und)
        pts = res[name]['points']
        assert ref['status'] == 0 and len(pts) == len(ref['xy']) >= 60, name
        assert [p['id'] for p in pts] == ref['id'].tolist(), name
        assert np.array_equal(np.array([[p['x'], p['y']] for p in pts]), ref['xy']), name
        assert res[name]['center_point'] == ref['center'].tolist(), name
