"""Full detect path at frame sizes whose one-bit planes (cpe_dev.h: 64 x 8 tiles) end in partial tiles -- h % 8 != 0 and
w % 64 != 0, so the last tile row and the last tile column straddle the image edge -- against the oracle, bit for bit.
1199 x 801 takes the ballot plane writer and the byte-reading labelling walks (w % 16 != 0), 1199 x 1200 the SWAR plane
writer and the walks that read the planes."""
import numpy as np
import pytest
import torch


@pytest.mark.gpu
@pytest.mark.parametrize('h,w,seed', [(1199, 801, 31), (1199, 1200, 32), (1003, 1000, 33)])
def test_detect_partial_tiles_matches_oracle(cpe, orc, gpu, h, w, seed):
    from cpe_amd import synth
    from oracle import stages as S
    b = synth.render_batch(2, h, w, seed=seed, with_gt=False)
    frames = torch.cat([b['left'], b['right']])
    det = cpe.api.detect_grid_batch(frames.to(gpu))
    torch.cuda.synchronize()
    ws = det['ws']
    planes = {k: ws.plane(k).cpu().numpy() for k in ('roi_h', 'roi_v', 'exp_h', 'exp_v')}
    state = ws.state()
    npy = frames.numpy()
    n_ok = 0
    for i in range(npy.shape[0]):
        ref = S.detect_grid(npy[i], debug=True)
        tag = f'{h}x{w} frame {i}'
        assert int(det['status'][i]) == ref['status'], (tag, state[i], ref['status'])
        if ref['status'] == 1:
            continue
        assert (state[i]['rect0'], state[i]['rect1'], state[i]['rect2'], state[i]['rect3']) == tuple(ref['rect']), tag
        assert state[i]['n_kp'] == ref['n_keypoints'], tag
        if ref['status'] == 2:
            continue
        assert state[i]['n_joints'] == ref['n_cyl_joints'], tag
        for k in planes:
            assert np.array_equal(planes[k][i], ref[k]), (tag, k)
        if ref['status'] != 0:
            continue
        n_ok += 1
        m = int(det['n'][i])
        assert m == len(ref['xy']), tag
        assert np.array_equal(det['id'][i, :m].cpu().numpy(), ref['id']), tag
        assert np.array_equal(det['center'][i].cpu().numpy(), ref['center']), tag
        assert np.array_equal(det['xy'][i, :m].cpu().numpy(), ref['xy']), tag
    assert n_ok >= 1
