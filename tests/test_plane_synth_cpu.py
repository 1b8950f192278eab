"""cpe_amd.synth with Scene(target='plane'): the board renders, its ground truth lies on the board and projects where the lines
cross; the default target still returns the bytes it returned before the planar target existed."""
import hashlib

import numpy as np
import pytest

import plane_fit_cases as PC


def test_default_target_is_bit_identical():
    from cpe_amd import synth
    b = synth.render_batch(2, 480, 640, seed=0)
    assert b['scene'].target == 'cylinder' and 'plane_n' not in b and 'Tp' not in b
    # sha1 of left + right and of the ground truth of this call, recorded on the commit before Scene.target
    assert hashlib.sha1(b['left'].numpy().tobytes() + b['right'].numpy().tobytes()).hexdigest() == '9781ce9fdd0e684e26be3618805df4188ee429fc'
    assert sum(len(g['X']) for g in b['gt']) == 127 and set(b['gt'][0]) == {'idx', 'X', 'uv1', 'uv2'}
    with pytest.raises(ValueError):
        synth.Scene(target='sphere')


def test_plane_renders_with_its_ground_truth():
    from cpe_amd import synth
    sc = synth.Scene(h=480, w=640, target='plane', tilt_deg=20.0)
    b = synth.render_batch(2, 480, 640, seed=4, scene=sc)
    assert b['left'].shape == (2, 480, 640) and b['left'].dtype.is_floating_point is False
    assert np.array_equal(b['Tp'], synth.make_rig(sc)[3]) and b['plane_n'].shape == (2, 3) and b['plane_d'].shape == (2,)
    for i, g in enumerate(b['gt']):
        n, d = b['plane_n'][i], b['plane_d'][i]
        assert np.array_equal(g['n'], n) and g['d'] == d and n[2] > 0 and abs(np.linalg.norm(n) - 1) < 1e-15
        assert len(g['X']) >= 70 and np.abs(g['X'] @ n - d).max() < 1e-10                      # the intersections lie on the board
        assert abs(b['axis_org'][i] @ n - d) < 1e-10
        r = PC.ref_fit_plane(g['X'], g['idx'], len(g['X']))
        assert PC.angle(r['P'][:3], n) < 1e-12 and abs(r['P'][3] + d) < 1e-9
        # the rendered lines cross at the projected intersections: brighter there than the frame's median by far
        for img, uv in ((b['left'][i].numpy(), g['uv1']), (b['right'][i].numpy(), g['uv2'])):
            at = img[np.rint(uv[:, 1]).astype(int), np.rint(uv[:, 0]).astype(int)].astype(float)
            assert np.median(at) > np.median(img) + 100
    # the board is flat: every row of intersections is straight in 3-D
    g = b['gt'][0]
    row = g['X'][g['idx'][:, 1] == 0]
    assert len(row) >= 5 and np.linalg.svd(row - row.mean(0), compute_uv=False)[1] < 1e-9
