"""Planar target on true-colour frames, the parts that need no GPU: the tinting helpers and the oracle composition the GPU
tests compare against (tests/plane_colour_oracle.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plane_colour_oracle as PC  # noqa: E402


def test_tint_helpers():
    rng = np.random.default_rng(0)
    g = np.tile(np.arange(256, dtype=np.uint8), (8, 1))
    bgr = PC.tint(g, rng)
    assert bgr.dtype == np.uint8 and bgr.shape == (8, 256, 3)
    lit = (g >= 200) & (g < 245)
    assert (bgr[..., 2][lit] > bgr[..., 1][lit]).all() and (bgr[..., 1][lit] > bgr[..., 0][lit]).all()   # R strong, G and B weak
    assert (bgr[g >= 245] == g[g >= 245][:, None]).all()                                                  # white bloom
    red = PC.red_laser(g, rng)
    assert red[..., :2][g < 245].max() <= 10 and red[..., 2].max() == 255 and (red[g >= 245] == 255).all()
    m = PC.any_channel_mask(np.array([[[0, 0, 128], [127, 127, 127], [200, 0, 0], [0, 128, 0]]], np.uint8))
    assert m.tolist() == [[255, 0, 255, 255]]


@pytest.mark.parametrize('h,w,seed', [(600, 800, 3), (483, 650, 9)])
def test_composition_is_the_oracle_on_grey_replicated_frames(orc, h, w, seed):
    """the restated chain with the colour looks swapped in gives S.detect_grid_plane exactly when B = G = R"""
    from oracle import stages as S
    frames = PC.plane_frames(h, w, 1, seed)
    for g in frames:
        ref = S.detect_grid_plane(g, debug=True)
        got = PC.detect_grid_plane_bgr(np.repeat(g[..., None], 3, 2))
        assert got['status'] == ref['status'] == 0
        assert got['rect'] == tuple(ref['rect']) and got['r0'] == ref['r0']
        assert np.array_equal(got['mask_contour'], ref['mask_contour'])
        assert (got['n_rows'], got['n_cols']) == (ref['n_rows'], ref['n_cols'])
        assert np.array_equal(got['xy'], ref['xy']) and np.array_equal(got['id'], ref['id'])
        assert np.array_equal(got['center'], ref['center'])


def test_red_laser_needs_the_colour_hull(orc):
    """on a red-only laser the luma (about 0.3 R) stays under 127 except at the white spot: the grey chain finds a hull around
    the spot only and a handful of points, the colour composition the whole grid"""
    from oracle import stages as S
    g = PC.plane_frames(600, 800, 1, 3)[0]
    bgr = PC.red_laser(g, np.random.default_rng(4))
    col = PC.detect_grid_plane_bgr(bgr)
    lum = S.detect_grid_plane(S.bgr2gray(bgr))
    assert col['status'] == 0 and len(col['xy']) >= 60
    assert lum['status'] != 0 or len(lum['xy']) < len(col['xy']) // 4
