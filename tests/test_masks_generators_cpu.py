"""CPU: the masks-stage generators (tests/masks_cases.py) put in front of the kernels what they are named for, checked with
the oracle alone -- so that a passing tests/test_masks_stage_gpu.py means something.  Also: the oracle's joint filter
against detect_grid, and scipy restatements of the openings against the oracle."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import masks_cases as M  # noqa: E402
from masks_cases import scipy_open20, scipy_open3, spot_mask  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _fragments(mask):
    """vertex counts of the external contours of the expansion's base = close3x3(roi)"""
    from oracle import stages as S
    return [len(p) for p, _ in S.find_contours(S.close_rect(mask, 3, 3), 'external', 'simple')]


def test_joint_filter_matches_detect_grid(orc):
    """stages.joints_in_rect is the filter orc_detect.c applies: its count is detect_grid's n_cyl_joints on the golden and
    rendered frames"""
    from oracle import stages as S
    from cpe_amd import synth
    z = np.load(os.path.join(GOLDEN, 'indexing.npz'))
    frames = [z[k] for k in z.files if k.startswith('img_')] + [np.load(os.path.join(GOLDEN, 'subpixel.npz'))['gray']]
    b = synth.render_batch(2, 480, 640, seed=1, with_gt=False)
    frames += list(b['left'].numpy()) + list(b['right'].numpy())
    seen = 0
    for g in frames:
        ref = S.detect_grid(g, debug=True)
        if ref['status'] == 1:
            continue
        assert len(S.joints_in_rect(ref['joints'], ref['rect'])) == ref['n_cyl_joints']
        assert len(ref['joints']) == ref['n_joints']
        seen += ref['n_cyl_joints'] > 0
    assert seen >= 4


def test_expand_dbg_reports_median_and_longest(orc):
    """the dbg of expand_line_roi: the f32 bits of the median angle and the longest length, 0 without valid fragments"""
    from oracle import stages as S
    c = M.get('fan_odd')
    ref = M.oracle(c)
    nc, nv, gang, glen = ref['seg_h']
    assert nv == 17 and nc >= nv
    assert np.float32(np.uint32(glen).view(np.float32)) > 60
    assert abs(float(np.uint32(gang).view(np.float32))) < 1 or abs(abs(float(np.uint32(gang).view(np.float32))) - 180) < 1
    _, dbg = S.expand_line_roi(np.zeros((64, 64), np.uint8), np.zeros((64, 64), np.uint8), 101)
    assert dbg == (0, 0, 0, 0)


@pytest.mark.parametrize('name', sorted(M.CASES))
def test_scipy_restatements_agree_with_the_oracle(orc, name):
    """hmask / vmask (20-tap openings) and roi (3x3 opening of mask & spot & mask_contour) by scipy equal the oracle's"""
    c = M.get(name)
    ref = M.oracle(c)
    assert np.array_equal(scipy_open20(c['binary'], True), ref['hmask'])
    assert np.array_equal(scipy_open20(c['binary'], False), ref['vmask'])
    if ref['status'] == 0:
        cm = spot_mask(c, ref['spot'], False)
        for key, m in (('roi_h', ref['hmask']), ('roi_v', ref['vmask'])):
            assert np.array_equal(scipy_open3(m & cm & c['mc']), ref[key]), key


def test_run_generators_reach_word_and_band_edges(orc):
    from oracle import stages as S
    c = M.get('runs_h')
    hm, _, _ = S.extract_joints(c['binary'])
    w = c['binary'].shape[1]
    runs = []
    for y in range(c['binary'].shape[0]):
        xs = np.flatnonzero(c['binary'][y])
        if len(xs):
            runs.append((len(xs), int(xs[0]), int(xs[-1]) + 1, bool(hm[y].any())))
    for L in M.RUN_LENS:
        assert {x0 % 64 for n, x0, x1, _ in runs if n == L} >= set(range(42, 64)) | {0, 1}    # every offset before a word edge
        # 19 goes, 20 and 21 stay -- except at the frame edges, where the border neither erodes nor dilates
        assert all(kept == (L >= 20) for n, x0, x1, kept in runs if n == L and x0 > 0 and x1 < w)
        assert all(kept for n, x0, x1, kept in runs if n == L and (x0 == 0 or x1 == w))
        assert any(x0 == 0 for n, x0, x1, _ in runs if n == L) and any(x1 == w for n, x0, x1, _ in runs if n == L)
    w = c['binary'].shape[1]
    assert c['binary'][:, 0].any() and c['binary'][:, w - 1].any()
    for h in (192, 193, 255):
        c = M.get(f'runs_v_{h}')
        assert c['binary'].shape[0] == h and c['binary'][0].any() and c['binary'][h - 1].any()
        ys = {int(np.flatnonzero(c['binary'][:, x])[0]) for x in range(c['binary'].shape[1]) if c['binary'][:, x].any()}
        assert {64 + d for d in range(-22, 21)} <= ys
    c = M.get('runs_v_bands32')                   # w > 2880: k_open20_joints<32>, bands of 32 rows
    assert c['binary'].shape == (128, 2881)
    ys = {int(np.flatnonzero(c['binary'][:, x])[0]) for x in range(2881) if c['binary'][:, x].any()}
    assert {32 + d for d in range(-22, 21)} | {64 + d for d in range(-22, 21)} <= ys


def test_joint_generators(orc):
    from oracle import stages as S
    c = M.get('joint_shapes')
    hm, vm, jall = S.extract_joints(c['binary'])
    jm = (hm > 0) & (vm > 0)
    cs = S.find_contours(jm, 'external', 'simple')
    areas = [S.contour_moments(p)[0] for p, _ in cs]
    assert areas.count(0) >= 2 and 1 in areas                              # zero-area joints (skipped) and a 2 x 2 one
    assert len(jall) == sum(1 for a in areas if a != 0)
    assert len(S.find_contours(jm, 'list', 'simple')) > len(cs)              # the joint in the ring's hole
    x, y, rw, rh = c['rect']
    inside = {tuple(j) for j in S.joints_in_rect(jall, c['rect'])}
    assert (x, 90) in inside and (x + rw - 1, 60) in inside and (170, y) in inside and (180, y + rh - 1) in inside
    assert not inside & {(x - 1, 125), (x + rw, 140), (130, y - 1), (140, y + rh)}
    assert any(j[0] <= 10 for j in jall) and any(j[1] >= c['binary'].shape[0] - 12 for j in jall)
    lat = M.oracle(M.get('joint_lattice'))
    assert len(lat['joints']) > M.MAXJ and lat['status'] == 0


def test_spot_generators(orc):
    from oracle import stages as S
    want = {'r0_21': 21, 'r0_22': 22, 'r0_23': 23, 'r0_29': 29, 'r0_30': 30, 'r0_85': 85, 'r0_86': 86}
    for name, r0 in want.items():
        ref = M.oracle(M.get(name))
        assert ref['status'] == 0 and ref['r0'] == r0, (name, ref['r0'])
    # round half to even: cr + 40 odd for r0 21 and 23
    assert M.oracle(M.get('r0_21'))['spot'][2:] == (40, 30) and M.oracle(M.get('r0_23'))['spot'][2:] == (42, 32)
    assert 91 + 85 == M.EXP_MAXKS
    for name in ('r0_85', 'r0_86'):                 # the expansion runs: a valid fragment no longer than 0.8 * glen
        nc, nv, gang, glen = M.oracle(M.get(name))['seg_h']
        assert nv >= 2
    assert M.oracle(M.get('plateau_no_spot'))['status'] == 2
    g = M.get('plateau_241')['gray']
    assert (S.blur19(g) > 240).any() and (g > 240).sum() > 1600 and (g == 255).any()
    assert g[:, 128 - 12:].max() == 241          # the block's tiles: every row sum <= 241 * 256, blurred 241 in the block
    one = M.oracle(M.get('one_pixel_spot'))
    assert one['spot_plane'].sum() == 1 and one['status'] == 0 and one['r0'] == 0
    eq = M.get('equal_spots')
    cs = S.find_contours(S.blur19(eq['gray']) > 240, 'external', 'simple')
    assert len(cs) == 2 and S.contour_moments(cs[0][0])[0] == S.contour_moments(cs[1][0])[0]
    cut = M.oracle(M.get('spot_cut'))
    assert cut['spot'][0] - cut['spot'][2] < 0
    tiles = M.get('spot_tiles')
    sp = S.blur19(tiles['gray']) > 240
    assert sp[0, 0] and sp[-1, -1] and sp[:, 320:].any()


def test_tall_spot_exceeds_the_row_buffer(orc):
    ref = M.oracle(M.get('spot_tall'))
    assert ref['status'] == 0 and 2 * ref['spot'][3] + 1 > M.SPOT_ROWS


def test_fragment_generators(orc):
    from oracle import stages as S
    ch = M.oracle(M.get('chamfers'))
    counts = _fragments(ch['roi_h'])
    assert {4, 5, 6, 7, 8, 15} <= set(counts), sorted(counts)
    for name, want in (('stairs_200', {199, 200, 202}),):
        assert want <= set(_fragments(M.oracle(M.get(name))['roi_h'])), name
    c = M.get('stairs_700')
    assert {699, 700, 702} <= set(_fragments(M.oracle(c, 'plane')['roi_h']))
    nest = M.oracle(M.get('nested'))
    base = S.close_rect(nest['roi_h'], 3, 3)
    assert len(S.find_contours(base, 'list', 'simple')) > len(S.find_contours(base, 'external', 'simple'))
    fan, even = M.oracle(M.get('fan_odd')), M.oracle(M.get('fan_even'))
    assert fan['seg_h'][:2] == fan['seg_v'][:2] == (17, 17) and even['seg_h'][:2] == even['seg_v'][:2] == (16, 16)
    many = M.oracle(M.get('many_fragments'))
    assert many['seg_h'][1] == 2206 > M.MAXSEG
    clip = M.get('clipped')
    ref = M.oracle(clip)
    assert ref['roi_h'][:, :8].any() and ref['roi_h'][:, -8:].any() and ref['roi_h'][:3].any()


@pytest.mark.parametrize('name,target,counts', [('counts_200', 'cylinder', (199, 200, 201, 202)),
                                                ('counts_plane', 'plane', (7, 8, 9, 699, 700, 701, 702))])
def test_vertex_limits_on_both_sides(orc, name, target, counts):
    """one fragment at every vertex count next to the limits of expand_line_roi's window: 200 / 700 in, 201 / 701 out; 8 in,
    7 out; the valid count is exactly the ones inside"""
    ref = M.oracle(M.get(name), target)
    got = sorted(n for n, _, _ in M.fragment_table(ref['roi_h']))
    assert got == sorted(counts), got
    lo, hi = (5, 200) if target == 'cylinder' else (8, 700)
    assert ref['seg_h'][1] == sum(lo <= c <= hi for c in counts)


@pytest.mark.parametrize('target', ['cylinder', 'plane'])
def test_angle_tie_is_exact(orc, target):
    """a fragment whose float32 angle is exactly 5.0f from the float32 median, and it is expanded (len <= 0.8 * glen)"""
    ref = M.oracle(M.get('angle_tie'), target)
    nc, nv, gang_bits, glen_bits = ref['seg_h']
    gang = np.uint32(gang_bits).view(np.float32)
    glen = np.uint32(glen_bits).view(np.float32)
    frags = M.fragment_table(ref['roi_h'])
    assert nv == len(frags) == 3
    assert gang == M.f32_angle(41, 7) and glen == M.f32_length(199, 3)
    tie = [(a, ln) for _, a, ln in frags if np.abs(np.float32(a - gang)) == np.float32(5.0)]
    assert len(tie) == 1 and tie[0][0] == M.f32_angle(103, 27)
    assert float(tie[0][1]) <= 0.8 * float(glen)


@pytest.mark.parametrize('target', ['cylinder', 'plane'])
def test_length_tie_is_exact(orc, target):
    """a fragment whose float32 length is exactly 0.8 * glen in double: the `len > 0.8 * glen` test is false, it is expanded"""
    ref = M.oracle(M.get('length_tie'), target)
    nc, nv, gang_bits, glen_bits = ref['seg_h']
    glen = np.uint32(glen_bits).view(np.float32)
    assert nv == 2 and glen == M.f32_length(35, 5)
    lens = sorted(float(ln) for _, _, ln in M.fragment_table(ref['roi_h']))
    assert lens[0] == 0.8 * float(glen) and lens[0] == float(M.f32_length(28, 4))
    # the expanded fragment adds pixels: the tie decides the output
    assert (ref['exp_h'] > ref['roi_h']).any()
