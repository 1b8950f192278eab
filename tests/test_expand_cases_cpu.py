"""CPU, oracle only: the generators of tests/expand_cases.py put in front of the expansion kernels what they are named for,
so that a passing tests/test_expand_direct_gpu.py means something."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import expand_cases as E  # noqa: E402
import masks_cases as M  # noqa: E402

_REF = {}


def oracle(key, make, target='cylinder'):
    if (key, target) not in _REF:
        c = make()
        _REF[(key, target)] = (c, M.oracle(c, target))
    return _REF[(key, target)]


def _expanded(ref, key):
    """fragments of a mask that the expansion handles: valid ones no longer than 0.8 x the longest"""
    from oracle import stages as S
    glen = np.uint32(ref['seg_' + key][3]).view(np.float32)
    n = 0
    for p1, p2, nv in E.end_points(ref['roi_' + key]):
        if 5 <= nv <= 200:
            d = np.float32(p2[0] - p1[0]), np.float32(p2[1] - p1[1])
            n += not (float(M.f32_length(*d)) > 0.8 * float(glen))
    return n


@pytest.mark.parametrize('notch', [False, True])
def test_polygon_contour_cuts_expansion_and_closing(orc, notch):
    """under the polygon the expanded masks differ from those under the full rectangle, both at pixels the expansion adds
    and at pixels the closing adds; with the notch, base sticks out of mask_contour"""
    from oracle import stages as S
    c, ref = oracle(('polygon', notch), lambda: E.gen_polygon(notch))
    cf, full = oracle(('polygon full', notch), lambda: E.full_rect(E.gen_polygon(notch)))
    assert ref['status'] == 0 and full['status'] == 0
    assert set(np.unique(c['mc'])) == {0, 255} and (c['mc'] != cf['mc']).any()
    for key in ('h', 'v'):
        base_full = S.close_rect(full['roi_' + key], 3, 3)
        closing = (base_full != 0) & (full['roi_' + key] == 0)
        expansion = (full['exp_' + key] != 0) & (base_full == 0)
        diff = ref['exp_' + key] != full['exp_' + key]
        assert (diff & closing).any(), (key, 'closing pixels')
        assert (diff & expansion).any(), (key, 'expansion pixels')
        assert ref['seg_' + key][1] >= 6, (key, ref['seg_' + key])
        # the polygon's edge runs through expansion supports: pixels the expansion adds next to pixels it may not add
        added = (ref['exp_' + key] != 0) & (S.close_rect(ref['roi_' + key], 3, 3) == 0)
        assert added.sum() > 500, (key, int(added.sum()))
        base = S.close_rect(ref['roi_' + key], 3, 3)
        out = (base != 0) & (c['mc'] == 0)
        if notch:
            assert out.sum() >= 10, (key, 'base outside mask_contour', int(out.sum()))
        assert not (ref['exp_' + key][c['mc'] == 0]).any()


@pytest.mark.parametrize('w', [640, 650, 801])
@pytest.mark.parametrize('r0', [21, 22])
def test_edge_layout_end_points(orc, w, r0):
    """r0 is 21 / 22, and the listed end points are the fragments' PCA end points: every residue 0, 1, 31, 32, 62, 63 (mod
    64), all four frame edges within 7 px, two corners"""
    c, ref = oracle(('edges', w, r0), lambda: E.gen_edges(w, r0))
    assert ref['status'] == 0 and ref['r0'] == r0
    _, hp, vp = E.edge_layout(w)
    h = c['binary'].shape[0]
    for key, want in (('h', hp), ('v', vp)):
        got = set()
        for p1, p2, nv in E.end_points(ref['roi_' + key]):
            assert 8 <= nv <= 200
            got.update([p1, p2])
        assert set(want) <= got, (key, sorted(set(want) - got))
        assert _expanded(ref, key) == len(want) // 2 - 1, key          # all but the longest
    cols = {x % 64 for x, _ in hp}
    assert set(E.RESIDUES) <= cols
    allp = hp + vp
    assert any(x <= 7 for x, _ in allp) and any(x >= w - 8 for x, _ in allp)
    assert any(y <= 7 for _, y in allp) and any(y >= h - 8 for _, y in allp)
    assert any(x <= 7 and y <= 7 for x, y in hp) and any(x >= w - 8 and y >= h - 8 for x, y in hp)
    assert {x % 64 for x, _ in vp} >= {62, 63, 0}


def test_many_fragments_below_the_cap(orc, cpe):
    """500 .. 700 valid fragments per mask (below MAXSEG: the expansion runs), more expanded ones than the expansion kernel
    has workgroups per frame, one clearly longest, a few vertex counts, and end points of different fragments 2 - 3 px apart"""
    c, ref = oracle('many', E.gen_many)
    assert ref['status'] == 0
    for key in ('h', 'v'):
        nc, nv, gang, glen = ref['seg_' + key]
        assert 500 <= nv <= 700 and nv < M.MAXSEG, (key, nv)
        assert _expanded(ref, key) > 32 and _expanded(ref, key) == nv - 1, key      # frame_waves(1, 32, 256) = 256 at most, 32 at least
        frs = [f for f in E.end_points(ref['roi_' + key]) if 5 <= f[2] <= 200]
        assert len({f[2] for f in frs}) >= 3, sorted({f[2] for f in frs})
        lens = sorted(float(np.hypot(p2[0] - p1[0], p2[1] - p1[1])) for p1, p2, _ in frs)
        assert lens[-1] > 2 * lens[-2]
        ends = np.array([p for f in frs for p in f[:2]], np.float64)
        owner = np.repeat(np.arange(len(frs)), 2)
        d = np.hypot(ends[:, None, 0] - ends[None, :, 0], ends[:, None, 1] - ends[None, :, 1])
        close = (d >= 2) & (d <= 3) & (owner[:, None] != owner[None, :])
        assert close.any(1).sum() >= 200, (key, int(close.any(1).sum()))


def test_strip_frame_is_far_from_the_busy_one(orc):
    """the strip frame's rect is 40 rows, none of which the busy frame's expanded masks touch, and it expands a fragment"""
    c, ref = oracle('strip', E.gen_strip)
    _, busy = oracle('busy', E.gen_busy)
    x, y, w, h = c['rect']
    assert h == 40 and ref['status'] == 0
    assert not busy['exp_h'][y:y + h].any() and not busy['exp_v'][y:y + h].any()
    assert (ref['exp_h'] > ref['roi_h']).any() and not ref['exp_h'][:y].any()
