"""CPU: the generators of tests/trace_step_cases.py put what they claim in front of the border followers, by the oracle's own
contours (cv2.findContours(RETR_LIST, CHAIN_APPROX_NONE) as oracle/stages restates it)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trace_step_cases as T  # noqa: E402

NTHR = 17


def _contours(img, k):
    from oracle import stages as S
    return S.find_contours(img > 50 + 10 * k, 'list', 'none')


def _accepted(img):
    """(border points, is_hole) of every contour the detector's area filter keeps, over the 17 thresholds"""
    from oracle import stages as S
    out = set()
    for k in range(NTHR):
        for pts, is_hole in _contours(img, k):
            if 10 <= S.contour_moments(pts)[0] < 5000:
                out.add((len(pts), bool(is_hole)))
    return out


def test_every_chunk_limit_occurs_among_the_accepted_blobs(orc):
    holes = {n for n, is_hole in _accepted(T.get('hole_lengths')) if is_hole}
    rings = {n for n, is_hole in _accepted(T.get('ring_lengths')) if not is_hole}
    # a border of one point encloses no area (minArea is 10): it is followed, and never accepted
    assert set(T.LENGTHS[1:]) <= holes, sorted(set(T.LENGTHS[1:]) - holes)
    assert set(T.LENGTHS[1:]) <= rings, sorted(set(T.LENGTHS[1:]) - rings)
    assert any(len(p) == 1 and not is_hole for p, is_hole in _contours(T.get('ring_lengths'), 0))
    for n in T.LENGTHS[1:]:
        a, b, _ = T.hole_dims(n)
        assert (a + 1) * (b + 1) < 5000
    assert {T.CH_PTS - 1, T.CH_PTS, T.CH_PTS + 1, 2 * T.CH_PTS, 4 * T.CH_PTS, 16 * T.CH_PTS} <= set(T.LENGTHS)


def test_revisited_pixels_and_turns(orc):
    img = T.get('revisits')
    twice = corners = 0
    for pts, is_hole in _contours(img, 0):
        p = np.asarray(pts).reshape(-1, 2)
        twice += len(p) - len({tuple(q) for q in p})
        if is_hole and len(p) > 100:
            d = np.diff(np.vstack([p, p[:1]]), axis=0)
            corners = max(corners, int((np.abs(np.diff(d, axis=0)).sum(1) > 0).sum()))
    assert twice >= 16, twice                       # spurs of 7, 6, 3 and 4 pixels: all but the tip are passed twice
    assert corners >= 40, corners                   # a staircase of 40 steps: at least one change of heading per step
    one_pixel = sum(1 for p, is_hole in _contours(img, 0) if is_hole and len(p) == 4)
    assert one_pixel >= 60, one_pixel


def test_window_phases_and_crossings(orc):
    firsts = set()
    for pts, is_hole in _contours(T.get('window_phases'), 0):
        if is_hole:
            p = np.asarray(pts).reshape(-1, 2)
            y = p[:, 1].min() + 1
            x = p[p[:, 1] == y - 1][:, 0].min()      # the hole's first pixel: below the leftmost point of the border's top row
            firsts.add((x % 32, y % 8))
    want = {(dx % 32, dy % 8) for dx in range(29, 36) for dy in range(5, 11)}
    assert want <= firsts, sorted(want - firsts)
    for name, rows, cols in (('window_crossings', 80, 200), ('long_holes', 400, 400)):
        spans = [np.ptp(np.asarray(p).reshape(-1, 2), axis=0) for p, is_hole in _contours(T.get(name), 0) if is_hole]
        assert max(s[0] for s in spans) >= cols and max(s[1] for s in spans) >= rows, (name, spans)
    assert T.get('long_holes').shape[1] % 16 != 0
    assert sum(1 for _, is_hole in _contours(T.get('long_holes'), 0) if is_hole) == 3
    img = T.get('frame_edges')
    h, w = img.shape
    lo = np.min([np.asarray(p).reshape(-1, 2).min(0) for p, is_hole in _contours(img, 0) if is_hole], axis=0)
    hi = np.max([np.asarray(p).reshape(-1, 2).max(0) for p, is_hole in _contours(img, 0) if is_hole], axis=0)
    assert tuple(lo) == (0, 0) and tuple(hi) == (w - 1, h - 1)       # hole borders run along all four frame edges


def test_lockstep_counts(orc):
    for name, n in (('one_long', 64), ('holes_65', 65)):
        lens = sorted(len(p) for p, is_hole in _contours(T.get(name), 0) if is_hole)
        assert len(lens) == n, (name, len(lens))
    assert lens.count(14) == 65
    lens = sorted(len(p) for p, is_hole in _contours(T.get('one_long'), 0) if is_hole)
    assert lens[-1] == 366 and lens[-2] == 14
    img = T.get('pool_runs_out')
    holes = [p for p, is_hole in _contours(img, 1) if is_hole]
    # every hole has 6 pixels: the tracer reserves ceil((8 * (int)sqrt(6) + 16) / 31) = 2 chunks for it
    assert 2 * len(holes) > T.MAXCH_SMALL and img.size // 256 < T.MAXCH_SMALL
    assert not any(is_hole for _, is_hole in _contours(img, 0)) and not any(is_hole for _, is_hole in _contours(img, 2))


@pytest.mark.parametrize('name', ['far_columns', 'far_rows'])
def test_large_frames_keep_their_holes_at_the_far_end(orc, name):
    img = T.get(name)
    assert max(img.shape) == 4096
    axis = 0 if name == 'far_columns' else 1
    far = [np.asarray(p).reshape(-1, 2)[:, axis] for p, is_hole in _contours(img, 0) if is_hole]
    assert len(far) >= 10 and sum(1 for v in far if v.min() >= 4096 - 64) >= 8 and max(v.max() for v in far) >= 4093
