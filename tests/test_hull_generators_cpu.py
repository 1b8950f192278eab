"""The generators of tests/hull_cases.py against the oracle alone: every case does what its name claims, the masks that run in
mode 0 keep that mode's precondition, and get_convex_hull is the composition of the oracle's primitives that the GPU test
takes its vertex lists from."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hull_cases as H  # noqa: E402

SMALL = [s for s in H.SHAPES if s[0] * s[1] <= (1 << 21)]
LARGE = [s for s in H.SHAPES if s[0] * s[1] > (1 << 21)]
EIGHT = np.ones((3, 3), bool)
_NV = {}                       # (case, mode) -> vertices of the oracle's hull, filled by every check (test_vertex_maximum)


def _labels(m):
    from scipy import ndimage
    return ndimage.label(m, EIGHT)


def _vset(hull):
    return {(int(x), int(y)) for x, y in hull}


def _on_edge_not_vertex(comp, hull):
    """column extents of the component (the points k_hull_fill's chains are made of) that lie on an edge of the hull without
    being one of its vertices: they must be dropped at cross = 0"""
    vs = _vset(hull)
    xs = np.nonzero(comp.any(0))[0]
    lo = comp.argmax(0)[xs]
    hi = comp.shape[0] - 1 - comp[::-1].argmax(0)[xs]
    pts = {(int(x), int(y)) for x, y in zip(xs, lo)} | {(int(x), int(y)) for x, y in zip(xs, hi)}
    c = np.asarray(sorted(pts - vs), np.int64).reshape(-1, 2)
    hit = np.zeros(len(c), bool)
    for a, b in zip(hull.astype(np.int64), np.roll(hull.astype(np.int64), -1, 0)):
        cr = (b[0] - a[0]) * (c[:, 1] - a[1]) - (b[1] - a[1]) * (c[:, 0] - a[0])
        hit |= cr == 0
    return int(hit.sum())


def _touches(rect, shape):
    x, y, rw, rh = rect
    return ''.join(k for k, on in (('t', y == 0), ('b', y + rh == shape[0]), ('l', x == 0), ('r', x + rw == shape[1])) if on)


def _row_spans(row):
    d = np.diff(np.concatenate([[0], row.astype(np.int8), [0]]))
    return list(zip(np.nonzero(d == 1)[0].tolist(), (np.nonzero(d == -1)[0] - 1).tolist()))


def _check_claims(name, S):
    m = H.mask(name)
    h, w = m.shape
    c = H.claims(name)
    lab, nc = _labels(m)
    tag = (name, c)
    if 'comps' in c:
        assert nc == c['comps'], (tag, nc)
    if 'min_comps' in c:
        assert nc >= c['min_comps'], (tag, nc)
    r0 = H.reference(m, 0)
    _NV[(name, 0)] = len(r0['hull'])
    want = c.get('status', 0)
    assert r0['status'] == want, tag
    if H.MODE0[name] and nc == 1:
        assert r0['status'] == 0 and r0['areas'][r0['best']] > 0, (tag, 'mode 0: a lone component must have positive area')
    if want:
        assert not any(a > 0 for a in r0['areas']) and not r0['mask'].any(), tag
        return r0
    hull, rect, areas = r0['hull'], r0['rect'], r0['areas']
    if 'nv' in c:
        assert len(hull) == c['nv'], (tag, len(hull))
    if 'min_nv' in c:
        assert len(hull) >= c['min_nv'], (tag, len(hull))
    if 'rect' in c:
        assert rect == c['rect'], (tag, rect)
    if 'winner_rect' in c:
        assert rect == c['winner_rect'], (tag, rect)
    if 'area' in c:
        assert areas[r0['best']] == c['area'], (tag, areas)
    if 'collinear' in c:
        comp = lab == lab[r0['contour'][0][1], r0['contour'][0][0]]
        assert _on_edge_not_vertex(comp, hull) >= c['collinear'], (tag, _on_edge_not_vertex(comp, hull))
    if 'same_hull_as' in c:
        other = H.reference(H.mask(c['same_hull_as']), 0)
        assert _vset(hull) == _vset(other['hull']) and not np.array_equal(m, H.mask(c['same_hull_as'])), tag
        assert np.array_equal(r0['mask'], other['mask']), tag
    if 'one_more_than' in c:
        other = _vset(H.reference(H.mask(c['one_more_than']), 0)['hull'])
        assert other < _vset(hull) and len(_vset(hull) - other) == 1, tag
    if 'first_col' in c:
        x0, x1 = rect[0], rect[0] + rect[2] - 1
        assert (int(m[:, x0].sum()), int(m[:, x1].sum())) == (c['first_col'], c['last_col']), tag
    if c.get('concave'):
        assert int(m.sum()) < 0.8 * int((r0['mask'] > 0).sum()), tag
    if 'holes' in c or c.get('carved'):
        holes = sum(1 for _, hole in S.find_contours(np.where(m, 255, 0), 'list') if hole)
        assert holes >= c.get('holes', 1), (tag, holes)
    if c.get('carved'):
        # the notches and holes took pixels, none of them a vertex pixel: the hull is the one the uncarved polygon has
        assert int(m.sum()) < 0.9 * int((r0['mask'] > 0).sum()) and not (m & ~(r0['mask'] > 0)).any(), tag
        assert all(m[y, x] for x, y in hull), tag
        assert len(hull) >= 5, tag
    if c.get('nested_larger'):
        sizes = np.bincount(lab.ravel())[1:]
        win = lab[r0['contour'][0][1], r0['contour'][0][0]]
        nested = int(np.argmax(sizes)) + 1
        assert nested != win and len(areas) == nc - 1, (tag, 'the component of most pixels lies in a hole: it has no external contour')
        free = [int(sizes[k - 1]) for k in range(1, nc + 1) if k not in (win, nested)]
        assert free and max(free) < sizes[nested - 1] and sizes[win - 1] < sizes[nested - 1], tag
    if 'tie' in c:
        assert sorted(areas)[-c['tie']:] == [max(areas)] * c['tie'] and areas.count(max(areas)) == c['tie'], (tag, areas)
    if 'margin' in c:
        top = sorted(areas)
        assert top[-1] - top[-2] == c['margin'], (tag, areas)
    if c.get('fewer_pixels_wins'):
        sizes = np.bincount(lab.ravel())[1:]
        win = lab[r0['contour'][0][1], r0['contour'][0][0]]
        assert sizes[win - 1] < sizes.max(), tag
    if 'touches' in c:
        t = {'top': 't', 'bottom': 'b', 'left': 'l', 'right': 'r'}.get(c['touches'], c['touches'])
        assert _touches(rect, (h, w)) == t, (tag, rect)
    if 'rect_y' in c:
        assert (rect[1], rect[3]) == (c['rect_y'], c['rect_h']), (tag, rect)
        # k_hull_rows fills rows rect[1] .. rect[1] + rect[3] - 2 in bands of HR_ROWS (the outline draws the last row)
        assert -(-(rect[3] - 1) // H.HR_ROWS) == c['bands'], tag
    if 'span' in c:
        x1, x2 = c['span']
        rows = [y for y in range(rect[1], rect[1] + rect[3]) if _row_spans(r0['mask'][y] > 0) == [(x1, x2)]]
        assert len(rows) >= 3, (tag, 'rows of the oracle mask with exactly this span')
        if 'x1_mod' in c:
            assert (x1 % 16, x2 % 16) == (c['x1_mod'], c['x2_mod']), tag
        if c.get('short'):
            assert x2 - x1 + 1 <= 16, tag
    if c.get('long') or 'span_over' in c:
        longest = max(b - a + 1 for y in range(rect[1], rect[1] + rect[3]) for a, b in _row_spans(r0['mask'][y] > 0))
        assert longest > 1024, (tag, longest)
    if 'long_edge' in c:
        edges = {(int(b[0] - a[0]), int(b[1] - a[1])) for a, b in zip(hull, np.roll(hull, -1, 0))}
        dx, dy = c['long_edge']
        assert (dx, dy) in edges or (-dx, -dy) in edges, (tag, edges)
        if abs(dx) < abs(dy):       # an x-major reading of the same edge: dy / dx is a fraction whose 16.16 form is not exact
            assert (abs(dx) << 16) % abs(dy) != 0, tag
    if 'same_as' in c:
        base = H.mask(c['same_as'])
        extra = m & ~base
        assert int(extra.sum()) == 1 and not (base & ~m).any() and nc == _labels(base)[1] + 1, tag
        b0 = H.reference(base, 0)
        assert np.array_equal(hull, b0['hull']) and rect == b0['rect'] and np.array_equal(r0['mask'], b0['mask']), tag
    return r0


def _check_grey(name, m, grey):
    """mode 1's input puts 127 beside 128 along the whole border of the set: every set pixel with a background neighbour is
    128, every background pixel with a set neighbour is 127, and the threshold splits the image into the mask"""
    from scipy.ndimage import binary_dilation
    assert np.array_equal(grey > 127, m), name
    edge_set, edge_bg = m & binary_dilation(~m, EIGHT), ~m & binary_dilation(m, EIGHT)
    assert (grey[edge_set] == 128).all() and (grey[edge_bg] == 127).all(), name
    if m.any() and not m.all():
        assert edge_set.any() and edge_bg.any(), name
        # 128 on a set border pixel with a 127 background neighbour
        assert (binary_dilation(grey == 127, EIGHT) & (grey == 128) & edge_set).sum() == edge_set.sum(), name
    if H.claims(name).get('grey_edge'):
        assert int(edge_set.sum()) >= 200 and int(edge_bg.sum()) >= 200 and m.any() and not m.all(), name


def _check_mode1(name, S, r0):
    """get_convex_hull(grey, 127, 5) = the primitives composed, with scipy's binary_dilation under ellipse_se(11)"""
    m = H.mask(name)
    c = H.claims(name)
    r1 = H.reference(m, 1)
    _NV[(name, 1)] = max(len(r1['hull']), len(r1['round1']['hull']))
    grey = H.grey_of(m)
    _check_grey(name, m, grey)
    st, mk, rect = S.get_convex_hull(grey, 127, 5)
    assert st == r1['status'] == c.get('status', 0), name
    assert np.array_equal(mk, r1['mask']), name
    if st == 0:
        assert rect == r1['rect'], (name, rect, r1['rect'])
        # the first round is mode 0's answer on the same set
        assert np.array_equal(r1['round1']['hull'], r0['hull']) and np.array_equal(r1['round1']['mask'], r0['mask']), name
    if 'rect1' in c:
        assert rect == c['rect1'], (name, rect)
    if 'dilation_clipped' in c:
        clipped = rect[2] < r0['rect'][2] + 10 or rect[3] < r0['rect'][3] + 10
        assert clipped == c['dilation_clipped'], (name, rect)
    if 'tile_d' in c:
        # 64 x 32 tiles of k_dilate_ellipse that hold no source pixel but have one within the 5-px apron
        src = r1['round1']['mask'] > 0
        h, w = src.shape
        n = 0
        for y0 in range(0, h, 32):
            for x0 in range(0, w, 64):
                if not src[y0:y0 + 32, x0:x0 + 64].any() and src[max(y0 - 5, 0):y0 + 37, max(x0 - 5, 0):x0 + 69].any():
                    n += 1
        assert (n > 0) == (abs(c['tile_d']) <= 4), (name, n)      # at +-5 the nearest empty tile's apron just misses the rectangle
    if 'same_as' in c:
        b1 = H.reference(H.mask(c['same_as']), 1)
        assert np.array_equal(r1['hull'], b1['hull']) and r1['rect'] == b1['rect'] and np.array_equal(r1['mask'], b1['mask']), name
    return r1


@pytest.mark.parametrize('shape', SMALL)
def test_cases_do_what_they_claim(orc, shape):
    from oracle import stages as S
    for name in H.names_of(shape):
        r0 = _check_claims(name, S)
        _check_mode1(name, S, r0)


@pytest.mark.parametrize('name', [k for s in LARGE for k in H.names_of(s) if not k.endswith('+px')])
def test_large_cases_do_what_they_claim(orc, name):
    from oracle import stages as S
    r0 = _check_claims(name, S)
    _check_mode1(name, S, r0)


def test_large_cases_with_a_far_pixel(orc):
    """the 2048 x 2048 masks with their isolated pixel: one pixel more, one component more (the hull needs no second look: the
    GPU test compares these runs with the runs of the plain masks)"""
    for name in [k for s in LARGE for k in H.names_of(s) if k.endswith('+px')]:
        base = H.mask(H.claims(name)['same_as'])
        m = H.mask(name)
        extra = np.argwhere(m & ~base)
        assert len(extra) == 1 and not (base & ~m).any(), name
        y, x = extra[0]
        assert not base[max(y - 2, 0):y + 3, max(x - 2, 0):x + 3].any(), name


def test_families_are_all_there():
    """the sizes and paths the cases exist for"""
    assert {64, 80, 83, 320, 336, 1104, 2048, 2049, 2064, 96, 4096} <= {s[1] for s in H.SHAPES}
    assert len(H.names_of((96, 320))) >= 20 and 320 % 64 == 0
    assert H.claims('grey_127_128').get('grey_edge')
    assert (4096, 96) in H.SHAPES and (2048, 2048) in H.SHAPES and (4096, 4096) in H.SHAPES
    assert H.G[1] % 16 == 0 and H.G[1] % 64 != 0 and H.G[0] % 32 != 0
    assert max(s[1] for s in H.SHAPES if s[1] <= H.LDS_W) == H.LDS_W and min(s[1] for s in H.SHAPES if s[1] > H.LDS_W) == H.LDS_W + 1
    assert 2064 % 16 == 0 and 2049 % 16 != 0 and 83 % 16 != 0
    for nm in H.SAME_2048_2064:
        a, b = H.mask(nm + '_w2048'), H.mask(nm + '_w2064')
        assert np.array_equal(a, b[:, :2048]) and not b[:, 2048:].any(), nm
    got = {(H.claims(k)['rect_h'], H.claims(k)['rect_y']) for k in H.REGISTRY if 'rect_h' in H.claims(k)}
    assert got == {(a, b) for a in (2, 63, 64, 65, 128, 129) for b in (0, 1, 63)}
    got = {(H.claims(k)['x1_mod'], H.claims(k)['x2_mod']) for k in H.REGISTRY if 'x1_mod' in H.claims(k)}
    assert got == {(a, b) for a in (0, 1, 15) for b in (14, 15, 0)}
    assert {H.claims(k)['tile_d'] for k in H.REGISTRY if 'tile_d' in H.claims(k)} == set(range(-5, 6))
    one = [k for k in H.REGISTRY if H.claims(k).get('comps') == 1 and H.MODE0[k]]
    px = {H.claims(k)['same_as'] for k in H.REGISTRY if 'same_as' in H.claims(k)}
    assert all(k in px or H.claims(k).get('rect') == (0, 0) + H.shape_of(k)[::-1] or H.shape_of(k) == H.HUGE for k in one)
    m = H.isolated_pixels()
    assert int(m.sum()) > H.MAXROOTS and _labels(m)[1] == int(m.sum())


def test_vertex_maximum(orc):
    """the largest vertex count any generator reaches, in either mode and either planar round, beside the two capacities it
    must stay under (DESIGN.md section 2 quotes these numbers): HULL_LDS_W - 1 = 2047 vertices in k_hull_fill's LDS list,
    HR_MAXV = 1024 staged by k_hull_rows.  The checks above leave their counts in _NV; what they did not see (this test run
    alone, the large masks with a far pixel) is measured here"""
    for name in H.REGISTRY:
        for mode in (0, 1):
            if (name, mode) not in _NV:
                r = H.reference(H.mask(name), mode)
                _NV[(name, mode)] = max(len(r['hull']), len(r.get('round1', r)['hull']))
    assert set(_NV) == {(name, mode) for name in H.REGISTRY for mode in (0, 1)}
    assert _NV[('disc_1020', 0)] == 340 and _NV[('disc_2040', 0)] == 540, (_NV[('disc_1020', 0)], _NV[('disc_2040', 0)])
    top = max(_NV, key=_NV.get)
    assert _NV[top] == 540 and top[0] == 'disc_2040', (top, _NV[top])      # the dilated discs have fewer: 284 and 488
    assert _NV[top] < 1024 < 2047
