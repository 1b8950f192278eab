"""CPU: the lines-stage generators (tests/lines_cases.py) put in front of the kernel what they are named for, checked with
the oracle alone -- so that a passing tests/test_lines_stage_gpu.py means something.  Also: the oracle's grouping against
scipy.ndimage.label, and the two figures (numpy.polyfit difference, intersection residual) the GPU file's bounds come from."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lines_cases as L  # noqa: E402

HAVE_LINES = (0, 3, 4)      # statuses after which the oracle's line sets are those of clean_and_relabel


def _groups_of(c, side):
    """group_points of the oracle on the crop (npts per group in min-y order, overflow flag aside)"""
    from oracle import stages as S
    x0, y0, rw, rh = c['rect']
    plane = (c['exp_h'], c['exp_v'])[side]
    _, lab = S.connected_components(plane[y0:y0 + rh, x0:x0 + rw])
    return S.group_points(c['joints'][:c['n_joints']], lab, x0, y0)


@pytest.mark.parametrize('name', sorted(L.CASES))
def test_case_is_well_formed(orc, name):
    """masks inside rect, the status the case is built for, finite equations, and the overflow flag set exactly where a
    capacity is exceeded"""
    c = L.get(name)
    r = L.ref(name)
    h, w = c['exp_h'].shape
    x0, y0, rw, rh = c['rect']
    inside = np.zeros((h, w), bool)
    inside[y0:y0 + rh, x0:x0 + rw] = True
    assert not (c['exp_h'][~inside].any() or c['exp_v'][~inside].any()), 'a mask pixel outside rect'
    assert 64 <= h <= 640 and 64 <= w <= 801
    assert bool(r['overflow']) == (name in L.OVERFLOWS)
    assert (r['status'] == 6) == (name in L.OVERFLOWS)
    if r['status'] in HAVE_LINES and c['status'] == 0:
        for ls in (r['rows'], r['cols']):
            assert np.isfinite(np.array(ls.equations(), np.float64).reshape(-1, 6)).all()
    if c['subpixel'] is not None:
        assert c['target'] == 'cylinder' and 1 <= c['subpixel'][0] <= 13


@pytest.mark.parametrize('name', sorted(n for n in L.CASES if L.get(n)['status'] == 0))
def test_oracle_groups_are_the_scipy_components(orc, name):
    """every joint's group by the oracle's connectedComponents + group_points = by scipy.ndimage.label with the 8-connected
    structure (up to the order of the groups, which the oracle has already sorted by min y)"""
    c = L.get(name)
    for side in (0, 1):
        ls = _groups_of(c, side)
        got = sorted(tuple((int(x), int(y)) for x, y in g) for g in ls.points())
        want = sorted(tuple(g[:L.MAXLP]) for g in L.scipy_groups(c)[side])
        if len(want) > L.MAXL:
            assert len(got) == L.MAXL and set(got) <= set(want)
        else:
            assert got == want


@pytest.mark.parametrize('side', ['row', 'col'])
@pytest.mark.parametrize('G', L.GROUP_COUNTS)
def test_group_count_cases_reach_their_count(orc, G, side):
    k = 0 if side == 'row' else 1
    for order in ('raster', 'shuffled'):
        name = f'groups_{side}_{G}_{order}'
        c, r = L.get(name), L.ref(name)
        assert len(L.scipy_groups(c)[k]) == G and len(L.scipy_groups(c)[1 - k]) == 3
        assert r['n_groups'][k] == min(G, L.MAXL) and r['n_groups'][1 - k] == 3
        if G > L.MAXL:
            assert r['status'] == 6 and r['overflow'] == 1 and len(r['xy']) == 0
            continue
        assert r['overflow'] == 0
        if G == 1:
            assert r['status'] == 3          # remove_label takes the only line
            continue
        # every line but the one remove_label takes meets a column, so the count shows in the result
        assert r['status'] == 0 and (r['n_rows'], r['n_cols'])[k] == G - 1 and 1 <= (r['n_rows'], r['n_cols'])[1 - k] <= 2
    a, b = L.get(f'groups_{side}_{G}_raster'), L.get(f'groups_{side}_{G}_shuffled')
    assert not np.array_equal(a['joints'], b['joints']) and np.array_equal(L.raster(a['joints']), L.raster(b['joints']))
    ja = a['joints'][:, ::-1] if side == 'col' else a['joints']
    assert np.array_equal(ja, L.raster(ja))


@pytest.mark.parametrize('side', ['row', 'col'])
def test_group_size_cases_sit_on_the_capacity(orc, side):
    k = 0 if side == 'row' else 1
    for N in (1023, 1024, 1025):
        name = f'group_size_{side}_{N}'
        c, r = L.get(name), L.ref(name)
        assert max(len(g) for g in L.scipy_groups(c)[k]) == N
        assert max(_groups_of(c, k).npts[:4]) == min(N, L.MAXLP)
        assert (r['status'], r['overflow']) == ((6, 1) if N > L.MAXLP else (0, 0))
        if N <= L.MAXLP:       # the large group is a line of the result
            assert (r['n_rows'], r['n_cols'])[k] == 3


def test_point_count_cases_sit_on_the_capacity(orc):
    r = L.ref('points_2048')
    assert r['status'] == 0 and len(r['xy']) == L.MAXP and r['overflow'] == 0
    assert (r['n_rows'], r['n_cols']) == (64, 40) and int(r['id'][:, 0].max()) == 31 and int(r['id'][:, 0].min()) == 0
    assert sum(len(p) for p in r['rows'].points()) == 2560 > 256       # more row points than threads
    r = L.ref('points_2112')
    assert r['status'] == 6 and len(r['xy']) == 0 and r['overflow'] == 1 and r['n_groups'] == (65, 42)


@pytest.mark.parametrize('where', L.LABEL_RECTS)
@pytest.mark.parametrize('w', L.LABEL_WIDTHS)
def test_label_cases_have_long_chains_across_tile_borders(orc, w, where):
    from scipy import ndimage
    c, r = L.get(f'labels_{w}_{where}'), L.ref(f'labels_{w}_{where}')
    h = c['exp_h'].shape[0]
    x0, y0, rw, rh = c['rect']
    assert (w % 16 == 0) == (w == 128)
    assert {'frame': (x0, y0, rw, rh) == (0, 0, w, h), 'tl': (x0, y0) == (0, 0) and rw < w and rh < h,
            'br': (x0 + rw, y0 + rh) == (w, h) and x0 > 0 and y0 > 0}[where]
    for plane in (c['exp_h'], c['exp_v']):
        lab, n = ndimage.label(plane != 0, structure=np.ones((3, 3)))
        assert n == 4
        spans = 0
        for sl in ndimage.find_objects(lab):
            ys, xs = sl
            spans += (xs.stop - 1) // 64 > xs.start // 64 and (ys.stop - 1) // 8 > ys.start // 8
        assert spans >= (3 if w > 128 else 1)          # components that cross 64 x 8 tile borders in both directions
    touched = (c['exp_h'] | c['exp_v'])[y0:y0 + rh, x0:x0 + rw]
    assert touched[0].any() and touched[-1].any() and touched[:, 0].any() and touched[:, -1].any()     # out to rect's edges
    # the joints sit hundreds of pixels of walking distance from their component's first pixel
    assert min(c['far']) >= rh and max(c['far']) >= rh * rw // 8
    assert r['status'] == 0 and (r['n_rows'], r['n_cols'], r['n_groups']) == (3, 3, (4, 4))      # every shape's line survives


def test_joint_lookup_cases(orc):
    c, r = L.get('lookup'), L.ref('lookup')
    h, w = c['exp_h'].shape
    j = c['joints']
    inb = (j[:, 0] >= 0) & (j[:, 0] < w) & (j[:, 1] >= 0) & (j[:, 1] < h)
    assert (~inb).sum() == 8 and (j[:, 0] == w).any() and (j[:, 1] == h).any() and (j < 0).any()
    on_h = c['exp_h'][j[inb, 1], j[inb, 0]] != 0
    on_v = c['exp_v'][j[inb, 1], j[inb, 0]] != 0
    assert (on_h & ~on_v).sum() == 3 and (~on_h & on_v).sum() == 3 and (~on_h & ~on_v).sum() == 4 and (on_h & on_v).sum() == 36
    assert r['status'] == 0 and r['n_groups'] == (6, 6)
    c, r = L.get('no_joints'), L.ref('no_joints')
    assert c['n_joints'] == 0 and len(c['joints']) == 36 and r['status'] == 3 and r['n_groups'] == (0, 0)
    c, r = L.get('all_joints'), L.ref('all_joints')
    assert c['n_joints'] == L.MAXJ and r['status'] == 0 and r['n_groups'] == (16, 16) and len(r['xy']) > 0
    assert max(_groups_of(c, 0).npts[:16]) == 128


def test_early_exit_cases(orc):
    for name, groups in (('one_row', (1, 3)), ('one_col', (3, 1)), ('apart', (4, 3))):
        r = L.ref(name)
        assert r['status'] == 3 and r['n_groups'] == groups and r['n_rows'] == 0, name
    r = L.ref('tiny_groups')
    sizes = [sorted(len(g) for g in side) for side in L.scipy_groups(L.get('tiny_groups'))]
    assert sizes[0][:2] == [1, 2] and sizes[1][:2] == [1, 2]
    assert r['status'] == 0 and [0.0] * 6 in r['rows'].equations() and [0.0] * 6 in r['cols'].equations()
    assert (0.0, 0.0) in [p for line in r['rows'].points() for p in line]       # the empty equation meets the column x = 0
    for st in (1, 2):
        assert L.get(f'status_{st}')['status'] == st and L.ref(f'status_{st}')['status'] == st


def test_centre_search_cases(orc):
    r = L.ref('constant_g7')
    pts = [p for line in r['rows'].points() for p in line]
    assert len(pts) == 361 > 256 and tuple(r['center']) == pts[0] and r['status'] == 0
    c, r = L.get('two_maxima'), L.ref('two_maxima')
    pts = [p for line in r['rows'].points() for p in line]
    from oracle import stages as S
    assert len(pts) == 361 and tuple(r['center']) == pts[200] and np.allclose(pts[260], (82, 88), atol=1e-9)
    for q in (200, 260):            # both windows are 255 throughout: an exact tie, in threads 200 and 4
        x, y = pts[q]
        assert (c['g7'][int(y - 3):int(y + 3), int(x - 3):int(x + 3)] == 255).all()
    assert 200 % 256 != 260 % 256
    for e in L.EDGES:
        c, r = L.get(f'edge_max_{e}'), L.ref(f'edge_max_{e}')
        h, w = c['g7'].shape
        x, y = r['center']
        assert np.allclose((x, y), c['want_center'], atol=1e-9) and r['status'] == 0
        assert {'left': int(x - 3) < 0, 'right': int(x + 3) > w, 'top': int(y - 3) < 0, 'bottom': int(y + 3) > h}[e]
    c, r = L.get('x_equals_w'), L.ref('x_equals_w')
    w = c['g7'].shape[1]
    assert r['status'] == 0 and abs(r['center'][0] - w) < 1e-9 and r['center'][0] <= w == c['rect'][0] + c['rect'][2]
    assert any(abs(x - w) < 1e-9 for x, _ in r['xy'])


def test_planar_cases(orc):
    for r0, half in zip(L.PLANE_R0, (0, 0, 1, 2)):
        c, r = L.get(f'plane_r0_{r0}'), L.ref(f'plane_r0_{r0}')
        assert int(r0 / 4.5) == half and r['status'] == 0 and len(r['xy']) == 49
        first = r['rows'].points()[0][0]
        assert (tuple(r['center']) == first) == (half == 0) or half > 0      # an empty window everywhere: the first point stays
        if half == 0:
            assert tuple(r['center']) == first
        assert sorted(map(tuple, r['id'].tolist())) == [(a, b) for a in range(r['id'][:, 0].min(), r['id'][:, 0].min() + 7)
                                                       for b in range(r['id'][:, 1].min(), r['id'][:, 1].min() + 7)]
        assert r['id'].tolist() == sorted(r['id'].tolist())             # (row, col) order, every column kept
    r = L.ref('plane_two_joints')
    assert r['status'] == 0 and len(r['xy']) == 25 and all(len(g) == 2 for side in L.scipy_groups(L.get('plane_two_joints')) for g in side)
    want = dict(exact=(6, 4, 0), plus1=(7, 5, 0), n1024=(5, 4, 0), n1025=(5, 0, 1), lone=(4, 3, 0))
    for k, (groups, ncols, ovf) in want.items():
        r = L.ref(f'plane_merge_{k}')
        assert (r['n_groups'][1], r['n_cols'], r['overflow']) == (groups, ncols, ovf), k
    # the merged column of `exact` carries the nine joints of its three pieces, over their whole extent
    eqs = L.ref('plane_merge_exact')['cols'].equations()
    assert sorted((e[2], e[3]) for e in eqs)[3] == (20 - 50, 220 + 50)
    g = L.scipy_groups(L.get('plane_merge_n1024'))[1]
    assert sorted(len(x) for x in g)[-2:] == [512, 512]
    g = L.scipy_groups(L.get('plane_merge_n1025'))[1]
    assert sorted(len(x) for x in g)[-2:] == [512, 513]
    c, r = L.get('plane_first_nan'), L.ref('plane_first_nan')
    pts = r['rows'].points()[0]
    w = c['g7'].shape[1]
    assert r['status'] == 0 and tuple(r['center']) == pts[0] and int(pts[0][0] - 1) >= w      # first window empty ...
    assert all(int(p[0] + 1) <= w for p in pts[1:]) and len(pts) == 3                       # ... the later ones are not


def test_subpixel_cases(orc):
    from oracle import stages as S
    for win in L.SP_WINDOWS:
        for step in L.SP_STEPS:
            r = L.ref(f'subpixel_w{win}_s{step}')
            assert r['status'] == 0 and r['overflow'] == 0 and len(r['xy']) > 0
        for side in ('row', 'col'):
            r = L.ref(f'subpixel_corner_{side}_w{win}')
            assert r['status'] == (7 if win < 13 else 0), (side, win)
    plain = L.oracle(dict(L.get('subpixel_w7_s1.0'), subpixel=None))
    assert not np.array_equal(plain['rows'].equations(), L.ref('subpixel_w7_s1.0')['rows'].equations())     # the refinement moves the lines
    assert L.ref('subpixel_long_s1.0')['status'] == 0 and L.ref('subpixel_long_s0.25')['status'] == 6
    cap = max(L.SP_SHAPE) + 128
    assert 180.0001 / 0.25 <= cap < 500.0001 / 0.25 and 500.0001 / 1.0 <= cap
    c = L.get('subpixel_long_s0.25')     # the oracle without the library's sample capacity has no overflow here
    assert S.lines_stage(c['exp_h'], c['exp_v'], c['joints'], c['rect'], c['r0'], c['g7'], c['gray'], subpixel=True, window=7, step=0.25,
                         sp_cap=0)['status'] == 0
    dark, lit = L.ref('subpixel_dark'), L.oracle(dict(L.get('subpixel_dark'), subpixel=None))
    assert dark['status'] == 0 and not L.get('subpixel_dark')['gray'].any()
    assert np.allclose(np.array(dark['rows'].equations()), np.array(lit['rows'].equations())[:, :6], atol=1e-3)   # unmoved samples, f32 storage
    r = L.ref('subpixel_tiny_groups')
    assert r['status'] == 0 and [0.0] * 6 in r['rows'].equations()          # K = 1 < 3: the empty equation is not refitted


def test_oracle_float_figures_are_the_recorded_ones(orc):
    """the two figures behind the GPU file's bounds: the oracle's fits against numpy.polyfit and its intersections against
    their polynomials, over every case with a result"""
    fit = res = 0.0
    for name in sorted(L.CASES):
        c, r = L.get(name), L.ref(name)
        if c['status'] != 0 or r['status'] not in HAVE_LINES:
            continue
        rows, cols = L.lines_of(r['rows']), L.lines_of(r['cols'])
        res = max(res, L.residual(c, rows, cols))
        if c['subpixel'] is None:
            fit = max(fit, L.fit_diff(c, rows, cols))
    print(f'largest numpy.polyfit difference {fit:.3e} px, largest residual {res:.3e} px')
    assert 0 < fit <= L.ORACLE_FIT_DIFF and 0 < res <= L.ORACLE_RESIDUAL
