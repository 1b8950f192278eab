"""The case generators and the numpy reference of tests/plane_fit_cases.py on their own (no GPU): the reference against
truth, the conditions under which the GPU tests may compare masks, counts, flags and statuses exactly, and the bounds of the
noisy tables."""
import math

import numpy as np
import pytest

import plane_fit_cases as C


def test_reference_gives_truth_on_noise_free_tables():
    n, P4 = C.board(-20.0, 15.0, 371.0)
    idx, X, Xt = C.board_table(n, P4, noise=0.0)
    r = C.ref_fit_plane(X, idx, len(X))
    assert r['status'] == C.ST_OK and r['flags'] == C.ORIGIN_POINT and r['n_inliers'] == 17 * 25
    # truth to the case's own derived tolerances (the triangulation's error, a 4 x 4 SVD per point, lies far below them)
    print(f'normal {C.angle(r["P"][:3], n):.2e} / {r["tol_angle"]:.2e}  P4 {abs(r["P"][3] - P4):.2e} / {r["tol_off"]:.2e}  max |r| {r["stats"][1]:.2e}')
    assert max(r['tol_angle'], r['tol_off'], r['tol_grid']) <= 1e-8
    assert C.angle(r['P'][:3], n) <= r['tol_angle'] and abs(r['P'][3] - P4) <= r['tol_off'] and r['stats'][1] <= 2 * r['tol_off']
    z = np.nonzero((idx == 0).all(1))[0][0]
    assert np.abs(r['T'][:3, 3] - Xt[z]).max() <= r['tol_off']
    T = r['T']
    assert np.abs(T[:3, :3].T @ T[:3, :3] - np.eye(3)).max() <= 1e-14 and np.linalg.det(T[:3, :3]) > 0
    assert abs(T[:3, 0] @ r['grid'][1]) > 0.99 * np.linalg.norm(r['grid'][1])      # x follows U
    # a board's grid is projective, not affine: the map fits to millimetres, not to the noise
    assert 0.05 < r['stats'][5] < 5.0


def test_laser_planes_and_centre_on_noise_free_tables():
    fr = C.multi_pose(0, 12, 0.0)
    X, I, cnt = C.pack(fr)
    r = C.ref_index_planes(X, I, cnt, -12, 12)
    assert (r['status'][0, 4:21] == C.ST_OK).all() and (r['status'][1] == C.ST_OK).all()
    assert (r['status'][0, :4] == C.ST_FEW_POINTS).all() and (r['count'][0, :4] == 0).all()
    for f in fr:
        p = C.ref_fit_plane(f['X'], f['idx'], len(f['X']))
        assert C.angle(p['P'][:3], f['n']) <= p['tol_angle'] and abs(p['P'][3] - f['P4']) <= p['tol_off']
    tl, Op = C.true_line_planes(-12, 12), C.rig()[5]
    for k in range(2):
        for j in range(25):
            if r['status'][k, j] == C.ST_OK:
                s = 1.0 if r['P'][k, j, :3] @ tl[k, j] > 0 else -1.0                     # (truth carries no sign convention)
                assert C.angle(r['P'][k, j, :3], s * tl[k, j]) <= r['tol_angle'][k, j], (k, j)
                assert abs(r['P'][k, j, 3] + s * tl[k, j] @ Op) <= r['tol_off'][k, j], (k, j)   # every laser plane holds the projector
    print(f'centre {np.abs(r["centre"][:3] - Op).max():.2e} / {r["tol_centre"]:.2e}  rms {r["centre"][3]:.2e}')
    assert 0 < r['tol_centre'] <= 1e-8 and np.abs(r['centre'][:3] - Op).max() <= r['tol_centre']
    # the centre's rms: every plane misses the projector by at most its own offset bound plus the centre's
    assert r['centre'][3] <= r['tol_off'].max() + r['tol_centre']
    assert (r['frames'][1] == 12).all() and (r['count'][1] == 17 * 12).all()


@pytest.mark.parametrize('tau', [0.0, C.TAU])
def test_fit_cases_allow_exact_comparison(tau):
    seen = set()
    for name in C.fit_cases(tau):
        r = C.fit_reference(tau, name)
        seen.add((r['status'], r['flags']))
        print(f'{name}: status {r["status"]} flags {r["flags"]} m {r["n_inliers"]} refits {r["stats"][6]:.0f} tol_angle '
              f'{r["tol_angle"]:.2e} tol_off {r["tol_off"]:.2e} tol_grid {r["tol_grid"]:.2e} margin {r["margin"]:.2e}')
        assert max(r['tol_angle'], r['tol_off'], r['tol_grid']) <= 1e-8, name
        assert r['margin'] > 1e-6, name
        assert r['spread_margin'] > 1e-6, name
        assert r['mask'][r['m'] if r['status'] else C.MAXP:].sum() == 0
    for want in ((C.ST_FEW_POINTS, 0), (C.ST_OK, 0), (C.ST_OK, C.NO_GRID), (C.ST_OK, C.ORIGIN_POINT), (C.ST_OK, C.NO_GRID | C.ORIGIN_POINT)):
        assert want in seen
    r = C.fit_reference(tau, 'outliers')
    assert (r['n_inliers'], r['stats'][6]) == ((270, 2) if tau > 0 else (300, 0))
    assert C.fit_reference(tau, 'nan point')['n_inliers'] == 118
    a, b = C.fit_reference(tau, 'origin point'), C.fit_reference(tau, 'origin twice')
    assert np.array_equal(a['T'][:3, 3], b['T'][:3, 3]) and not np.array_equal(a['grid'], b['grid'])     # the first (0,0) is the origin
    if tau > 0:
        assert C.fit_reference(tau, 'trim to few')['status'] == C.ST_FEW_POINTS


def test_slow_trim_case_needs_more_refits_than_it_gets():
    fr, tau = C.slow_trim_case()
    got = {mr: C.ref_fit_plane(fr['X'], fr['idx'], len(fr['X']), tau, mr) for mr in (0, 2, 4, 8)}
    assert [got[mr]['stats'][6] for mr in (0, 2, 4, 8)] == [0, 2, 4, 5]
    for r in got.values():
        assert r['status'] == C.ST_OK and r['margin'] > 1e-6 and max(r['tol_angle'], r['tol_off'], r['tol_grid']) <= 1e-8
    assert len({r['n_inliers'] for r in got.values()}) == 4


def test_index_cases_allow_exact_comparison():
    for name, case in C.index_cases().items():
        r = C.index_reference(name)
        L = case['hi'] - case['lo'] + 1
        assert r['P'].shape == (2, L, 4)
        print(f'{name}: ok lines {int((r["status"] == 0).sum())} centre status {r["centre_status"]} cond {r["cond"]:.3g} tol_angle '
              f'{r["tol_angle"].max():.2e} tol_off {r["tol_off"].max():.2e} tol_centre {r["tol_centre"]:.2e}')
        assert max(r['tol_angle'].max(), r['tol_off'].max(), r['tol_centre']) <= 1e-8, name
        assert r['spread_margin'] > 1e-6, name
    ok = lambda name: C.index_reference(name)['status'] == C.ST_OK
    assert not ok('1 frame').any() and C.index_reference('1 frame')['count'].sum() == 2 * 425
    assert ok('2 frames').sum() == 42 and ok('45 frames').sum() == 18 and ok('L 256').sum() == 42
    assert not ok('empty tables').any() and not ok('no frames').any()
    r = C.index_reference('line in one frame')
    assert r['status'][0, 21] == C.ST_FEW_POINTS and r['count'][0, 21] == 25 and r['frames'][0, 21] == 1
    assert (C.index_reference('frame_ok')['frames'][1] == 4).all()
    r = C.index_reference('use')
    assert (r['frames'][1] == 5).all() and r['count'].sum() < 0.75 * 2 * 5 * 425
    r = C.index_reference('one family')
    assert ok('one family')[0].sum() == 17 and not ok('one family')[1].any() and r['centre_status'] == C.ST_FEW_POINTS
    assert C.index_reference('L 1')['centre_status'] == C.ST_FEW_POINTS and C.index_reference('L 3')['centre_status'] == C.ST_OK
    assert C.index_reference('indices outside')['count'].sum() == 4 * (11 * 25 + 17 * 11)


def test_noisy_tables_stay_within_the_measured_bounds():
    """the figures of the module docstring: the bounds are twice the worst value over the seeds"""
    worst = dict.fromkeys(C.NOISY_BOUNDS, 0.0)
    for seed in C.NOISY_SEEDS:
        fr = C.multi_pose(seed)
        X, I, cnt = C.pack(fr)
        ip = C.ref_index_planes(X, I, cnt, -12, 12)
        assert ip['centre_status'] == C.ST_OK and (ip['status'] == C.ST_OK).sum() == 42
        e = C.noisy_errors([C.ref_fit_plane(f['X'], f['idx'], len(f['X']))['P'] for f in fr], ip['P'], ip['status'], ip['centre'], fr, -12)
        print(seed, e, 'cond', ip['cond'])
        for k in worst:
            worst[k] = max(worst[k], e[k])
    for k, b in C.NOISY_BOUNDS.items():
        assert b / 2 * 0.99 <= worst[k] <= b / 2 * 1.01, (k, worst[k], b)     # the docstring's figures are the measured ones
        assert worst[k] <= b


def test_compare_refuses_what_it_should():
    r = C.fit_reference(0.0, 'count 65')
    good = dict(P=r['P'], T=r['T'], grid=r['grid'], stats=r['stats'], n_inliers=r['n_inliers'], mask=r['mask'], flags=r['flags'], status=0)
    C.compare_fit(good, r)
    for key, delta in (('P', 1e-7), ('T', 1e-7), ('grid', 1e-7), ('stats', 1e-6)):
        bad = dict(good)
        bad[key] = good[key] + delta
        with pytest.raises(AssertionError):
            C.compare_fit(bad, r)
    bad = dict(good, mask=np.roll(r['mask'], 1))
    with pytest.raises(AssertionError):
        C.compare_fit(bad, r)
    ir = C.index_reference('2 frames')
    C.compare_index_planes(ir, ir)
    with pytest.raises(AssertionError):
        C.compare_index_planes(dict(ir, centre=ir['centre'] + 1e-7), ir)
    with pytest.raises(AssertionError):
        C.compare_index_planes(dict(ir, P=ir['P'] + 1e-7), ir)
