"""cpe_est_curvatures_batch and cpe_curvature_consensus_batch on the GPU against the two references of curvature_cases.py.

One batch (curvature_cases.FRAMES: every count that can go wrong, the mixed batch with an empty, a 5-point and a clamped
frame, duplicates, the tie grid, an exact plane, the grid beside a background plane; NaN past every count) is run once per
(mode, k) and shared by the tests.  Neighbour lists and gates are compared as integers, exactly; column 0 of the point the
fit's start picks has the bits of the fit's own initial direction and of the oracle's; values are compared against LAPACK at
the tolerance curvature_cases.tol() derives per point."""
import math

import numpy as np
import pytest
import torch

import curvature_cases as cc

pytestmark = pytest.mark.gpu
MODES_KS = [(m, k) for m in (cc.REFERENCE, cc.INTERCEPT) for k in cc.KS[m]]
NAMES = [n for n, _ in cc.FRAMES]


def _np(d):
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in d.items()}


@pytest.fixture(scope='module')
def dev_batch(gpu):
    X, cnt = cc.batch()
    return torch.from_numpy(X).to(gpu), torch.from_numpy(cnt).to(gpu)


@pytest.fixture(scope='module')
def runs(gpu, dev_batch):
    """(mode, k) -> (curvatures, consensus at the default gate) of the batch, as numpy"""
    from cpe_amd import fit
    X, cnt = dev_batch
    out = {}
    for mode, k in MODES_KS:
        cv = fit.est_curvatures_batch(X, cnt, k=k, mode=mode, want_neighbours=True)
        out[mode, k] = (_np(cv), _np(fit.curvature_consensus_batch(X, cnt, cv)))
    torch.cuda.synchronize()
    return out


def _frames(min_points=0):
    return [(f, n, cc.used(c)) for f, (n, c) in enumerate(cc.FRAMES) if cc.used(c) >= min_points]


@pytest.mark.parametrize('mode,k', MODES_KS)
def test_status_zeros_and_no_poison(runs, mode, k):
    cv, con = runs[mode, k]
    for f, name, m in _frames():
        few = m < cc.UNKNOWNS[mode]
        assert cv['status'][f] == (5 if few else 0), name
        live = 0 if few else m
        for key in ('Kdir', 'L', 'normal', 'nbr', 'pt_status'):
            assert not cv[key][f, live:].any(), (name, key)              # zero past the count, and all of a frame with too few points
        assert not con['gate'][f, live:].any(), name
        if few:
            assert con['status'][f] == 5 and con['n_gated'][f] == 0 and not con['axis'][f].any(), name
    for key in ('Kdir', 'L', 'normal'):
        assert np.isfinite(cv[key]).all(), key
    assert np.isfinite(con['axis']).all()
    assert set(np.unique(cv['pt_status'])) <= {0, 1}
    bad = cv['pt_status'] != 0
    assert not cv['Kdir'][bad].any() and not cv['L'][bad].any() and not cv['normal'][bad].any()


@pytest.mark.parametrize('mode,k', MODES_KS)
def test_neighbours_equal_the_reference_exactly(runs, mode, k):
    cv, _ = runs[mode, k]
    for f, name, m in _frames(cc.UNKNOWNS[mode]):
        ref = cc.named_neighbours(name, k)
        K = ref.shape[1]
        assert K == min(k, m)
        assert np.array_equal(cv['nbr'][f, :m, :K], ref), name
        assert (cv['nbr'][f, :m, K:] == -1).all(), name
    f = NAMES.index('dup')
    for p in (3, 7, 100, 200):                                          # ties resolve by index
        assert cv['nbr'][f, p, :4].tolist() == [3, 7, 100, 200]


def test_column_0_has_the_bits_of_the_fits_initial_direction(runs, dev_batch, orc):
    from cpe_amd import fit
    X, cnt = dev_batch
    cv, _ = runs[cc.REFERENCE, 20]
    fitted = _np(fit.fit_cylinder_batch(X, cnt, cc.R, mode=fit.FIT_LM))
    checked = 0
    for f, name, m in _frames(5):
        if name in ('plane', 'tiegrid'):
            continue                # (without noise several points are equally near the axis: which one the start picks is rounding)
        P = cc.named_points(name)
        im = cc.pick_im(P)
        o = orc.fit_cylinder(P, cc.R, mode=1)
        assert fitted['status'][f] == o['status'] == 0, name
        assert cv['pt_status'][f, im] == 0
        got = cv['Kdir'][f, im, 0]
        assert got.tobytes() == fitted['cyl_raw'][f, 0, 3:6].tobytes(), (name, im, got, fitted['cyl_raw'][f, 0, 3:6])
        assert got.tobytes() == o['cyl0'][3:].tobytes(), (name, im)
        checked += 1
    assert checked == 18


@pytest.mark.parametrize('mode,k', MODES_KS)
def test_values_against_lapack(runs, mode, k):
    cv, _ = runs[mode, k]
    worst = 0.0
    for f, name, m in _frames(cc.UNKNOWNS[mode]):
        if name == 'plane' or k not in cc.ks_of(name, mode):
            continue
        ref = cc.reference(name, k, mode, 'lapack')
        fair = ref['cond'] < cc.COND_MAX
        if not fair.any():
            continue                                                    # (as many points as unknowns: the quadric interpolates)
        got = {key: cv[key][f, :m] for key in ('Kdir', 'L', 'normal')}
        assert (cv['pt_status'][f, :m][fair] == 0).all(), name
        eL, eK = cc.value_errors(got, ref)
        den = (ref['cond'] ** 2 + 64.0) * cc.EPS
        ratio = float(max((eL / den)[fair].max(), (eK / den)[fair].max()))
        worst = max(worst, ratio)
        assert ratio <= cc.C_TOL, (name, ratio)
        # the frame: the normal is unit; mode 1: unit columns orthogonal to it; mode 0: both columns have the frame's length
        t = cc.tol(ref['cond'])[fair]
        N, Kd = got['normal'][fair], got['Kdir'][fair]
        assert (np.abs((N ** 2).sum(1) - 1) <= 64 * cc.EPS).all(), name
        assert (np.abs((Kd * N[:, None, :]).sum(2)).max(1) <= t).all(), name
        length = np.sqrt((Kd ** 2).sum(2))
        x0 = np.where(np.abs(N[:, :1]) > 0.9, np.array([[0.0, 1.0, 0.0]]), np.array([[1.0, 0.0, 0.0]]))
        want = 1.0 if mode == cc.INTERCEPT else np.sqrt(1.0 - (N * x0).sum(1) ** 2)[:, None]
        assert (np.abs(length - want).max(1) <= t).all(), name
    print(f'mode {mode} k {k}: largest error / ((cond2^2 + 64) eps) = {worst:.3g}')


@pytest.mark.parametrize('mode,k', MODES_KS)
def test_plane_frame_has_no_curvature_and_no_gated_point(runs, mode, k):
    cv, con = runs[mode, k]
    f = NAMES.index('plane')
    m = len(cc.named_points('plane'))
    cond = cc.reference('plane', k, mode, 'lapack')['cond']
    assert (np.abs(cv['L'][f, :m]).max(1) <= cc.tol(cond)).all()
    assert con['n_gated'][f] == 0 and con['status'][f] == 5 and not con['axis'][f].any() and not con['gate'][f].any()


def test_two_calls_give_equal_bits(runs, dev_batch):
    from cpe_amd import fit
    X, cnt = dev_batch
    for mode, k in ((cc.REFERENCE, 20), (cc.INTERCEPT, 32)):
        cv = fit.est_curvatures_batch(X, cnt, k=k, mode=mode, want_neighbours=True)
        con = _np(fit.curvature_consensus_batch(X, cnt, cv))
        cv = _np(cv)
        for a, b in ((cv, runs[mode, k][0]), (con, runs[mode, k][1])):
            for key in b:
                if isinstance(b[key], np.ndarray):
                    assert a[key].tobytes() == b[key].tobytes(), (mode, k, key)


def test_without_neighbours_and_empty_batch(dev_batch, runs, gpu):
    from cpe_amd import fit
    X, cnt = dev_batch
    cv = _np(fit.est_curvatures_batch(X, cnt))
    assert cv['nbr'] is None and cv['Kdir'].tobytes() == runs[cc.REFERENCE, 20][0]['Kdir'].tobytes()
    e = fit.est_curvatures_batch(X[:0], cnt[:0])
    assert e['L'].shape == (0, cc.MAXP, 2)
    assert fit.curvature_consensus_batch(X[:0], cnt[:0], e)['axis'].shape == (0, 8)


@pytest.mark.parametrize('k,mode', [(4, 0), (5, 1), (33, 0), (33, 1), (20, 2)])
def test_library_refuses_k_and_mode_out_of_range(gpu, dev_batch, k, mode):
    from cpe_amd import lib
    L = lib.load()
    X, cnt = dev_batch
    o = torch.zeros(64, dtype=torch.float64, device=gpu)               # never written: the arguments are refused first
    rc = L.cpe_est_curvatures_batch(X.data_ptr(), cnt.data_ptr(), 1, k, mode, o.data_ptr(), o.data_ptr(), o.data_ptr(), None,
                                    o.data_ptr(), o.data_ptr(), None)
    assert rc == lib.const.ERR_ARG
    assert 'cpe_est_curvatures_batch' in L.cpe_last_error_string().decode()
    assert not o.any()


def _consensus_tolerances(P, ref_cv, ref_con, cond):
    """how far dir, origin and spread of two consensus results may differ when their curvatures differ by tol(cond) per point:
    a unit t moves by at most e_t = 8 tau (its column by tau max |L| / gap <= 4 tau / 3 at rho <= 0.25, then the division by a
    length >= 0.43); sum t t' by 2 g e_t, its first eigenvector by that over the absolute gap; a centre X + n / lambda by
    r (tau + tau); the spread by two such moves and the turn of the axis over the centres' extent"""
    g = ref_con['gate']
    tau = float(cc.tol(cond)[g].max())
    e_dir = 2 * 8 * tau / ref_con['gap'] + 64 * cc.EPS
    r = ref_con['radii'].max()
    e_c = 2 * r * tau + 8 * cc.EPS * np.abs(P).max()
    amax, _, _, big = cc.gate_values(ref_cv['L'])
    c = P[g] + ref_cv['normal'][g] / ref_cv['L'][np.arange(len(P)), big][g, None]
    extent = np.linalg.norm(c - c.mean(0), axis=1).max()
    return e_dir, e_c, 2 * e_c + extent * e_dir


@pytest.mark.parametrize('mode', [cc.REFERENCE, cc.INTERCEPT])
def test_consensus_against_the_reference(runs, mode):
    cv, con = runs[mode, 20]
    seen = 0
    for f, name, m in _frames(cc.UNKNOWNS[mode]):
        if name not in cc.CONSENSUS_NAMES:
            continue
        P = cc.named_points(name)
        ref_cv = cc.reference(name, 20, mode, 'ordered')
        assert cc.clear_of_bounds(ref_cv, cc.GATE_DEFAULT), name
        ref = cc.consensus(P, ref_cv)
        assert np.array_equal(con['gate'][f, :m] != 0, ref['gate']) and con['n_gated'][f] == ref['n_gated'], name
        assert con['status'][f] == ref['status'], name
        if ref['status'] != 0:
            continue
        seen += 1
        # the radius is one of the GPU's own 1 / |lambda|max, the one at the reference's rank
        own = np.sort(cc.gate_values(cv['L'][f, :m])[2][ref['gate']])
        assert con['axis'][f, 6] == own[ref['rank']], name
        e_dir, e_c, e_spread = _consensus_tolerances(P, ref_cv, ref, cc.reference(name, 20, mode, 'lapack')['cond'])
        d = con['axis'][f, 3:6]
        assert d[np.argmax(np.abs(d))] > 0 and abs(np.linalg.norm(d) - 1) < 64 * cc.EPS, name
        assert np.abs(d - ref['axis'][3:6]).max() <= e_dir, (name, np.abs(d - ref['axis'][3:6]).max(), e_dir)
        assert np.abs(con['axis'][f, :3] - ref['axis'][:3]).max() <= e_c, (name, e_c)
        assert abs(con['axis'][f, 7] - ref['axis'][7]) <= e_spread, (name, e_spread)
    assert seen == len(cc.CONSENSUS_NAMES)


@pytest.fixture(scope='module')
def wall(gpu):
    """the grid + plane case through the stereo tables: (tables 1, 2, rig, the numpy + oracle chain)"""
    import oracle
    from cpe_amd import fit
    P, is_cyl, org, d = cc.grid_plus_plane(0)
    t1, t2 = cc.tables_of(P, cc.wall_ids())
    K1, K2, T21 = cc.rig()
    c1, c2, idx = oracle.find_correspondences(t1, t2)
    X, _ = oracle.triangulate(c1, c2, K1, K2, T21)
    assert len(X) == len(P) and np.abs(X - P).max() < 1e-6             # the join keeps the table order here
    cv = cc.ordered(X, 20, cc.INTERCEPT)
    con = cc.consensus(X, cv, cc.GATE_BAND)
    assert cc.clear_of_bounds(cv, cc.GATE_BAND)
    chain = dict(X=X, con=con, gated=oracle.fit_cylinder(X[con['gate']], cc.R, mode=1), plain=oracle.fit_cylinder(X, cc.R, mode=1))
    g1, g2 = fit.GridTables.from_lists([t1], gpu), fit.GridTables.from_lists([t2], gpu)
    return g1, g2, (K1, K2, T21), chain, is_cyl, org, d


def test_grid_beside_a_plane_gates_exactly_the_cylinder(runs, dev_batch):
    from cpe_amd import fit
    X, cnt = dev_batch
    f = NAMES.index('wall')
    P, is_cyl, org, d = cc.grid_plus_plane(0)
    cv = fit.est_curvatures_batch(X[f:f + 1], cnt[f:f + 1], k=20, mode=fit.CURV_INTERCEPT)
    con = _np(fit.curvature_consensus_batch(X[f:f + 1], cnt[f:f + 1], cv, r_min=cc.GATE_BAND[1], r_max=cc.GATE_BAND[2]))
    assert con['n_gated'][0] == 425 and np.array_equal(con['gate'][0, :len(P)] != 0, is_cyl) and con['status'][0] == 0
    assert cc.angle_deg(con['axis'][0, 3:6], d) < 1.0


def test_gated_fit_ends_nearer_the_true_axis_than_the_plain_fit(wall):
    from cpe_amd import fit
    g1, g2, (K1, K2, T21), chain, is_cyl, org, d = wall
    kw = dict(selector=fit.SEL_JOIN, mode=fit.FIT_LM)
    gated = _np({k: v for k, v in fit.fit_single_cylinder_gated_batch(g1, g2, K1, K2, T21, cc.R, curvature=dict(r_min=cc.GATE_BAND[1],
                                                                      r_max=cc.GATE_BAND[2]), **kw).items() if not k.startswith('_')})
    plain = _np({k: v for k, v in fit.fit_single_cylinder_batch(g1, g2, K1, K2, T21, cc.R, **kw).items() if not k.startswith('_')})
    assert gated['status'][0] == plain['status'][0] == chain['gated']['status'] == chain['plain']['status'] == 0
    assert np.array_equal(gated['gate'][0, :len(is_cyl)] != 0, chain['con']['gate']) and gated['n_gated'][0] == 425
    assert np.array_equal(gated['pts3'][0, :len(is_cyl)], chain['X'])
    assert np.array_equal(gated['pts3_gated'][0, :425], chain['X'][chain['con']['gate']]) and not gated['pts3_gated'][0, 425:].any()
    dist = lambda c: cc.line_distance(c[:3], c[3:], org, d)
    want_gated, want_plain = dist(chain['gated']['cyl']), dist(chain['plain']['cyl'])
    got_gated, got_plain = dist(gated['cyl_raw'][0, 1]), dist(plain['cyl_raw'][0, 1])
    print(f'distance of the fitted axis from the true one, mm: gated {got_gated:.4f} (chain {want_gated:.4f}), '
          f'plain {got_plain:.4f} (chain {want_plain:.4f})')
    assert want_gated < want_plain
    assert abs(got_gated - want_gated) <= 1e-6 * want_gated and abs(got_plain - want_plain) <= 1e-6 * want_plain
    assert got_gated < got_plain
    for key in ('offset', 'match_score', 'match_flags', 'curv_axis', 'curv_status', 'cyl', 'T', 'fvals', 'iters', 'm', 'idx'):
        assert key in gated


def test_gated_fit_of_a_clean_frame_has_the_bits_of_the_plain_fit(gpu):
    from cpe_amd import fit
    from test_fit_gpu import make_tables
    t1, t2, K1, K2, T21, fp, sc = make_tables(5, 3, noise=0.03, h=1200, w=1920)
    t1[1] = t1[1][:4]                                                   # a frame that keeps too few points ends like any other
    g1, g2 = fit.GridTables.from_lists(t1, gpu), fit.GridTables.from_lists(t2, gpu)
    wide = dict(rho_max=1e300, r_min=0.0, r_max=math.inf)              # every point with a curvature at all is gated in
    gated = fit.fit_single_cylinder_gated_batch(g1, g2, K1, K2, T21, 45.0, curvature=wide, mode=fit.FIT_LM)
    plain = fit.fit_single_cylinder_batch(g1, g2, K1, K2, T21, 45.0, mode=fit.FIT_LM)
    assert gated['n_gated'].tolist() == [int(plain['m'][0]), 0, int(plain['m'][2])] and int(plain['m'][0]) > 30
    assert gated['status'].tolist() == plain['status'].tolist() == [0, 5, 0]
    for key, v in plain.items():
        if not key.startswith('_'):
            assert gated[key].cpu().numpy().tobytes() == v.cpu().numpy().tobytes(), key


def test_run_experiment_curvature_leaves_the_fits_alone(gpu, tmp_path):
    from cpe_amd import experiment, fit
    from test_plane_pipeline_gpu import _cylinders, _folder
    b = _cylinders()
    args = _folder(tmp_path, b, ['-10', '01']) + (b['radius'],)
    plain = experiment.run_experiment(*args, device=gpu, chunk=1, multi_frame=False)
    res = experiment.run_experiment(*args, device=gpu, chunk=1, multi_frame=False, curvature={})
    assert set(res) == set(plain) | {'curvature'} and res['skipped'] == plain['skipped'] == []
    for key in ('records', 'pts3', 'cnt', 'cyl_raw'):
        assert res[key].cpu().numpy().tobytes() == plain[key].cpu().numpy().tobytes(), key
    cv = fit.est_curvatures_batch(res['pts3'], res['cnt'], k=20, mode=fit.CURV_INTERCEPT)
    con = fit.curvature_consensus_batch(res['pts3'], res['cnt'], cv, r_min=b['radius'] * (1 - 1 / 3), r_max=b['radius'] * (1 + 1 / 3))
    got = res['curvature']
    for key in ('Kdir', 'L', 'normal', 'pt_status'):
        assert got[key].cpu().numpy().tobytes() == cv[key].cpu().numpy().tobytes(), key
    for key in ('axis', 'n_gated', 'gate', 'status'):
        assert got[key].cpu().numpy().tobytes() == con[key].cpu().numpy().tobytes(), key
    assert got['curv_status'].tolist() == [0, 0] and (got['mode'], got['k']) == (fit.CURV_INTERCEPT, 20)
    with pytest.raises(ValueError, match='run_experiment: k 40 must be 6..32 in mode 1'):
        experiment.run_experiment(*args, device=gpu, curvature=dict(k=40))
