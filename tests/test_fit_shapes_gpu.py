"""The geometric kernels (csrc/fit.hip) at the point counts and index ranges they can be given, not only the ones synthetic
scenes happen to produce: wave tails (63 / 64 / 65, 127 / 128 / 129), full CPE_MAXP = 2048 tables, counts the kernels clamp
(> CPE_MAXP, < 0), the small counts where the initial cylinder degenerates, and the 128-wide (col,row) index table.

Every case is run three ways, and the three must agree bit for bit:
  * in a mixed batch whose padding (every slot past a frame's count) is poison -- NaN coordinates, +-9999 indices;
  * the same frames in reverse order, with zero padding;
  * each frame as a batch of one, with poison padding.
The GPU equals the oracle bit for bit (the oracle gets the first min(max(cnt, 0), CPE_MAXP) points), and the numbers that
have an independent statement are checked against one: the cylinder objective in extended precision + math.fsum, the
triangulation against LAPACK's SVD, the mean reprojection error and the multi-frame objective against math.fsum."""
import math

import numpy as np
import pytest
import torch

from test_ransac_gpu import _cyl_points

R = 45.0
EPS = np.finfo(np.float64).eps


def _maxp():
    from cpe_amd.fit import MAXP
    return MAXP


# ---------------------------------------------------------------------------------------------------------- helpers
def _used(cnt):
    return min(max(int(cnt), 0), _maxp())


def _pts_batch(frames, poison):
    """frames: list of (cnt, P (k,3)) -> X f64[n,MAXP,3] (slots past the count are NaN or 0), cnt i32[n]"""
    MAXP = _maxp()
    X = np.full((len(frames), MAXP, 3), np.nan if poison else 0.0)
    cnt = np.zeros(len(frames), np.int32)
    for i, (c, P) in enumerate(frames):
        k = _used(c)
        X[i, :k] = P[:k]
        cnt[i] = c
    return X, cnt


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items() if not k.startswith('_')}


def _same(a, b):
    """bit-identical per-frame outputs (dicts of arrays with the frame on axis 0)"""
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k], equal_nan=True), k


def _three_ways(run, frames, build):
    """run(batch) -> dict of numpy arrays; build(frames, poison) -> batch.  Mixed batch with poison padding, reversed batch
    with zero padding, each frame alone with poison padding: all bit-identical.  Returns the first."""
    n = len(frames)
    mixed = run(build(frames, True))
    rev = run(build(frames[::-1], False))
    for i in range(n):
        _same({k: v[i] for k, v in mixed.items()}, {k: v[n - 1 - i] for k, v in rev.items()})
        alone = run(build(frames[i:i + 1], True))
        _same({k: v[i] for k, v in mixed.items()}, {k: v[0] for k, v in alone.items()})
    return mixed


def _objective_hp(x, P):
    """sum (dist(p, axis) - R)^2 of fitCylinderWPts3.m:44-49, independently of the oracle: the line through x(1:3) and
    x(1:3) + x(4:6) (getDistPts3ToLine's two points, formed in float64 as the reference does), distances in extended
    precision, the sum by math.fsum.  Returns (value, tolerance): 1e-12 relative, or -- where a float64 evaluation of this
    objective cannot be that close -- the rounding model of one: every distance off by ~4 ulp of the largest coordinate
    involved (|p|, |o|, |p - o|; the last one grows without bound when Nelder-Mead slides the origin along the axis, which
    the objective cannot see), the errors independent, so |df| ~ 2 delta sqrt(f) + n delta^2."""
    L = np.longdouble
    x = np.asarray(x, np.float64)
    p1 = x[:3]
    p2 = x[:3] + x[3:]
    v = p2.astype(L) - p1.astype(L)
    Q = P.astype(L) - p1.astype(L)
    al = (Q @ v) / (v @ v)
    e = Q - np.outer(al, v)
    r = (np.sqrt((e * e).sum(1)) - L(R)).astype(np.float64)
    f = math.fsum(r * r)
    M = max(np.abs(P).max(), np.abs(p1).max(), np.linalg.norm(P - p1, axis=1).max())
    delta = 4 * EPS * M
    return f, max(1e-12 * f, 2 * delta * math.sqrt(f) + len(P) * delta * delta)


# ------------------------------------------------------------------------------------------- §1 fit_cylinder_batch
FIT_COUNTS = [0, 1, 2, 3, 4, 5, 6, 19, 20, 21, 63, 64, 65, 127, 128, 129, 1000, 1400, 2047, 2048]


def _lattice():
    """99 noise-free points on a regular (angle, height) lattice of the surface, axis exactly y, in shuffled order: the
    20 nearest neighbours of a point have exactly tied distances (same angle, height +-10, +-20, ...), so the choice
    among them is decided by the ties-by-index rule"""
    th = np.linspace(-0.6, 0.6, 9) + np.pi
    yy = np.arange(-50.0, 51.0, 10.0)
    T, Y = np.meshgrid(th, yy, indexing='ij')
    P = np.stack([R * np.sin(T.ravel()), Y.ravel(), 450.0 + R * np.cos(T.ravel())], 1)
    return P[np.random.default_rng(77).permutation(len(P))], np.array([0, 1.0, 0])


def _fit_frames():
    MAXP = _maxp()
    frames, axes = [], []
    for n in FIT_COUNTS:
        P, ax = _cyl_points(np.random.default_rng(1000 * n + 1), max(n, 1))
        frames.append((n, P[:n])); axes.append(ax)
    full = frames[FIT_COUNTS.index(MAXP)][1]
    for c in (MAXP + 1, 5000):                          # clamped to MAXP: the same 2048 points
        frames.append((c, full)); axes.append(axes[FIT_COUNTS.index(MAXP)])
    frames.append((-1, full[:0])); axes.append(None)
    P, ax = _lattice()
    frames.append((len(P), P)); axes.append(ax)
    return frames, axes


@pytest.mark.gpu
@pytest.mark.parametrize('mode', [0, 1])
def test_fit_cylinder_counts(cpe, orc, gpu, mode):
    from cpe_amd import fit
    MAXP = _maxp()
    frames, axes = _fit_frames()

    def run(b):
        X, cnt = b
        out = fit.fit_cylinder_batch(torch.from_numpy(X).to(gpu), torch.from_numpy(cnt).to(gpu), R, mode=mode)
        torch.cuda.synchronize()
        return _np(out)

    out = _three_ways(run, frames, _pts_batch)
    i_full = FIT_COUNTS.index(MAXP)
    for i, (c, P) in enumerate(frames):
        k = _used(c)
        st = int(out['status'][i])
        ref = orc.fit_cylinder(P[:k], R, mode=mode)
        assert st == ref['status'], (c, st, ref['status'])
        if k < 3:
            assert st == 5, c
        if c > MAXP:                                    # clamped: exactly the cnt = MAXP frame
            _same({q: v[i] for q, v in out.items()}, {q: v[i_full] for q, v in out.items()})
        if st != 0:
            assert st == 5, c
            for q in ('cyl_raw', 'cyl', 'T', 'fvals', 'iters'):
                assert not out[q][i].any(), (c, q)
            continue
        # status 0 implies finite outputs (n = 3, 4 used to return status 0 with NaN)
        assert k >= fit.FIT_MIN_POINTS, c
        for q in ('cyl_raw', 'cyl', 'T', 'fvals'):
            assert np.isfinite(out[q][i]).all(), (c, q)
        # the oracle, bit for bit
        assert np.array_equal(out['cyl_raw'][i, 0], ref['cyl0']), c
        assert np.array_equal(out['cyl_raw'][i, 1], ref['cyl']), c
        assert np.array_equal(out['fvals'][i], ref['fvals']), c
        assert out['iters'][i].tolist() == [ref['iters'], ref['evals']], c
        for r in range(2):
            assert np.array_equal(out['cyl'][i, r], orc.apply_prior(out['cyl_raw'][i, r], P[:k])), (c, r)
        assert np.array_equal(out['T'][i], orc.cyl2T(out['cyl'][i, 1])), c
        # the objective, independently of the oracle
        for r in range(2):
            f, tol = _objective_hp(out['cyl_raw'][i, r], P[:k])
            assert abs(out['fvals'][i, r] - f) <= tol, (c, r, out['fvals'][i, r], f, tol)
        assert out['fvals'][i, 1] <= out['fvals'][i, 0], c
        # what it is for: the axis (gauge-fixed: direction only)
        if k >= 21:
            d = out['cyl'][i, 1, 3:] / np.linalg.norm(out['cyl'][i, 1, 3:])
            ang = np.degrees(np.arccos(min(1.0, abs(float(d @ axes[i])))))
            assert ang < 0.5, (c, ang)
    # the small counts: 3 and 4 points are too few for the local quadric, 5 and 6 are enough
    st = {c: int(out['status'][i]) for i, (c, _) in enumerate(frames)}
    assert [st[c] for c in (0, 1, 2, 3, 4, -1)] == [5] * 6
    assert [st[c] for c in (5, 6, 19, 20, 21, MAXP, MAXP + 1, 5000)] == [0] * 8


# -------------------------------------------------------------------- §2 selection, chooseIdx, triangulation
def _rig():
    from cpe_amd import synth
    sc = synth.Scene(h=2160, w=3840)
    K1, K2, T21, _ = synth.make_rig(sc)
    return np.asarray(K1, np.float64), np.asarray(K2, np.float64), np.asarray(T21, np.float64)


def _project(K, T, X):
    h = np.c_[X, np.ones(len(X))] @ (K @ T[:3]).T
    return h[:, :2] / h[:, 2:]


def _grid(rig, cols, rows, seed, noise=0.05):
    """the (col,row) grid points cols x rows of a cylinder surface in front of the rig, projected into both cameras with pixel
    noise: two full tables [x y col row] in the same (col,row) order"""
    K1, K2, T21 = rig
    C, Rw = np.meshgrid(np.asarray(cols), np.asarray(rows), indexing='ij')
    c, r = C.ravel(), Rw.ravel()
    th = 0.009 * (c - c.mean()) + np.pi
    X = np.stack([R * np.sin(th), 0.9 * (r - r.mean()), 450.0 + R * np.cos(th)], 1)
    rng = np.random.default_rng(seed)
    u1 = _project(K1, np.eye(4), X) + noise * rng.standard_normal((len(X), 2))
    u2 = _project(K2, T21, X) + noise * rng.standard_normal((len(X), 2))
    ids = np.stack([c, r], 1).astype(np.float64)
    return np.c_[u1, ids], np.c_[u2, ids]


def _table_batch(pairs, poison):
    """pairs: list of (t1, t2, cnt1, cnt2) -> (GridTables, GridTables); padding: NaN pixels, +-9999 indices"""
    from cpe_amd import fit
    MAXP = _maxp()
    n = len(pairs)
    out = []
    for side in range(2):
        xy = np.full((n, MAXP, 2), np.nan if poison else 0.0)
        ids = np.zeros((n, MAXP, 2), np.int32)
        if poison:
            ids[:, 0::2] = 9999; ids[:, 1::2] = -9999
        cnt = np.zeros(n, np.int32)
        for i, p in enumerate(pairs):
            t, c = p[side], p[2 + side]
            k = min(_used(c), len(t))
            xy[i, :k] = t[:k, :2]; ids[i, :k] = t[:k, 2:4]
            cnt[i] = c
        out.append(fit.GridTables(torch.from_numpy(xy).cuda(), torch.from_numpy(ids).cuda(), torch.from_numpy(cnt).cuda()))
    return out


def _sel_cases(rig):
    """(name, t1, t2, cnt1, cnt2, expect_overflow)"""
    MAXP = _maxp()
    g1, g2 = _grid(rig, range(-20, 26), range(-10, 36), 1)        # 46 x 46 = 2116 points, negative indices included
    rng = np.random.default_rng(2)
    cases = []
    for n1, n2 in [(1, 1), (63, 64), (64, 65), (65, 63), (1400, 1400), (2047, 2048), (2048, 65), (2048, 2048), (64, 2048)]:
        # the first n1 / n2 grid points in column order (a block, so chooseIdx finds whole 3 x 3 patches), each table in
        # an order of its own; the bigger table holds every key of the smaller one
        a = g1[:n1][rng.permutation(n1)]
        b = g2[:n2][rng.permutation(n2)]
        cases.append((f'{n1}x{n2}', a, b, n1, n2, False))
    # the counts the kernels clamp: a full table with cnt 5000, an empty one with cnt -1
    a, b = g1[:MAXP], g2[:MAXP]
    cases.append(('cnt5000', a, b, 5000, MAXP, False))
    cases.append(('cnt-1', a, b, -1, MAXP, False))
    # duplicate (col,row) keys on both sides, with different pixels: the first occurrence is the one matched
    s1, s2 = _grid(rig, range(0, 12), range(0, 12), 3)
    d1, d2 = _grid(rig, range(0, 12), range(0, 12), 4)
    dup = np.random.default_rng(5).permutation(144)[:40]
    t1 = np.concatenate([s1, d1[dup]])[np.random.default_rng(6).permutation(184)]
    t2 = np.concatenate([d2[dup[::-1]], s2])
    cases.append(('duplicates', t1, t2, len(t1), len(t2), False))
    # index span: 127 accepted, 128 flagged -- in col, then in row; both tables count
    for name, cols, rows in [('span127c', range(-40, 88), range(0, 10)), ('span127r', range(0, 10), range(-70, 58))]:
        a, b = _grid(rig, cols, rows, 7)
        cases.append((name, a, b, len(a), len(b), False))
    for name, axis in [('span128c', 2), ('span128r', 3)]:
        a, b = _grid(rig, range(0, 12), range(0, 12), 8)
        extra = b[:1].copy(); extra[0, axis] = 12 + 116              # one key of table 2 only, 128 away from index 0
        cases.append((name, a, np.concatenate([b, extra]), len(a), len(b) + 1, True))
    # index magnitude: |index| = 9999 accepted, 10000 flagged
    a, b = _grid(rig, range(9988, 10000), range(-9999, -9987), 9)
    cases.append(('mag9999', a, b, len(a), len(b), False))
    for name, (cols, rows) in [('col10000', (range(9989, 10001), range(0, 12))), ('row-10000', (range(0, 12), range(-10000, -9988)))]:
        a, b = _grid(rig, cols, rows, 10)
        cases.append((name, a, b, len(a), len(b), True))
    return cases


def _oracle_select(orc, selector, t1, t2, rig, th):
    K1, K2, T21 = rig
    if selector == 0:
        return orc.choose_idx(t1, t2, K1, K2, T21, 3, th)
    if selector == 1:
        return orc.triangulate_with_threshold(t1, t2, K1, K2, T21, th)
    c1, c2, idx = orc.find_correspondences(t1, t2)
    return c1, c2, idx, False


@pytest.mark.gpu
@pytest.mark.parametrize('selector,th', [(0, 0.3), (1, 0.12), (2, 0.0)])
def test_select_triangulate_shapes(cpe, orc, gpu, selector, th):
    from cpe_amd import fit
    MAXP = _maxp()
    rig = _rig()
    K1, K2, T21 = rig
    cases = _sel_cases(rig)
    frames = [(t1, t2, c1, c2) for _, t1, t2, c1, c2, _ in cases]

    def run(pairs):
        g1, g2 = pairs
        sel = fit.select_triangulate_batch(g1, g2, K1, K2, T21, selector=selector, th=th)
        out = _np(sel)
        if selector == 0:                    # the two halves as entry points of their own: the same numbers
            ch = _np(fit.choose_idx_batch(g1, g2, K1, K2, T21, 3, th))
            for q in ('p1', 'p2', 'idx', 'm', 'flags'):
                assert np.array_equal(ch[q], out[q]), q
        # triangulate_batch on the selected pairs, padding past m poisoned
        p1, p2 = sel['p1'].clone(), sel['p2'].clone()
        pad = torch.arange(MAXP, device=gpu)[None, :] >= sel['m'][:, None]
        p1[pad] = float('nan'); p2[pad] = float('nan')
        tri = _np(fit.triangulate_batch(p1, p2, sel['m'], K1, K2, T21))
        torch.cuda.synchronize()
        assert np.array_equal(tri['pts3'], out['pts3']) and np.array_equal(tri['err'], out['err'])
        assert np.array_equal(tri['mean_err'], out['mean_err'])
        return out

    out = _three_ways(run, frames, _table_batch)
    seen_fallback = False
    for i, (name, t1, t2, c1, c2, over) in enumerate(cases):
        m = int(out['m'][i]); fl = int(out['flags'][i])
        assert bool(fl & fit.FLAG_OVERFLOW) == over, name
        if over or c1 <= 0:
            assert m == 0 and out['mean_err'][i] == 0.0, name
            for q in ('p1', 'p2', 'idx', 'pts3', 'err'):
                assert not out[q][i].any(), (name, q)
            continue
        a, b = t1[:_used(c1)], t2[:_used(c2)]
        r1, r2, idx, fb = _oracle_select(orc, selector, a, b, rig, th)
        assert m == len(r1), (name, m, len(r1))
        assert bool(fl & fit.FLAG_FALLBACK) == fb, name
        seen_fallback |= fb
        assert np.array_equal(out['p1'][i, :m], r1) and np.array_equal(out['p2'][i, :m], r2), name
        assert np.array_equal(out['idx'][i, :m], idx), name
        X, err = orc.triangulate(r1, r2, K1, K2, T21)
        assert np.array_equal(out['pts3'][i, :m], X) and np.array_equal(out['err'][i, :m], err), name
        for q in ('p1', 'p2', 'idx', 'pts3', 'err'):               # nothing written past m
            assert not out[q][i, m:].any(), (name, q)
        if m:
            me = math.fsum(out['err'][i, :m]) / m
            assert abs(out['mean_err'][i] - me) <= 1e-13 * me, (name, out['mean_err'][i], me)
    big = [int(out['m'][i]) for i, c in enumerate(cases) if c[0] == '2048x2048'][0]
    assert big > (1000 if selector != 2 else 2000), big
    if selector == 0:
        assert seen_fallback                                       # the 1 x 1 frame has no 3 x 3 patch


@pytest.mark.gpu
def test_triangulation_at_maxp_matches_lapack(cpe, orc, gpu):
    """m = CPE_MAXP pairs through cpe_triangulate_batch against the DLT restated with LAPACK's SVD (the restatement
    test_fit_init_cpu.py::test_triangulation_matches_lapack_svd applies to the oracle), and meanError against math.fsum"""
    from cpe_amd import fit
    MAXP = _maxp()
    rig = _rig()
    K1, K2, T21 = rig
    t1, t2 = _grid(rig, range(0, 32), range(0, 64), 11, noise=0.3)
    assert len(t1) == MAXP
    p1 = torch.from_numpy(np.ascontiguousarray(t1[None, :, :2])).to(gpu)
    p2 = torch.from_numpy(np.ascontiguousarray(t2[None, :, :2])).to(gpu)
    out = _np(fit.triangulate_batch(p1, p2, torch.tensor([MAXP], dtype=torch.int32, device=gpu), K1, K2, T21))
    X, err = out['pts3'][0], out['err'][0]
    P1 = K1 @ np.eye(4)[:3]; P2 = K2 @ T21[:3]
    u1, u2 = t1[:, :2], t2[:, :2]
    A = np.stack([u1[:, :1] * P1[2] - P1[0], u1[:, 1:] * P1[2] - P1[1], u2[:, :1] * P2[2] - P2[0], u2[:, 1:] * P2[2] - P2[1]], 1)
    v = np.linalg.svd(A)[2][:, -1]
    Xl = v[:, :3] / v[:, 3:]
    assert (np.linalg.norm(X - Xl, axis=1) <= 1e-9 * np.linalg.norm(Xl, axis=1)).all(), np.abs(X - Xl).max()
    h = np.c_[Xl, np.ones(MAXP)]
    q1 = h @ P1.T; q2 = h @ P2.T
    el = (np.linalg.norm(u1 - q1[:, :2] / q1[:, 2:], axis=1) + np.linalg.norm(u2 - q2[:, :2] / q2[:, 2:], axis=1)) / 2
    assert (np.abs(err - el) <= 1e-9 * el).all(), np.abs(err / el - 1).max()
    me = math.fsum(err) / MAXP
    assert abs(out['mean_err'][0] - me) <= 1e-13 * me


@pytest.mark.gpu
def test_overflowing_frame_in_the_whole_chain(cpe, orc, gpu):
    """fit_single_cylinder_batch with a frame whose indices span 128 in the middle of good frames: that frame ends in
    CPE_ST_OVERFLOW with zero outputs, its neighbours are exactly what they are without it"""
    from cpe_amd import fit
    rig = _rig()
    K1, K2, T21 = rig
    good = [_grid(rig, range(0, 14), range(0, 20), 20 + s) for s in range(4)]
    a, b = _grid(rig, range(0, 14), range(0, 20), 30)
    extra = a[:1].copy(); extra[0, 2] = 128                        # one left-table key 128 columns away
    bad = (np.concatenate([a, extra]), b)
    with_bad = good[:2] + [bad] + good[2:]

    def run(tabs):
        g1, g2 = _table_batch([(p, q, len(p), len(q)) for p, q in tabs], True)
        out = _np(fit.fit_single_cylinder_batch(g1, g2, K1, K2, T21, R))
        torch.cuda.synchronize()
        return out

    out, ref = run(with_bad), run(good)
    assert int(out['flags'][2]) & fit.FLAG_OVERFLOW
    assert int(out['status'][2]) == fit.ST_OVERFLOW and int(out['m'][2]) == 0
    for q in ('cyl_raw', 'cyl', 'T', 'fvals', 'iters', 'pts3', 'mean_err'):
        assert not out[q][2].any(), q
    for i, j in [(0, 0), (1, 1), (3, 2), (4, 3)]:
        assert int(out['status'][i]) == 0
        _same({q: v[i] for q, v in out.items()}, {q: v[j] for q, v in ref.items()})
        r = orc.fit_single_cylinder(good[j][0], good[j][1], K1, K2, T21, R)
        assert np.array_equal(out['cyl'][i], r['cyl']) and np.array_equal(out['T'][i], r['T'])


# ---------------------------------------------------------------------------- §3 RANSAC at config-5 shapes
RANSAC_KW = dict(hypotheses=64, sample=12, tau=0.4, seed=77, hyp_iters=8)


def _ransac_check(orc, out, frames, mode, frame0):
    MAXP = _maxp()
    for i, (c, P) in enumerate(frames):
        k = _used(c)
        ref = orc.fit_cylinder_ransac(P[:k], R, frame=frame0 + i, mode=mode, **RANSAC_KW)
        st = int(out['status'][i])
        assert st == ref['status'], (c, st)
        assert not out['inlier_mask'][i, k:].any(), c
        if st != 0:
            assert st == 5, c
            assert int(out['n_inliers'][i]) == 0 and not out['inlier_mask'][i].any(), c
            for q in ('cyl_raw', 'cyl', 'T', 'fvals', 'iters'):
                assert not out[q][i].any(), (c, q)
            continue
        for q in ('cyl_raw', 'cyl', 'T', 'fvals'):
            assert np.isfinite(out[q][i]).all(), (c, q)
        assert int(out['n_inliers'][i]) == ref['n_inliers'], c
        assert np.array_equal(out['inlier_mask'][i, :k], ref['mask']), c
        assert np.array_equal(out['cyl_raw'][i, 0], ref['cyl0']), c
        assert np.array_equal(out['cyl_raw'][i, 1], ref['cyl']), c
        assert np.array_equal(out['fvals'][i], ref['fvals']), c
        assert out['iters'][i].tolist() == [ref['iters'], ref['evals']], c
        Q = P[:k][ref['mask'] > 0]
        assert np.array_equal(out['cyl'][i, 1], orc.apply_prior(ref['cyl'], Q)), c
        assert k <= MAXP


def _ransac_three_ways(gpu, mode, frames, frame0):
    """as _three_ways, except that a hypothesis' subset is drawn from (seed, frame0 + f, h, k): a frame moved to another
    batch position keeps its stream when frame0 moves with it"""
    from cpe_amd import fit

    def run(fr, f0, poison):
        X, cnt = _pts_batch(fr, poison)
        out = fit.fit_cylinder_ransac_batch(torch.from_numpy(X).to(gpu), torch.from_numpy(cnt).to(gpu), R, frame0=f0,
                                            mode=mode, **RANSAC_KW)
        torch.cuda.synchronize()
        return _np(out)

    n = len(frames)
    mixed = run(frames, frame0, True)
    rev = run(frames[::-1], frame0 - (n - 1), False)      # frame i sits at position n-1-i: frame0 + i all the same
    for i in range(n):
        _same({k: v[i] for k, v in mixed.items()}, {k: v[n - 1 - i] for k, v in rev.items()})
        alone = run(frames[i:i + 1], frame0 + i, True)
        _same({k: v[i] for k, v in mixed.items()}, {k: v[0] for k, v in alone.items()})
    return mixed


@pytest.mark.gpu
@pytest.mark.parametrize('mode', [1, 0])
def test_ransac_config5_counts(cpe, orc, gpu, mode):
    """n = 1400 (a 3840x2160 frame) and 2048 = CPE_MAXP, 64 hypotheses of 12, gross outliers in both"""
    rng = np.random.default_rng(41)
    frames, n_out = [], [60, 100]
    for n, no in zip([1400, 2048], n_out):
        P, _ = _cyl_points(rng, n, n_out=no)
        frames.append((n, P))
    out = _ransac_three_ways(gpu, mode, frames, 3)
    _ransac_check(orc, out, frames, mode, 3)
    for i, (n, _) in enumerate(frames):
        assert int(out['status'][i]) == 0 and int(out['n_inliers'][i]) >= 0.9 * (n - n_out[i])


@pytest.mark.gpu
@pytest.mark.parametrize('mode', [1, 0])
def test_ransac_small_counts(cpe, orc, gpu, mode):
    """3 to 11 points: fewer than the sample size, so every hypothesis takes all of them"""
    rng = np.random.default_rng(43)
    frames = [(n, _cyl_points(rng, n)[0]) for n in range(3, 12)]
    out = _ransac_three_ways(gpu, mode, frames, 20)
    _ransac_check(orc, out, frames, mode, 20)
    assert [int(s) for s in out['status'][:2]] == [5, 5]


# ---------------------------------------------------------------------------------- §4 multi-frame objective
@pytest.mark.gpu
def test_multi_frame_terms_counts(cpe, orc, gpu):
    from cpe_amd import multiframe
    from test_multiframe_gpu import make_scene
    MAXP = _maxp()
    counts = [0, 1, 64, 65, MAXP]
    P, _, angles, Ttrue = make_scene(F=len(counts), seed=3, npts=MAXP)
    TAGV = np.stack([orc.get_TAGVcyl(*a) for a in angles])
    x0 = orc.T2vec(Ttrue)

    def objective(idx, poison):
        Q = np.full((len(idx), MAXP, 3), np.nan if poison else 0.0)
        cnt = np.array([counts[i] for i in idx], np.int32)
        for j, i in enumerate(idx):
            Q[j, :counts[i]] = P[i, :counts[i]]
        obj = multiframe.MultiFrameObjective(torch.from_numpy(Q).to(gpu), torch.from_numpy(cnt).to(gpu),
                                             TAGV[idx].ravel().tolist(), R)
        return obj, Q, cnt

    order = list(range(len(counts)))
    for x in (x0, x0 + 0.01):
        obj, Q, cnt = objective(order, True)
        v = obj(list(x))
        assert v == orc.multi_objective(x, np.where(np.isnan(Q), 0.0, Q), cnt, TAGV, R)
        assert v == objective(order, False)[0](list(x))
        # each frame alone (batch of one, poison padding) gives the term the batch added, in frame order
        terms = [objective([i], True)[0](list(x)) for i in order]
        s = 0.0
        for t in terms:
            s = s + t
        assert s == v
        rev = objective(order[::-1], False)[0]
        rev(list(x))
        assert rev.terms.tolist() == terms[::-1]
        # math.fsum restatement: sum over frames of mean((d - R)^2), distances in extended precision
        T = np.asarray(orc.vec2T(x)).reshape(4, 4)
        L = np.longdouble
        ref = []
        for i, n in enumerate(counts):
            if n == 0:
                ref.append(0.0)
                continue
            A = T @ TAGV[i].reshape(4, 4)
            o, dy = A[:3, 3], A[:3, 1]
            vv = (o + dy).astype(L) - o.astype(L)
            Qd = P[i, :n].astype(L) - o.astype(L)
            e = Qd - np.outer((Qd @ vv) / (vv @ vv), vv)
            r = (np.sqrt((e * e).sum(1)) - L(R)).astype(np.float64)
            ref.append(math.fsum(r * r) / n)
        want = math.fsum(ref)
        assert abs(v - want) <= 1e-12 * want, (v, want)
