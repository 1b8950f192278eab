"""Cases and a numpy reference for single-camera triangulation from the laser-plane table (include/cpe.h
cpe_table_triangulate_batch).  The rig, the boards and the table helpers are those of
tests/plane_fit_cases.py.

ref_table_triangulate restates the numbered rule of the header in float64 numpy.  The kernel evaluates the same closed form, so
the comparison is at rounding level; the tolerances are derived per accepted point from the reference's own numbers (eps = 2^-52):

    X      tol_X   = 64 eps (|X| + sum_k |a_k| (|n_k.o| + |P4_k|) / den)
                     (X = o + s d, s = -sum a_k b_k / den: the products and sums that make s carry a few eps of their magnitudes,
                     as do o, d and the final sum; 64 covers the few dozen roundings on the way)
    res    tol_res = tol_X + 64 eps (|n.X| + |P4|)      (|n| = 1: the point's error, plus the cancellation in n.X + P4)
    stats  rms and max |res|: the largest tol_res of the frame (neither can move by more than a residual does)

Cases are generated so that every tolerance is <= 1e-8 and no decision lies within a relative 1e-6 of its gate (den against
min_sin^2, s against 0 measured as |sum a b| / sum |a b|, |res| against max_res); tests/test_table_tri_cases_cpu.py asserts
both.  Then m, counts, idx, src and the order are compared exactly.

Measured on this reference (the table of ref_index_planes over multi_pose(seed, 12): 12 boards, 0.25 px noise; an R = 45 mm
cylinder at 365 mm, grid -8..8 x -12..12, 0.25 px pixel noise; oracle.fit_cylinder(mode=1) on the points; seeds 0..4, the worst
seed):

    camera 1    points mean 0.1618 mm, worst 0.7149 mm off truth; axis 0.0428 deg, 0.0431 mm off the true axis
    camera 2    points mean 0.1669 mm, worst 0.6556 mm off truth; axis 0.0772 deg, 0.0372 mm off the true axis

(seed 0, camera 1: mean 0.1481 mm, worst 0.5676 mm, plane residuals 0.0199 mm rms, objective 9.90 mm^2.)  The fit is the
build's Levenberg-Marquardt mode, oracle.fit_cylinder(mode=1): the reference's simplex stalls at an objective of 41 and 113 mm^2
on seeds 0 and 1 of camera 1, 1.2 and 2.4 degrees off the axis, which says nothing about the points.

NOISY_TRI_BOUNDS below are twice these, the practice of plane_fit_cases.NOISY_BOUNDS."""
import functools
import math

import numpy as np

import plane_fit_cases as PC

MAXP, MAXL, EPS, ST_OK, ST_FEW_POINTS = PC.MAXP, PC.MAXL, PC.EPS, PC.ST_OK, PC.ST_FEW_POINTS
NOISY_SEEDS = PC.NOISY_SEEDS
RADIUS = 45.0
DEFAULTS = dict(swap=0, need_both=0, min_sin=0.01, max_res=0.0)
# twice the worst value measured over NOISY_SEEDS (module docstring); per camera: mean and worst point error in mm, the fitted
# axis' angle to the true one in degrees and the distance of the true axis point from the fitted axis in mm
NOISY_TRI_BOUNDS = {1: dict(mean_mm=2 * 0.1618, worst_mm=2 * 0.7149, axis_deg=2 * 0.0428, axis_mm=2 * 0.0431),
                    2: dict(mean_mm=2 * 0.1669, worst_mm=2 * 0.6556, axis_deg=2 * 0.0772, axis_mm=2 * 0.0372)}


# ------------------------------------------------------------------------------------------------------ the reference
def ref_table_triangulate(xy, ids, cnt, K, Tc, P, status, lo, hi, swap=0, need_both=0, min_sin=0.01, max_res=0.0):
    """one frame.  xy (>=cnt,2), ids (>=cnt,2), K (3,3), Tc (4,4) or None, P (2,L,4), status (2,L) -> dict(X (m,3), idx (m,2),
    res (m,2), src (m,2), m, counts (4,), stats (2,), tol_X (m,), tol_res (m,2), margin: the smallest relative distance of a
    decision from its gate)"""
    n = min(max(int(cnt), 0), MAXP)
    xy = np.asarray(xy, np.float64).reshape(-1, 2)[:n]
    ids = np.asarray(ids).reshape(-1, 2)[:n]
    K = np.asarray(K, np.float64).reshape(3, 3)
    T = np.eye(4) if Tc is None else np.asarray(Tc, np.float64).reshape(4, 4)
    R, t = T[:3, :3], T[:3, 3]
    P, status = np.asarray(P, np.float64), np.asarray(status)
    L = hi - lo + 1
    assert P.shape == (2, L, 4) and status.shape == (2, L)
    o = -(R.T @ t)
    X, idx, res, src, tol_X, tol_res = [], [], [], [], [], []
    counts = [0, 0, 0, 0]
    margin = math.inf
    with np.errstate(all='ignore'):
        for k in range(n):
            x, y = xy[k]
            vy = (y - K[1, 2]) / K[1, 1]
            vx = (x - K[0, 2] - K[0, 1] * vy) / K[0, 0]
            d = R.T @ np.array([vx, vy, 1.0])
            d = d / np.sqrt(d @ d)
            used = []
            for c in (0, 1):
                fam, v = c ^ swap, int(ids[k, c])
                if lo <= v <= hi and status[fam, v - lo] == ST_OK:
                    pl = P[fam, v - lo]
                    used.append((c, pl, float(pl[:3] @ d), float(pl[:3] @ o + pl[3])))
            if not (np.isfinite(x) and np.isfinite(y)) or not used or (need_both and len(used) < 2):
                counts[2] += 1
                continue
            den = sum(a * a for _, _, a, _ in used)
            if min_sin > 0 and np.isfinite(den):
                margin = min(margin, abs(den / (min_sin * min_sin) - 1))
            if den < min_sin * min_sin or not np.isfinite(den):
                counts[2] += 1
                continue
            sab = sum(a * b for _, _, a, b in used)
            s = -sab / den
            mag = sum(abs(a * b) for _, _, a, b in used)
            if np.isfinite(s) and mag > 0:
                margin = min(margin, abs(sab) / mag)
            if not s > 0 or not np.isfinite(s):
                counts[3] += 1
                continue
            Xk = o + s * d
            r, bits = np.zeros(2), 0
            tX = 64 * EPS * (np.linalg.norm(Xk) + sum(abs(a) * (abs(pl[:3] @ o) + abs(pl[3])) for _, pl, a, _ in used) / den)
            tr = np.zeros(2)
            for c, pl, _, _ in used:
                r[c] = pl[:3] @ Xk + pl[3]
                tr[c] = tX + 64 * EPS * (abs(pl[:3] @ Xk) + abs(pl[3]))
                bits |= 1 << c
            if max_res > 0:
                margin = min(margin, min(abs(abs(r[c]) / max_res - 1) for c, _, _, _ in used))
                if any(abs(r[c]) > max_res for c, _, _, _ in used):
                    counts[3] += 1
                    continue
            X.append(Xk); idx.append(ids[k]); res.append(r); src.append((bits, k)); tol_X.append(tX); tol_res.append(tr)
            counts[1] += len(used) == 2
    m = len(X)
    counts[0] = m
    res_a = np.array(res).reshape(m, 2)
    nu = m + counts[1]
    stats = np.array([math.sqrt((res_a ** 2).sum() / nu), np.abs(res_a).max()]) if m else np.zeros(2)
    return dict(X=np.array(X).reshape(m, 3), idx=np.array(idx, np.int32).reshape(m, 2), res=res_a, src=np.array(src, np.int32).reshape(m, 2),
                m=m, counts=np.array(counts, np.int32), stats=stats, tol_X=np.array(tol_X).reshape(m), tol_res=np.array(tol_res).reshape(m, 2),
                margin=margin)


def compare_frame(got, ref, what=''):
    """got: dict(pts3 (MAXP,3), idx, res, src (MAXP,2), m, counts (4,), stats (2,)) of one frame against ref_table_triangulate's"""
    m = ref['m']
    assert int(got['m']) == m, f'{what}: m {int(got["m"])} != {m}'
    assert np.array_equal(np.asarray(got['counts']), ref['counts']), f'{what}: counts {np.asarray(got["counts"])} != {ref["counts"]}'
    assert np.array_equal(np.asarray(got['idx'])[:m], ref['idx']), f'{what}: idx differs'
    assert np.array_equal(np.asarray(got['src'])[:m], ref['src']), f'{what}: src (planes used, source slot) differs'
    X, r, S = np.asarray(got['pts3'])[:m], np.asarray(got['res'])[:m], np.asarray(got['stats'])
    assert np.isfinite(X).all() and np.isfinite(r).all() and np.isfinite(S).all(), f'{what}: not finite'
    if m == 0:
        assert not S.any(), f'{what}: stats of a frame without points are not zero'
        return
    eX = np.abs(X - ref['X']).max(1)
    assert (eX <= ref['tol_X']).all(), f'{what}: X off by {eX.max():.3e}, tolerance {ref["tol_X"][eX.argmax()]:.3e}'
    er = np.abs(r - ref['res'])
    assert (er <= ref['tol_res']).all(), f'{what}: res off by {er.max():.3e} > {ref["tol_res"].max():.3e}'
    ts = ref['tol_res'].max()
    assert np.abs(S - ref['stats']).max() <= ts, f'{what}: stats {S} != {ref["stats"]} within {ts:.3e}'


# ------------------------------------------------------------------------------------------------------ tables of planes
def table_from_normals(normals, centre, lo, hi):
    """unit normals (2,L,3) of planes through `centre` -> dict(P, status, lo, hi), every line OK"""
    P = np.concatenate([normals, -(normals @ centre)[..., None]], 2)
    return dict(P=P, status=np.zeros(P.shape[:2], np.int32), lo=lo, hi=hi)


@functools.lru_cache(maxsize=None)
def rig_table(lo, hi):
    """the true laser planes of plane_fit_cases.rig(): family 0 = col"""
    return table_from_normals(PC.true_line_planes(lo, hi), PC.rig()[5], lo, hi)


def true_table(scene):
    """the true laser planes of any cpe_amd.synth.Scene, family 0 = col (the first index of synth.ground_truth): lines
    -N..N with N the larger of the scene's half_lines and half_lines_v -> dict(P, status, lo, hi, K1, K2, T21)"""
    from cpe_amd import synth
    K1, K2, T21, Tp = synth.make_rig(scene)
    delta = scene.pitch_px / scene.focal
    N = max(scene.half_lines, scene.half_lines_v)
    nrm = np.zeros((2, 2 * N + 1, 3))
    for j, v in enumerate(range(-N, N + 1)):
        for k, nn in enumerate((np.array([1.0, 0, -v * delta]), np.array([0, 1.0, -v * delta]))):
            w = nn @ Tp[:3, :3]
            nrm[k, j] = w / np.linalg.norm(w)
    return dict(table_from_normals(nrm, -Tp[:3, :3].T @ Tp[:3, 3], -N, N), K1=K1, K2=K2, T21=T21)


def with_status(table, bad0=(), bad1=()):
    """a copy with the named indices of family 0 / 1 refused the way cpe_index_planes_batch writes it: status 5, plane zero"""
    t = dict(table, P=table['P'].copy(), status=table['status'].copy())
    for k, bad in enumerate((bad0, bad1)):
        for v in bad:
            t['P'][k, v - t['lo']] = 0
            t['status'][k, v - t['lo']] = ST_FEW_POINTS
    return t


def transposed(table):
    """the same planes with the families exchanged (a table whose family 0 holds the other index)"""
    return dict(table, P=table['P'][::-1].copy(), status=table['status'][::-1].copy())


@functools.lru_cache(maxsize=None)
def noisy_table(seed):
    """what cpe_index_planes_batch makes of 12 noisy board poses, by its reference: 42 of the 50 lines OK"""
    X, I, cnt = PC.pack([dict(X=f['X'], idx=f['idx']) for f in PC.multi_pose(seed)])
    r = PC.ref_index_planes(X, I, cnt, -12, 12)
    return dict(P=r['P'], status=r['status'], lo=-12, hi=12)


# ------------------------------------------------------------------------------------------------------ hits
CYL_C, CYL_A = np.array([27.0, 0.0, 365.0]), np.array([math.sin(math.radians(3.0)), math.cos(math.radians(3.0)), 0.0])


def cylinder_hits(c=CYL_C, a=CYL_A, R=RADIUS, cols=range(-8, 9), rows=range(-12, 13)):
    """the projector's rays of the indices cols x rows cut with the cylinder (point c, unit axis a, radius R), the nearer cut ->
    idx (m,2) (col,row) int32, X (m,3) exact; rays that miss are left out"""
    K1, K2, T21, Tp, delta, Op = PC.rig()
    ii, jj = np.meshgrid(np.asarray(cols), np.asarray(rows), indexing='ij')
    d = np.stack([ii.ravel() * delta, jj.ravel() * delta, np.ones(ii.size)], 1) @ Tp[:3, :3]
    wv = Op - c
    dp = d - (d @ a)[:, None] * a
    wp = wv - (wv @ a) * a
    A, B, Cc = (dp * dp).sum(1), 2 * dp @ wp, wp @ wp - R * R
    disc = B * B - 4 * A * Cc
    ok = disc > 0
    s = (-B[ok] - np.sqrt(disc[ok])) / (2 * A[ok])
    return np.stack([ii.ravel(), jj.ravel()], 1).astype(np.int32)[ok], Op + s[:, None] * d[ok]


def camera(which):
    """K, Tc of camera 1 or 2 of the rig"""
    K1, K2, T21 = PC.rig()[:3]
    return (K1, None) if which == 1 else (K2, T21)


@functools.lru_cache(maxsize=None)
def cylinder_frame(noise=0.25, seed=0):
    """-> idx (m,2), Xtrue (m,3), uv1, uv2 (m,2): the pixels of both cameras with N(0, noise) px added"""
    idx, X = cylinder_hits()
    uv1, uv2 = PC.project_pair(X, noise, np.random.default_rng(7000 + seed))
    return idx, X, uv1, uv2


def axis_errors(cyl, c=CYL_C, a=CYL_A):
    """a fitted [point, direction] against the true axis -> degrees between the directions, mm from c to the fitted axis"""
    o, d = np.asarray(cyl[:3], np.float64), np.asarray(cyl[3:6], np.float64)
    d = d / np.linalg.norm(d)
    ang = PC.angle(d, a)
    return math.degrees(min(ang, math.pi - ang)), float(np.linalg.norm(np.cross(c - o, d)))


def noisy_errors(X, Xtrue, cyl):
    """in the units of NOISY_TRI_BOUNDS"""
    e = np.linalg.norm(np.asarray(X) - Xtrue, axis=1)
    deg, mm = axis_errors(cyl)
    return dict(mean_mm=float(e.mean()), worst_mm=float(e.max()), axis_deg=deg, axis_mm=mm)


def pack(frames, poison=None):
    """frames: list of dict(xy (m,2), id (m,2), cnt=declared count (default m)) -> xy f64[n,MAXP,2], id i32[n,MAXP,2], cnt i32[n];
    slots from min(m, MAXP) on hold zeros, or with poison=seed NaN / huge pixels and garbage indices"""
    n = len(frames)
    xy, I, cnt = np.zeros((n, MAXP, 2)), np.zeros((n, MAXP, 2), np.int32), np.zeros(n, np.int32)
    if poison is not None:
        rng = np.random.default_rng(poison)
        xy[:] = rng.choice([np.nan, np.inf, -1e300, 1e9, 412.5], size=xy.shape)
        I[:] = rng.choice([0, 1, -2 ** 31, 2 ** 31 - 1, -3], size=I.shape)
    for f, fr in enumerate(frames):
        m = min(len(fr['xy']), MAXP)
        xy[f, :m], I[f, :m] = fr['xy'][:m], fr['id'][:m]
        cnt[f] = fr.get('cnt', len(fr['xy']))
        assert min(max(int(cnt[f]), 0), MAXP) <= m, 'a declared count may not uncover unfilled slots'
    return xy, I, cnt


# ------------------------------------------------------------------------------------------------------ cases
LO, HI = -16, 16
BAD0, BAD1 = (3, 7), (-4, 7)          # refused lines of the main table: 3 in family 0 only, -4 in family 1 only, 7 in both


@functools.lru_cache(maxsize=None)
def main_table():
    return with_status(rig_table(LO, HI), BAD0, BAD1)


@functools.lru_cache(maxsize=None)
def frame_cases():
    """name -> dict(xy, id[, cnt]) of camera 1, for calls with main_table().  Counts -1, 0, 1, 63, 64, 65, 127, 128, 129, 2048,
    3000; refused points at slots 62-66 and 126-130; every point refused; none refused; indices below lo and above hi; NaN and
    infinite pixels"""
    idx, _, uv1, _ = cylinder_frame()
    order = np.random.default_rng(5).permutation(len(idx))
    idx, uv = idx[order], uv1[order]
    c = {}
    for k in (1, 63, 64, 65, 127, 128, 129):
        c[f'count {k}'] = dict(xy=uv[:k], id=idx[:k])
    c['count -1'] = dict(xy=uv[:10], id=idx[:10], cnt=-1)
    c['count 0'] = dict(xy=uv[:10], id=idx[:10], cnt=0)
    # 46 x 46 indices on a near board: -22..23, so indices below lo and above hi are among them
    bi, bX = PC.board_hits(*PC.board(-9.0, 14.0, 190.0), range(-22, 24), range(-22, 24))
    buv = PC.project_pair(bX, 0.25, np.random.default_rng(11))[0]
    c['count 2048'] = dict(xy=buv[:MAXP], id=bi[:MAXP])
    c['count 3000'] = dict(xy=buv[:MAXP], id=bi[:MAXP], cnt=3000)
    good = ~np.isin(idx[:, 0], BAD0 + (7,)) & ~np.isin(idx[:, 1], BAD1 + (7,))
    g_uv, g_idx = uv[good], idx[good]
    c['none refused'] = dict(xy=g_uv[:200], id=g_idx[:200])
    ri = g_idx[:200].copy()
    ri[62:67] = 100                                                # above hi in both components
    ri[126:131] = [-17, -100]                                      # below lo
    c['refused across rounds'] = dict(xy=g_uv[:200], id=ri)
    c['all refused'] = dict(xy=g_uv[:150], id=g_idx[:150] + np.int32(1000))
    one = g_idx[:150].copy()
    one[::3, 0] = 2 ** 31 - 1                                      # one component out of range: the other plane alone
    one[1::3, 1] = -2 ** 31
    c['one component out of range'] = dict(xy=g_uv[:150], id=one)
    nx = uv[:140].copy()
    nx[5, 0] = np.nan; nx[63, 1] = np.inf; nx[64] = -np.inf; nx[139, 1] = np.nan
    c['nan pixels'] = dict(xy=nx, id=idx[:140])
    return c


def batches():
    """the cases of frame_cases() in batches of 1, 3 and 65 frames -> list of (names, frames)"""
    c = frame_cases()
    names = list(c)
    b65 = [names[i % len(names)] for i in range(65)]
    return [(nm, [c[k] for k in nm]) for nm in (['count 65'], ['count 1', 'refused across rounds', 'count 2048'], b65)]


@functools.lru_cache(maxsize=None)
def frame_reference(name, need_both=0, cam=1):
    v = frame_cases()[name]
    t = main_table()
    K, Tc = camera(cam)
    return ref_table_triangulate(v['xy'], v['id'], v.get('cnt', len(v['xy'])), K, Tc, t['P'], t['status'], t['lo'], t['hi'],
                                 need_both=need_both)


@functools.lru_cache(maxsize=None)
def call_cases():
    """name -> dict(frames, table, cam, params): calls whose table or parameters are not the main ones.  Every line refused;
    L = 1 and L = 256; camera 2; a plane that contains the ray (min_sin 0.01 refuses it alone, min_sin 0 accepts it beside a good
    one); a plane behind the camera; the max_res gate on a table with one line's index moved by one; need_both on a noisy table"""
    idx, Xt, uv1, uv2 = cylinder_frame()
    fr1, fr2 = dict(xy=uv1, id=idx), dict(xy=uv2, id=idx)
    c = {}
    t = rig_table(LO, HI)
    c['every line refused'] = dict(frames=[fr1], cam=1, params={},
                                   table=with_status(t, tuple(range(LO, HI + 1)), tuple(range(LO, HI + 1))))
    c['L 1'] = dict(frames=[fr1, frame_cases()['count 2048']], cam=1, table=rig_table(0, 0), params={})
    c['L 256'] = dict(frames=[fr1, frame_cases()['count 2048']], cam=1, table=rig_table(-128, 127), params={})
    c['camera 2'] = dict(frames=[fr2, dict(xy=uv2[:70], id=idx[:70])], cam=2, table=main_table(), params={})
    c['camera 2 both'] = dict(frames=[fr2], cam=2, table=main_table(), params=dict(need_both=1))
    c['noisy table'] = dict(frames=[fr1], cam=1, table=noisy_table(0), params={})
    c['noisy table both'] = dict(frames=[fr1], cam=1, table=noisy_table(0), params=dict(need_both=1))
    # one point, index (2, 5); its ray in camera-1 coordinates is the pixel's
    j = int(np.nonzero((idx[:, 0] == 2) & (idx[:, 1] == 5))[0][0])
    K1 = PC.rig()[0]
    d = np.linalg.solve(K1, np.array([uv1[j, 0], uv1[j, 1], 1.0]))
    d /= np.linalg.norm(d)
    nn = np.cross(d, np.array([0.3, 1.0, 0.2]))
    nn /= np.linalg.norm(nn)                                       # a plane through the camera centre that contains the ray
    contain = dict(t, P=t['P'].copy())
    contain['P'][1, 5 - LO] = [*nn, 0.0]
    one = dict(xy=uv1[j:j + 1], id=idx[j:j + 1])
    c['plane contains the ray, alone'] = dict(frames=[one], cam=1, table=with_status(contain, (2,), ()), params={})
    c['plane contains the ray, beside a good one'] = dict(frames=[one], cam=1, table=contain, params=dict(min_sin=0.0))
    c['plane contains the ray, default min_sin'] = dict(frames=[one], cam=1, table=contain, params={})
    behind = dict(t, P=t['P'].copy())
    behind['P'][0, 2 - LO, 3] = t['P'][0, 2 - LO, :3] @ Xt[j]      # the plane of column 2 moved through -X
    c['plane behind the camera'] = dict(frames=[one], cam=1, table=with_status(behind, (), (5,)), params={})
    moved = dict(t, P=t['P'].copy())
    moved['P'][0, 1 - LO] = t['P'][0, 2 - LO]                      # column 1 holds the plane of column 2: an index off by one
    c['index off by one, no gate'] = dict(frames=[fr1], cam=1, table=moved, params={})
    c['index off by one, max_res'] = dict(frames=[fr1], cam=1, table=moved, params=dict(max_res=0.5))
    c['index off by one, max_res, both'] = dict(frames=[fr1], cam=1, table=moved, params=dict(max_res=0.5, need_both=1))
    return c


@functools.lru_cache(maxsize=None)
def call_reference(name):
    """-> list of ref_table_triangulate results, one per frame of the call"""
    case = call_cases()[name]
    K, Tc = camera(case['cam'])
    t = case['table']
    return [ref_table_triangulate(f['xy'], f['id'], f.get('cnt', len(f['xy'])), K, Tc, t['P'], t['status'], t['lo'], t['hi'], **case['params'])
            for f in case['frames']]


# ------------------------------------------------------------------------------------------------------ noisy chain
@functools.lru_cache(maxsize=None)
def noisy_case(seed, cam):
    """the 12-pose noisy table of the seed and the cylinder's pixels with 0.25 px noise -> dict(frame, table, Xtrue, ref)"""
    idx, Xt, uv1, uv2 = cylinder_frame(0.25, seed)
    t = noisy_table(seed)
    K, Tc = camera(cam)
    uv = uv1 if cam == 1 else uv2
    ref = ref_table_triangulate(uv, idx, len(uv), K, Tc, t['P'], t['status'], t['lo'], t['hi'])
    return dict(frame=dict(xy=uv, id=idx), table=t, Xtrue=Xt[ref['src'][:, 1]], ref=ref)
