"""Cases and a numpy reference for fused triangulation: both cameras' rays and the laser planes in one solve (include/cpe.h
cpe_fused_triangulate_batch).  The rig, the cylinder, the tables of planes and the one-camera reference
are those of tests/table_tri_cases.py.

ref_fused_triangulate restates the numbered rule of the header in float64 numpy; a one-ray candidate goes through
table_tri_cases.ref_table_triangulate, as the kernel sends it through the one-camera device function.  The tolerances are
derived per accepted point from the reference's own numbers (eps = 2^-52):

    X, pair     tol_X   = 64 eps cond(A) (|X| + max |o_j| + max |P4_k|), A the matrix of step 6 (its right-hand side is made of
                          products of A's terms with o_j and P4_k, so its rounding is eps times these magnitudes, and the solve
                          multiplies it by cond(A); the weights move by a few eps of themselves, which cond(A) covers too)
    X, one ray  tol_X of ref_table_triangulate
    res, plane  tol_X + 64 eps (|n.X| + |P4|), as table_tri_cases derives tol_res
    res, ray    (K_j[0] / s_j) (1 + dist / s_j) (tol_X + 64 eps (|X| + |o_j|)): the distance moves by the point's error and the
                rounding of X - o_j, the depth s_j by as much; 0 for a one-ray point, which holds an exact 0
    stats       the largest ray tolerance (px) and the largest plane tolerance (mm) of the frame

Cases are generated so that every tol_X is <= 1e-6 mm and no decision lies within a relative 1e-6 of its gate
(tests/test_fused_tri_cases_cpu.py asserts both), so m, counts, idx, src, flags and the order are compared exactly.

Measured on this reference (table_tri_cases.cylinder_frame(0.25, seed): an R = 45 mm cylinder at 365 mm, 424 grid points, 0.25 px
pixel noise; defaults sigma_px 0.25, sigma_mm 0.02; seeds 0..4; every point paired), mean point error in mm, best - worst seed:

    table                     fused             two-ray start point X0
    rig_table(-12, 12)        0.1045 - 0.1164   0.1138 - 0.1271
    noisy_table(seed)         0.1044 - 0.1168   0.1138 - 0.1271

With every third point missing from table 2 and another third from table 1 (noisy_case(seed, kind, drop=True)) all 424 points
come back; worst seed: pairs 0.1167 (rig) and 0.1174 (noisy), camera 1 alone 0.1665 and 0.1684, camera 2 alone 0.1656 and 0.1661,
the one-ray values inside table_tri_cases.NOISY_TRI_BOUNDS.  `python tests/fused_tri_cases.py` prints these figures.
NOISY_FUSED_BOUNDS below is twice the worst seed, the practice of table_tri_cases.NOISY_TRI_BOUNDS."""
import functools
import math

import numpy as np

import plane_fit_cases as PC
import table_tri_cases as TC

MAXP, MAXL, EPS, ST_OK = TC.MAXP, TC.MAXL, TC.EPS, TC.ST_OK
TBL = 128                                            # CPE_FIT_TABLE_DIM
FLAG_OVERFLOW, FLAG_TRUNCATED = 2, 4                 # CPE_FIT_FLAG_OVERFLOW, CPE_FUSED_FLAG_TRUNCATED
RAY1, RAY2, PLANE0, PLANE1 = 1, 2, 4, 8
DEFAULTS = dict(swap=0, need_both=0, min_sin=0.01, sigma_px=0.25, sigma_mm=0.02, max_res=0.0, max_px=0.0)
NOISY_SEEDS = TC.NOISY_SEEDS
# twice the worst mean point error in mm over NOISY_SEEDS (module docstring), per table kind, of frames whose points are all pairs
NOISY_FUSED_BOUNDS = dict(rig=dict(mean_mm=2 * 0.1164), noisy=dict(mean_mm=2 * 0.1168))


# ------------------------------------------------------------------------------------------------------ the reference
def _ray(K, T, xy):
    R, t = T[:3, :3], T[:3, 3]
    vy = (xy[1] - K[1, 2]) / K[1, 1]
    vx = (xy[0] - K[0, 2] - K[0, 1] * vy) / K[0, 0]
    d = R.T @ np.array([vx, vy, 1.0])
    return -(R.T @ t), d / np.sqrt(d @ d)


def two_ray_point(rays):
    """the unweighted least-squares point of rays [(o, d), ...]"""
    A = sum(np.eye(3) - np.outer(d, d) for _, d in rays)
    b = sum((np.eye(3) - np.outer(d, d)) @ o for o, d in rays)
    return np.linalg.solve(A, b)


def ref_fused_triangulate(t1, t2, K1, K2, T21, P, status, lo, hi, swap=0, need_both=0, min_sin=0.01, sigma_px=0.25, sigma_mm=0.02,
                          max_res=0.0, max_px=0.0):
    """one frame.  t1, t2: dict(xy (>=cnt,2), id (>=cnt,2)[, cnt]) -> dict(X (m,3), idx (m,2), res (m,4), src (m,3), m, counts
    (6,), stats (4,), flags, X0 (m,3) (the start point; the point itself for one ray), tol_X (m,), tol_res (m,4), cond (m,),
    margin)"""
    K = [np.asarray(K1, np.float64).reshape(3, 3), np.asarray(K2, np.float64).reshape(3, 3)]
    T = [np.eye(4), np.asarray(T21, np.float64).reshape(4, 4)]
    P, status = np.asarray(P, np.float64), np.asarray(status)
    tab = []
    for t in (t1, t2):
        n = min(max(int(t.get('cnt', len(t['xy']))), 0), MAXP)
        tab.append((np.asarray(t['xy'], np.float64).reshape(-1, 2)[:n], np.asarray(t['id']).reshape(-1, 2)[:n].astype(np.int64), n))
    (xy1, id1, n1), (xy2, id2, n2) = tab
    empty = dict(X=np.zeros((0, 3)), idx=np.zeros((0, 2), np.int32), res=np.zeros((0, 4)), src=np.zeros((0, 3), np.int32), m=0,
                 counts=np.zeros(6, np.int32), stats=np.zeros(4), flags=0, X0=np.zeros((0, 3)), tol_X=np.zeros(0), tol_res=np.zeros((0, 4)),
                 cond=np.zeros(0), margin=math.inf)
    first2 = {}
    if n1 > 0 and n2 > 0:
        ids = np.concatenate([id1, id2])
        if (np.ptp(ids, axis=0) >= TBL).any() or (np.abs(ids) > 9999).any():
            return dict(empty, flags=FLAG_OVERFLOW)
        for k in range(n2):
            first2.setdefault((int(id2[k, 0]), int(id2[k, 1])), k)
    cands, taken = [], set()
    for k in range(n1):
        j = first2.get((int(id1[k, 0]), int(id1[k, 1])), -1)
        if j >= 0:
            taken.add(j)
        cands.append((k, j))
    cands += [(-1, k) for k in range(n2) if k not in taken]
    out = {k: [] for k in ('X', 'idx', 'res', 'src', 'X0', 'tol_X', 'tol_res', 'cond')}
    counts = [0] * 6
    margin = math.inf
    one_kw = dict(swap=swap, need_both=need_both, min_sin=min_sin, max_res=max_res)
    with np.errstate(all='ignore'):
        for k1, k2 in cands:
            v = id1[k1] if k1 >= 0 else id2[k2]
            if k1 < 0 or k2 < 0:                                   # one ray: the one-camera rule, unchanged
                cam = 0 if k1 >= 0 else 1
                xy = xy1[k1] if cam == 0 else xy2[k2]
                r = TC.ref_table_triangulate(xy[None], v[None], 1, K[cam], None if cam == 0 else T[1], P, status, lo, hi, **one_kw)
                margin = min(margin, r['margin'])
                if r['m'] == 0:
                    counts[4] += 1
                    continue
                rec = dict(X=r['X'][0], idx=v, res=np.array([0, 0, *r['res'][0]]), src=(1 << cam | int(r['src'][0, 0]) << 2, k1, k2),
                           X0=r['X'][0], tol_X=r['tol_X'][0], tol_res=np.array([0, 0, *r['tol_res'][0]]), cond=1.0)
                kind = 2 + cam
            else:
                px = np.array([*xy1[k1], *xy2[k2]])
                if not np.isfinite(px).all():
                    counts[4] += 1
                    continue
                rays = [_ray(K[0], T[0], xy1[k1]), _ray(K[1], T[1], xy2[k2])]
                X0 = two_ray_point(rays)
                s = [float((X0 - o) @ d) for o, d in rays]
                margin = min([margin] + [abs(sj) / np.linalg.norm(X0 - o) for sj, (o, _) in zip(s, rays)])
                if not all(sj > 0 and np.isfinite(sj) for sj in s):
                    counts[4] += 1
                    continue
                planes = []
                for c in (0, 1):
                    fam, vc = c ^ swap, int(v[c])
                    if lo <= vc <= hi and status[fam, vc - lo] == ST_OK:
                        planes.append((c, P[fam, vc - lo]))
                A, b = np.zeros((3, 3)), np.zeros(3)
                for sj, Kj, (o, d) in zip(s, K, rays):
                    w2 = (Kj[0, 0] / (sj * sigma_px)) ** 2
                    A += w2 * (np.eye(3) - np.outer(d, d))
                    b += w2 * ((np.eye(3) - np.outer(d, d)) @ o)
                for _, pl in planes:
                    A += np.outer(pl[:3], pl[:3]) / sigma_mm ** 2
                    b -= pl[3] * pl[:3] / sigma_mm ** 2
                X = np.linalg.solve(A, b)
                cond = float(np.linalg.cond(A))
                tX = 64 * EPS * cond * (np.linalg.norm(X) + max(np.linalg.norm(o) for o, _ in rays) + max([abs(pl[3]) for _, pl in planes] + [0.0]))
                res, tr, bits = np.zeros(4), np.zeros(4), RAY1 | RAY2
                for j, (Kj, (o, d)) in enumerate(zip(K, rays)):
                    u = X - o
                    sj = u @ d
                    dist = np.linalg.norm(u - sj * d)
                    res[j] = dist * (Kj[0, 0] / sj)
                    tr[j] = (Kj[0, 0] / sj) * (1 + dist / sj) * (tX + 64 * EPS * (np.linalg.norm(X) + np.linalg.norm(o)))
                for c, pl in planes:
                    res[2 + c] = pl[:3] @ X + pl[3]
                    tr[2 + c] = tX + 64 * EPS * (abs(pl[:3] @ X) + abs(pl[3]))
                    bits |= PLANE0 << c
                if not (np.isfinite(X).all() and np.isfinite(res).all() and (res[:2] >= 0).all()):
                    counts[4] += 1
                    continue
                gates = []
                if max_px > 0:
                    gates += [res[j] / max_px for j in (0, 1)]
                if max_res > 0:
                    gates += [abs(res[2 + c]) / max_res for c, _ in planes]
                margin = min([margin] + [abs(g - 1) for g in gates])
                if any(g > 1 for g in gates):
                    counts[4] += 1
                    continue
                rec = dict(X=X, idx=v, res=res, src=(bits, k1, k2), X0=X0, tol_X=tX, tol_res=tr, cond=cond)
                kind = 1
            if len(out['X']) == MAXP:
                counts[5] += 1
                continue
            counts[kind] += 1
            for k, val in rec.items():
                out[k].append(val)
    m = len(out['X'])
    counts[0] = m
    res, src = np.array(out['res']).reshape(m, 4), np.array(out['src'], np.int32).reshape(m, 3)
    stats = np.zeros(4)
    pair = (src[:, 0] & 3) == 3
    if pair.any():
        stats[0], stats[1] = math.sqrt((res[pair, :2] ** 2).sum() / (2 * pair.sum())), res[pair, :2].max()
    nplanes = int(((src[:, 0] & PLANE0) != 0).sum() + ((src[:, 0] & PLANE1) != 0).sum())
    if nplanes:
        stats[2], stats[3] = math.sqrt((res[:, 2:] ** 2).sum() / nplanes), np.abs(res[:, 2:]).max()
    return dict(X=np.array(out['X']).reshape(m, 3), idx=np.array(out['idx'], np.int32).reshape(m, 2), res=res, src=src, m=m,
                counts=np.array(counts, np.int32), stats=stats, flags=FLAG_TRUNCATED if counts[5] else 0,
                X0=np.array(out['X0']).reshape(m, 3), tol_X=np.array(out['tol_X']).reshape(m), tol_res=np.array(out['tol_res']).reshape(m, 4),
                cond=np.array(out['cond']).reshape(m), margin=margin)


def compare_frame(got, ref, what=''):
    """got: dict(pts3 (MAXP,3), idx, res (MAXP,4), src (MAXP,3), m, counts (6,), stats (4,), flags) of one frame against
    ref_fused_triangulate's"""
    m = ref['m']
    assert int(got['m']) == m, f'{what}: m {int(got["m"])} != {m}'
    assert int(got['flags']) == ref['flags'], f'{what}: flags {int(got["flags"])} != {ref["flags"]}'
    assert np.array_equal(np.asarray(got['counts']), ref['counts']), f'{what}: counts {np.asarray(got["counts"])} != {ref["counts"]}'
    assert np.array_equal(np.asarray(got['idx'])[:m], ref['idx']), f'{what}: idx differs'
    assert np.array_equal(np.asarray(got['src'])[:m], ref['src']), f'{what}: src (constraints used, source slots) differs'
    X, r, S = np.asarray(got['pts3'])[:m], np.asarray(got['res'])[:m], np.asarray(got['stats'])
    assert np.isfinite(X).all() and np.isfinite(r).all() and np.isfinite(S).all(), f'{what}: not finite'
    if m == 0:
        assert not S.any(), f'{what}: stats of a frame without points are not zero'
        return
    eX = np.abs(X - ref['X']).max(1)
    assert (eX <= ref['tol_X']).all(), f'{what}: X off by {eX.max():.3e}, tolerance {ref["tol_X"][eX.argmax()]:.3e}'
    er = np.abs(r - ref['res'])
    assert (er <= ref['tol_res']).all(), f'{what}: res off by {er.max(0)} > {ref["tol_res"].max(0)}'
    ts = np.repeat([ref['tol_res'][:, :2].max(), ref['tol_res'][:, 2:].max()], 2)
    assert (np.abs(S - ref['stats']) <= ts).all(), f'{what}: stats {S} != {ref["stats"]} within {ts}'


# ------------------------------------------------------------------------------------------------------ cases
def _tab(uv, idx, sel, cnt=None):
    t = dict(xy=uv[sel], id=idx[sel])
    if cnt is not None:
        t['cnt'] = cnt
    return t


@functools.lru_cache(maxsize=None)
def _orders():
    idx, _, uv1, uv2 = TC.cylinder_frame()
    return idx, uv1, uv2, np.random.default_rng(5).permutation(len(idx)), np.random.default_rng(6).permutation(len(idx))


@functools.lru_cache(maxsize=None)
def board2116():
    """46 x 46 indices -22..23 on a near board (table_tri_cases' 'count 2048'): idx, uv1, uv2"""
    bi, bX = PC.board_hits(*PC.board(-9.0, 14.0, 190.0), range(-22, 24), range(-22, 24))
    uv1, uv2 = PC.project_pair(bX, 0.25, np.random.default_rng(11))
    return bi, uv1, uv2


@functools.lru_cache(maxsize=None)
def frame_cases():
    """name -> (t1, t2) for calls with TC.main_table().  Either table in its own order, so pairs, left-only and right-only points
    interleave; counts -1, 0, 1, 63, 64, 65, 2048 and 3000 on either side; an empty table on either side; duplicates in either
    table; NaN and infinite pixels in either table; indices outside the table of planes; a frame whose indices overflow the
    dense table"""
    idx, uv1, uv2, o1, o2 = _orders()
    n = len(idx)
    c = {}
    for k in (1, 63, 64, 65):
        c[f'counts {k} / all'] = (_tab(uv1, idx, o1[:k]), _tab(uv2, idx, o2))
        c[f'counts all / {k}'] = (_tab(uv1, idx, o1), _tab(uv2, idx, o2[:k]))
    c['counts 200 / 130'] = (_tab(uv1, idx, o1[:200]), _tab(uv2, idx, o2[:130]))
    c['count -1 left'] = (_tab(uv1, idx, o1[:10], -1), _tab(uv2, idx, o2[:150]))
    c['count 0 right'] = (_tab(uv1, idx, o1[:150]), _tab(uv2, idx, o2[:10], 0))
    c['both empty'] = (_tab(uv1, idx, o1[:10], 0), _tab(uv2, idx, o2[:10], -5))
    bi, b1, b2 = board2116()
    c['counts 2048 / 3000'] = (dict(xy=b1[:MAXP], id=bi[:MAXP]), dict(xy=b2[-MAXP:], id=bi[-MAXP:], cnt=3000))
    c['thirds'] = (_tab(uv1, idx, np.arange(n)[np.arange(n) % 3 != 1]), _tab(uv2, idx, np.arange(n)[np.arange(n) % 3 != 2]))
    far = idx + np.int32(1000)                                     # outside [lo, hi]: pairs without a plane, no one-ray point
    c['indices outside the table'] = (dict(xy=uv1[o1[:150]], id=far[o1[:150]]), dict(xy=uv2[o2[:170]], id=far[o2[:170]]))
    # duplicates: slots 3, 70 and 140 of table 1 repeat the index of slot 0 (other pixels); slots 5 and 90 of table 2 repeat the
    # index of its slot 1, slot 100 repeats an index that table 1 does not hold
    d1, d2 = _tab(uv1, idx, o1[:160]), _tab(uv2, idx, o2)
    d1['id'] = d1['id'].copy(); d2['id'] = d2['id'].copy()
    d1['id'][[3, 70, 140]] = d1['id'][0]
    d2['id'][[5, 90]] = d2['id'][1]
    d2['id'][100] = d2['id'][101]
    c['duplicates'] = (d1, d2)
    x1, x2 = _tab(uv1, idx, o1[:140]), _tab(uv2, idx, o2[:300])
    x1['xy'] = x1['xy'].copy(); x2['xy'] = x2['xy'].copy()
    x1['xy'][5, 0] = np.nan; x1['xy'][63, 1] = np.inf; x1['xy'][64] = -np.inf; x1['xy'][139, 1] = np.nan
    x2['xy'][2, 1] = np.nan; x2['xy'][64, 0] = np.inf; x2['xy'][200] = np.nan; x2['xy'][299, 0] = -np.inf
    c['nan pixels'] = (x1, x2)
    ov = _tab(uv1, idx, o1[:100])
    ov['id'] = ov['id'].copy(); ov['id'][77, 0] = idx[:, 0].min() + TBL
    c['index span overflow'] = (ov, _tab(uv2, idx, o2[:100]))
    return c


def batches():
    """the cases of frame_cases() in batches of 1, 3 and 65 frames -> list of (names, frames)"""
    c = frame_cases()
    names = list(c)
    b65 = [names[i % len(names)] for i in range(65)]
    return [(nm, [c[k] for k in nm]) for nm in (['counts 65 / all'], ['counts 1 / all', 'duplicates', 'counts 2048 / 3000'], b65)]


def rig_cams():
    return PC.rig()[:3]


def reference(frame, table, **params):
    K1, K2, T21 = rig_cams()
    return ref_fused_triangulate(frame[0], frame[1], K1, K2, T21, table['P'], table['status'], table['lo'], table['hi'], **params)


@functools.lru_cache(maxsize=None)
def frame_reference(name, need_both=0):
    return reference(frame_cases()[name], TC.main_table(), need_both=need_both)


@functools.lru_cache(maxsize=None)
def truncation_frame():
    """two disjoint tables of 2048 and 100 points, every index with both planes in rig_table(-24, 23): 2148 accepted"""
    bi, bX = PC.board_hits(*PC.board(-9.0, 14.0, 190.0), range(-24, 24), range(-24, 24))
    uv1, uv2 = PC.project_pair(bX, 0.25, np.random.default_rng(12))
    assert len(bi) >= MAXP + 100
    return dict(xy=uv1[:MAXP], id=bi[:MAXP]), dict(xy=uv2[MAXP:MAXP + 100], id=bi[MAXP:MAXP + 100])


@functools.lru_cache(maxsize=None)
def call_cases():
    """name -> dict(frames [(t1, t2), ...], table, params): calls whose table or parameters are not the main ones"""
    idx, uv1, uv2, o1, o2 = _orders()
    fr = (_tab(uv1, idx, o1[:300]), _tab(uv2, idx, o2[:320]))
    t = TC.rig_table(TC.LO, TC.HI)
    allv = tuple(range(TC.LO, TC.HI + 1))
    c = {}
    c['every line refused'] = dict(frames=[fr], table=TC.with_status(t, allv, allv), params={})
    c['L 1'] = dict(frames=[fr, frame_cases()['counts 2048 / 3000']], table=TC.rig_table(0, 0), params={})
    c['L 256'] = dict(frames=[fr, frame_cases()['counts 2048 / 3000']], table=TC.rig_table(-128, 127), params={})
    c['swap'] = dict(frames=[fr], table=TC.transposed(TC.main_table()), params=dict(swap=1))
    c['need_both'] = dict(frames=[fr, frame_cases()['thirds']], table=TC.main_table(), params=dict(need_both=1))
    c['noisy table'] = dict(frames=[fr], table=TC.noisy_table(0), params={})
    c['sigmas'] = dict(frames=[fr], table=TC.main_table(), params=dict(sigma_px=1.0, sigma_mm=0.005))
    moved = dict(t, P=t['P'].copy())
    moved['P'][0, 1 - TC.LO] = t['P'][0, 2 - TC.LO]                # column 1 holds the plane of column 2: an index off by one
    c['index off by one, no gate'] = dict(frames=[fr], table=moved, params={})
    c['index off by one, max_res'] = dict(frames=[fr], table=moved, params=dict(max_res=0.5))
    c['index off by one, max_px'] = dict(frames=[fr], table=moved, params=dict(max_px=2.0))
    c['max_px'] = dict(frames=[fr, frame_cases()['thirds']], table=TC.main_table(), params=dict(max_px=0.3))
    c['max_res'] = dict(frames=[fr], table=TC.noisy_table(0), params=dict(max_res=0.035))
    c['truncation'] = dict(frames=[truncation_frame()], table=TC.rig_table(-24, 23), params={})
    return c


@functools.lru_cache(maxsize=None)
def call_reference(name):
    case = call_cases()[name]
    return [reference(f, case['table'], **case['params']) for f in case['frames']]


def pack2(frames, poison=None):
    """frames: [(t1, t2), ...] -> (xy1, id1, cnt1), (xy2, id2, cnt2) as table_tri_cases.pack makes them"""
    return (TC.pack([f[0] for f in frames], poison), TC.pack([f[1] for f in frames], None if poison is None else poison + 1))


# ------------------------------------------------------------------------------------------------------ noisy chain
@functools.lru_cache(maxsize=None)
def noisy_case(seed, kind, drop=False):
    """the cylinder's pixels of the seed with 0.25 px noise against rig_table(-12, 12) ('rig') or noisy_table(seed) ('noisy');
    drop: every third point missing from table 2, another third from table 1 -> dict(frame, table, Xtrue (of the accepted
    points), ref)"""
    idx, Xt, uv1, uv2 = TC.cylinder_frame(0.25, seed)
    table = TC.rig_table(-12, 12) if kind == 'rig' else TC.noisy_table(seed)
    k = np.arange(len(idx))
    s1, s2 = (k[k % 3 != 1], k[k % 3 != 2]) if drop else (k, k)
    frame = (dict(xy=uv1[s1], id=idx[s1]), dict(xy=uv2[s2], id=idx[s2]))
    ref = reference(frame, table)
    src = ref['src']
    truth = np.where((src[:, 1] >= 0)[:, None], Xt[s1][np.maximum(src[:, 1], 0)], Xt[s2][np.maximum(src[:, 2], 0)])
    return dict(frame=frame, table=table, Xtrue=truth, ref=ref, n_points=len(idx))


def mean_errors(case):
    """mean point error in mm of the fused points that are pairs, of their two-ray start points, and of the one-ray points of
    camera 1 and camera 2 (nan without such points)"""
    r = case['ref']
    e = np.linalg.norm(r['X'] - case['Xtrue'], axis=1)
    e0 = np.linalg.norm(r['X0'] - case['Xtrue'], axis=1)
    rays = r['src'][:, 0] & 3
    mean = lambda a: float(a.mean()) if len(a) else math.nan
    return dict(fused=mean(e[rays == 3]), two_ray=mean(e0[rays == 3]), left=mean(e[rays == 1]), right=mean(e[rays == 2]))


if __name__ == '__main__':
    for kind in ('rig', 'noisy'):
        rows = [mean_errors(noisy_case(s, kind)) for s in NOISY_SEEDS]
        print(kind, 'fused %.4f - %.4f' % (min(r['fused'] for r in rows), max(r['fused'] for r in rows)),
              'two-ray %.4f - %.4f' % (min(r['two_ray'] for r in rows), max(r['two_ray'] for r in rows)))
        rows = [mean_errors(noisy_case(s, kind, True)) for s in NOISY_SEEDS]
        print(kind, 'thirds: fused pairs worst %.4f, left worst %.4f, right worst %.4f' %
              tuple(max(r[k] for r in rows) for k in ('fused', 'left', 'right')))
