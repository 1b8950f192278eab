"""Cases and numpy references for the predicted grid and the re-numbering against it (include/cpe.h cpe_grid_predict_batch and
cpe_grid_assign_batch).  The rig, the tables and the cylinder frame are those of tests/table_tri_cases.py.

ref_grid_predict and ref_grid_assign restate the numbered rules of the header in float64 numpy, in the header's operation order.
The kernels evaluate the same closed forms, so the comparison is at rounding level; the tolerances are derived per node from the
reference's own numbers.  With u = 64 eps (eps = 2^-52; 64 covers the few dozen roundings on the way), per node:

    dq    = u (|p0| + |p1|) / |w|^2          q = (-p0 n1 x w - p1 w x n0) / |w|^2: |n x w| = |w|, and w = n0 x n1 carries an
                                             absolute rounding of a few eps, a relative one of eps / |w|
    eta   = u / |w| + u                      the error of the unit vectors wh and ah
    de    = dq + u (|q| + |o_c|)             e = q - o_c
    dA    = 2 |wp| eta + u A                 A = |wp|^2
    dB    = |ep| eta + |wp| de + u |ep| |wp| B = ep.wp
    dC    = 2 |ep| de + u (|ep|^2 + R^2)     C = |ep|^2 - R^2
    dt    = (dA t^2 + 2 dB |t| + dC) / (2 sqrt(disc)) + u (|B| + sqrt(disc)) / A
                                             t is a root of F(t) = A t^2 + 2 B t + C with F'(t) = +-2 sqrt(disc): a change of
                                             the coefficients moves it by dF / |F'|.  This is the 1 / sqrt(disc) amplification;
                                             step 9 (|nu.wh| = sqrt(disc) / R >= min_cos) bounds it by 1 / (min_cos R)
    tol_X = dq + dt + |t| eta + u (|q| + |t|)                       X = q + t wh
    dXc   = tol_X + u (|X| + |t_j|)                                 Xc = R_j X + t_j
    tol_px = (|K0| + |K1| + |K4|) dXc / Z (1 + max(|Xc|, |Yc|) / Z) + u (|x| + |y| + |K2| + |K5|)

and for the assignment, whose inputs are the same bits on both sides: d1 = sqrt(dx dx + dy dy) with dx, dy single roundings of
exact differences, so tol_dist = 8 eps d1.  stats[1], the largest d1: the largest tol_dist of the image.  stats[0] = sqrt(S / m),
S the sum of the m squares d1^2: a square carries twice its d1's relative error (16 eps) and its own rounding; a sum of m
non-negative terms, added in ANY order (the kernel adds per lane, then by a butterfly, then over the waves; numpy pairwise),
is within (m - 1) eps of the exact sum, relatively.  So either side's S is within (m + 16) eps of the exact one, the two differ by
at most twice that, the root halves it, and the division and the root add a rounding each: tol_rms = (m + 18) eps rms.

Measured over every case here: tol_X <= 3.7e-9 mm and tol_px <= 8.4e-8 px (the reference is 4e-12 mm and 4e-12 px off the
truth at the true pose); TOL_X_BOUND = 1e-8 mm and TOL_PX_BOUND = 2e-7 px below are the bounds the CPU test holds them to.  The
smallest margin of any decision is 2.5e-6 (the gate is 1e-6): disc against 0 at a silhouette node.

`margin` is the smallest relative distance of a decision from its gate: |w|^2 against CPE_PRED_MIN_W2, disc against 0 (disc /
(B^2 + |A C|)), the root choice (||t- - tC| - |t+ - tC|| over their sum), |nu.wh| against min_cos, per camera the depth (Z /
|Xc|), the facing test and the image bound (a conjunction: the smallest margin of the tests when all hold, the largest margin
of a failing test otherwise), d1 against tau_px, d1 against ratio d2, nearest against second nearest ((d2 - d1) / d2 over the
points that bid for a node), and the winner of a node against the runner-up (an exact tie is decided by the slot, an integer,
and has no margin).  Cases are generated so that every margin is above 1e-6; tests/test_grid_predict_cases_cpu.py asserts it
for every case.  Integers, the order and src are compared exactly.

Refinement chain on the CPU (refine_chain below: oracle choose_idx -> triangulate -> fit_cylinder(mode=1), then per round
ref_grid_predict -> ref_grid_assign per image -> join by equal index -> triangulate -> fit_cylinder(mode=1)), on
table_tri_cases.cylinder_frame(0.25, seed), seeds 0..4, 424 points per image, tau_px 4, ratio 0.5; the worst seed:

    scenario                                   first fit                        round 1                          round 2
    off_by_one (10 % of each image's points    117-185 pairs; axis 0.23-1.82    412-423 kept per image, 40-42    418-423 kept; axis 0.016-0.049
      one off in a random component)           deg, 0.24-1.35 mm off            re-numbered; 0.016-0.046 deg     deg, 0.005-0.048 mm
    column_shift (right image: col >= 2        395-398 pairs; 12.1-12.3 mm      54-60 kept per image; 0.23-0.83  415-424 kept, 175 re-numbered;
      numbered one up)                         off                              deg, 0.13-0.93 mm                0.016-0.051 deg, 0.005-0.050 mm
    third_missing (a third of each image's     182-193 pairs (seed 3: 9 pairs,  all but 0-2 detections kept      0.012-0.101 deg, 0.015-0.054 mm
      points missing, independently)           15.5 deg off)                    (seed 3: 157, 149)               (seed 3: 0.027 deg, 0.015 mm)

on rig_table(-16, 16); with noisy_table(seed) the kept counts differ by at most 2 and the axis errors by at most 0.0002 deg and
0.0001 mm in the last round (column_shift seed 4: 0.0512 deg, 0.0503 mm).  No kept point carried a wrong index in any round, seed,
scenario or table.  REFINE_BOUNDS below are twice the worst seed of the last round, the practice of plane_fit_cases.NOISY_BOUNDS."""
import functools
import math

import numpy as np

import plane_fit_cases as PC
import table_tri_cases as TC

MAXP, MAXL, EPS, ST_OK = PC.MAXP, PC.MAXL, PC.EPS, PC.ST_OK
PRED_MAXN, MIN_W2 = 4096, 1e-6
OK, NO_FRAME, NO_PLANE, PARALLEL, MISS, GRAZING = range(6)
U = 64 * EPS
TOL_X_BOUND, TOL_PX_BOUND = 1e-8, 2e-7
RADIUS = TC.RADIUS


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _norm(a):
    return np.sqrt(_dot(a, a))


def _min_margin(cur, vals, mask):
    vals = np.asarray(vals, np.float64)[mask]
    vals = vals[np.isfinite(vals)]
    return min(cur, float(vals.min())) if vals.size else cur


# ------------------------------------------------------------------------------------------------------ the references
def ref_grid_predict(cyl, use, R, K1, K2, T21, P, status, lo, hi, centre, win_lo=None, win_hi=None, min_cos=0.1, img_w=0, img_h=0):
    """one frame.  cyl (6,), use bool -> dict(X (N,3), px (2,N,2), state (N,), vis (N,), counts (4,), tol_X (N,), tol_px (2,N),
    margin, Nu, Nv)"""
    win_lo = (lo, lo) if win_lo is None else win_lo
    win_hi = (hi, hi) if win_hi is None else win_hi
    Nu, Nv = win_hi[0] - win_lo[0] + 1, win_hi[1] - win_lo[1] + 1
    N = Nu * Nv
    assert 1 <= N <= PRED_MAXN and lo <= win_lo[0] and win_hi[0] <= hi and lo <= win_lo[1] and win_hi[1] <= hi
    cyl = np.asarray(cyl, np.float64)
    P, status = np.asarray(P, np.float64), np.asarray(status)
    K = [np.asarray(K1, np.float64).reshape(3, 3), np.asarray(K2, np.float64).reshape(3, 3)]
    T = [np.eye(4), np.asarray(T21, np.float64).reshape(4, 4)]
    centre = np.asarray(centre, np.float64)[:3]
    out = dict(X=np.zeros((N, 3)), px=np.zeros((2, N, 2)), state=np.zeros(N, np.int32), vis=np.zeros(N, np.int32),
               tol_X=np.zeros(N), tol_px=np.zeros((2, N)), Nu=Nu, Nv=Nv)
    margin = math.inf
    with np.errstate(all='ignore'):
        oc, a = cyl[:3], cyl[3:]
        an = float(_norm(a))
        if not use or not np.isfinite(cyl).all() or not np.isfinite(an) or an == 0.0:
            out['state'][:] = NO_FRAME
            out.update(counts=np.zeros(4, np.int32), margin=margin, margins={})
            return out
        ah = a / an
        j = np.arange(N)
        l0, l1 = win_lo[0] + j // Nv - lo, win_lo[1] + j % Nv - lo
        state = np.zeros(N, np.int32)
        alive = np.ones(N, bool)

        def refuse(cond, code):
            nonlocal alive
            hit = alive & cond
            state[hit] = code
            alive = alive & ~cond

        refuse((status[0, l0] != ST_OK) | (status[1, l1] != ST_OK), NO_PLANE)
        n0, p0, n1, p1 = P[0, l0, :3], P[0, l0, 3], P[1, l1, :3], P[1, l1, 3]
        w = _cross(n0, n1)
        w2 = _dot(w, w)
        margins = {}

        def note(name, vals, mask):
            margins[name] = _min_margin(margins.get(name, math.inf), vals, mask)

        note('w2', np.abs(w2 / MIN_W2 - 1), alive)
        refuse(~(w2 >= MIN_W2) | ~np.isfinite(w2), PARALLEL)
        c1, c0 = _cross(n1, w), _cross(w, n0)
        wn = np.sqrt(w2)
        q = ((-p0)[:, None] * c1 - p1[:, None] * c0) / w2[:, None]
        wh = w / wn[:, None]
        e = q - oc
        ea, wa = _dot(e, ah), _dot(wh, ah)
        ep, wp = e - ea[:, None] * ah, wh - wa[:, None] * ah
        A, B, Cq = _dot(wp, wp), _dot(ep, wp), _dot(ep, ep) - R * R
        disc = B * B - A * Cq
        fin = np.isfinite(A) & np.isfinite(B) & np.isfinite(Cq) & np.isfinite(disc)
        note('disc', np.abs(disc) / (B * B + np.abs(A * Cq)), alive & fin & (A != 0))
        refuse(~fin | (A == 0) | ~(disc > 0), MISS)
        s = np.sqrt(disc)
        tm, tp = (-B - s) / A, (-B + s) / A
        tC = _dot(centre - q, wh)
        dm, dp = np.abs(tm - tC), np.abs(tp - tC)
        note('root', np.abs(dm - dp) / (dm + dp), alive)
        t = np.where(dm <= dp, tm, tp)
        X = q + t[:, None] * wh
        refuse(~np.isfinite(X).all(1), MISS)
        g = X - oc
        ga = _dot(g, ah)
        nu = (g - ga[:, None] * ah) / R
        cg = np.abs(_dot(nu, wh))
        note('grazing', np.abs(cg / min_cos - 1), alive)
        refuse(~(cg >= min_cos), GRAZING)
        # the tolerances (module docstring)
        dq = U * (np.abs(p0) + np.abs(p1)) / w2
        eta = U / wn + U
        de = dq + U * (_norm(q) + _norm(oc))
        epn, wpn = _norm(ep), np.sqrt(A)
        dA, dB, dC = 2 * wpn * eta + U * A, epn * eta + wpn * de + U * epn * wpn, 2 * epn * de + U * (epn * epn + R * R)
        dt = (dA * t * t + 2 * dB * np.abs(t) + dC) / (2 * s) + U * (np.abs(B) + s) / A
        tol_X = dq + dt + np.abs(t) * eta + U * (_norm(q) + np.abs(t))
        vis = np.zeros(N, np.int32)
        for c in (0, 1):
            Rj, tj = T[c][:3, :3], T[c][:3, 3]
            oj = -((Rj[0] * tj[0] + Rj[1] * tj[1]) + Rj[2] * tj[2])
            Xc = X if c == 0 else np.stack([((Rj[r, 0] * X[:, 0] + Rj[r, 1] * X[:, 1]) + Rj[r, 2] * X[:, 2]) + tj[r] for r in range(3)], 1)
            Z = Xc[:, 2]
            v = oj - X
            vn = _norm(v)
            nv = _dot(nu, v)
            xn, yn = Xc[:, 0] / Z, Xc[:, 1] / Z
            x = (K[c][0, 0] * xn + K[c][0, 1] * yn) + K[c][0, 2]
            y = K[c][1, 1] * yn + K[c][1, 2]
            tests = [(Z > 0, np.abs(Z) / _norm(Xc)), (nv > min_cos * vn, np.abs(nv / (min_cos * vn) - 1))]
            if img_w > 0 and img_h > 0:
                inside = (x >= 0) & (x < img_w) & (y >= 0) & (y < img_h)
                tests.append((inside, np.minimum(np.minimum(np.abs(x) / img_w, np.abs(x / img_w - 1)),
                                                 np.minimum(np.abs(y) / img_h, np.abs(y / img_h - 1)))))
            allok = np.ones(N, bool)
            m_ok, m_fail = np.full(N, np.inf), np.zeros(N)
            for cond, mg in tests:
                allok &= cond
                m_ok = np.minimum(m_ok, np.where(cond, mg, np.inf))
                m_fail = np.maximum(m_fail, np.where(cond, 0.0, np.nan_to_num(mg, nan=np.inf)))
            seen = alive & allok & np.isfinite(x) & np.isfinite(y)
            note(f'visible {c + 1}', np.where(allok, m_ok, m_fail), alive)
            vis[seen] |= 1 << c
            out['px'][c, seen, 0], out['px'][c, seen, 1] = x[seen], y[seen]
            dXc = tol_X + U * (_norm(X) + float(_norm(tj)))
            kk = abs(K[c][0, 0]) + abs(K[c][0, 1]) + abs(K[c][1, 1])
            tpx = kk * dXc / Z * (1 + np.maximum(np.abs(Xc[:, 0]), np.abs(Xc[:, 1])) / Z) + \
                U * (np.abs(x) + np.abs(y) + abs(K[c][0, 2]) + abs(K[c][1, 2]))
            out['tol_px'][c, seen] = tpx[seen]
        out['X'][alive] = X[alive]
        out['tol_X'][alive] = tol_X[alive]
        out['state'], out['vis'] = state, vis
    out['counts'] = np.array([alive.sum(), (vis & 1).sum(), (vis >> 1).sum(), (vis == 3).sum()], np.int32)
    out['margins'] = margins
    out['margin'] = min(margins.values(), default=math.inf)
    return out


def ref_grid_assign(xy, ids, cnt, px, vis, cam_bit, win_lo, Nu, Nv, tau_px=4.0, ratio=0.5, swap=0):
    """one image.  xy (>=cnt,2), ids (>=cnt,2), px (N,2), vis (N,) -> dict(xy (m,2), id (m,2), src (m,), dist (m,), m, counts (8,),
    stats (2,), node_slot (N,), tol_dist (m,), margin)"""
    n = min(max(int(cnt), 0), MAXP)
    xy = np.asarray(xy, np.float64).reshape(-1, 2)[:n]
    ids = np.asarray(ids).reshape(-1, 2)[:n]
    px, vis = np.asarray(px, np.float64).reshape(-1, 2), np.asarray(vis).reshape(-1)
    N = Nu * Nv
    assert px.shape == (N, 2) and vis.shape == (N,)
    seen = ((vis >> cam_bit) & 1).astype(bool) & np.isfinite(px).all(1)
    margin = math.inf
    node = np.full(n, -1)
    d1, d2 = np.full(n, np.inf), np.full(n, np.inf)
    with np.errstate(all='ignore'):
        for k0 in range(0, n, 256):
            x, y = xy[k0:k0 + 256, 0, None], xy[k0:k0 + 256, 1, None]
            dx, dy = x - px[None, :, 0], y - px[None, :, 1]
            D = dx * dx + dy * dy
            D[:, ~seen] = np.inf
            D[np.isnan(D)] = np.inf
            j1 = D.argmin(1)                                            # the first of the smallest
            b1 = D[np.arange(len(j1)), j1]
            D[np.arange(len(j1)), j1] = np.inf
            b2 = D.min(1) if N > 1 else np.full(len(j1), np.inf)
            node[k0:k0 + 256] = np.where(b1 < np.inf, j1, -1)
            d1[k0:k0 + 256], d2[k0:k0 + 256] = np.sqrt(b1), np.sqrt(b2)
        none = ~np.isfinite(xy).all(1) | (node < 0)
        margin = _min_margin(margin, np.abs(d1 / tau_px - 1), ~none)
        far = ~none & (d1 >= tau_px)
        rest = ~none & ~far
        margin = _min_margin(margin, np.abs(d1 / (ratio * d2) - 1), rest & np.isfinite(d2))
        amb = rest & (d1 > ratio * d2)
        bid = rest & ~amb
        margin = _min_margin(margin, (d2 - d1) / d2, bid & np.isfinite(d2))
    node_slot = np.full(N, -1, np.int32)
    kept = np.zeros(n, bool)
    for jn in np.unique(node[bid]):
        ks = np.nonzero(bid & (node == jn))[0]
        order = sorted(ks, key=lambda k: (d1[k], k))
        kept[order[0]] = True
        node_slot[jn] = order[0]
        if len(order) > 1 and d1[order[1]] != d1[order[0]]:
            margin = min(margin, float(abs(d1[order[1]] - d1[order[0]]) / d1[order[1]]))
    src = np.nonzero(kept)[0].astype(np.int32)
    m = len(src)
    u, v = win_lo[0] + node[src] // Nv, win_lo[1] + node[src] % Nv
    new_id = np.stack([v, u] if swap else [u, v], 1).astype(np.int32).reshape(m, 2)
    same = (new_id == ids[src]).all(1)
    dist = d1[src]
    counts = np.array([m, same.sum(), m - same.sum(), none.sum(), far.sum(), amb.sum(), (bid & ~kept).sum(), 0], np.int32)
    stats = np.array([math.sqrt((dist * dist).sum() / m), dist.max()]) if m else np.zeros(2)
    return dict(xy=xy[src].reshape(m, 2), id=new_id, src=src, dist=dist, m=m, counts=counts, stats=stats, node_slot=node_slot,
                tol_dist=8 * EPS * dist, tol_stats=np.array([(m + 18) * EPS * stats[0], 8 * EPS * stats[1]]), margin=margin)


def compare_predict(got, ref, what=''):
    """got: dict(X (N,3), px (2,N,2), state, vis (N,), counts (4,)) of one frame against ref_grid_predict's"""
    assert np.array_equal(np.asarray(got['state']), ref['state']), f'{what}: state differs'
    assert np.array_equal(np.asarray(got['vis']), ref['vis']), f'{what}: vis differs'
    assert np.array_equal(np.asarray(got['counts']), ref['counts']), f'{what}: counts {np.asarray(got["counts"])} != {ref["counts"]}'
    X, px = np.asarray(got['X']), np.asarray(got['px'])
    assert np.isfinite(X).all() and np.isfinite(px).all(), f'{what}: not finite'
    bad = ref['state'] != OK
    assert not X[bad].any(), f'{what}: X of a refused node is not zero'
    eX = np.abs(X - ref['X']).max(1)
    assert (eX <= ref['tol_X']).all(), f'{what}: X off by {eX.max():.3e}, tolerance {ref["tol_X"][eX.argmax()]:.3e}'
    for c in (0, 1):
        unseen = (ref['vis'] >> c) & 1 == 0
        assert not px[c][unseen].any(), f'{what}: px of camera {c + 1} is not zero where the node is not visible'
        ep = np.abs(px[c] - ref['px'][c]).max(1)
        assert (ep <= ref['tol_px'][c]).all(), f'{what}: px of camera {c + 1} off by {ep.max():.3e}, tolerance {ref["tol_px"][c][ep.argmax()]:.3e}'


def compare_assign(got, ref, what=''):
    """got: dict(xy (MAXP,2), id (MAXP,2), src (MAXP,), dist (MAXP,), m, counts (8,), stats (2,)[, node_slot (N,)]) of one image"""
    m = ref['m']
    assert int(got['m']) == m, f'{what}: m {int(got["m"])} != {m}'
    assert np.array_equal(np.asarray(got['counts']), ref['counts']), f'{what}: counts {np.asarray(got["counts"])} != {ref["counts"]}'
    assert np.array_equal(np.asarray(got['src'])[:m], ref['src']), f'{what}: src differs'
    assert np.array_equal(np.asarray(got['id'])[:m], ref['id']), f'{what}: id differs'
    assert np.array_equal(np.asarray(got['xy'])[:m], ref['xy']), f'{what}: xy is not a copy'
    if got.get('node_slot') is not None:
        assert np.array_equal(np.asarray(got['node_slot']), ref['node_slot']), f'{what}: node_slot differs'
    d, S = np.asarray(got['dist'])[:m], np.asarray(got['stats'])
    assert np.isfinite(d).all() and np.isfinite(S).all(), f'{what}: not finite'
    if m == 0:
        assert not S.any(), f'{what}: stats of an image without kept points are not zero'
        return
    assert (np.abs(d - ref['dist']) <= ref['tol_dist']).all(), f'{what}: dist off by {np.abs(d - ref["dist"]).max():.3e}'
    assert (np.abs(S - ref['stats']) <= ref['tol_stats']).all(), f'{what}: stats {S} != {ref["stats"]} within {ref["tol_stats"]}'


# ------------------------------------------------------------------------------------------------------ poses and tables
def pose(deg=0.0, mm=0.0, c=TC.CYL_C, a=TC.CYL_A):
    """the true cylinder, its axis turned by `deg` about a fixed direction across it and moved by `mm` across it -> cyl (6,)"""
    a = np.asarray(a, np.float64)
    k = np.cross(a, [0.3, 0.1, 1.0]); k /= np.linalg.norm(k)
    th = math.radians(deg)
    a2 = a * math.cos(th) + np.cross(k, a) * math.sin(th) + k * (k @ a) * (1 - math.cos(th))
    side = np.cross(a, k)
    return np.concatenate([np.asarray(c, np.float64) + mm * (0.6 * k + 0.8 * side), 1.7 * a2])      # (the direction is not unit)


POSES = {'true': pose(), 'near': pose(0.4, 0.3), 'far': pose(2.0, 2.0)}
LO, HI = TC.LO, TC.HI


@functools.lru_cache(maxsize=None)
def predict_cases():
    """name -> dict(cyl (n,6), use (n,) or None, table, window or None, params): one call each"""
    t = TC.rig_table(LO, HI)
    three = np.stack([POSES['true'], POSES['near'], POSES['far']])
    c = {}
    c['rig table, three poses'] = dict(cyl=three, use=None, table=t, window=None, params={})
    c['one frame'] = dict(cyl=three[:1], use=None, table=t, window=None, params={})
    c['partly missed'] = dict(cyl=np.stack([pose(0, 0, c=TC.CYL_C + np.array([38.0, 0, 9.0])), pose(1.0, 0.5, c=TC.CYL_C - np.array([41.0, 3.0, 0]))]),
                              use=None, table=t, window=((-8, 8), (-12, 12)), params={})
    c['behind the cameras'] = dict(cyl=np.stack([pose(0, 0, c=np.array([27.0, 0.0, -365.0])), POSES['true']]), use=None, table=t,
                                   window=None, params={})
    c['refused lines'] = dict(cyl=three, use=None, table=TC.main_table(), window=None, params={})
    c['transposed table'] = dict(cyl=three[:2], use=None, table=TC.transposed(TC.main_table()), window=((-12, 12), (-8, 9)), params={})
    c['noisy table'] = dict(cyl=three, use=None, table=TC.noisy_table(0), window=None, params={})
    for name, win in (('1 node', ((0, 0), (0, 0))), ('63 nodes', ((-3, 3), (-4, 4))), ('64 nodes', ((-4, 3), (-4, 3))),
                      ('65 nodes', ((-2, 2), (-6, 6)))):
        c['window of ' + name] = dict(cyl=three[:2], use=None, table=t, window=win, params={})
    c['window of 4096 nodes'] = dict(cyl=three[:2], use=None, table=TC.rig_table(-32, 31), window=None, params={})
    bad = np.stack([POSES['true']] * 7)
    bad[1, 0] = np.nan; bad[2, 4] = np.inf; bad[3, 3:] = 0.0; bad[4, 5] = -np.inf; bad[5, 3:] = 1e200
    c['unusable frames'] = dict(cyl=bad, use=np.array([1, 1, 1, 1, 1, 1, 0], np.uint8), table=t, window=None, params={})
    c['image bound'] = dict(cyl=three, use=None, table=t, window=None, params=dict(img_w=1010, img_h=640))
    c['min_cos 0.4'] = dict(cyl=three[:1], use=None, table=t, window=None, params=dict(min_cos=0.4))
    b65 = np.stack([pose(0.05 * i, 0.03 * i) for i in range(65)])
    c['65 frames'] = dict(cyl=b65, use=(np.arange(65) % 7 != 3).astype(np.uint8), table=t, window=((-8, 8), (-12, 12)), params={})
    for name, case in c.items():
        _settle(name, case)
    return c


_REFS = {}


def _one_reference(case, f):
    a = predict_call_arrays(case)
    use = True if case['use'] is None else bool(case['use'][f])
    return ref_grid_predict(case['cyl'][f], use, RADIUS, a['K1'], a['K2'], a['T21'], a['P'], a['status'], a['lo'], a['hi'], a['centre'],
                            a['win_lo'], a['win_hi'], a['min_cos'], a['img_w'], a['img_h'])


def _settle(name, case):
    """a silhouette node of some pose comes within 1e-6 of disc = 0 now and then: such a frame's axis point is moved along x in steps
    of 1/64 mm until every margin of the frame is above 2e-6 (deterministic; the references are kept for predict_reference)"""
    case['cyl'] = case['cyl'].copy()
    refs = []
    for f in range(len(case['cyl'])):
        for _ in range(16):
            r = _one_reference(case, f)
            if r['margin'] > 2e-6:
                break
            case['cyl'][f, 0] += 1.0 / 64
        refs.append(r)
    _REFS[name] = refs


REFUSED_CALLS = {                                                            # name -> (table range, window, params)
    '4097 nodes': ((-120, 120), ((-8, 8), (-120, 120)), {}),
    'window below lo': ((LO, HI), ((LO - 1, 3), (0, 3)), {}),
    'window above hi': ((LO, HI), ((0, 3), (0, HI + 1)), {}),
    'empty window': ((LO, HI), ((3, 2), (0, 3)), {}),
    'min_cos 0': ((LO, HI), ((0, 3), (0, 3)), dict(min_cos=0.0)),
    'min_cos 1': ((LO, HI), ((0, 3), (0, 3)), dict(min_cos=1.0)),
}


def predict_call_arrays(case):
    """-> dict(K1, K2, T21, P, status, lo, hi, centre, win_lo, win_hi, min_cos, img_w, img_h) of a case of predict_cases()"""
    K1, K2, T21 = PC.rig()[:3]
    t = case['table']
    win = case['window'] or ((t['lo'], t['hi']), (t['lo'], t['hi']))
    prm = dict(dict(min_cos=0.1, img_w=0, img_h=0), **case['params'])
    return dict(K1=K1, K2=K2, T21=T21, P=t['P'], status=t['status'], lo=t['lo'], hi=t['hi'], centre=PC.rig()[5],
                win_lo=(win[0][0], win[1][0]), win_hi=(win[0][1], win[1][1]), **prm)


@functools.lru_cache(maxsize=None)
def predict_reference(name):
    """-> list of ref_grid_predict results, one per frame of the call"""
    predict_cases()
    return _REFS[name]


# ------------------------------------------------------------------------------------------------------ assign cases
def main_pixels():
    """(px (3,2,N,2), vis (3,N)) of the reference for 'rig table, three poses': frame 0 true, 1 near, 2 far"""
    r = predict_reference('rig table, three poses')
    return np.stack([x['px'] for x in r]), np.stack([x['vis'] for x in r])


def main_frames():
    """name -> dict(xy, id[, cnt], pose 0..2, cam 0 / 1): images for calls with the pixels of 'rig table, three poses' (33 x 33
    nodes).  Counts -1, 0, 1, 63, 64, 65; both cameras; every pose; NaN and infinite pixels; indices one off"""
    idx, _, uv1, uv2 = TC.cylinder_frame()
    order = np.random.default_rng(5).permutation(len(idx))
    idx, uv1, uv2 = idx[order], uv1[order], uv2[order]
    c = {}
    for k in (1, 63, 64, 65):
        c[f'count {k}'] = dict(xy=uv1[:k], id=idx[:k], pose=0, cam=0)
    c['count -1'] = dict(xy=uv1[:10], id=idx[:10], cnt=-1, pose=0, cam=0)
    c['count 0'] = dict(xy=uv1[:10], id=idx[:10], cnt=0, pose=0, cam=0)
    for p, name in enumerate(('true', 'near', 'far')):
        c[f'camera 1, {name} pose'] = dict(xy=uv1, id=idx, pose=p, cam=0)
        c[f'camera 2, {name} pose'] = dict(xy=uv2, id=idx, pose=p, cam=1)
    off = idx.copy()
    off[::10, 0] += 1; off[5::10, 1] -= 1
    c['indices one off'] = dict(xy=uv2, id=off, pose=1, cam=1)
    nx = uv1[:300].copy()
    nx[5, 0] = np.nan; nx[63, 1] = np.inf; nx[64] = -np.inf; nx[255, 1] = np.nan; nx[256, 0] = 1e300; nx[299] = [-5000.0, 90.0]
    c['nan pixels'] = dict(xy=nx, id=idx[:300], pose=0, cam=0)
    dup = np.concatenate([uv1[:200], uv1[:40] + np.random.default_rng(9).normal(0, 0.4, (40, 2)), uv1[100:130] + 0.125])
    c['duplicates'] = dict(xy=dup, id=np.concatenate([idx[:200], idx[:40], idx[100:130]]), pose=0, cam=0)
    return c


def main_batches():
    """the images of main_frames() in batches of 1, 3 and 65 -> list of lists of names.  A call has one cam_bit, so every batch
    holds the images of one camera and is ONE call of main_group_calls: 1 and 65 images of camera 1, 3 and 65 of camera 2, the 65
    cycling through all of that camera's images (and with them through the three poses)"""
    fr = main_frames()
    cam1, cam2 = [k for k in fr if fr[k]['cam'] == 0], [k for k in fr if fr[k]['cam'] == 1]
    return [['count 65'], ['camera 2, true pose', 'indices one off', 'camera 2, far pose'], [cam1[i % len(cam1)] for i in range(65)],
            [cam2[i % len(cam2)] for i in range(65)]]


@functools.lru_cache(maxsize=None)
def special_calls():
    """name -> dict(frames, px (n,N,2), vis (n,N), cam_bit, win_lo, Nu, Nv, params): calls with tables of their own.  Conflicts with
    equal distances from mirrored pixels on a dyadic 5 x 5 table; a single visible node; no visible node; a node with a non-finite
    pixel; ratio 1 and a small tau; 2048 and 3000 points against 4096 nodes; swap"""
    c = {}
    jj = np.arange(25)
    grid = np.stack([100.0 + 20.0 * (jj // 5), 200.0 + 20.0 * (jj % 5)], 1)          # node (u, v) = (-2 + j / 5, 3 + j % 5)
    allv = np.full(25, 3, np.int32)
    n12 = grid[12]
    det = np.array([n12 + [0.5, 0.25], n12 - [0.5, 0.25], n12 + [0.5, -0.25], n12 + [1.0, 0.0],        # three at equal d1, then one farther
                    grid[3] + [0.25, 0.0], grid[3] + [0.125, 0.0], grid[3] - [0.125, 0.0],               # the later two tie, both beat slot 4
                    grid[7] + [3.0, 2.0], grid[7] + [9.5, 0.0], grid[8] + [4.5, 0.0], grid[20] + [0.0, 3.9375],
                    grid[24] + [0.0, 4.25], grid[0] - [1.0, 1.0]])
    ids = np.zeros((len(det), 2), np.int32); ids[0] = [0, 5]; ids[5] = [-2, 6]; ids[12] = [-2, 3]
    c['mirrored ties'] = dict(frames=[dict(xy=det, id=ids)], px=grid[None], vis=allv[None], cam_bit=0, win_lo=(-2, 3), Nu=5, Nv=5, params={})
    c['mirrored ties, swap'] = dict(c['mirrored ties'], params=dict(swap=1), cam_bit=1)
    # (a 20 px grid has no ambiguous point below tau_px 4: a wider gate, and two points between nodes)
    c['ambiguous at tau 12'] = dict(c['mirrored ties'], params=dict(tau_px=12.0),
                                    frames=[dict(xy=np.concatenate([det, [grid[16] + [0.0, 9.0], grid[21] + [7.0, 7.0]]]),
                                                 id=np.concatenate([ids, [[1, 4], [2, 4]]]).astype(np.int32))])
    c['ratio 1, tau 0.75'] =dict(c['mirrored ties'], params=dict(ratio=1.0, tau_px=0.75))
    one = np.zeros(25, np.int32); one[12] = 1
    c['single visible node'] = dict(frames=[dict(xy=det, id=ids), dict(xy=det[:1], id=ids[:1])], px=np.stack([grid, grid]),
                                    vis=np.stack([one, one]), cam_bit=0, win_lo=(-2, 3), Nu=5, Nv=5, params={})
    c['no visible node'] = dict(frames=[dict(xy=det, id=ids)], px=grid[None], vis=(allv * 0 + 2)[None], cam_bit=0, win_lo=(-2, 3), Nu=5, Nv=5,
                                params={})
    gn = grid.copy(); gn[12] = [np.nan, 240.0]; gn[3, 1] = np.inf
    c['non-finite node pixels'] = dict(frames=[dict(xy=det, id=ids)], px=gn[None], vis=allv[None], cam_bit=0, win_lo=(-2, 3), Nu=5, Nv=5,
                                       params={})
    c['one node'] = dict(frames=[dict(xy=det, id=ids)], px=grid[None, 12:13], vis=allv[None, :1], cam_bit=1, win_lo=(7, -7), Nu=1, Nv=1,
                         params={})
    big = predict_reference('window of 4096 nodes')[0]
    seen = np.nonzero(big['vis'] & 1)[0]
    rng = np.random.default_rng(21)
    pts = np.concatenate([big['px'][0][seen] + rng.normal(0, 0.3, (len(seen), 2)),
                          big['px'][0][seen[:500]] + rng.normal(0, 0.5, (500, 2)),
                          rng.uniform([300, 0], [1500, 1200], (MAXP, 2))])[:MAXP]
    pts = pts[rng.permutation(MAXP)]
    bid = rng.integers(-40, 40, (MAXP, 2)).astype(np.int32)
    c['count 2048'] = dict(frames=[dict(xy=pts, id=bid), dict(xy=pts, id=bid, cnt=3000), dict(xy=pts[:100], id=bid[:100])],
                           px=np.stack([big['px'][0]] * 3), vis=np.stack([big['vis']] * 3), cam_bit=0, win_lo=(-32, -32), Nu=64, Nv=64,
                           params={})
    return c


def assign_reference(call):
    """call: dict(frames, px, vis, cam_bit, win_lo, Nu, Nv, params) -> list of ref_grid_assign results"""
    return [ref_grid_assign(f['xy'], f['id'], f.get('cnt', len(f['xy'])), call['px'][i], call['vis'][i], call['cam_bit'], call['win_lo'],
                            call['Nu'], call['Nv'], **call['params']) for i, f in enumerate(call['frames'])]


def main_group_calls(names, px, vis):
    """the images `names` of main_frames() as one call per camera (a call has one cam_bit) -> list of call dicts"""
    fr = main_frames()
    calls = []
    for cam in (0, 1):
        ks = [k for k in names if fr[k]['cam'] == cam]
        if ks:
            calls.append(dict(names=ks, frames=[fr[k] for k in ks], px=np.stack([px[fr[k]['pose'], cam] for k in ks]),
                              vis=np.stack([vis[fr[k]['pose']] for k in ks]), cam_bit=cam, win_lo=(LO, LO), Nu=HI - LO + 1,
                              Nv=HI - LO + 1, params={}))
    return calls


# ------------------------------------------------------------------------------------------------------ the refinement chain
SCENARIOS = ('off_by_one', 'column_shift', 'third_missing')


@functools.lru_cache(maxsize=None)
def scenario(name, seed):
    """-> dict(gp1, gp2 (m,4) [x y col row] as the detector would hand them over, true1, true2 (m,2): the true indices)"""
    idx, _, uv1, uv2 = TC.cylinder_frame(0.25, seed)
    rng = np.random.default_rng(8000 + seed)
    i1, i2, k1, k2 = idx.copy(), idx.copy(), np.arange(len(idx)), np.arange(len(idx))
    if name == 'off_by_one':
        for ii in (i1, i2):
            bad = rng.permutation(len(idx))[:len(idx) // 10]
            ii[bad, rng.integers(0, 2, len(bad))] += rng.choice([-1, 1], len(bad)).astype(np.int32)
    elif name == 'column_shift':
        i2[i2[:, 0] >= 2, 0] += 1
    elif name == 'third_missing':
        k1 = np.sort(rng.permutation(len(idx))[:len(idx) - len(idx) // 3])
        k2 = np.sort(rng.permutation(len(idx))[:len(idx) - len(idx) // 3])
    else:
        raise KeyError(name)
    return dict(gp1=np.concatenate([uv1[k1], i1[k1]], 1), gp2=np.concatenate([uv2[k2], i2[k2]], 1), true1=idx[k1], true2=idx[k2])


def refine_chain(gp1, gp2, table, rounds=2, tau_px=4.0, ratio=0.5, points='stereo', cams=None, centre=None, radius=RADIUS, mode=1,
                 image_size=None):
    """the chain of the module docstring on one frame -> dict(first (the first fit's cyl (6,), pairs), rounds: list of dict(a1, a2
    (ref_grid_assign's), pairs, cyl (6,), status)).  points='fused': a round's points are those of
    fused_tri_cases.ref_fused_triangulate on the re-numbered tables, as fit.fit_single_cylinder_refined_batch makes them, and the
    poses are the fit's after applyCylParamsPrior; cams (K1, K2, T21), centre: another rig than plane_fit_cases.rig()"""
    import oracle
    oracle.build()
    K1, K2, T21 = PC.rig()[:3] if cams is None else cams
    centre = PC.rig()[5] if centre is None else centre
    iw, ih = (0, 0) if image_size is None else (image_size[1], image_size[0])
    c1, c2, _, _ = oracle.choose_idx(gp1, gp2, K1, K2, T21)
    X, _ = oracle.triangulate(c1, c2, K1, K2, T21)
    fit = oracle.fit_cylinder(X, radius, mode=mode)
    if points == 'fused':
        fit['cyl'] = oracle.apply_prior(fit['cyl'], X)
    out = dict(first=dict(cyl=fit['cyl'], pairs=len(c1), status=fit['status']), rounds=[])
    cyl, status = fit['cyl'], fit['status']
    for _ in range(rounds):
        if status != 0:
            break
        pr = ref_grid_predict(cyl, True, radius, K1, K2, T21, table['P'], table['status'], table['lo'], table['hi'], centre, img_w=iw,
                              img_h=ih)
        win_lo, Nu, Nv = (table['lo'], table['lo']), pr['Nu'], pr['Nv']
        a1 = ref_grid_assign(gp1[:, :2], gp1[:, 2:].astype(np.int32), len(gp1), pr['px'][0], pr['vis'], 0, win_lo, Nu, Nv, tau_px, ratio)
        a2 = ref_grid_assign(gp2[:, :2], gp2[:, 2:].astype(np.int32), len(gp2), pr['px'][1], pr['vis'], 1, win_lo, Nu, Nv, tau_px, ratio)
        slot2 = {tuple(i): k for k, i in enumerate(a2['id'])}
        pairs = [(k, slot2[tuple(i)]) for k, i in enumerate(a1['id']) if tuple(i) in slot2]
        rec = dict(a1=a1, a2=a2, pairs=len(pairs), cyl=None, status=5, pr=pr)
        if points == 'fused':
            import fused_tri_cases as FC
            tri = FC.ref_fused_triangulate(dict(xy=a1['xy'], id=a1['id']), dict(xy=a2['xy'], id=a2['id']), K1, K2, T21, table['P'],
                                           table['status'], table['lo'], table['hi'])
            rec.update(tri=tri)
            X = tri['X']
        elif len(pairs) >= 5:
            X, _ = oracle.triangulate(a1['xy'][[p for p, _ in pairs]], a2['xy'][[p for _, p in pairs]], K1, K2, T21)
        else:
            X = np.zeros((0, 3))
        if len(X) >= 5:
            fit = oracle.fit_cylinder(X, radius, mode=mode)
            if points == 'fused':
                fit['cyl'] = oracle.apply_prior(fit['cyl'], X)
            rec.update(cyl=fit['cyl'], status=fit['status'])
            if fit['status'] == 0:
                cyl = fit['cyl']
        out['rounds'].append(rec)
    out['cyl'] = cyl
    return out


# twice the worst seed measured, either table (module docstring): degrees between the axes, mm from the true axis point to the
# fitted axis, after the last round
REFINE_BOUNDS = dict(off_by_one=dict(axis_deg=2 * 0.0490, axis_mm=2 * 0.0483), column_shift=dict(axis_deg=2 * 0.0514, axis_mm=2 * 0.0504),
                     third_missing=dict(axis_deg=2 * 0.1012, axis_mm=2 * 0.0543))
