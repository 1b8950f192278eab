"""Cases and the numpy reference for the cylinder pose fitted to the pixels of both images (include/cpe.h
cpe_fit_cylinder_pixels_batch).  The rig, the tables and the cylinder frame are those of
tests/table_tri_cases.py; the prediction is that of tests/grid_predict_cases.py.

ref_pixel_fit restates the header's numbered rule in float64 numpy: `node` holds steps 3 - 9 of ref_grid_predict for one node per
detection (the same expressions in the same order, with the same tolerances; tests/test_pixel_fit_cases_cpu.py asserts that it
gives ref_grid_predict's bits), `project` step 10's formula, `jacobian` rule 7, and `lm_minimize` the loop described in the
comment above lm_minimize in csrc/fit.hip (the damped system is solved by numpy's LU instead of the kernel's elimination).

What the GPU is held to:
    counts, pt_state, status       exactly: every decision of a case (planes, |w|^2, disc, root, grazing, depth, gate) has a
                                   relative margin above 1e-6, which the CPU test asserts for every frame of every case
    res, X at the RETURNED pose    the reference evaluated at that pose, within ref_grid_predict's own tol_px / tol_X, plus
                                   2 eps |p| for the subtraction of the detected pixel
    fvals[1], stats                the sums of those residuals: a sum of m non-negative squares added in any order is within
                                   (m - 1) eps of the exact one, so two such sums differ by (2 m + 18) eps relatively at most
                                   (grid_predict_cases' bound, here without halving by the root)
    cyl, fvals[1]                  scipy.optimize.least_squares(method='lm', analytic Jacobian, xtol = ftol = gtol = 1e-15)
                                   from the same start: the gauge-fixed pose (unit direction with d_y >= 0; the axis point nearest
                                   to cyl0's point) within PIXFIT_POSE_BOUND, f / f_ls - 1 within PIXFIT_F_BOUND.  Both are twice
                                   the worst the restated loop itself shows against scipy over every well-posed frame of every
                                   case here whose loop met no NaN trial (measured, tests/test_pixel_fit_cases_cpu.py prints them):
                                   pose 7.31e-8 (mm or radians; the worst are frames of one camera, whose valley is flat: their
                                   f agrees to 3e-13), f / f_ls - 1 6.27e-13.  A frame is well-posed when the Jacobian at scipy's
                                   optimum has four singular values above 1e-6 of the largest (six unknowns, two gauge
                                   directions); the pose of the others (a single node) is not unique and only f is compared.  A
                                   frame whose restated loop met a NaN trial (a member of S reached the grazing gate: 'min_cos
                                   0.4' frame 0) minimises under a constraint scipy does not have and is compared with neither.
    iters[0]                       at most 3 x the restated loop's

Accuracy (accuracy_chain below; seeds 0..29, table_tri_cases.cylinder_frame(0.25, seed), 424 points per image; the start is the
oracle chain choose_idx -> triangulate -> fit_cylinder(mode=1); axis angle and distance of the true axis point from the fitted
axis, rms over the seeds, the worst seed in brackets; LM iterations 3 - 6, pixel rms 0.342 - 0.368 = 0.25 sqrt 2 with all
detections):

    table                  detections                      start (3-D fit)                            pixel fit
    rig_table(-16, 16)     all                             0.0352 deg (0.0654), 0.0207 mm (0.0482)    0.0238 deg (0.0519), 0.0117 mm (0.0225)
    noisy_table(seed % 5)  all                             0.0352 deg (0.0654), 0.0207 mm (0.0482)    0.0242 deg (0.0553), 0.0120 mm (0.0234)
    rig_table(-16, 16)     a third of each image missing   23.5 deg (88.4), 5.30 mm (21.7)            20.8 deg (86.3), 0.83 mm (4.07)
      the 25 seeds whose start is within 1 deg             0.1038 deg (0.4478), 0.0343 mm (0.0996)    0.0486 deg (0.1766), 0.0226 mm (0.0762)
    noisy_table(seed % 5)  a third missing, those 25       0.1038 deg (0.4478), 0.0343 mm (0.0996)    0.0492 deg (0.1788), 0.0230 mm (0.0772)

With a third of each image missing choose_idx loses most pairs on seeds 4, 11, 20, 22 and 28 and the oracle chain's start is 3 -
88 degrees off.  The pixel fit brings seeds 11, 20 and 28 back (0.05, 0.02, 0.01 deg) and not seeds 4 and 22, whose starts are 88
degrees off: half of their detections have no node at such a pose.  On seeds 25 and 26 (seed 25: a start 0.45 deg off) members of S
reach the grazing gate on the way, the NaN trials hold the loop back (44 iterations on seed 25) and it ends 0.18 deg off: S is
fixed at the start pose, so the fit is as good as the start is near.  ACCURACY_BOUNDS are twice the worst seed, for `third` over
those 25 seeds.

Scenarios (grid_predict_cases.scenario, seeds 0..4): after refine_chain's last round the pixel fit with gate_px = 4 on the
re-numbered tables stays inside REFINE_BOUNDS (0.007 - 0.034 deg, 0.002 - 0.032 mm; the round's own fit: 0.016 - 0.051 deg, 0.005 -
0.050 mm).  WITHOUT re-numbering, from that same good start, the gate repairs nothing and is not claimed to: it drops the
detections whose wrong index moves the predicted pixel by 4 px or more (82 - 84 of 84 in off_by_one, all 175 in column_shift: one
index step is 15 - 25 px; the rest are refused for a missing plane or node), and the fit of what is left is as good (0.004 - 0.042
deg).  From a start that the wrong indices have already spoiled the gate would drop most of the image instead."""
import functools
import math

import numpy as np

import grid_predict_cases as G
import plane_fit_cases as PC
import table_tri_cases as TC

MAXP, EPS, ST_OK, ST_FEW_POINTS = PC.MAXP, PC.EPS, PC.ST_OK, PC.ST_FEW_POINTS
MIN_PTS = 6
RADIUS = TC.RADIUS
U = G.U
PIXFIT_POSE_BOUND, PIXFIT_F_BOUND = 2 * 7.31e-8, 2 * 6.27e-13
# twice the worst seed of the pixel fit (module docstring; `third`: over the seeds with a start within 1 degree): table kind ->
# detections -> (degrees, mm)
ACCURACY_BOUNDS = dict(rig=dict(all=(2 * 0.0519, 2 * 0.0225), third=(2 * 0.1766, 2 * 0.0762)),
                       noisy=dict(all=(2 * 0.0553, 2 * 0.0234), third=(2 * 0.1788, 2 * 0.0772)))
_dot, _cross, _norm = G._dot, G._cross, G._norm


# ------------------------------------------------------------------------------------------------------ the pieces of the rule
def node(cyl, n0, p0, n1, p1, R, centre, min_cos=0.1):
    """steps 3 - 9 of ref_grid_predict at the pose cyl for the nodes of the plane pairs ([n0, p0], [n1, p1]), (m,3) and (m,) ->
    dict(state (m,), X (m,3), wh (m,3), tol_X (m,), margins: name -> the smallest relative margin)"""
    cyl = np.asarray(cyl, np.float64)
    m = len(p0)
    with np.errstate(all='ignore'):
        oc, a = cyl[:3], cyl[3:]
        an = float(_norm(a))
        ah = a / an
        state = np.zeros(m, np.int32)
        alive = np.ones(m, bool)
        margins = {}

        def refuse(cond, code):
            nonlocal alive
            state[alive & cond] = code
            alive = alive & ~cond

        def note(name, vals, mask):
            margins[name] = G._min_margin(margins.get(name, math.inf), vals, mask)

        w = _cross(n0, n1)
        w2 = _dot(w, w)
        note('w2', np.abs(w2 / G.MIN_W2 - 1), alive)
        refuse(~(w2 >= G.MIN_W2) | ~np.isfinite(w2), G.PARALLEL)
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
        refuse(~fin | (A == 0) | ~(disc > 0), G.MISS)
        s = np.sqrt(disc)
        tm, tp = (-B - s) / A, (-B + s) / A
        tC = _dot(centre - q, wh)
        dm, dp = np.abs(tm - tC), np.abs(tp - tC)
        note('root', np.abs(dm - dp) / (dm + dp), alive)
        t = np.where(dm <= dp, tm, tp)
        X = q + t[:, None] * wh
        refuse(~np.isfinite(X).all(1), G.MISS)
        g = X - oc
        ga = _dot(g, ah)
        nu = (g - ga[:, None] * ah) / R
        cg = np.abs(_dot(nu, wh))
        note('grazing', np.abs(cg / min_cos - 1), alive)
        refuse(~(cg >= min_cos), G.GRAZING)
        dq = U * (np.abs(p0) + np.abs(p1)) / w2
        eta = U / wn + U
        de = dq + U * (_norm(q) + _norm(oc))
        epn, wpn = _norm(ep), np.sqrt(A)
        dA, dB, dC = 2 * wpn * eta + U * A, epn * eta + wpn * de + U * epn * wpn, 2 * epn * de + U * (epn * epn + R * R)
        dt = (dA * t * t + 2 * dB * np.abs(t) + dC) / (2 * s) + U * (np.abs(B) + s) / A
        tol_X = dq + dt + np.abs(t) * eta + U * (_norm(q) + np.abs(t))
    return dict(state=state, X=X, wh=wh, tol_X=tol_X, margins=margins, an=an, ah=ah)


def project(X, tol_X, cam, K, T):
    """step 10's formula for camera cam[i] (0 / 1) of point i -> Xc (m,3), px (m,2), tol_px (m,), depth margin (m,)"""
    with np.errstate(all='ignore'):
        Rj, tj = T[1][:3, :3], T[1][:3, 3]
        X2 = np.stack([((Rj[r, 0] * X[:, 0] + Rj[r, 1] * X[:, 1]) + Rj[r, 2] * X[:, 2]) + tj[r] for r in range(3)], 1)
        c2 = cam.astype(bool)
        Xc = np.where(c2[:, None], X2, X)
        k = np.where(c2[:, None], K[1].reshape(9), K[0].reshape(9))
        Z = Xc[:, 2]
        xn, yn = Xc[:, 0] / Z, Xc[:, 1] / Z
        x = (k[:, 0] * xn + k[:, 1] * yn) + k[:, 2]
        y = k[:, 4] * yn + k[:, 5]
        dXc = tol_X + U * (_norm(X) + np.where(c2, float(_norm(tj)), 0.0))
        kk = np.abs(k[:, 0]) + np.abs(k[:, 1]) + np.abs(k[:, 4])
        tol = kk * dXc / Z * (1 + np.maximum(np.abs(Xc[:, 0]), np.abs(Xc[:, 1])) / Z) + U * (np.abs(x) + np.abs(y) + np.abs(k[:, 2]) + np.abs(k[:, 5]))
    return Xc, np.stack([x, y], 1), tol, np.abs(Z) / _norm(Xc)


class Problem:
    """the detections of one frame against one table: the concatenated list (camera 1's slots, then camera 2's) and rule 2's
    tests that do not depend on the pose"""

    def __init__(self, fr1, fr2, K1, K2, T21, table, centre, R=RADIUS, swap=0, min_cos=0.1):
        self.K = [np.asarray(K1, np.float64).reshape(3, 3), np.asarray(K2, np.float64).reshape(3, 3)]
        self.T = [np.eye(4), np.asarray(T21, np.float64).reshape(4, 4)]
        self.R, self.min_cos, self.centre = float(R), float(min_cos), np.asarray(centre, np.float64)[:3]
        P, status, lo, hi = np.asarray(table['P'], np.float64), np.asarray(table['status']), table['lo'], table['hi']
        xy, ids, cam, self.n = [], [], [], []
        for c, fr in enumerate((fr1, fr2)):
            n = 0 if fr is None else min(max(int(fr.get('cnt', len(fr['xy']))), 0), MAXP)
            self.n.append(n)
            if n:
                xy.append(np.asarray(fr['xy'], np.float64).reshape(-1, 2)[:n])
                ids.append(np.asarray(fr['id']).reshape(-1, 2)[:n].astype(np.int64))
                cam.append(np.full(n, c))
        m = sum(self.n)
        self.p = np.concatenate(xy) if m else np.zeros((0, 2))
        ids = np.concatenate(ids) if m else np.zeros((0, 2), np.int64)
        self.cam = np.concatenate(cam) if m else np.zeros(0, int)
        u0, u1 = ids[:, swap], ids[:, 1 - swap]
        inr = (u0 >= lo) & (u0 <= hi) & (u1 >= lo) & (u1 <= hi)
        l0, l1 = np.where(inr, u0 - lo, 0), np.where(inr, u1 - lo, 0)
        self.static_ok = inr & (status[0, l0] == ST_OK) & (status[1, l1] == ST_OK) & np.isfinite(self.p).all(1)
        self.n0, self.p0, self.n1, self.p1 = P[0, l0, :3], P[0, l0, 3], P[1, l1, :3], P[1, l1, 3]

    def evaluate(self, x, sel):
        """the nodes of the detections sel (indices) at the pose x -> dict(ok (k,), r (k,2), X, wh, Xc, tol_X, tol_px, margins)"""
        nd = node(x, self.n0[sel], self.p0[sel], self.n1[sel], self.p1[sel], self.R, self.centre, self.min_cos)
        Xc, px, tol_px, zm = project(nd['X'], nd['tol_X'], self.cam[sel], self.K, self.T)
        with np.errstate(all='ignore'):
            node_ok = nd['state'] == G.OK
            ok = node_ok & (Xc[:, 2] > 0) & np.isfinite(px).all(1)
            nd['margins']['depth'] = G._min_margin(math.inf, zm, node_ok)
            r = px - self.p[sel]
        pose_ok = bool(np.isfinite(np.asarray(x)).all() and np.isfinite(nd['an']) and nd['an'] != 0.0)
        return dict(nd, ok=ok & pose_ok, r=r, Xc=Xc, px=px, tol_px=tol_px, cam=self.cam[sel])

    def objective(self, x, S):
        e = self.evaluate(x, S)
        if not e['ok'].all():
            return math.nan
        with np.errstate(all='ignore'):
            return float((e['r'][:, 0] * e['r'][:, 0] + e['r'][:, 1] * e['r'][:, 1]).sum())

    def jacobian(self, x, S, e=None):
        """rule 7 -> r (2k,) and J (2k,6), the x row of a detection before its y row"""
        e = self.evaluate(x, S) if e is None else e
        x = np.asarray(x, np.float64)
        with np.errstate(all='ignore'):
            ah, an = e['ah'], e['an']
            g = e['X'] - x[:3]
            ga = _dot(g, ah)
            gp = g - ga[:, None] * ah
            den = _dot(gp, e['wh'])
            dt = np.concatenate([gp / den[:, None], ((ga[:, None] * gp) / an) / den[:, None]], 1)
            c2 = e['cam'].astype(bool)
            Rw = np.where(c2[:, None], e['wh'] @ self.T[1][:3, :3].T, e['wh'])
            k = np.where(c2[:, None], self.K[1].reshape(9), self.K[0].reshape(9))
            Xc = e['Xc']
            Z = Xc[:, 2]
            sx = ((k[:, 0] / Z) * Rw[:, 0] + (k[:, 1] / Z) * Rw[:, 1]) + (-(k[:, 0] * Xc[:, 0] + k[:, 1] * Xc[:, 1]) / (Z * Z)) * Rw[:, 2]
            sy = (k[:, 4] / Z) * Rw[:, 1] + (-(k[:, 4] * Xc[:, 1]) / (Z * Z)) * Rw[:, 2]
            J = np.stack([sx[:, None] * dt, sy[:, None] * dt], 1).reshape(-1, 6)
        return e['r'].reshape(-1), J


def lm_minimize(fun, normal, x0, f0, tolx, tolf, maxiter):
    """the loop of lm_minimize in csrc/fit.hip, from its comment: normal(x) -> (J'J, J'r); -> x, f, iterations, evaluations and
    how many of them gave NaN (trials that left the set where every member of S has a node)"""
    x, fx, lam, it, evals, nans = np.array(x0, np.float64), float(f0), 1e-3, 0, 1, 0
    while it < maxiter and it < 200:
        A, g = normal(x)
        it += 1
        accepted, dmax, fprev = False, 0.0, fx
        for _ in range(12):
            M = A.copy()
            M[np.diag_indices(6)] = np.diag(A) + lam * np.diag(A) + 1e-12 * np.trace(A)
            try:
                with np.errstate(all='ignore'):
                    dl = np.linalg.solve(M, -g)
            except np.linalg.LinAlgError:
                lam *= 10
                continue
            fn = fun(x + dl)
            evals += 1
            nans += math.isnan(fn)
            if fn < fx:
                dmax, x, fx, lam, accepted = float(np.abs(dl).max()), x + dl, fn, max(lam / 10, 1e-12), True
                break
            lam *= 10
        if not accepted:
            break
        if (fprev - fx) <= tolf * 1e-3 * (1.0 + fx) and dmax <= tolx:
            break
    return x, fx, it, evals, nans


def ref_pixel_fit(fr1, fr2, cyl0, use, K1, K2, T21, table, centre, R=RADIUS, swap=0, min_cos=0.1, gate_px=0.0, tol_x=1e-9, tol_f=1e-9,
                  max_iter=100):
    """one frame, the header's rule.  fr1, fr2: dict(xy, id[, cnt]) or None -> dict(cyl (6,), fvals (2,), iters (2,), counts (4,),
    stats (4,), status, res (2,MAXP,2), pt_state (2,MAXP), X (2,MAXP,3), S (indices into the concatenated list), prob, margin:
    the smallest relative margin of a decision at the start pose)"""
    prob = Problem(fr1, fr2, K1, K2, T21, table, centre, R, swap, min_cos)
    n1, n2 = prob.n
    m = n1 + n2
    cyl0 = np.asarray(cyl0, np.float64)
    out = dict(cyl=np.zeros(6), fvals=np.zeros(2), iters=np.zeros(2, np.int32), counts=np.zeros(4, np.int32), stats=np.zeros(4),
               status=ST_FEW_POINTS, res=np.zeros((2, MAXP, 2)), pt_state=np.full((2, MAXP), -1, np.int32), X=np.zeros((2, MAXP, 3)),
               S=np.zeros(0, int), prob=prob, margin=math.inf, margins={}, nan_trials=0)
    state = np.ones(m, np.int32)

    def spread(v, shape):
        a = np.zeros((2, MAXP) + shape, v.dtype)
        a[0, :n1], a[1, :n2] = v[:n1], v[n1:]
        return a

    def finish():
        out['pt_state'][0, :n1], out['pt_state'][1, :n2] = state[:n1], state[n1:]
        return out

    with np.errstate(all='ignore'):
        an = float(_norm(cyl0[3:]))
    if not use or not np.isfinite(cyl0).all() or not np.isfinite(an) or an == 0.0:
        return finish()
    cand = np.nonzero(prob.static_ok)[0]
    e = prob.evaluate(cyl0, cand)
    margins = dict(e['margins'])
    usable = cand[e['ok']]
    rn = np.sqrt(e['r'][:, 0] * e['r'][:, 0] + e['r'][:, 1] * e['r'][:, 1])[e['ok']]
    if gate_px > 0:
        margins['gate'] = G._min_margin(math.inf, np.abs(rn / gate_px - 1), np.ones(len(rn), bool))
        gated = rn >= gate_px
    else:
        gated = np.zeros(len(rn), bool)
    S = usable[~gated]
    state[S] = 0
    state[usable[gated]] = 2
    out.update(S=S, margins=margins, margin=min(margins.values(), default=math.inf))
    out['counts'][:] = [(S < n1).sum(), (S >= n1).sum(), m - len(usable), gated.sum()]
    if len(S) < MIN_PTS:
        return finish()
    f0 = prob.objective(cyl0, S)

    def normal(x):
        r, J = prob.jacobian(x, S)
        with np.errstate(all='ignore'):
            return J.T @ J, J.T @ r

    x, fx, it, evals, out['nan_trials'] = lm_minimize(lambda v: prob.objective(v, S), normal, cyl0, f0, tol_x, tol_f, max_iter)
    if not (np.isfinite(x).all() and np.isfinite(fx)):
        return finish()
    ef = prob.evaluate(x, S)
    r2 = ef['r'][:, 0] ** 2 + ef['r'][:, 1] ** 2
    c1 = S < n1
    full = np.zeros((m, 2)); full[S] = ef['r']
    fullX = np.zeros((m, 3)); fullX[S] = ef['X']
    out.update(cyl=x, fvals=np.array([f0, fx]), iters=np.array([it, evals], np.int32), status=ST_OK, res=spread(full, (2,)), X=spread(fullX, (3,)),
               stats=np.array([math.sqrt(r2[c1].sum() / c1.sum()) if c1.any() else 0.0, math.sqrt(r2[~c1].sum() / (~c1).sum()) if (~c1).any() else 0.0,
                               math.sqrt(fx / len(S)), math.sqrt(r2.max())]))
    return finish()


def evaluate_at(ref, cyl):
    """the residuals and points of the frame's set S at ANOTHER pose (the one a GPU call returned) -> dict(res, X (2,MAXP,.), tol_res,
    tol_X (2,MAXP), f, stats (4,), ok)"""
    prob, S = ref['prob'], ref['S']
    n1, n2 = prob.n
    e = prob.evaluate(np.asarray(cyl, np.float64), S)
    m = n1 + n2

    def spread(v, shape=()):
        full = np.zeros((m,) + shape); full[S] = v
        a = np.zeros((2, MAXP) + shape)
        a[0, :n1], a[1, :n2] = full[:n1], full[n1:]
        return a

    r2 = e['r'][:, 0] ** 2 + e['r'][:, 1] ** 2
    c1 = S < n1
    stats = np.array([math.sqrt(r2[c1].sum() / c1.sum()) if c1.any() else 0.0, math.sqrt(r2[~c1].sum() / (~c1).sum()) if (~c1).any() else 0.0,
                      math.sqrt(r2.sum() / len(S)), math.sqrt(r2.max())])
    return dict(res=spread(e['r'], (2,)), X=spread(e['X'], (3,)), tol_res=spread(e['tol_px'] + 2 * EPS * np.abs(prob.p[S]).max(1)),
                tol_X=spread(e['tol_X']), f=float(r2.sum()), stats=stats, ok=bool(e['ok'].all()), m=len(S))


# ------------------------------------------------------------------------------------------------------ scipy's optimum
def gauge_fixed(cyl, near):
    """the unit direction with d_y >= 0 and the axis point nearest to `near` -> (6,)"""
    cyl = np.asarray(cyl, np.float64)
    d = cyl[3:] / np.linalg.norm(cyl[3:])
    if d[1] < 0:
        d = -d
    return np.concatenate([cyl[:3] + ((np.asarray(near) - cyl[:3]) @ d) * d, d])


def scipy_optimum(ref, cyl0):
    """least_squares(method='lm') with the analytic Jacobian from cyl0 on the frame's S -> dict(cyl, f, well_posed)"""
    from scipy.optimize import least_squares
    prob, S = ref['prob'], ref['S']

    def res(x):
        e = prob.evaluate(x, S)
        return np.where(e['ok'][:, None], e['r'], 1e6).reshape(-1)

    ls = least_squares(res, np.asarray(cyl0, np.float64), jac=lambda x: prob.jacobian(x, S)[1], method='lm', xtol=1e-15, ftol=1e-15, gtol=1e-15,
                       max_nfev=2000)
    sv = np.linalg.svd(prob.jacobian(ls.x, S)[1], compute_uv=False)
    return dict(cyl=ls.x, f=float(2 * ls.cost), well_posed=bool(len(sv) >= 4 and sv[3] > 1e-6 * sv[0]),
                feasible=bool(prob.evaluate(ls.x, S)['ok'].all()))


def against_scipy(cyl, f, opt, cyl0):
    """-> (the largest difference of the gauge-fixed poses, f / f_ls - 1)"""
    return float(np.abs(gauge_fixed(cyl, cyl0[:3]) - gauge_fixed(opt['cyl'], cyl0[:3])).max()), f / opt['f'] - 1


# ------------------------------------------------------------------------------------------------------ cases
def _frames(seed, k1=None, k2=None, order_seed=5):
    """the cylinder frame of the seed in a fixed random order -> (fr1, fr2) with the first k1 / k2 detections (None: all)"""
    idx, _, uv1, uv2 = TC.cylinder_frame(0.25, seed)
    o = np.random.default_rng(order_seed).permutation(len(idx))
    o2 = np.random.default_rng(order_seed + 1).permutation(len(idx))
    return dict(xy=uv1[o][:k1], id=idx[o][:k1]), dict(xy=uv2[o2][:k2], id=idx[o2][:k2])


def _repeated(seed, count):
    """`count` detections per camera: the frame's nodes again and again, each time with noise of its own"""
    idx, X, _, _ = TC.cylinder_frame(0.25, seed)
    rng = np.random.default_rng(9100 + seed)
    reps = -(-count // len(idx))
    uv = [PC.project_pair(X, 0.25, rng) for _ in range(reps)]
    ii = np.concatenate([idx] * reps)[:count]
    return dict(xy=np.concatenate([u[0] for u in uv])[:count], id=ii), dict(xy=np.concatenate([u[1] for u in uv])[:count], id=ii)


START = G.pose(0.25, 0.2)                              # a start as good as a 3-D fit leaves it, for the shape cases
OFF = G.pose(1.6, 2.0)                                 # 2 mm / 1.6 degrees off: some silhouette nodes miss at the start


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(fr1, fr2: lists of n frames (dict(xy, id[, cnt]) or None per camera: None for the whole list = camera absent),
    cyl0 (n,6), use (n,) or None, table, swap, min_cos, gate_px, poison): one call each"""
    t = TC.rig_table(TC.LO, TC.HI)
    c = {}

    def call(pairs, cyl0=None, **kw):
        n = len(pairs)
        d = dict(fr1=[p[0] for p in pairs], fr2=[p[1] for p in pairs], cyl0=np.stack([START] * n) if cyl0 is None else np.asarray(cyl0),
                 use=None, table=t, swap=0, min_cos=0.1, gate_px=0.0, poison=31)
        d.update(kw)
        for k in ('fr1', 'fr2'):
            if all(f is None for f in d[k]):
                d[k] = None
        return d

    counts = [(0, 0), (1, 0), (5, 0), (0, 6), (3, 3), (63, 64), (64, 65), (65, 63), (250, 250), (0, 250), (250, 0)]
    c['counts'] = call([_frames(i % 3, a, b) for i, (a, b) in enumerate(counts)])
    c['one frame'] = call([_frames(0, 250, 250)])
    c['full tables, L 256'] = call([_repeated(1, MAXP)], table=TC.rig_table(-128, 127))
    c['count above the capacity'] = call([tuple(dict(f, cnt=3000) for f in _repeated(2, MAXP))], table=TC.rig_table(-128, 127))
    c['camera 1 only'] = call([(_frames(s, 250)[0], None) for s in range(3)])
    c['camera 2 only'] = call([(None, _frames(s, None, 250)[1]) for s in range(3)])
    one = np.nonzero((TC.cylinder_frame(0.25, 0)[0] == 0).all(1))[0]
    rng = np.random.default_rng(77)
    X00 = TC.cylinder_frame(0.25, 0)[1][one]
    uv = [PC.project_pair(np.repeat(X00, 40, 0), 0.25, rng)]
    c['L 1'] = call([(dict(xy=uv[0][0], id=np.zeros((40, 2), np.int32)), dict(xy=uv[0][1], id=np.zeros((40, 2), np.int32))),
                     _frames(0, 100, 100)], table=TC.rig_table(0, 0))
    c['swap 1'] = call([_frames(0, 250, 250), _frames(1, 65, 250)], table=TC.transposed(t), swap=1)
    c['swap 0, row-first ids'] = call([tuple(dict(f, id=f['id'][:, ::-1]) for f in _frames(0, 250, 250))], table=TC.transposed(t))
    cyl65 = np.stack([G.pose(0.1 + 0.004 * i, 0.05 + 0.004 * i) for i in range(65)])
    cyl65[7, 1] = np.nan; cyl65[20, 3:] = 0.0; cyl65[33, 5] = np.inf
    c['65 frames'] = call([_frames(i % 30, 40 + i, 104 - i, order_seed=i) for i in range(65)], cyl0=cyl65, use=(np.arange(65) % 9 != 4).astype(np.uint8))
    c['refused planes'] = call([_frames(0), _frames(1, 200, 130)], table=TC.main_table())
    c['nodes that miss at the start'] = call([_frames(0), _frames(2)], cyl0=np.stack([OFF, OFF]))
    g1, g2 = _frames(3, 250, 250)
    g1, g2 = dict(g1, xy=g1['xy'].copy()), dict(g2, xy=g2['xy'].copy())
    g1['xy'][[3, 64, 200]] += [[5.0, 3.0], [-6.0, 0.5], [0.0, 9.0]]
    g2['xy'][[0, 249]] += [[4.0, -4.0], [30.0, 0.0]]
    bad = dict(g1, xy=g1['xy'].copy())
    bad['xy'][[5, 70]] = [[np.nan, 3.0], [100.0, np.inf]]
    c['gate 4 px'] = call([(g1, g2), (bad, g2)], gate_px=4.0)
    c['noisy table'] = call([_frames(0), _frames(1)], table=TC.noisy_table(0))
    c['min_cos 0.4'] = call([_frames(0), _frames(1)], min_cos=0.4)
    return c


def call_arrays(case):
    """-> dict(xy1, id1, cnt1, xy2, id2, cnt2 (None for an absent camera), n) as the C call reads them, poisoned past the counts"""
    n = len(case['cyl0'])
    out = dict(n=n)
    for c, k in ((1, 'fr1'), (2, 'fr2')):
        if case[k] is None:
            out.update({f'xy{c}': None, f'id{c}': None, f'cnt{c}': None})
            continue
        frames = [dict(xy=np.zeros((0, 2)), id=np.zeros((0, 2), np.int32)) if f is None else f for f in case[k]]
        out[f'xy{c}'], out[f'id{c}'], out[f'cnt{c}'] = TC.pack(frames, None if case['poison'] is None else case['poison'] + c)
    return out


def _reference(case, f):
    K1, K2, T21 = PC.rig()[:3]
    use = True if case['use'] is None else bool(case['use'][f])
    fr1 = None if case['fr1'] is None else case['fr1'][f]
    fr2 = None if case['fr2'] is None else case['fr2'][f]
    return ref_pixel_fit(fr1, fr2, case['cyl0'][f], use, K1, K2, T21, case['table'], PC.rig()[5], RADIUS, case['swap'], case['min_cos'],
                         case['gate_px'])


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> list of dict(ref_pixel_fit's, opt: scipy_optimum's or None) per frame of the call; computed once and shared"""
    case = cases()[name]
    out = []
    for f in range(len(case['cyl0'])):
        r = _reference(case, f)
        r['opt'] = scipy_optimum(r, case['cyl0'][f]) if r['status'] == ST_OK else None
        out.append(r)
    return out


# ------------------------------------------------------------------------------------------------------ accuracy
def third_missing(gp, seed, cam):
    rng = np.random.default_rng(8100 + 2 * seed + cam)
    keep = np.sort(rng.permutation(len(gp))[:len(gp) - len(gp) // 3])
    return gp[keep]


def oracle_start(gp1, gp2):
    """the oracle chain choose_idx -> triangulate -> fit_cylinder(mode=1) on two (m,4) tables -> cyl (6,), status"""
    import oracle
    oracle.build()
    K1, K2, T21 = PC.rig()[:3]
    c1, c2, _, _ = oracle.choose_idx(gp1, gp2, K1, K2, T21)
    X, _ = oracle.triangulate(c1, c2, K1, K2, T21)
    fit = oracle.fit_cylinder(X, RADIUS, mode=1)
    return fit['cyl'][1] if np.ndim(fit['cyl']) == 2 else fit['cyl'], fit['status']


def _fr(gp):
    return dict(xy=gp[:, :2], id=gp[:, 2:].astype(np.int32))


@functools.lru_cache(maxsize=None)
def accuracy_chain(kind, which, seed):
    """kind 'rig' / 'noisy', which 'all' / 'third' -> dict(start, fit: (degrees, mm) off the true axis, ref)"""
    idx, _, uv1, uv2 = TC.cylinder_frame(0.25, seed)
    gp1, gp2 = np.concatenate([uv1, idx], 1), np.concatenate([uv2, idx], 1)
    if which == 'third':
        gp1, gp2 = third_missing(gp1, seed, 0), third_missing(gp2, seed, 1)
    table = TC.rig_table(TC.LO, TC.HI) if kind == 'rig' else TC.noisy_table(seed % 5)
    cyl0, st = oracle_start(gp1, gp2)
    assert st == 0
    K1, K2, T21 = PC.rig()[:3]
    ref = ref_pixel_fit(_fr(gp1), _fr(gp2), cyl0, True, K1, K2, T21, table, PC.rig()[5])
    return dict(start=TC.axis_errors(cyl0), fit=TC.axis_errors(ref['cyl']), ref=ref, cyl0=cyl0)
