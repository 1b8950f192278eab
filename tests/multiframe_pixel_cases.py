"""Cases and the numpy reference for T_Cam_AGV fitted to the pixels of all frames of a group (include/cpe.h
cpe_multi_frame_fit_pixels_batch).  The per-detection pieces are tests/pixel_fit_cases.py's (Problem,
node, project, jacobian), the pose step and the loop are those of tests/multiframe_lm_cases.py, the rig and the table those of
tests/plane_fit_cases.py / tests/table_tri_cases.py.

What the GPU is held to (tests/test_multiframe_pixels_gpu.py):
    counts, pt_state, n_used, status   exactly: every decision of every case has a relative margin above 1e-6 at the start pose
                                       (tests/test_multiframe_pixel_cases_cpu.py asserts it)
    res, frame_stats, stats, fvals[1]  the reference evaluated at the frame poses the call returned, within evaluate()'s own
                                       tolerances and the (2 m + 18) eps bound of a sum of m squares
    frame_cyl                          T * TAGVcyl of the returned T within 16 * 2^-53 * (|T| |A|) per entry
    x, fvals[1]                        scipy.optimize.least_squares(method='lm', xtol = ftol = gtol = 1e-15) from the same start on
                                       the same S, within PIXMF_POSE_BOUND (rotation angle between the two T in radians plus the
                                       translation difference in mm) and PIXMF_F_BOUND (f / f_ls - 1): twice the worst the
                                       restated loop itself shows against scipy over the 14 fitted groups of the cases here (measured:
                                       pose 2.33e-7, the valley of a few frames is flat; f / f_ls - 1 1.83e-13; the CPU test prints them)
    N                                  the reference J'J at the returned pose within PIXMF_N_BOUND, relative to sqrt(N_aa N_bb):
                                       16 x the largest difference between the float64 and the long-double J'J of the cases
                                       (measured 1.00e-15)
    iters[0]                           at most 3 x the restated loop's

Accuracy of the restated loop (scene(F, seed, ...): pan +-0.35 rad, tilt +-0.2 rad, 0.25 px noise, rig_table(-16, 16); the start
0.04 - 0.4 degrees and 0.4 - 1.4 mm off; rms over the frames of the angle between the true and the fitted axis and of the distance
of the true axis point from the fitted axis; sel_cos 0.35, min_cos 0.1).  `third`: camera 1 without the lowest third of the
columns, camera 2 without the highest third (a third of the nodes are stereo pairs).  per-frame: pixel_fit_cases.ref_pixel_fit of
every frame alone from the same start.  point-based: multiframe_lm_cases.fit from the same start on the oracle's DLT points of the
stereo pairs (point_fit_errors).  LM iterations 5 - 6, no NaN trial in any run.

    scene                 all frames at once            per-frame pixel fits           point-based LM on DLT points
    all,   F  8 seed 0    0.0048 deg  0.0063 mm         0.0755 deg  0.1543 mm      0.0070 deg  0.0070 mm
    all,   F  8 seed 1    0.0012      0.0094            0.1830      0.3531         0.0105      0.0094
    all,   F  8 seed 2    0.0031      0.0116            0.2570      0.3670         0.0084      0.0184
    all,   F 17 seed 0    0.0053      0.0079            0.1392      0.2428         0.0033      0.0072
    all,   F 45 seed 0    0.0025      0.0021            0.2504      0.2752         0.0019      0.0046
    third, F  8 seed 0    0.0146      0.0225            0.0898      0.0953         0.0218      0.0210
    third, F  8 seed 1    0.0045      0.0113            0.1839      0.3583         0.0111      0.0194
    third, F  8 seed 2    0.0085      0.0065            0.2665      0.3609         0.0087      0.0141
    third, F 17 seed 0    0.0133      0.0149            0.1658      0.2460         0.0213      0.0095
    third, F 45 seed 0    0.0057      0.0040            0.2686      0.2796         0.0065      0.0129

The pixel rms at the optimum is 0.351 - 0.360 px = 0.25 sqrt 2 throughout.  ACCURACY_BOUNDS are twice the worst of the ten rows.
The result depends on S, and S on the start: from the pose of the point-based fit instead of the scene's start, `all, F 8 seed 2`
takes 40 more silhouette detections into S (2768 instead of 2728) and ends 0.0108 deg / 0.0184 mm off instead of 0.0031 / 0.0116
(0.3578 px instead of 0.3588; the reference and the kernel agree on this, tests/test_multiframe_pixels_pipeline_gpu.py prints it).
Membership near the silhouette moves the optimum by as much as the pixel noise does, so twice the worst `all` row alone (0.0106
deg) would not hold for every start; the bound over all ten rows does.
The all-frame fit is 4 - 150 x nearer than the per-frame fits, and about level with the point-based fit on complete data (0.3 - 3 x).
With sel_cos = min_cos = 0.1 the restated loop stalls on all three F = 8 scenes, as the scipy prototype did (STALL: seed -> LM
iterations, NaN trials, pixel rms at the end): silhouette nodes that exist at the start cease to exist a step later and every
such trial is refused.  With sel_cos = 0.35 the same scenes meet no NaN trial and end at 0.355 - 0.359 px."""
import functools
import math

import numpy as np

import grid_predict_cases as G
import multiframe_cases as MC
import multiframe_lm_cases as LM
import pixel_fit_cases as X
import plane_fit_cases as PC
import table_tri_cases as TC

MAXP, EPS, ST_OK, ST_FEW_POINTS, ST_OVERFLOW = X.MAXP, X.EPS, X.ST_OK, X.ST_FEW_POINTS, 6
MIN_PTS, RADIUS, MAXF = X.MIN_PTS, X.RADIUS, 1024
WAVES = 4                                                  # MFPX_WAVES of csrc/fit.hip: the shapes of the GPU cases follow it
PIXMF_POSE_BOUND, PIXMF_F_BOUND = 2 * 2.34e-7, 2 * 1.83e-13
PIXMF_N_BOUND = 16 * 1.01e-15
# twice the worst rms (degrees, mm) of the all-frame fit over the ten runs of the table above (third, F 8 seed 0)
ACCURACY_BOUNDS = (2 * 0.0146, 2 * 0.0225)
STALL = {0: (51, 64, 0.4237), 1: (50, 63, 0.5517), 2: (44, 56, 0.4145)}


# ------------------------------------------------------------------------------------------------------ the rule
def frame_cyl(T, A):
    """rule 2 (frame_axis): (o_i, a_i) of the frame with getTAGVcyl A at the pose T -> (6,)"""
    T, A = np.asarray(T, np.float64).reshape(4, 4), np.asarray(A, np.float64).reshape(4, 4)
    return np.concatenate([(T @ A[:, 3])[:3], (T @ A[:, 1])[:3]])


class Group:
    """the kept frames of one group: one pixel_fit_cases.Problem each"""

    def __init__(self, fr1, fr2, TAGV, table, swap=0, min_cos=0.1, sel_cos=0.35, gate_px=0.0, R=RADIUS):
        K1, K2, T21 = PC.rig()[:3]
        self.A = np.asarray(TAGV, np.float64).reshape(-1, 4, 4)
        self.min_cos, self.sel_cos, self.gate_px = min_cos, sel_cos, gate_px
        self.probs = [X.Problem(a, b, K1, K2, T21, table, PC.rig()[5], R, swap, min_cos) for a, b in zip(fr1, fr2)]

    def cyls(self, x):
        T = LM.vec2T(x)
        return [frame_cyl(T, A) for A in self.A]

    def select(self, x0):
        """rule 3 -> S (list of index arrays), state (list of (m,) arrays), margins"""
        S, states, margins = [], [], {}
        for prob, cyl in zip(self.probs, self.cyls(x0)):
            m = sum(prob.n)
            st = np.ones(m, np.int32)
            cand = np.nonzero(prob.static_ok)[0]
            prob.min_cos = self.sel_cos
            e = prob.evaluate(cyl, cand)
            prob.min_cos = self.min_cos
            for k, v in e['margins'].items():
                margins[k] = min(margins.get(k, math.inf), v)
            usable = cand[e['ok']]
            rn = np.sqrt(e['r'][:, 0] * e['r'][:, 0] + e['r'][:, 1] * e['r'][:, 1])[e['ok']]
            gated = rn >= self.gate_px if self.gate_px > 0 else np.zeros(len(rn), bool)
            if self.gate_px > 0 and len(rn):
                margins['gate'] = min(margins.get('gate', math.inf), float(np.abs(rn / self.gate_px - 1).min()))
            st[usable[~gated]], st[usable[gated]] = 0, 2
            S.append(usable[~gated]); states.append(st)
        return S, states, margins

    def evaluate(self, cyls, S):
        return [p.evaluate(c, s) for p, c, s in zip(self.probs, cyls, S)]

    def objective(self, x, S):
        """rule 4"""
        if not np.isfinite(np.asarray(x)).all():
            return math.nan
        f = 0.0
        for e in self.evaluate(self.cyls(x), S):
            if not e['ok'].all():
                return math.nan
            with np.errstate(all='ignore'):
                f = f + float((e['r'][:, 0] * e['r'][:, 0] + e['r'][:, 1] * e['r'][:, 1]).sum())
        return f

    def residuals(self, x, S, penalty=1e6):
        out = []
        for e in self.evaluate(self.cyls(x), S):
            out.append(np.where(e['ok'][:, None], e['r'], penalty).reshape(-1))
        return np.concatenate(out)

    def jacobian(self, x, S, dtype=np.float64, cyls=None, T=None):
        """rule 6 -> r (2m,), J (2m,6) in the step's coordinates (dw, dt), the x row of a detection before its y row"""
        T = LM.vec2T(x) if T is None else np.asarray(T, np.float64).reshape(4, 4)
        cyls = [frame_cyl(T, A) for A in self.A] if cyls is None else cyls
        rs, Js = [], []
        for prob, A, cyl, s in zip(self.probs, self.A, cyls, S):
            r, Jc = prob.jacobian(cyl, s)
            m_i = (T[:3, :3] @ A[:3, 3]).astype(dtype)
            Ju, Jw = Jc[:, :3].astype(dtype), Jc[:, 3:].astype(dtype)
            jw = np.cross(m_i[None], Ju) + np.cross(cyl[3:].astype(dtype)[None], Jw)
            rs.append(r.astype(dtype)); Js.append(np.concatenate([jw, Ju], 1))
        return np.concatenate(rs), np.concatenate(Js)


def lm(fun, normal, x0, f0, tolx=1e-9, tolf=1e-9, maxiter=100):
    """lm_minimize of csrc/fit.hip with MultiPoseProblem::candidate -> x, f, iterations, evaluations, NaN trials, accepted poses"""
    x, fx, lam, it, evals, nans, path = np.array(x0, np.float64), float(f0), 1e-3, 0, 1, 0, []
    while it < maxiter and it < 200:
        A, g = normal(x)
        T = LM.vec2T(x)
        it += 1
        accepted, dmax, fprev = False, 0.0, fx
        for _ in range(12):
            M = A + np.diag(lam * np.diag(A) + 1e-12 * np.trace(A))
            try:
                with np.errstate(all='ignore'):
                    dl = np.linalg.solve(M, -g)
            except np.linalg.LinAlgError:
                lam *= 10
                continue
            Tn = np.eye(4)
            Tn[:3, :3] = LM.rot_exp(dl[:3]) @ T[:3, :3]
            Tn[:3, 3] = T[:3, 3] + dl[3:]
            xn = LM.T2vec(Tn)
            fn = fun(xn)
            evals += 1
            nans += math.isnan(fn)
            if fn < fx:
                dmax, x, fx, lam, accepted = float(np.abs(dl).max()), xn, fn, max(lam / 10, 1e-12), True
                path.append(xn)
                break
            lam *= 10
        if not accepted:
            break
        if (fprev - fx) <= tolf * 1e-3 * (1.0 + fx) and dmax <= tolx:
            break
    return x, fx, it, evals, nans, path


def pack_N(M):
    return np.asarray(M)[np.triu_indices(6)]


def ref_group(fr1, fr2, TAGV, x0, table, swap=0, min_cos=0.1, sel_cos=0.35, gate_px=0.0, tol_x=1e-9, tol_f=1e-9, max_iter=100):
    """the header's rule for the KEPT frames of one group (two at least) -> dict(status, x, T, fvals, iters, counts, stats, N, S,
    states, frame_cyl, frame_stats, grp, margins, nan_trials, path)"""
    grp = Group(fr1, fr2, TAGV, table, swap, min_cos, sel_cos, gate_px)
    x0 = np.asarray(x0, np.float64)
    out = dict(status=ST_FEW_POINTS, x=np.zeros(6), T=np.zeros(16), fvals=np.zeros(2), iters=np.zeros(2, np.int32), counts=np.zeros(4, np.int32),
               stats=np.zeros(4), N=np.zeros(21), grp=grp, S=None, states=[np.ones(sum(p.n), np.int32) for p in grp.probs], margins={},
               nan_trials=0, path=[], n1=[p.n[0] for p in grp.probs])
    if len(grp.probs) < 2 or not np.isfinite(x0).all():
        return out
    S, states, margins = grp.select(x0)
    out.update(S=S, states=states, margins=margins)
    n1 = out['n1']
    c1 = sum(int((s < a).sum()) for s, a in zip(S, n1))
    nS = sum(len(s) for s in S)
    counts = np.array([c1, nS - c1, sum(int((st == 1).sum()) for st in states), sum(int((st == 2).sum()) for st in states)], np.int32)
    if nS < MIN_PTS or sum(len(s) > 0 for s in S) < 2:
        return out
    f0 = grp.objective(x0, S)
    if not math.isfinite(f0):
        return out

    def normal(x):
        r, J = grp.jacobian(x, S)
        with np.errstate(all='ignore'):
            return J.T @ J, J.T @ r

    x, fx, it, evals, nans, path = lm(lambda v: grp.objective(v, S), normal, x0, f0, tol_x, tol_f, max_iter)
    out.update(nan_trials=nans, path=path)
    if not (np.isfinite(x).all() and math.isfinite(fx)):
        return out
    ev = evaluate_at(out, LM.vec2T(x))
    out.update(status=ST_OK, x=x, T=LM.vec2T(x).reshape(16), fvals=np.array([f0, fx]), iters=np.array([it, evals], np.int32), counts=counts,
               stats=ev['stats'], N=ev['N'], frame_cyl=ev['frame_cyl'], frame_stats=ev['frame_stats'])
    return out


def _rms(v, k):
    return math.sqrt(v / k) if k else 0.0


def evaluate_at(ref, T, cyls=None):
    """the group's S at ANOTHER pose T (4x4) and, when given, at the frame poses `cyls` a call returned -> dict(res, tol_res (lists
    of (2,MAXP,.) per kept frame), f, stats, frame_stats, frame_cyl, N, ok, m)"""
    grp, S = ref['grp'], ref['S']
    T = np.asarray(T, np.float64).reshape(4, 4)
    own = [frame_cyl(T, A) for A in grp.A]
    cyls = own if cyls is None else cyls
    ev = grp.evaluate(cyls, S)
    res, tol, fstats, s1 = [], [], [], [0.0, 0.0, 0.0]
    for prob, e, s in zip(grp.probs, ev, S):
        n1, n2 = prob.n
        r2 = e['r'][:, 0] ** 2 + e['r'][:, 1] ** 2
        a = s < n1
        full = np.zeros((n1 + n2, 2)); full[s] = e['r']
        ft = np.zeros(n1 + n2); ft[s] = e['tol_px'] + 2 * EPS * np.abs(prob.p[s]).max(1) if len(s) else 0.0
        R, Tl = np.zeros((2, MAXP, 2)), np.zeros((2, MAXP))
        R[0, :n1], R[1, :n2], Tl[0, :n1], Tl[1, :n2] = full[:n1], full[n1:], ft[:n1], ft[n1:]
        res.append(R); tol.append(Tl)
        fstats.append([_rms(r2[a].sum(), a.sum()), _rms(r2[~a].sum(), (~a).sum()), _rms(r2.sum(), len(s)), math.sqrt(r2.max()) if len(s) else 0.0])
        s1 = [s1[0] + r2[a].sum(), s1[1] + r2[~a].sum(), max(s1[2], math.sqrt(r2.max()) if len(s) else 0.0)]
    c1 = sum(int((s < p.n[0]).sum()) for s, p in zip(S, grp.probs))
    m = sum(len(s) for s in S)
    r, J = grp.jacobian(None, S, cyls=cyls, T=T)
    return dict(res=res, tol_res=tol, f=float(s1[0] + s1[1]), stats=np.array([_rms(s1[0], c1), _rms(s1[1], m - c1), _rms(s1[0] + s1[1], m), s1[2]]),
                frame_stats=np.array(fstats), frame_cyl=np.array(own), N=pack_N(J.T @ J), ok=all(bool(e['ok'].all()) for e in ev), m=m)


def frame_cyl_tol(T, A):
    """16 * 2^-53 * (|T| |A|) for the entries of frame_cyl"""
    T, A = np.abs(np.asarray(T).reshape(4, 4)), np.abs(np.asarray(A).reshape(4, 4))
    return 16 * 2.0 ** -53 * np.concatenate([(T @ A[:, 3])[:3], (T @ A[:, 1])[:3]])


def pose_difference(Ta, Tb):
    """the rotation angle between two poses (radians) plus the difference of their translations (mm)"""
    Ta, Tb = np.asarray(Ta).reshape(4, 4), np.asarray(Tb).reshape(4, 4)
    return LM.rotation_between(Ta[:3, :3], Tb[:3, :3]) + float(np.linalg.norm(Ta[:3, 3] - Tb[:3, 3]))


def scipy_optimum(ref, x0):
    """least_squares(method='lm') on the residual vector of the group's S from x0 (central differences in the rotation vector,
    whose chart is not the step's; analytic in t) -> dict(x, T, f, feasible)"""
    from scipy.optimize import least_squares
    grp, S = ref['grp'], ref['S']

    def jac(x, h=1e-6):
        J = grp.jacobian(x, S)[1].copy()
        for k in range(3):
            dx = np.zeros(6); dx[k] = h
            J[:, k] = (grp.residuals(x + dx, S) - grp.residuals(x - dx, S)) / (2 * h)
        return J

    ls = least_squares(lambda x: grp.residuals(x, S), np.asarray(x0, np.float64), jac=jac, method='lm', xtol=1e-15, ftol=1e-15, gtol=1e-15,
                       max_nfev=2000)
    return dict(x=ls.x, T=LM.vec2T(ls.x), f=float(2 * ls.cost), feasible=math.isfinite(grp.objective(ls.x, S)))


# ------------------------------------------------------------------------------------------------------ scenes
def _true_pose():
    """T_Cam_AGV that puts the cylinder of pan = tilt = 0 at table_tri_cases' (CYL_C, about +y)"""
    A0 = MC.get_TAGVcyl(0.0, 0.0)
    Rz = np.array([[0, -1, 0], [-1, 0, 0], [0, 0, -1.0]]).T
    ang = 0.05
    Rt = np.array([[1, 0, 0], [0, math.cos(ang), -math.sin(ang)], [0, math.sin(ang), math.cos(ang)]]) @ Rz
    T = np.eye(4); T[:3, :3] = Rt; T[:3, 3] = TC.CYL_C - Rt @ A0[:3, 3]
    return T


TTRUE = _true_pose()
LOW_THIRD = lambda idx: idx[:, 0] > -8 + 17 // 3 - 1       # camera 1 without the lowest third of the columns (-8 .. -4 of -8 .. 8)
HIGH_THIRD = lambda idx: idx[:, 0] < 8 - 17 // 3 + 1       # camera 2 without the highest third (4 .. 8)


def start_pose(seed):
    """0.04 - 0.4 degrees and 0.4 - 1.4 mm off TTRUE, as a pose vector"""
    rng = np.random.default_rng(5200 + seed)
    dw, dt = rng.standard_normal(3), rng.standard_normal(3)
    dw *= math.radians(rng.uniform(0.04, 0.4)) / np.linalg.norm(dw)
    dt *= rng.uniform(0.4, 1.4) / np.linalg.norm(dt)
    T = np.eye(4); T[:3, :3] = LM.rot_exp(dw) @ TTRUE[:3, :3]; T[:3, 3] = TTRUE[:3, 3] + dt
    return LM.T2vec(T)


@functools.lru_cache(maxsize=None)
def scene(F, seed, keep1=None, keep2=None, noise=0.25):
    """F frames at random pan (+-0.35 rad) and tilt (+-0.2 rad) -> dict(fr1, fr2: lists of dict(xy, id), angles (F,2), TAGV (F,4,4),
    true: the frames' true (c, a), x0: start_pose(seed)); keep1 / keep2: functions of the indices (m,2) -> the mask a camera keeps"""
    rng = np.random.default_rng(4200 + seed)
    angles = np.stack([rng.uniform(-0.35, 0.35, F), rng.uniform(-0.2, 0.2, F)], 1)
    TAGV = np.stack([MC.get_TAGVcyl(*a) for a in angles]) if F else np.zeros((0, 4, 4))
    fr1, fr2, true = [], [], []
    for A in TAGV:
        Tc = TTRUE @ A
        c, a = Tc[:3, 3], Tc[:3, 1]
        idx, P = TC.cylinder_hits(c, a)
        uv1, uv2 = PC.project_pair(P, noise, rng)
        m1 = keep1(idx) if keep1 else np.ones(len(idx), bool)
        m2 = keep2(idx) if keep2 else np.ones(len(idx), bool)
        o1, o2 = rng.permutation(int(m1.sum())), rng.permutation(int(m2.sum()))
        fr1.append(dict(xy=uv1[m1][o1], id=idx[m1][o1])); fr2.append(dict(xy=uv2[m2][o2], id=idx[m2][o2]))
        true.append((c, a))
    return dict(fr1=fr1, fr2=fr2, angles=angles, TAGV=TAGV, true=true, x0=start_pose(seed))


def axis_rms(T, sc):
    """rms over the frames of TC.axis_errors of the frames' fitted axes against the true ones -> (degrees, mm)"""
    e = np.array([TC.axis_errors(frame_cyl(T, A), c, a) for A, (c, a) in zip(sc['TAGV'], sc['true'])])
    return tuple(np.sqrt((e * e).mean(0)))


ACCURACY_RUNS = [(8, 0), (8, 1), (8, 2), (17, 0), (45, 0)]
KEEP = dict(all=(None, None), third=(LOW_THIRD, HIGH_THIRD))


@functools.lru_cache(maxsize=None)
def accuracy_run(F, seed, which, sel_cos=0.35):
    sc = scene(F, seed, *KEEP[which])
    ref = ref_group(sc['fr1'], sc['fr2'], sc['TAGV'], sc['x0'], TC.rig_table(TC.LO, TC.HI), sel_cos=sel_cos)
    return dict(scene=sc, ref=ref, err=axis_rms(ref['T'], sc) if ref['status'] == ST_OK else None)


def per_frame_errors(F, seed, which):
    """every frame fitted alone by pixel_fit_cases.ref_pixel_fit from the same start -> rms (degrees, mm) over the fitted frames"""
    sc = scene(F, seed, *KEEP[which])
    K1, K2, T21 = PC.rig()[:3]
    T0 = LM.vec2T(sc['x0'])
    e = []
    for a, b, A, (c, ax) in zip(sc['fr1'], sc['fr2'], sc['TAGV'], sc['true']):
        r = X.ref_pixel_fit(a, b, frame_cyl(T0, A), True, K1, K2, T21, TC.rig_table(TC.LO, TC.HI), PC.rig()[5])
        if r['status'] == ST_OK:
            e.append(TC.axis_errors(r['cyl'], c, ax))
    e = np.array(e)
    return tuple(np.sqrt((e * e).mean(0)))


def dlt_points(sc):
    """the oracle's DLT points of every frame's stereo pairs (joined by index) -> P f64[F,MAXP,3], cnt i32[F]"""
    import oracle
    oracle.build()
    K1, K2, T21 = PC.rig()[:3]
    F = len(sc['fr1'])
    P, cnt = np.zeros((F, MAXP, 3)), np.zeros(F, np.int32)
    for i, (a, b) in enumerate(zip(sc['fr1'], sc['fr2'])):
        ka = {tuple(v): k for k, v in enumerate(a['id'])}
        pairs = [(ka[tuple(v)], k) for k, v in enumerate(b['id']) if tuple(v) in ka]
        if pairs:
            ia, ib = np.array(pairs).T
            pts = oracle.triangulate(a['xy'][ia], b['xy'][ib], K1, K2, T21)[0]
            P[i, :len(pts)], cnt[i] = pts, len(pts)
    return P, cnt


def point_fit_errors(F, seed, which):
    """multiframe_lm_cases.fit from the same start on the DLT points of the frames that have a stereo pair -> rms (degrees, mm)"""
    sc = scene(F, seed, *KEEP[which])
    P, cnt = dlt_points(sc)
    keep = cnt > 0
    fit = LM.fit(LM.Problem(P[keep], cnt[keep], sc['TAGV'][keep]), None, x0=sc['x0'])
    return axis_rms(fit['T'], sc)


# ------------------------------------------------------------------------------------------------------ GPU cases
def _cut(fr, k):
    return dict(xy=fr['xy'][:k], id=fr['id'][:k])


def _frames(F, seed, counts=None, **kw):
    """the scene's frames with the first counts[i] = (k1, k2) detections of frame i (None: all)"""
    sc = scene(F, seed, **kw)
    counts = counts or [(None, None)] * F
    return ([_cut(f, c[0]) for f, c in zip(sc['fr1'], counts)], [_cut(f, c[1]) for f, c in zip(sc['fr2'], counts)], sc)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(fr1, fr2 (lists of n frames, or None: the camera is absent), TAGV (n,4,4), frame_ok (n,) or None, group_start,
    x0 (G,6), table, swap, min_cos, sel_cos, gate_px, poison): one call each"""
    t = TC.rig_table(TC.LO, TC.HI)
    c = {}

    def call(groups, frame_ok=None, **kw):
        fr1 = [f for g in groups for f in g[0]]
        fr2 = [f for g in groups for f in g[1]]
        gs = np.cumsum([0] + [len(g[0]) for g in groups]).astype(np.int32)
        d = dict(fr1=fr1, fr2=fr2, TAGV=np.concatenate([g[2]['TAGV'][:len(g[0])] for g in groups]) if fr1 else np.zeros((0, 4, 4)),
                 frame_ok=frame_ok, group_start=gs, x0=np.stack([g[2]['x0'] for g in groups]), table=t, swap=0, min_cos=0.1, sel_cos=0.35,
                 gate_px=0.0, poison=41)
        d.update(kw)
        return d

    def group(F, seed, counts=None, **kw):
        a, b, sc = _frames(F, seed, counts, **kw)
        return a, b, sc

    cyc = [(0, 0), (5, 0), (63, 64), (64, 65), (65, 63), (130, 130), (0, 130), (None, None), (130, 5)]
    c['two frames'] = call([group(2, 0)])
    c['three frames, tails'] = call([group(3, 1, [(63, 64), (65, 130), (5, 0)])])
    c['WAVES + 1 frames'] = call([group(WAVES + 1, 22, cyc[:WAVES + 1])])
    c['2 WAVES + 1 frames'] = call([group(2 * WAVES + 1, 3, cyc[:2 * WAVES + 1])])
    c['camera 1 only'] = call([group(3, 5, [(130, 130)] * 3)], fr2=None)
    c['camera 2 only'] = call([group(3, 6, [(130, 130)] * 3)], fr1=None)
    ok = np.ones(2 + 5 + 0 + 2, np.int32); ok[3] = 0; ok[8] = 0
    c['three groups'] = call([group(2, 7, [(130, 130)] * 2), group(5, 8, [(65, 64)] * 5), group(0, 9), group(2, 10, [(130, 130)] * 2)], frame_ok=ok)
    c['refused lines'] = call([group(3, 11)], table=TC.main_table())
    c['transposed, swap 1'] = call([group(3, 12, [(130, 130)] * 3)], table=TC.transposed(t), swap=1)
    a, b, sc = _frames(3, 13, [(250, 250)] * 3)
    a = [dict(f, xy=f['xy'].copy()) for f in a]
    a[0]['xy'][[3, 10]] += [[10.0, 0.0], [0.0, -10.0]]
    a[2]['xy'][200] += [-7.0, 7.2]
    c['gate 4 px'] = call([(a, b, sc)], gate_px=4.0)
    two = call([group(2, 14, [(130, 130)] * 2), group(3, 15, [(65, 65)] * 3)])
    two['x0'] = two['x0'].copy(); two['x0'][0, 4] = np.nan
    c['NaN start in one group'] = two
    c['sel_cos = min_cos'] = call([group(3, 16)], sel_cos=0.1)
    return c


def full_table_case():
    """one frame at CPE_MAXP detections per camera (pixel_fit_cases._repeated) beside two ordinary ones, table L 256.  The repeated
    frame is table_tri_cases' cylinder (CYL_C, CYL_A), which is no frame of a scene: its TAGVcyl is made so that TTRUE * TAGVcyl
    has that axis and origin (columns 2 and 4 are all the call reads)"""
    a, b, sc = _frames(2, 17, [(130, 130)] * 2)
    f1, f2 = X._repeated(1, MAXP)
    A = np.eye(4)
    Ti = np.linalg.inv(TTRUE)
    A[:3, 1], A[:3, 3] = Ti[:3, :3] @ TC.CYL_A, Ti[:3, :3] @ TC.CYL_C + Ti[:3, 3]
    return dict(fr1=[a[0], f1, a[1]], fr2=[b[0], f2, b[1]], TAGV=np.stack([sc['TAGV'][0], A, sc['TAGV'][1]]), frame_ok=None,
                group_start=np.array([0, 3], np.int32), x0=sc['x0'][None], table=TC.rig_table(-128, 127), swap=0, min_cos=0.1, sel_cos=0.35,
                gate_px=0.0, poison=43)


def call_arrays(case):
    """-> dict(xy1, id1, cnt1, xy2, id2, cnt2 (None for an absent camera), n) as the C call reads them, poisoned past the counts"""
    n = len(case['TAGV'])
    out = dict(n=n)
    for cam, k in ((1, 'fr1'), (2, 'fr2')):
        if case[k] is None:
            out.update({f'xy{cam}': None, f'id{cam}': None, f'cnt{cam}': None})
        else:
            out[f'xy{cam}'], out[f'id{cam}'], out[f'cnt{cam}'] = TC.pack(case[k], None if case['poison'] is None else case['poison'] + cam)
    return out


def case_reference(case):
    """-> list over the groups of dict(ref_group's, kept: the frames' numbers in the call, rng: (a, b))"""
    n = len(case['TAGV'])
    ok = np.ones(n, bool) if case['frame_ok'] is None else np.asarray(case['frame_ok']) != 0
    out = []
    for g in range(len(case['group_start']) - 1):
        a, b = int(case['group_start'][g]), int(case['group_start'][g + 1])
        kept = [f for f in range(a, b) if ok[f]]
        pick = lambda k: [None] * len(kept) if case[k] is None else [case[k][f] for f in kept]
        r = ref_group(pick('fr1'), pick('fr2'), case['TAGV'][kept], case['x0'][g], case['table'], case['swap'], case['min_cos'], case['sel_cos'],
                      case['gate_px'])
        r.update(kept=kept, rng=(a, b), n_used=len(kept) if r['status'] == ST_OK else 0)
        r['opt'] = scipy_optimum(r, case['x0'][g]) if r['status'] == ST_OK else None
        out.append(r)
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    return case_reference(full_table_case() if name == 'full tables' else cases()[name])


def expected_pt_state(case, refs):
    """pt_state i32[n,2,MAXP] of the call: -1 where no group's range holds the frame"""
    n = len(case['TAGV'])
    out = np.full((n, 2, MAXP), -1, np.int32)
    cnt = lambda k, f: 0 if case[k] is None else min(max(int(case[k][f].get('cnt', len(case[k][f]['xy']))), 0), MAXP)
    for r in refs:
        for f in range(*r['rng']):
            out[f, 0, :cnt('fr1', f)], out[f, 1, :cnt('fr2', f)] = 1, 1
        for f, st, n1 in zip(r['kept'], r['states'], r['n1']):
            out[f, 0, :n1], out[f, 1, :len(st) - n1] = st[:n1], st[n1:]
    return out
