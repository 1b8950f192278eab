"""The build-defined frame-angle solver (cpe_frame_angles_lm_batch: pan and tilt of a frame from a calibrated camera-AGV pose),
restated in numpy: the chain's columns 2 and 4 and their derivatives in closed form, the closed-form start, the two-parameter
Levenberg-Marquardt with fit_lm's damping and stop rule, and scipy's optimum of the same least-squares problem as the
yardstick.  Nothing here is bit-exact with the kernel: sums are numpy's, sin / cos / tan the host libm's.

    chain       A(q) = getTAGVcyl(pan, tilt) = Rz(pan) Tx(-143.1) Tz(-143.1 tan(tilt)) Ry'(-tilt) T2C, with c = cos(-tilt),
                s = sin(-tilt):  column 2  a = Rz(pan) (-c, 0, s)
                                 column 4  p = Rz(pan) (-143.1 + 321.1 c + 110 s, 0, -143.1 tan(tilt) - 321.1 s + 110 c)
    objective   f(q) = mean_k (d_k - R)^2,  d_k = distance of point k to the line through o = Rot p + t along v = Rot a,
                [Rot t] = T_Cam_AGV; values always from the full product (multiframe_cases.get_TAGVcyl)
    residuals   r_k = (d_k - R) / sqrt(n)
    Jacobian    e = (P - o) - v al, al = ((P - o).v)/|v|^2:  dr/do = -e/d, dr/dv = -(al/d) e (fit_lm's), both / sqrt(n), chained
                with do/dq = Rot dp/dq, dv/dq = Rot da/dq
    start       a = Rot' d (d the frame's fitted direction, normalised), negated when a_x > 0, pan = atan2(-a_y, -a_x),
                tilt = asin(clamp(-a_z, -1, 1)): assumes |pan| < pi/2
"""
import math

import numpy as np

import multiframe_cases as mc

RADIUS = mc.RADIUS
LINKS = 143.1 + 321.1 + 110.0            # 574.2: the link lengths column 4 is made of
TILT_LIMIT = math.pi / 2 - 1e-3

# the frame fits of the zero-start finding: make_scene(12, seed, noise), counts from COUNT_CYCLE
FIT_SEEDS, FIT_NOISES, FIT_FRAMES = tuple(range(10)), (0.0, 0.05, 0.3), 12
START_OFF = 0.02                         # rad: how far the direction the start is made from lies off the true axis


# ---------------------------------------------------------------------------------------------------------- the chain
def chain_columns(pan, tilt):
    """-> a [..., 3], p [..., 3]: columns 2 and 4 of getTAGVcyl(pan, tilt) in closed form (arrays broadcast)"""
    pan, tilt = np.asarray(pan, dtype=np.float64), np.asarray(tilt, dtype=np.float64)
    cp, sp, c, s = np.cos(pan), np.sin(pan), np.cos(-tilt), np.sin(-tilt)
    ax, az = -c, s
    px, pz = -143.1 + 321.1 * c + 110.0 * s, -143.1 * np.tan(tilt) - 321.1 * s + 110.0 * c
    return np.stack([cp * ax, sp * ax, az + 0 * pan], -1), np.stack([cp * px, sp * px, pz + 0 * pan], -1)


def chain_derivatives(pan, tilt):
    """-> da/dpan, da/dtilt, dp/dpan, dp/dtilt, each [..., 3] (dc/dtilt = s, ds/dtilt = -c)"""
    pan, tilt = np.asarray(pan, dtype=np.float64), np.asarray(tilt, dtype=np.float64)
    cp, sp, c, s = np.cos(pan), np.sin(pan), np.cos(-tilt), np.sin(-tilt)
    ax, px = -c, -143.1 + 321.1 * c + 110.0 * s
    dax, daz = -s, -c
    dpx, dpz = 321.1 * s - 110.0 * c, -143.1 / (c * c) + 321.1 * c + 110.0 * s
    z = 0 * (pan + tilt)
    return (np.stack([-sp * ax, cp * ax, z], -1), np.stack([cp * dax, sp * dax, daz + z], -1),
            np.stack([-sp * px, cp * px, z], -1), np.stack([cp * dpx, sp * dpx, dpz + z], -1))


def start_from_direction(T, d):
    """the closed-form start: T 4x4 (T_Cam_AGV), d the fitted axis direction in the camera frame -> (pan, tilt)"""
    d = np.asarray(d, dtype=np.float64)
    a = np.asarray(T)[:3, :3].T @ (d / np.linalg.norm(d))
    if a[0] > 0:
        a = -a
    return np.array([math.atan2(-a[1], -a[0]), math.asin(min(1.0, max(-1.0, -a[2])))])


def usable(cnt, row):
    """multi_usable's rule for the fitted row cyl_raw[f,1,:]"""
    return bool(cnt >= 1 and np.isfinite(row).all() and np.linalg.norm(row[3:]) > 0)


def tcyl_product(T, A):
    """T * A (flat row-major 16 each) with every entry as ((a*b + c*d) + e*f) + g*h: separate multiplies and adds"""
    T, A = np.asarray(T, dtype=np.float64).reshape(4, 4), np.asarray(A, dtype=np.float64).reshape(4, 4)
    out = np.empty((4, 4))
    for r in range(4):
        for c in range(4):
            m = [np.float64(T[r, k]) * np.float64(A[k, c]) for k in range(4)]
            out[r, c] = ((m[0] + m[1]) + m[2]) + m[3]
    return out.ravel()


# -------------------------------------------------------------------------------------------------------- the problem
class FrameProblem:
    """one frame's points [n,3] against one pose T (4x4)"""

    def __init__(self, pts, T, radius=RADIUS):
        self.pts, self.T, self.R = np.ascontiguousarray(pts, dtype=np.float64), np.asarray(T, dtype=np.float64).reshape(4, 4), radius
        self.n = len(self.pts)
        self.sc = 1.0 / math.sqrt(self.n)

    def _geometry(self, q):
        Tc = self.T @ mc.get_TAGVcyl(float(q[0]), float(q[1]))                 # values: the full product
        o, dy = Tc[:3, 3], Tc[:3, 1]
        v = (o + dy) - o
        w = self.pts - o
        al = (w @ v) / ((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        e = w - al[:, None] * v
        return al, e, np.sqrt(np.einsum('ij,ij->i', e, e))

    def residuals(self, q):
        return (self._geometry(q)[2] - self.R) * self.sc

    def f(self, q):
        w = self._geometry(q)[2] - self.R
        return float(np.sum(w * w) / self.n)

    def residuals_jacobian(self, q):
        al, e, d = self._geometry(q)
        Rot = self.T[:3, :3]
        da_pan, da_tilt, dp_pan, dp_tilt = chain_derivatives(float(q[0]), float(q[1]))
        ok = d > 0
        c1 = np.where(ok, -self.sc / np.where(ok, d, 1.0), 0.0)
        c2 = c1 * al
        J = np.stack([c1 * (e @ (Rot @ dp)) + c2 * (e @ (Rot @ da)) for dp, da in ((dp_pan, da_pan), (dp_tilt, da_tilt))], 1)
        return np.where(ok, (d - self.R) * self.sc, 0.0), J


# ------------------------------------------------------------------------------------------------------------- the LM
def lm(prob, q0, tolx=1e-5, tolf=1e-5, maxiter=100000):
    """fit_lm's loop on (pan, tilt): lambda from 1e-3, /10 on acceptance (floor 1e-12), x10 on rejection, up to 12 trials per
    iteration, diagonal M_aa (1 + lambda) + 1e-12 trace, the 2x2 system in closed form, stop when (f_prev - f) <= tolf 1e-3
    (1 + f) and max|delta| <= tolx; a singular system, a candidate that is not finite or has |tilt| >= pi/2 - 1e-3 and a
    non-finite objective are rejected trials.  -> q, f, iterations, objective evaluations (f(q0) included)"""
    q = np.array(q0, dtype=np.float64)
    fx, lam, iters, evals = prob.f(q), 1e-3, 0, 1
    while iters < maxiter and iters < 200:
        r, J = prob.residuals_jacobian(q)
        s00, s01, s11 = float(J[:, 0] @ J[:, 0]), float(J[:, 0] @ J[:, 1]), float(J[:, 1] @ J[:, 1])
        g0, g1 = float(J[:, 0] @ r), float(J[:, 1] @ r)
        iters += 1
        accepted, fprev, dmax = False, fx, 0.0
        for _ in range(12):
            tr = s00 + s11
            m00, m11 = s00 + lam * s00 + 1e-12 * tr, s11 + lam * s11 + 1e-12 * tr
            det = m00 * m11 - s01 * s01
            if det == 0:
                lam *= 10
                continue
            dl = np.array([(s01 * g1 - m11 * g0) / det, (s01 * g0 - m00 * g1) / det])
            qn = q + dl
            if not (np.isfinite(qn).all() and abs(qn[1]) < TILT_LIMIT):
                lam *= 10
                continue
            fn = prob.f(qn)
            evals += 1
            if fn < fx:
                dmax, q, fx, lam, accepted = float(np.abs(dl).max()), qn, fn, max(lam / 10, 1e-12), True
                break
            lam *= 10
        if not accepted:
            break
        if (fprev - fx) <= tolf * 1e-3 * (1.0 + fx) and dmax <= tolx:
            break
    return q, fx, iters, evals


def scipy_optimum(prob, q_start):
    """least_squares(method='lm') with tolerances at the limit of f64 -> q, f (by the objective the fits use)"""
    from scipy.optimize import least_squares
    res = least_squares(prob.residuals, np.asarray(q_start, dtype=np.float64), jac=lambda q: prob.residuals_jacobian(q)[1],
                        method='lm', xtol=1e-14, ftol=1e-14, gtol=1e-14)
    return res.x, prob.f(res.x)


# -------------------------------------------------------------------------------------------------------------- scenes
def perturbed_direction(d, rng, off=START_OFF):
    """a unit vector `off` rad away from d, in a random direction"""
    d = d / np.linalg.norm(d)
    u = np.cross(d, rng.standard_normal(3))
    u /= np.linalg.norm(u)
    return math.cos(off) * d + math.sin(off) * u


def frame_fits(seeds=FIT_SEEDS, noises=FIT_NOISES, F=FIT_FRAMES):
    """the frame fits of the zero-start finding: dicts of prob, truth (pan, tilt), noise, n, and `start`: the closed-form start
    from a direction START_OFF off the frame's true axis"""
    out = []
    for noise in noises:
        for seed in seeds:
            P, cnt, angles, Ttrue = mc.make_scene(F, seed, noise)
            rng = np.random.default_rng(1000 + seed)
            for i in range(F):
                axis = (Ttrue @ mc.get_TAGVcyl(*angles[i]))[:3, 1]
                out.append(dict(prob=FrameProblem(P[i, :cnt[i]], Ttrue), truth=angles[i].copy(), noise=noise, n=int(cnt[i]),
                                start=start_from_direction(Ttrue, perturbed_direction(axis, rng))))
    return out


GPU_FRAMES, GPU_NOISES = (1, 2, 13, 65), (0.0, 0.05)
# A cylinder of known radius has four unknowns, so five points do not pin it down: the per-frame fit of a 5-point frame ends more
# than 0.1 rad from the true axis in about a quarter of the frames (up to 1.55 rad; test_frame_angles_cpu.py measures it), and a
# start made from such an axis is no start.  That is a limit of the input, not of the solver, so the scenes are chosen by a
# condition on the input alone: the first seed for which the per-frame fit of every frame (the oracle's, bit-identical to the
# GPU's) lies within AXIS_OFF of the frame's true axis -- less than a third of the way to the second minima, which lie 0.35-0.46
# rad from the truth.  test_frame_angles_cpu.py checks the condition for every seed here.
AXIS_OFF = 0.1
GPU_SEEDS = {(1, 0.0): 0, (1, 0.05): 0, (2, 0.0): 0, (2, 0.05): 0, (13, 0.0): 0, (13, 0.05): 0, (65, 0.0): 177, (65, 0.05): 188}
FAR_FIT = dict(F=13, seed=13, noise=0.0, frame=12)        # a 5-point frame whose fitted axis lies 1.47 rad from the true one


def gpu_scene(F, noise):
    """-> P, cnt, angles, Ttrue of make_scene(F, GPU_SEEDS[F, noise], noise): counts 5, 63, 64, 65, 160, 2048 in turn"""
    return mc.make_scene(F, GPU_SEEDS[(F, noise)], noise)


def axis_off(Ttrue, angles_i, d):
    """the angle between a fitted direction d (either sign) and the true axis of the frame"""
    axis = (Ttrue @ mc.get_TAGVcyl(*angles_i))[:3, 1]
    return math.acos(min(1.0, abs(float(d @ axis)) / float(np.linalg.norm(d))))


def angle_distance(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max())
