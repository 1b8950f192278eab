"""The build-defined LM form of the multi-frame camera-AGV fit (cpe_multi_frame_fit_lm_batch), restated in numpy: the
all-frame closed-form initial pose, the Levenberg-Marquardt loop with fit_lm's damping and stop rule, and scipy's optimum of
the same least-squares problem as the yardstick.  Nothing here is bit-exact with the kernel: the restatement uses LAPACK's
eigenvectors and solver where the kernel runs its own Jacobi sweeps and Gaussian elimination, and sums in numpy's order.

    objective   v(x) = sum_i mean_k (d_ik - R)^2,  d_ik = distance of point k of frame i to the line through o_i = Rot p_i + t
                along v_i = Rot a_i, [Rot t] = vec2T(x), a_i / p_i = columns 2 / 4 of getTAGVcyl of frame i
    residuals   r_ik = (d_ik - R) / sqrt(n_i), so sum r^2 = v
    step        Rot <- exp([dw]x) Rot, t <- t + dt (left perturbation), x = T2vec
    Jacobian    e = (P - o) - v al, al = ((P - o).v)/|v|^2:  dr/dt = -e/d,  dr/dw = -((Rot p + al v) x e)/d,  both / sqrt(n_i)
"""
import math

import numpy as np

import multiframe_cases as mc

RADIUS = mc.RADIUS


# ------------------------------------------------------------------------------------------------------------- poses
def vec2T(x):
    return np.array(mc.vec2T([float(v) for v in x])).reshape(4, 4)


def T2vec(T):
    from cpe_amd import multiframe
    return np.array(multiframe.T2vec([float(v) for v in np.asarray(T).ravel()]))


def rot_exp(w):
    """exp([w]x) = I + A [w]x + B [w]x^2, A = sin(th)/th, B = (1 - cos th)/th^2, by their series below th = 1e-4"""
    w = np.asarray(w, dtype=np.float64)
    th2 = float((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    th = math.sqrt(th2)
    if th < 1e-4:
        A, B = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0
    else:
        A, B = math.sin(th) / th, (1.0 - math.cos(th)) / th2
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0.0]])
    return np.eye(3) + A * K + B * (K @ K)


def rotation_between(Ra, Rb):
    """||Ra' Rb - I||_F / sqrt(2): the rotation angle between two rotations, resolved down to ~1e-16 (acos of the trace
    resolves only ~1.5e-8 near the identity)"""
    return float(np.linalg.norm(Ra.T @ Rb - np.eye(3)) / math.sqrt(2.0))


# -------------------------------------------------------------------------------------------------------- the problem
class Problem:
    """one group of frames: flat point table, per-point frame index and 1/sqrt(n_i)"""

    def __init__(self, P, cnt, TAGV, radius=RADIUS):
        cnt = np.asarray(cnt)
        self.P, self.cnt, self.A, self.R = P, cnt, np.asarray(TAGV, dtype=np.float64).reshape(-1, 4, 4), radius
        self.pts = np.concatenate([P[i, :cnt[i]] for i in range(len(cnt))])
        self.frame = np.repeat(np.arange(len(cnt)), cnt)
        self.s = 1.0 / np.sqrt(cnt[self.frame].astype(np.float64))
        self.obj = mc.NumpyObjective(P, cnt, self.A, radius)

    def f(self, x):
        return self.obj([float(v) for v in x])

    def frame_terms(self, x):
        r = self.residuals(x)
        return np.bincount(self.frame, weights=r * r, minlength=len(self.cnt))

    def _geometry(self, T):
        Rot, t = T[:3, :3], T[:3, 3]
        q = self.A[:, :3, 3] @ Rot.T                       # Rot p_i
        v = self.A[:, :3, 1] @ Rot.T                       # Rot a_i
        o = q + t
        fr = self.frame
        w = self.pts - o[fr]
        vv = v[fr]
        al = np.einsum('ij,ij->i', w, vv) / np.einsum('ij,ij->i', vv, vv)
        e = w - vv * al[:, None]
        d = np.sqrt(np.einsum('ij,ij->i', e, e))
        return q[fr], vv, al, e, d

    def residuals(self, x):
        _, _, _, _, d = self._geometry(vec2T(x))
        return (d - self.R) * self.s

    def residuals_jacobian(self, x):
        q, vv, al, e, d = self._geometry(vec2T(x))
        ok = d > 0
        c = np.where(ok, -self.s / np.where(ok, d, 1.0), 0.0)
        m = q + vv * al[:, None]
        J = np.concatenate([np.cross(m, e), e], 1) * c[:, None]
        r = np.where(ok, (d - self.R) * self.s, 0.0)
        return r, J


# ---------------------------------------------------------------------------------------------------- initial pose
def horn_rotation(a, b):
    """the proper rotation maximising sum (Rot a_i).b_i: eigenvector of the largest eigenvalue of Horn's 4x4"""
    S = a.T @ b
    N = np.array([[S[0, 0] + S[1, 1] + S[2, 2], S[1, 2] - S[2, 1], S[2, 0] - S[0, 2], S[0, 1] - S[1, 0]],
                  [S[1, 2] - S[2, 1], S[0, 0] - S[1, 1] - S[2, 2], S[0, 1] + S[1, 0], S[2, 0] + S[0, 2]],
                  [S[2, 0] - S[0, 2], S[0, 1] + S[1, 0], -S[0, 0] + S[1, 1] - S[2, 2], S[1, 2] + S[2, 1]],
                  [S[0, 1] - S[1, 0], S[2, 0] + S[0, 2], S[1, 2] + S[2, 1], -S[0, 0] - S[1, 1] + S[2, 2]]])
    w, V = np.linalg.eigh(N)
    q0, qx, qy, qz = V[:, 3] / np.linalg.norm(V[:, 3])
    return np.array([[q0 * q0 + qx * qx - qy * qy - qz * qz, 2 * (qx * qy - q0 * qz), 2 * (qx * qz + q0 * qy)],
                     [2 * (qy * qx + q0 * qz), q0 * q0 - qx * qx + qy * qy - qz * qz, 2 * (qy * qz - q0 * qx)],
                     [2 * (qz * qx - q0 * qy), 2 * (qz * qy + q0 * qx), q0 * q0 - qx * qx - qy * qy + qz * qz]])


def usable_frames(cnt, raw):
    out = []
    for i in range(len(cnt)):
        row = raw[i, 1]
        if cnt[i] >= 1 and np.isfinite(row).all() and np.linalg.norm(row[3:]) > 0:
            out.append(i)
    return out


def initial_pose(prob, raw):
    """x0 of the LM form: rotation from all usable frames' fitted directions (both signs of the direction field tried, the
    lower objective kept, a tie to +1), translation by linear least squares on the fitted origins.  None: < 2 usable frames"""
    use = usable_frames(prob.cnt, raw)
    if len(use) < 2:
        return None
    o = raw[use, 1, 0:3]
    d = raw[use, 1, 3:6] / np.linalg.norm(raw[use, 1, 3:6], axis=1)[:, None]
    d = np.where((d @ d[0] < 0)[:, None], -d, d)
    a, p = prob.A[use, :3, 1], prob.A[use, :3, 3]
    Pr = np.eye(3)[None] - d[:, :, None] * d[:, None, :]                 # I - d d'
    best = None
    for sigma in (1.0, -1.0):
        R0 = horn_rotation(a, sigma * d)
        M = Pr.sum(0)
        M = M + 1e-12 * np.trace(M) * np.eye(3)
        rhs = np.einsum('ijk,ik->j', Pr, o - p @ R0.T)
        t0 = np.linalg.solve(M, rhs)
        T0 = np.eye(4); T0[:3, :3] = R0; T0[:3, 3] = t0
        x = T2vec(T0)
        f = prob.f(x)
        if best is None or f < best[0]:
            best = (f, x)
    return best[1]


# ------------------------------------------------------------------------------------------------------------- the LM
def lm(prob, x0, tolx=1e-5, tolf=1e-5, maxiter=100000):
    """fit_lm's loop (csrc/fit.hip) on the pose: lambda from 1e-3, /10 on acceptance (floor 1e-12), x10 on rejection, up to 12
    trials per iteration, diagonal M_aa (1 + lambda) + 1e-12 trace, stop when (f_prev - f) <= tolf 1e-3 (1 + f) and max|delta| <=
    tolx.  -> x, f, iterations, objective evaluations (f(x0) included)"""
    x = np.array(x0, dtype=np.float64)
    fx, lam, iters, evals = prob.f(x), 1e-3, 0, 1
    while iters < maxiter and iters < 200:
        r, J = prob.residuals_jacobian(x)
        A, g = J.T @ J, J.T @ r
        T = vec2T(x)
        iters += 1
        accepted, fprev, dmax = False, fx, 0.0
        for _ in range(12):
            M = A + np.diag(lam * np.diag(A) + 1e-12 * np.trace(A))
            try:
                dl = np.linalg.solve(M, -g)
            except np.linalg.LinAlgError:
                lam *= 10
                continue
            Tn = np.eye(4)
            Tn[:3, :3] = rot_exp(dl[:3]) @ T[:3, :3]
            Tn[:3, 3] = T[:3, 3] + dl[3:]
            xn = T2vec(Tn)
            fn = prob.f(xn)
            evals += 1
            if fn < fx:
                dmax, x, fx, lam, accepted = float(np.abs(dl).max()), xn, fn, max(lam / 10, 1e-12), True
                break
            lam *= 10
        if not accepted:
            break
        if (fprev - fx) <= tolf * 1e-3 * (1.0 + fx) and dmax <= tolx:
            break
    return x, fx, iters, evals


def fit(prob, raw, x0=None):
    """initial pose + LM -> dict(x0, x, T, fvals, iters, evals), or None with fewer than two usable frames"""
    if x0 is None:
        x0 = initial_pose(prob, raw)
        if x0 is None:
            return None
    f0 = prob.f(x0)
    x, f, iters, evals = lm(prob, x0)
    return dict(x0=np.array(x0), x=x, T=vec2T(x), fvals=[f0, f], iters=iters, evals=evals)


def scipy_optimum(prob, Ttrue):
    """least_squares(method='lm') from the true pose, tolerances at the limit of f64 -> x, f (by the objective the fits use)"""
    from scipy.optimize import least_squares
    res = least_squares(prob.residuals, T2vec(Ttrue), jac=lambda x: _rotvec_jacobian(prob, x), method='lm', xtol=1e-14, ftol=1e-14,
                        gtol=1e-14)
    return res.x, prob.f(res.x)


def _rotvec_jacobian(prob, x, h=1e-6):
    """d residuals / d x for scipy, central differences in the rotation vector (its chart is not the LM's), analytic in t"""
    _, J = prob.residuals_jacobian(x)
    out = np.empty_like(J)
    out[:, 3:] = J[:, 3:]
    for k in range(3):
        dx = np.zeros(6); dx[k] = h
        out[:, k] = (prob.residuals(x + dx) - prob.residuals(x - dx)) / (2 * h)
    return out


def rotation_error_deg(T, Ttrue):
    """the angle of the rotation between two poses, in degrees (||R - I||_F / sqrt(2) = 2 sin(angle / 2))"""
    return math.degrees(2.0 * math.asin(min(1.0, rotation_between(np.asarray(T).reshape(4, 4)[:3, :3], Ttrue[:3, :3]) / 2.0)))
