"""Cases and a numpy / scipy reference for the projector model (include/cpe.h cpe_fit_projector_model,
cpe_projector_model_table).

The reference restates the header's rule on the POINTS in float64: every residual r = n.(X - C) / |n| of every kept point is
a row of scipy.optimize.least_squares, whereas the kernels work on the per-line moments N, m, S alone -- so the two are
independent statements of the same least-squares problem.  The start is the header's closed form (np.linalg.eigh and lstsq in
place of Jacobi and elimination), the trimming loop is the header's.  After scipy the reference takes its own Gauss-Newton
steps (np.linalg.lstsq on the point Jacobian) until the step is below 1e-13, so its optimum does not lean on scipy's stopping
rule; gn_step(x) gives that step at any x, which is the stationarity check the GPU test applies to the kernel's result.

Tolerance of a case (x in mm for C, unit-free for a and b; the steps likewise):

    tol = 10 tolx + 64 eps cond max|X|

with eps = 2^-52, max|X| the largest point norm and cond the condition number of J'J after its columns have been scaled to unit
length (Jacobi scaling).  The kernel's LM stops on a step below tolx, and solves the damped normal equations, whose damping
term lambda diag(J'J) is exactly that scaling, by elimination with partial pivoting: the relative error of such a solve is
bounded by a small multiple of eps cond of the scaled matrix.  This is smaller, so stricter, than the same expression with a
factor m (the number of residuals) for the sums behind J'J and J'r, and than any expression with the unscaled J'J, whose
condition number (mm against radians against 1 / index) is 1e9 and more and says nothing about either solver: with either of
those no case could reach the 1e-6 that the cases are held to below.

Cases are generated so that every tolerance is <= 1e-6 and no residual of a trimming round lies within a relative 1e-6 of tau
(tests/test_proj_model_cases_cpu.py asserts both); then masks, counts, frame counts and statuses are compared exactly.

Measured on this reference (0.25 px noise, NOISY_SEEDS, the worst value over the seeds; NOISY_BOUNDS are twice these; the
normal error is the worst angle over the lines -12..12 of both families against true_line_planes, the offset error the worst
distance of the true centre from a fitted plane):

    12 board poses (17 x 25 grid)                        normal {boards_deg} deg, offset {boards_mm} mm
    12 cylinder frames, columns 0..8, rows -12..12       normal {cyl_deg} deg, offset {cyl_mm} mm  (columns -12..-1 never seen)
    the same with frames 3 and 7 numbered one column up, tau = 1 mm: after two refits exactly the 2 x 225 column residuals of
    those frames are trimmed, their row residuals kept, and the errors are those of the clean fit (0.0100 deg, 0.0354 mm)
"""
import functools
import math

import numpy as np

import plane_fit_cases as PC
import table_tri_cases as TC

MAXP, MAXL = PC.MAXP, PC.MAXL
ST_OK, ST_FEW_POINTS = 0, 5
EPS = PC.EPS
NOISY_SEEDS = PC.NOISY_SEEDS
TAU = 1.0
DEFAULTS = dict(tau=0.0, max_rounds=4, min_spread=1e-4, tolx=1e-9, tolf=1e-9, maxiter=100)
# twice the worst value measured over NOISY_SEEDS (tests/test_proj_model_cases_cpu.py measures them again)
NOISY_BOUNDS = dict(boards=dict(normal_deg=2 * 0.0045, offset_mm=2 * 0.0218), cyl=dict(normal_deg=2 * 0.0094, offset_mm=2 * 0.0410))
__doc__ = __doc__.format(boards_deg=NOISY_BOUNDS['boards']['normal_deg'] / 2, boards_mm=NOISY_BOUNDS['boards']['offset_mm'] / 2,
                         cyl_deg=NOISY_BOUNDS['cyl']['normal_deg'] / 2, cyl_mm=NOISY_BOUNDS['cyl']['offset_mm'] / 2)


# ------------------------------------------------------------------------------------------------------ the model
def true_model():
    """the rig's projector as x[15]: C, a_0, b_0, a_1, b_1 (family 0 = col)"""
    K1, K2, T21, Tp, delta, Op = PC.rig()
    R = Tp[:3, :3]
    return np.concatenate([Op, R.T @ [1.0, 0, 0], -delta * (R.T @ [0, 0, 1.0]), R.T @ [0, 1.0, 0], -delta * (R.T @ [0, 0, 1.0])])


def normals(x, fam, v):
    """unit normals (len(v),3) of the lines v of a family, and |a + v b|"""
    a, b = x[3 + 6 * fam:6 + 6 * fam], x[6 + 6 * fam:9 + 6 * fam]
    n = a + np.asarray(v, np.float64)[:, None] * b
    ln = np.linalg.norm(n, axis=1)
    return n / ln[:, None], ln


def tangent(a):
    """the header's basis of the tangent plane at a"""
    k = int(np.argmin(np.abs(a)))                # the first of the smallest
    ax = np.zeros(3)
    ax[k] = 1
    e1 = ax - (ax @ a) * a
    e1 = e1 / np.linalg.norm(e1)
    return e1, np.cross(a, e1)


def retract(x, dl):
    xn = np.array(x, np.float64)
    xn[:3] += dl[:3]
    for k in range(2):
        a = x[3 + 6 * k:6 + 6 * k]
        e1, e2 = tangent(a)
        t = a + dl[3 + 5 * k] * e1 + dl[4 + 5 * k] * e2
        xn[3 + 6 * k:6 + 6 * k] = t / np.linalg.norm(t)
        xn[6 + 6 * k:9 + 6 * k] = x[6 + 6 * k:9 + 6 * k] + dl[5 + 5 * k:8 + 5 * k]
    return xn


class Residuals:
    """the usable residuals of a call: per family the points, their indices, frames and slots"""

    def __init__(self, X, I, cnt, lo, hi, use=None, frame_ok=None):
        X = np.asarray(X, np.float64).reshape(-1, MAXP, 3)
        I = np.asarray(I).reshape(-1, MAXP, 2)
        cnt = np.asarray(cnt).reshape(-1)
        self.n, self.lo, self.hi = len(cnt), lo, hi
        self.P, self.v, self.f, self.k = [], [], [], []
        for fam in range(2):
            P, v, ff, kk = [np.zeros((0, 3))], [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
            for f in range(self.n):
                if frame_ok is not None and frame_ok[f] == 0:
                    continue
                c = min(max(int(cnt[f]), 0), MAXP)
                ok = np.isfinite(X[f, :c]).all(1)
                if use is not None:
                    ok &= np.asarray(use).reshape(-1, MAXP)[f, :c] != 0
                iv = I[f, :c, fam].astype(np.int64)
                ok &= (iv >= lo) & (iv <= hi)
                s = np.nonzero(ok)[0]
                P.append(X[f, s]); v.append(iv[s]); ff.append(np.full(len(s), f)); kk.append(s)
            self.P.append(np.concatenate(P)); self.v.append(np.concatenate(v)); self.f.append(np.concatenate(ff))
            self.k.append(np.concatenate(kk))

    def r(self, x, fam, keep=None):
        sel = slice(None) if keep is None else keep
        nh, _ = normals(x, fam, self.v[fam][sel])
        return ((self.P[fam][sel] - x[:3]) * nh).sum(1)

    def res(self, x, keep):
        return np.concatenate([self.r(x, 0, keep[0]), self.r(x, 1, keep[1])])

    def jac(self, x, keep):
        """rows: d r / d (dC, t_0, db_0, t_1, db_1) at x"""
        rows = []
        for fam in range(2):
            v = self.v[fam][keep[fam]].astype(np.float64)
            nh, ln = normals(x, fam, v)
            y = self.P[fam][keep[fam]] - x[:3]
            w = (y - (y * nh).sum(1)[:, None] * nh) / ln[:, None]
            e1, e2 = tangent(x[3 + 6 * fam:6 + 6 * fam])
            J = np.zeros((len(v), 13))
            J[:, :3] = -nh
            J[:, 3 + 5 * fam] = w @ e1
            J[:, 4 + 5 * fam] = w @ e2
            J[:, 5 + 5 * fam:8 + 5 * fam] = v[:, None] * w
            rows.append(J)
        return np.concatenate(rows)


def _lines(R, keep, min_spread):
    """moments and free planes of the kept residuals -> per family dict v -> (N, m, S, frames, normal or None)"""
    out = []
    for fam in range(2):
        d = {}
        P, v, f = R.P[fam][keep[fam]], R.v[fam][keep[fam]], R.f[fam][keep[fam]]
        for vv in np.unique(v):
            s = v == vv
            Q = P[s]
            m = Q.mean(0)
            E = Q - m
            S = E.T @ E
            fr = len(np.unique(f[s]))
            nrm = None
            if len(Q) >= 3 and fr >= 2:
                w, V = np.linalg.eigh(S)
                if w[2] > 0 and not w[1] / w[2] < min_spread:
                    nrm = V[:, 0]
            d[int(vv)] = (len(Q), m, S, fr, nrm)
        out.append(d)
    return out


def start(lines):
    """the header's closed-form start from the free planes; None: CPE_ST_FEW_POINTS"""
    us = [[(v, l[4], l[1]) for v, l in sorted(d.items()) if l[4] is not None] for d in lines]
    if len(us[0]) < 2 or len(us[1]) < 2:
        return None
    N = np.array([n for u in us for _, n, _ in u])
    d = np.array([n @ m for u in us for _, n, m in u])
    if np.linalg.cond(N) > 1e12:
        return None
    x = np.zeros(15)
    x[:3] = np.linalg.lstsq(N, d, rcond=None)[0]
    for fam, u in enumerate(us):
        Nf = np.array([n for _, n, _ in u])
        vs = np.array([v for v, _, _ in u], np.float64)
        axis = np.linalg.eigh(Nf.T @ Nf)[1][:, 0]
        ref = min(range(len(u)), key=lambda i: (abs(u[i][0]), u[i][0]))
        e1 = PC._orient_big(Nf[ref])
        e1 = e1 - (e1 @ axis) * axis
        e1 = e1 / np.linalg.norm(e1)
        e2 = np.cross(axis, e1)
        t = (Nf @ e2) / (Nf @ e1)
        dv = vs - vs.mean()
        beta = (dv @ t) / (dv @ dv)
        alpha = t.mean() - beta * vs.mean()
        a = e1 + alpha * e2
        x[3 + 6 * fam:6 + 6 * fam] = a / np.linalg.norm(a)
        x[6 + 6 * fam:9 + 6 * fam] = beta * e2 / np.linalg.norm(a)
    return x


def gn_step(R, keep, x):
    """the Gauss-Newton step of the point problem at x (13 numbers), and cond of the column-scaled J'J"""
    J, r = R.jac(x, keep), R.res(x, keep)
    sc = np.linalg.norm(J, axis=0)
    sc[sc == 0] = 1
    step = np.linalg.lstsq(J / sc, -r, rcond=None)[0] / sc
    return step, float(np.linalg.cond(J / sc)) ** 2


def minimise(R, keep, x0):
    """scipy on a 13-number chart about x0, then Gauss-Newton steps of the reference's own until they vanish"""
    from scipy.optimize import least_squares
    sol = least_squares(lambda p: R.res(retract(x0, p), keep), np.zeros(13), method='lm', xtol=1e-15, ftol=1e-15, gtol=1e-15,
                        x_scale='jac', max_nfev=2000)
    x = retract(x0, sol.x)
    for _ in range(20):
        step, _ = gn_step(R, keep, x)
        x = retract(x, step)
        if np.abs(step).max() < 1e-13:
            break
    return x


def ref_projector_model(X, I, cnt, lo, hi, use=None, frame_ok=None, tau=0.0, max_rounds=4, min_spread=1e-4, tolx=1e-9, x0=None,
                        **_):
    """-> dict(x (15,), f, status, rounds, kept (2,), mask u8 (2,n,MAXP), count, frames (2,L), frame_counts (n,4), moments
    (2,L,12), R, keep, tol, cond, margin).  A failed fit has x = 0."""
    R = Residuals(X, I, cnt, lo, hi, use, frame_ok)
    L = hi - lo + 1
    keep = [np.ones(len(R.v[k]), bool) for k in range(2)]
    x, status, rounds, margin = None, ST_OK, 0, math.inf
    for rnd in range((max_rounds if tau > 0 else 0) + 1):
        if rnd > 0:
            new = []
            for k in range(2):
                r = np.abs(R.r(x, k))
                if len(r):
                    margin = min(margin, float(np.min(np.abs(r - tau)) / tau))
                new.append(r < tau)
            if all(np.array_equal(a, b) for a, b in zip(new, keep)):
                break
            keep = new
            rounds = rnd
        lines = _lines(R, keep, min_spread)
        s = start(lines)
        if s is None:
            status = ST_FEW_POINTS
            break
        if rnd == 0 and x0 is not None:
            s = np.asarray(x0, np.float64)
        x = minimise(R, keep, s if rnd == 0 else x)
        if not np.isfinite(x).all():
            status = ST_FEW_POINTS
            break
    out = dict(status=status, rounds=rounds, kept=np.array([k.sum() for k in keep]), R=R, keep=keep, margin=margin)
    mask = np.zeros((2, R.n, MAXP), np.uint8)
    count, frames = np.zeros((2, L), np.int32), np.zeros((2, L), np.int32)
    fc = np.zeros((R.n, 4), np.int32)
    mom = np.zeros((2, L, 12))
    for k in range(2):
        mask[k, R.f[k][keep[k]], R.k[k][keep[k]]] = 1
        np.add.at(fc[:, 2 * k], R.f[k][keep[k]], 1)
        np.add.at(fc[:, 2 * k + 1], R.f[k][~keep[k]], 1)
        for v, (N, m, S, fr, _) in _lines(R, keep, min_spread)[k].items():
            count[k, v - lo], frames[k, v - lo] = N, fr
            mom[k, v - lo, :10] = [N, *m, S[0, 0], S[0, 1], S[0, 2], S[1, 1], S[1, 2], S[2, 2]]
    out.update(mask=mask, count=count, frames=frames, frame_counts=fc, moments=mom)
    if status != ST_OK:
        out.update(x=np.zeros(15), f=0.0, tol=0.0, cond=math.inf)
        return out
    r = R.res(x, keep)
    _, cond = gn_step(R, keep, x)
    xmax = max(float(np.linalg.norm(R.P[k][keep[k]], axis=1).max()) for k in range(2))
    for k in range(2):
        rk, vk = R.r(x, k, keep[k]), R.v[k][keep[k]]
        for v in np.unique(vk):
            mom[k, v - lo, 10] = math.sqrt((rk[vk == v] ** 2).mean())
    out.update(x=x, f=float(r @ r), cond=cond, xmax=xmax, tol=10 * tolx + 64 * EPS * cond * xmax)
    return out


def model_errors(x, lo=-12, hi=12):
    """a model against the rig's: the worst angle of a line's normal in degrees, the worst distance of the true centre from a
    line's plane in mm, over the lines lo..hi of both families"""
    tl, Op = PC.true_line_planes(lo, hi), PC.rig()[5]
    deg = mm = 0.0
    for k in range(2):
        nh, _ = normals(np.asarray(x, np.float64), k, np.arange(lo, hi + 1))
        for j in range(hi - lo + 1):
            a = PC.angle(nh[j], tl[k, j])
            deg = max(deg, math.degrees(min(a, math.pi - a)))
            mm = max(mm, abs(float(nh[j] @ (Op - x[:3]))))
    return dict(normal_deg=deg, offset_mm=mm)


# ------------------------------------------------------------------------------------------------------ tables
def cylinder_poses(seed, count):
    """seeded cylinders of TC.RADIUS in front of the rig: axis within 10 deg of y, centre within 10 mm, depth 345-385 mm"""
    rng = np.random.default_rng(2000 + seed)
    out = []
    for _ in range(count):
        az, el = np.radians(rng.uniform(-10, 10, 2))
        a = np.array([math.sin(az) * math.cos(el), math.cos(az) * math.cos(el), math.sin(el)])
        out.append((np.array([27.0 + rng.uniform(-10, 10), rng.uniform(-10, 10), rng.uniform(345, 385)]), a))
    return out


@functools.lru_cache(maxsize=None)
def cylinder_frames(seed=0, count=12, noise=0.25, cols=(0, 9), rows=(-12, 13)):
    """`count` frames of the grid cols x rows on seeded cylinders -> list of dict(idx, X, Xtrue); the cylinder's detector never
    gives a negative column, hence cols 0..8"""
    out = []
    for i, (c, a) in enumerate(cylinder_poses(seed, count)):
        idx, Xt = TC.cylinder_hits(c, a, TC.RADIUS, range(*cols), range(*rows))
        X = PC.triangulated(Xt, noise, np.random.default_rng(3000 + 100 * seed + i)) if noise > 0 else Xt
        out.append(dict(idx=idx, X=X, Xtrue=Xt))
    return out


SHIFTED = (3, 7)


def shifted_frames(seed=0):
    """cylinder_frames with the frames SHIFTED numbered one column too high"""
    fr = [dict(X=f['X'], idx=f['idx'].copy()) for f in cylinder_frames(seed)]
    for f in SHIFTED:
        fr[f]['idx'][:, 0] += 1
    return fr


def _plain(frames):
    return [dict(X=f['X'], idx=f['idx']) for f in frames]


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(frames, lo, hi[, use, frame_ok, x0, params...])"""
    mp = _plain(PC.multi_pose(0))
    cy = _plain(cylinder_frames(0))
    small = _plain(PC.multi_pose(7, 65, 0.25, 2, 3))             # 65 frames of 9 x 9 points
    c = {}
    c['boards 12'] = dict(frames=mp, lo=-12, hi=12)
    c['boards 3'] = dict(frames=mp[:3], lo=-12, hi=12)
    c['boards 65'] = dict(frames=small, lo=-12, hi=12)
    c['cylinder 12'] = dict(frames=cy, lo=-12, hi=12)
    c['shifted'] = dict(frames=shifted_frames(0), lo=-12, hi=12, tau=TAU)
    c['shifted 1 round'] = dict(frames=shifted_frames(0), lo=-12, hi=12, tau=TAU, max_rounds=1)
    c['shifted 0 rounds'] = dict(frames=shifted_frames(0), lo=-12, hi=12, tau=TAU, max_rounds=0)
    c['trimmed clean'] = dict(frames=mp[:3], lo=-12, hi=12, tau=TAU)
    # two lines per family leave b_k free along a gauge direction: GAUGE cases are compared through the objective, not through x
    c['L 2'] = dict(frames=mp[:4], lo=0, hi=1)
    c['L 256'] = dict(frames=mp[:3], lo=-128, hi=127)
    c['indices outside'] = dict(frames=mp[:4], lo=-5, hi=5)
    # counts -1, 0, 2, 3, 63, 64, 65 beside three full frames; 2048 and 3000 on a near board of 46 x 46 indices
    order = np.random.default_rng(5).permutation(len(mp[3]['X']))
    sub = lambda k, **kw: dict(X=mp[3]['X'][order][:k], idx=mp[3]['idx'][order][:k], **kw)
    c['counts'] = dict(frames=mp[:3] + [sub(10, cnt=-1), sub(10, cnt=0), sub(2), sub(3), sub(63), sub(64), sub(65)], lo=-12, hi=12)
    big = []
    for i, (tx, ty, z) in enumerate(((-9.0, 14.0, 190.0), (11.0, -8.0, 205.0), (4.0, 17.0, 180.0))):
        bi, bX, _ = PC.board_table(*PC.board(tx, ty, z), cols=range(-20, 26), rows=range(-10, 36), seed=11 + i)
        big.append(dict(X=bX[:MAXP], idx=bi[:MAXP], cnt=(MAXP, 3000, MAXP)[i]))
    c['counts 2048 3000'] = dict(frames=big, lo=-20, hi=35)
    nanf = dict(X=mp[1]['X'].copy(), idx=mp[1]['idx'])
    nanf['X'][::17, 2] = np.nan
    nanf['X'][5::29, 0] = np.inf
    c['nan points'] = dict(frames=[mp[0], nanf, mp[2]], lo=-12, hi=12)
    c['frame_ok'] = dict(frames=mp[:6], lo=-12, hi=12, frame_ok=np.array([1, 0, 1, 1, 0, 7], np.int32))
    use = (np.random.default_rng(9).random((6, MAXP)) < 0.7).astype(np.uint8)
    use[3] = 0
    c['use'] = dict(frames=mp[:6], lo=-12, hi=12, use=use)
    c['x0'] = dict(frames=mp[:3], lo=-12, hi=12, x0=retract(true_model(), np.array([.5, -.4, .8, 2e-3, -1e-3, 1e-4, 0, 0, -1e-3, 2e-3, 0, 1e-4, 0])))
    # CPE_ST_FEW_POINTS
    c['one pose'] = dict(frames=mp[:1], lo=-12, hi=12)
    c['one family'] = dict(frames=[dict(X=f['X'], idx=f['idx'] + np.array([0, 1000], np.int32)) for f in mp[:4]], lo=-12, hi=12)
    c['no frames'] = dict(frames=[], lo=-2, hi=2)
    c['empty tables'] = dict(frames=[dict(X=mp[0]['X'], idx=mp[0]['idx'], cnt=0), dict(X=mp[1]['X'], idx=mp[1]['idx'], cnt=-3)], lo=-12, hi=12)
    return c


GAUGE = ('L 2',)
FEW = ('one pose', 'one family', 'no frames', 'empty tables')


def params(case):
    return {k: case.get(k, d) for k, d in DEFAULTS.items()}


def arrays(case, poison=None):
    X, I, cnt = PC.pack(case['frames'], poison)
    return X, I, cnt, case.get('use'), case.get('frame_ok')


@functools.lru_cache(maxsize=None)
def reference(name):
    case = cases()[name]
    X, I, cnt, use, ok = arrays(case)
    return ref_projector_model(X, I, cnt, case['lo'], case['hi'], use, ok, x0=case.get('x0'), **params(case))


@functools.lru_cache(maxsize=None)
def noisy_reference(kind, seed):
    fr = _plain(PC.multi_pose(seed)) if kind == 'boards' else _plain(cylinder_frames(seed))
    X, I, cnt = PC.pack(fr)
    return ref_projector_model(X, I, cnt, -12, 12)


# ------------------------------------------------------------------------------------------------------ rendered frames
def table_errors(P, lo, true):
    """a table P (2,L,4) for the lines lo.. against TC.true_table's dict over the lines both hold: the worst angle of a normal in
    degrees, the worst distance of the true centre from a plane in mm"""
    tp = true['P'].reshape(-1, 4)
    C = np.linalg.lstsq(tp[:, :3], -tp[:, 3], rcond=None)[0]
    deg = mm = 0.0
    for k in range(2):
        for v in range(max(lo, true['lo']), min(lo + P.shape[1] - 1, true['hi']) + 1):
            p, q = P[k, v - lo], true['P'][k, v - true['lo']]
            a = PC.angle(p[:3], q[:3])
            deg = max(deg, math.degrees(min(a, math.pi - a)))
            mm = max(mm, abs(float(p[:3] @ C + p[3])))
    return deg, mm


def oracle_chain(orc, b, match=True, tau=TAU):
    """the oracle's statement of run_experiment(projector=dict(tau=tau), match_offset={} if match else None) on a rendered
    batch b of synth.render_batch: oracle detect on both images, the index shift by match_offset_cases.reference, chooseIdx,
    triangulate, then ref_projector_model over the seen index range -> its dict with lo, hi"""
    import match_offset_cases as MO
    from oracle import stages as S
    frames = []
    for i in range(len(b['left'])):
        dl, dr = S.detect_grid(b['left'][i].numpy()), S.detect_grid(b['right'][i].numpy())
        assert dl['status'] == 0 and dr['status'] == 0
        t1 = np.concatenate([dl['xy'], dl['id']], 1).astype(np.float64)
        t2 = np.concatenate([dr['xy'], dr['id']], 1).astype(np.float64)
        if match:
            mo = MO.reference(orc, t1, len(t1), t2, len(t2), b['K1'], b['K2'], b['T21'], b['radius'])
            assert not mo['flags'] & MO.WEAK
            t1[:, 2:4] = mo['id1_out']
        c1, c2, idx, _ = orc.choose_idx(t1, t2, b['K1'], b['K2'], b['T21'])
        frames.append(dict(X=orc.triangulate(c1, c2, b['K1'], b['K2'], b['T21'])[0], idx=idx))
    X, I, cnt = PC.pack(frames)
    lo, hi = min(int(f['idx'].min()) for f in frames), max(int(f['idx'].max()) for f in frames)
    return dict(ref_projector_model(X, I, cnt, lo, hi, tau=tau), lo=lo, hi=hi, frames=frames)
