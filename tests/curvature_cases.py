"""Cases and references for cpe_est_curvatures_batch / cpe_curvature_consensus_batch (include/cpe.h), shared by
test_curvature_cases_cpu.py and test_curvature_gpu.py.  Nothing here needs a GPU or the library.

Generators: seeded cylinders as test_fit_init_cpu._points makes them; a regular 17 x 25 grid on the same cylinder (before the
noise and the rotation its neighbours tie exactly in d2, afterwards none do); a frame with three exact duplicates of one
point; a frame on an exact plane; the grid beside a 9 x 13 patch of a background plane.  pack() writes NaN past every count.

Two references, both float64 numpy:
  ordered(P, k, mode)  follows the header's operation order for d2, the ranking by (d2, index), the means, the covariance and
                       the normal equations (sums run over the neighbours in rank order); eigenvectors and the solve are
                       LAPACK's.  Its neighbour lists and gates are what the kernels must give exactly.
  lapack(P, k, mode)   in the manner of test_fit_init_cpu._init_numpy for every point and both columns: np.cov, eigh, lstsq
                       on the design matrix (no normal equations), eigh of the 2 x 2; it also returns cond2 of the design.

Tolerance of a point (tol()): C_TOL (cond2(A)^2 + 64) eps, relative to max |L| for L, scaled by max |L| / |l2 - l1| for the
columns.  Largest ratio error / ((cond2^2 + 64) eps) seen, numpy normal equations against lstsq over all cases here: 1.1;
the kernels on an MI355X against lapack(): see MAX_RATIO_GPU below."""
import functools
import math

import numpy as np

from test_fit_init_cpu import _points

MAXP = 2048
MAXK = 32
EPS = np.finfo(np.float64).eps
REFERENCE, INTERCEPT = 0, 1
UNKNOWNS = {REFERENCE: 5, INTERCEPT: 6}
C_TOL = 8.0
# values are compared where cond2 of the design is below this: beyond it the neighbourhood does not determine a quadric (four
# duplicates and one more point; the five nearest of a regular grid, a cross), and tol() itself passes 1e-3
COND_MAX = 1e6
# the largest ratio the kernels reached on an MI355X (test_curvature_gpu.py::test_values_against_lapack prints it per mode and k):
# mode 0: 0.662 (k 5), 0.568 (k 20), 0.206 (k 32); mode 1: 0.324 (k 6), 0.205 (k 20), 0.00287 (k 32)
MAX_RATIO_GPU = 0.662
R = 45.0
GATE_DEFAULT = (0.25, 0.0, math.inf)
GATE_BAND = (0.25, 30.0, 68.0)        # the gate of the grid + plane case, mm
COUNTS = [4, 5, 6, 19, 20, 21, 63, 64, 65, 256, 257, 2048]
KS = {REFERENCE: [5, 20, 32], INTERCEPT: [6, 20, 32]}


# ---------------------------------------------------------------------------------------------------------------- generators
def cylinder_points(seed, n=240, noise=0.02):
    return _points(seed, n=n, R=R, noise=noise)


def _rot(seed):
    rng = np.random.default_rng(1000 + seed)
    a, b = rng.uniform(-0.4, 0.4, 2)
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Rz = np.array([[np.cos(b), -np.sin(b), 0], [np.sin(b), np.cos(b), 0], [0, 0, 1]])
    return Rz @ Rx


def grid_points(seed=0, noise=0.05, rotate=True, nu=17, nv=25):
    """a regular nu x nv grid on the cylinder of _points (axis ~ y through (0, ., 500)).  noise = 0, rotate = False: the steps
    along the axis are exact in float64 (5 mm), so the neighbours at +- one step tie exactly in d2.  -> (P, axis point, axis dir)"""
    th = np.linspace(-0.9, 0.9, nu); t = -60.0 + 5.0 * np.arange(nv)
    T, TH = np.meshgrid(t, th)
    P = np.stack([R * np.sin(TH.ravel()), T.ravel(), 500.0 - R * np.cos(TH.ravel())], 1)
    org, d = np.array([0.0, 0.0, 500.0]), np.array([0.0, 1.0, 0.0])
    if rotate:
        Q, c = _rot(seed), P.mean(0)
        P = (P - c) @ Q.T + c; org = Q @ (org - c) + c; d = Q @ d
    if noise:
        P = P + np.random.default_rng(2000 + seed).normal(0, noise, P.shape)
    return P, org, d


def duplicates_points(seed=3, n=240):
    """slots 3, 7, 100 and 200 hold the same point: its three duplicates are the nearest neighbours of each other, by index"""
    P = cylinder_points(seed, n)
    P[[7, 100, 200]] = P[3]
    return P


def plane_points(seed=0, n=120):
    """an exact plane z = 500 with coordinates on a 1/8 mm lattice: every e.z is exactly 0, so every lambda is exactly 0"""
    rng = np.random.default_rng(3000 + seed)
    return np.stack([rng.integers(-400, 400, n) / 8.0, rng.integers(-400, 400, n) / 8.0, np.full(n, 500.0)], 1)


def grid_plus_plane(seed=0, noise=0.05):
    """the 425 grid points, then a 9 x 13 patch (117 points) of a background plane beside the cylinder.
    -> (P, is_cylinder bool[542], axis point, axis dir)"""
    G, org, d = grid_points(seed, noise=0.0, rotate=False)
    x = 50.0 + 5.0 * np.arange(9); y = -60.0 + 10.0 * np.arange(13)
    Xg, Yg = np.meshgrid(x, y)
    W = np.stack([Xg.ravel(), Yg.ravel(), np.full(Xg.size, 505.0)], 1)
    P = np.concatenate([G, W])
    Q, c = _rot(seed), G.mean(0)
    P = (P - c) @ Q.T + c + np.random.default_rng(4000 + seed).normal(0, noise, P.shape)
    return P, np.arange(len(P)) < len(G), Q @ (org - c) + c, Q @ d


def used(cnt):
    return min(max(int(cnt), 0), MAXP)


def pack(frames):
    """frames: list of (cnt, P) -> X f64[n,MAXP,3] with NaN past every count, cnt i32[n] (as given: the kernels clamp it)"""
    X = np.full((len(frames), MAXP, 3), np.nan)
    cnt = np.zeros(len(frames), np.int32)
    for i, (c, P) in enumerate(frames):
        X[i, :used(c)] = P[:used(c)]
        cnt[i] = c
    return X, cnt


# ---------------------------------------------------------------------------------------------------------------- references
def neighbours(P, k):
    """-> (nbr i32[n,K], d2 f64[n,n]): K = min(k, n) smallest by (d2, index), d2 = (a*a + b*b) + c*c"""
    a = P[None, :, 0] - P[:, None, 0]; b = P[None, :, 1] - P[:, None, 1]; c = P[None, :, 2] - P[:, None, 2]
    d2 = (a * a + b * b) + c * c
    return np.argsort(d2, axis=1, kind='stable')[:, :min(k, len(P))].astype(np.int32), d2


def _frame_of(z, mode):
    z = np.where(z[:, 2:3] < 0, -z, z)
    x0 = np.where(np.abs(z[:, :1]) > 0.9, np.array([[0.0, 1.0, 0.0]]), np.array([[1.0, 0.0, 0.0]]))
    y = np.cross(z, x0)
    if mode == INTERCEPT:
        y = y / np.sqrt((y[:, :1] ** 2 + y[:, 1:2] ** 2) + y[:, 2:3] ** 2)
    return np.cross(y, z), y, z


def _eig_pair(co, x, y):
    """L f64[n,2] ascending and K f64[n,2,3] from the quadric's coefficients, by eigh of [[2 co0, co1], [co1, 2 co2]]"""
    H = np.stack([np.stack([2 * co[:, 0], co[:, 1]], 1), np.stack([co[:, 1], 2 * co[:, 2]], 1)], 1)
    L, V = np.linalg.eigh(H)
    K = x[:, None, :] * V[:, 0, :, None] + y[:, None, :] * V[:, 1, :, None]
    return L, K


def ordered(P, k=20, mode=REFERENCE):
    """reference 1 -> dict(nbr, Kdir [n,2,3], L [n,2], normal [n,3])"""
    n = len(P)
    nbr, _ = neighbours(P, k)
    K = nbr.shape[1]
    mu = np.zeros((n, 3))
    for r in range(K):
        mu = mu + P[nbr[:, r]]
    mu = mu / float(K)
    Cv = np.zeros((n, 3, 3))
    for r in range(K):
        e = P[nbr[:, r]] - mu
        Cv = Cv + e[:, :, None] * e[:, None, :]
    Cv = Cv / float(K - 1)
    x, y, z = _frame_of(np.linalg.eigh(Cv)[1][:, :, 0], mode)
    nu = UNKNOWNS[mode]
    M = np.zeros((n, nu, nu)); rhs = np.zeros((n, nu))
    for r in range(K):
        e = P[nbr[:, r]] - mu
        lx = (e[:, 0] * x[:, 0] + e[:, 1] * x[:, 1]) + e[:, 2] * x[:, 2]
        ly = (e[:, 0] * y[:, 0] + e[:, 1] * y[:, 1]) + e[:, 2] * y[:, 2]
        lz = (e[:, 0] * z[:, 0] + e[:, 1] * z[:, 1]) + e[:, 2] * z[:, 2]
        row = np.stack([lx * lx, lx * ly, ly * ly, lx, ly] + ([np.ones(n)] if mode == INTERCEPT else []), 1)
        M = M + row[:, :, None] * row[:, None, :]
        rhs = rhs + row * lz[:, None]
    try:
        co = np.linalg.solve(M, rhs[:, :, None])[:, :, 0]
    except np.linalg.LinAlgError:                       # an exactly singular neighbourhood (a cross of a regular grid): zeros there
        co = np.zeros((n, nu))
        for p in range(n):
            try:
                co[p] = np.linalg.solve(M[p], rhs[p])
            except np.linalg.LinAlgError:
                pass
    L, Kd = _eig_pair(co, x, y)
    return dict(nbr=nbr, Kdir=Kd, L=L, normal=z)


def lapack(P, k=20, mode=REFERENCE):
    """reference 2 -> dict(Kdir, L, normal, cond [n]): LAPACK for every solve, no normal equations"""
    n = len(P)
    nbr, _ = neighbours(P, k)
    Kd = np.zeros((n, 2, 3)); L = np.zeros((n, 2)); N = np.zeros((n, 3)); cond = np.zeros(n)
    for p in range(n):
        Q = P[nbr[p]]
        z = np.linalg.eigh(np.cov(Q.T))[1][:, 0]
        x, y, z = _frame_of(z[None], mode)
        Lc = (Q - Q.mean(0)) @ np.stack([x[0], y[0], z[0]], 1)
        A = np.stack([Lc[:, 0] ** 2, Lc[:, 0] * Lc[:, 1], Lc[:, 1] ** 2, Lc[:, 0], Lc[:, 1]] +
                     ([np.ones(len(Q))] if mode == INTERCEPT else []), 1)
        co = np.linalg.lstsq(A, Lc[:, 2], rcond=None)[0]
        L[p], K2 = _eig_pair(co[None], x, y)
        Kd[p] = K2[0]; N[p] = z[0]; cond[p] = np.linalg.cond(A)
    return dict(Kdir=Kd, L=L, normal=N, cond=cond)


def tol(cond):
    return C_TOL * (cond ** 2 + 64.0) * EPS


def value_errors(got, ref):
    """the errors of L and of the columns (up to the sign of each) of `got` against lapack()'s `ref`, each divided by the scale
    the tolerance is relative to, so that `err <= tol(cond)` is the check: -> (eL [n], eK [n])"""
    sc = np.abs(ref['L']).max(1)
    gap = np.abs(ref['L'][:, 1] - ref['L'][:, 0])
    eL = np.abs(got['L'] - ref['L']).max(1) / sc
    dK = np.minimum(np.abs(got['Kdir'] - ref['Kdir']).max(2), np.abs(got['Kdir'] + ref['Kdir']).max(2)).max(1)
    return eL, dK / (sc / gap)


def gate_values(L):
    """(|lambda|max, |lambda|min / |lambda|max, 1 / |lambda|max, index of the bigger) per point, as the header states them"""
    a = np.abs(L)
    big = (a[:, 1] > a[:, 0]).astype(int)
    amax = a[np.arange(len(L)), big]; amin = a[np.arange(len(L)), 1 - big]
    with np.errstate(divide='ignore', invalid='ignore'):
        return amax, amin / amax, 1.0 / amax, big


def consensus(P, curv, gate=GATE_DEFAULT):
    """the consensus rule of the header on a reference's curvatures -> dict(gate bool[n], n_gated, rank, axis [8] or zeros,
    status, gap: the eigen-gap of sum t t' relative to its largest eigenvalue)"""
    rho_max, r_min, r_max = gate
    amax, rho, r, big = gate_values(curv['L'])
    idx = np.arange(len(P))
    t = curv['Kdir'][idx, 1 - big]
    tn = np.sqrt((t[:, 0] ** 2 + t[:, 1] ** 2) + t[:, 2] ** 2)
    g = (amax > 0) & (rho <= rho_max) & (r_min < r) & (r < r_max) & (tn > 0)
    ng = int(g.sum())
    out = dict(gate=g, n_gated=ng, rank=(ng - 1) // 2, axis=np.zeros(8), status=5, gap=0.0)
    if ng < 3:
        return out
    t = t[g] / tn[g, None]
    w, V = np.linalg.eigh(t.T @ t)
    d = V[:, 2]
    if d[np.argmax(np.abs(d))] < 0:
        d = -d
    c = P[g] + curv['normal'][g] / curv['L'][idx, big][g, None]
    org = c.mean(0)
    e = c - org
    e = e - np.outer(e @ d, d)
    out.update(axis=np.r_[org, d, np.sort(r[g])[out['rank']], np.sqrt((e ** 2).sum(1).mean())], status=0, gap=(w[2] - w[1]) / w[2],
               radii=r[g])
    return out


def clear_of_bounds(curv, gate, rel=1e-6):
    """no point's ratio or radius lies within `rel` (relative) of a gate bound: a rounding difference cannot move a point"""
    rho_max, r_min, r_max = gate
    amax, rho, r, _ = gate_values(curv['L'])
    ok = amax > 0
    far = lambda v, b: np.abs(v[ok] - b) > rel * max(abs(b), 1e-300) if math.isfinite(b) and b > 0 else np.ones(ok.sum(), bool)
    return bool(far(rho, rho_max).all() and far(r, r_min).all() and far(r, r_max).all())


def angle_deg(a, b):
    c = abs(a @ b) / (np.linalg.norm(a) * np.linalg.norm(b))
    return float(np.degrees(np.arccos(min(c, 1.0))))


def line_distance(org, d, org0, d0, half=60.0):
    """how far the line (org, d) runs from the true axis (org0, d0): the larger distance of the true axis' two end points
    (+- half along it) from the line"""
    d = d / np.linalg.norm(d)
    ends = np.stack([org0 + half * d0, org0 - half * d0])
    e = ends - org
    return float(np.linalg.norm(e - np.outer(e @ d, d), axis=1).max())


def pick_im(P):
    """the point fit_init picks (fitCylinderWPts3.m:7-21): nearest to the line through the mean along the 3rd pca axis"""
    ctr = P.mean(0)
    Vt = np.linalg.svd(P - ctr, full_matrices=False)[2]
    rdir = Vt[2] if Vt[2, 2] >= 0 else -Vt[2]
    v = P - ctr
    return int(np.argmin(np.linalg.norm(v - np.outer(v @ rdir, rdir), axis=1)))


# ---------------------------------------------------------------------------------------------------------------- the cases
@functools.lru_cache(maxsize=None)
def count_frames():
    """one frame per count of COUNTS, each from its own seed"""
    return [(c, cylinder_points(10 + i, max(c, 1), noise=0.05)[:c]) for i, c in enumerate(COUNTS)]


@functools.lru_cache(maxsize=None)
def mixed_batch():
    """counts 0, 5, 240 and one above MAXP (clamped)"""
    return [(0, np.zeros((0, 3))), (5, cylinder_points(31, 5)), (240, cylinder_points(32, 240)), (MAXP + 7, cylinder_points(33, MAXP))]


@functools.lru_cache(maxsize=None)
def reference(name, k, mode, which):
    """cached references of the named frames (their first used(cnt) points): which = 'ordered' or 'lapack'"""
    P = named_points(name)
    return (ordered if which == 'ordered' else lapack)(P, k, mode)


@functools.lru_cache(maxsize=None)
def named_neighbours(name, k):
    return neighbours(named_points(name), k)[0]


@functools.lru_cache(maxsize=None)
def named_points(name):
    """the points of a named frame that the kernels read"""
    if name.startswith('count'):
        return dict((f'count{c}', P) for c, P in count_frames())[name]
    if name.startswith('mixed'):
        c, P = mixed_batch()[int(name[5:])]
        return P[:used(c)]
    if name.startswith('cyl'):
        return cylinder_points(int(name[3:]))
    return dict(grid=lambda: grid_points(0)[0], tiegrid=lambda: grid_points(0, noise=0.0, rotate=False)[0], dup=duplicates_points,
                plane=plane_points, wall=lambda: grid_plus_plane(0)[0])[name]()


# the one batch the GPU tests run: (name, count as given to the kernels)
FRAMES = ([(f'count{c}', c) for c in COUNTS] + [(f'mixed{i}', c) for i, (c, _) in enumerate(mixed_batch())] +
          [(n, len(named_points(n))) for n in ('cyl0', 'grid', 'tiegrid', 'dup', 'plane', 'wall')])


# the frames whose consensus is compared with the reference's (the CPU test asserts that none of their gate values is near a bound)
CONSENSUS_NAMES = ('count64', 'count65', 'count256', 'count257', 'mixed2', 'cyl0', 'grid', 'dup', 'wall')


def batch():
    return pack([(c, named_points(n)) for n, c in FRAMES])


def ks_of(name, mode):
    """the k a frame's values are compared at: all three; k = 20 alone for the two full tables (the LAPACK reference is a loop);
    20 and 32 for the tie grid, whose five or six nearest are a cross or an L of the lattice -- an exactly singular design, or
    a quadric through the points with curvatures of 1e-14, which no relative tolerance fits (its neighbour lists are compared
    at every k)"""
    if name == 'tiegrid':
        return [20, 32]
    return [20] if len(named_points(name)) >= MAXP else KS[mode]


# ---------------------------------------------------------------------------------------------------------------- a stereo rig
def rig():
    """(K1, K2, T21) of test_fit_init_cpu.test_triangulation_matches_lapack_svd"""
    K1 = np.array([[2400.0, 0, 960], [0, 2400, 600], [0, 0, 1]]); K2 = np.array([[2390.0, 0, 955], [0, 2395, 610], [0, 0, 1]])
    a = 0.12
    T21 = np.eye(4); T21[:3, :3] = [[np.cos(a), 0, -np.sin(a)], [0, 1, 0], [np.sin(a), 0, np.cos(a)]]; T21[:3, 3] = [-120.0, 1.5, 8.0]
    return K1, K2, T21


def tables_of(P, ids):
    """the two images' grid-point tables [x y col row] of the 3-D points P (camera-1 coordinates) with the indices ids [n,2]"""
    K1, K2, T21 = rig()
    h = np.c_[P, np.ones(len(P))]
    p1 = h @ (K1 @ np.eye(4)[:3]).T; p2 = h @ (K2 @ T21[:3]).T
    return np.c_[p1[:, :2] / p1[:, 2:], ids], np.c_[p2[:, :2] / p2[:, 2:], ids]


def wall_ids():
    """(col, row) of the grid + plane case: the grid's 17 x 25 nodes, then the patch's 9 x 13 at columns 20..28"""
    g = np.stack(np.meshgrid(np.arange(25), np.arange(17)), -1).reshape(-1, 2)[:, ::-1]
    w = np.stack(np.meshgrid(20 + np.arange(9), np.arange(13)), -1).reshape(-1, 2)
    return np.concatenate([g, w]).astype(np.int64)
