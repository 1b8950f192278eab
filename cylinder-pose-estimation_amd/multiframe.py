"""Row f-1: the multi-frame camera<->AGV fit, utils/fitCylinderWPts3sAngs.m (+ getTAGVcyl.m, vec2T.m,
T2vec.m), the immediate consumer of the per-frame outputs (exp_gridDetection.m:87).

One 6-parameter Nelder-Mead (MATLAB fminsearch order) over  v(agvPose) = sum_i mean((d_i - R)^2), in two forms:

fit_multi_frame      the data-parallel part -- distances of every frame's points to that frame's predicted axis -- is the
                     HIP kernel behind cpe_multi_frame_terms (one wavefront per frame, points stay in HBM); the simplex logic
                     is host code in plain Python floats (IEEE double, libm sin/cos/acos), which is what MATLAB's interpreter
                     does for the reference.  Bit-identical to the oracle; one host round trip per objective evaluation.
fit_multi_frame_gpu  the whole fit in one call of cpe_multi_frame_fit_batch: initial pose, simplex and objective on the
                     device, one workgroup per group of frames, nothing read back.  Same terms, same simplex order; sin / cos
                     / acos are the device math library's, so f agrees with the host form to about 1e-12 relative, not bit
                     for bit.
                     method='lm' (build-defined, cpe_multi_frame_fit_lm_batch): the same objective minimised by
                     Levenberg-Marquardt from an initial pose made of all frames -- about ten passes over the points.

[ext] rotvec2mat3d / rotmat2vec3d / mrdivide / fminsearch are restated as in oracle/src/orc_fit.c (parity unpinned).
Reproduced quirk: cylParams{i} is the 2x6 [cylParams0; cylParams] matrix and applyCylParamsPrior indexes it linearly
(applyCylParamsPrior.m:6-7), so the "origin"/"direction" used for the initial pose mix the two rows.
"""
import ctypes
import math

import torch

from . import lib as _lib


def get_TAGVcyl(pan, tilt):
    """getTAGVcyl.m (default config), row-major 4x4 as a flat list"""
    cp, sp, ct, st = math.cos(pan), math.sin(pan), math.cos(-tilt), math.sin(-tilt)
    TAP = [cp, -sp, 0, 0, sp, cp, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]
    TPT0 = [1, 0, 0, -143.1, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]
    L = math.sqrt((-143.1 * -143.1 + 0.0 * 0.0) + 0.0 * 0.0)
    mtr = -math.tan(tilt) * L
    T01 = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, mtr, 0, 0, 0, 1]
    T12 = [ct, 0, st, 0, 0, 1, 0, 0, -st, 0, ct, 0, 0, 0, 0, 1]
    T2C = [0, -1, 0, 321.1, -1, 0, 0, 0, 0, 0, -1, 110, 0, 0, 0, 1]
    acc = [float(v) for v in TAP]
    for M in (TPT0, T01, T12, T2C):
        nxt = [0.0] * 16
        for r in range(4):
            for c in range(4):
                s = 0.0
                for k in range(4):
                    s = s + acc[r * 4 + k] * M[k * 4 + c]
                nxt[r * 4 + c] = s
        acc = nxt
    return acc


def _rotvec2mat(v):
    th = math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    if th < 1e-6:
        return [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0]
    u = [v[0] / th, v[1] / th, v[2] / th]
    c, s, t = math.cos(th), math.sin(th), 1 - math.cos(th)
    K = [0, -u[2], u[1], u[2], 0, -u[0], -u[1], u[0], 0]
    return [(c * (1.0 if r == q else 0.0) + t * (u[r] * u[q])) + s * K[r * 3 + q] for r in range(3) for q in range(3)]


def _mat2rotvec(R):
    t = (R[0] + R[4]) + R[8]
    ca = min(1.0, max(-1.0, (t - 1) / 2))
    th = math.acos(ca)
    r = [R[7] - R[5], R[2] - R[6], R[3] - R[1]]
    if math.sin(th) >= 1e-4:
        vth = 1 / (2 * math.sin(th))
        return [th * (r[k] * vth) for k in range(3)]
    if t - 1 > 0:
        return [(.5 - (t - 3) / 12) * r[k] for k in range(3)]
    a = 0
    if R[4] > R[a * 4]:
        a = 1
    if R[8] > R[a * 4]:
        a = 2
    b, c = (a + 1) % 3, (a + 2) % 3
    s = math.sqrt(R[a * 4] - R[b * 4] - R[c * 4] + 1)
    w = [0.0, 0.0, 0.0]
    w[a] = s / 2
    w[b] = (R[b * 3 + a] + R[a * 3 + b]) / (2 * s)
    w[c] = (R[c * 3 + a] + R[a * 3 + c]) / (2 * s)
    nw = math.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    return [th * w[k] / nw for k in range(3)]


def vec2T(x):
    """vec2T.m -> flat row-major 4x4"""
    R = _rotvec2mat(x)
    T = [0.0] * 16
    for r in range(3):
        for c in range(3):
            T[r * 4 + c] = R[r * 3 + c]
        T[r * 4 + 3] = x[3 + r]
    T[15] = 1.0
    return T


def T2vec(T):
    R = [T[r * 4 + c] for r in range(3) for c in range(3)]
    return _mat2rotvec(R) + [T[3], T[7], T[11]]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _apply_prior(cyl, ymin):
    o, d = list(cyl[:3]), list(cyl[3:])
    if d[1] < 0:
        d = [-d[0], -d[1], -d[2]]
    t = 0.0
    if not (abs(d[1]) < 2.220446049250313e-16):
        t = (ymin - o[1]) / d[1]
    return [o[c] + t * d[c] for c in range(3)] + d


def initial_pose(cyl_raw01, ymin01, TAGV01):
    """T0 of fitCylinderWPts3sAngs.m:40-69 as a rotation-vector pose (6 floats)"""
    cp = []
    for i in range(2):
        M = cyl_raw01[i]                                  # 2 x 6 nested list [cylParams0; cylParams]
        lin = [M[k % 2][k // 2] for k in range(6)]        # MATLAB linear (column-major) indexing of the 2x6 matrix
        cp.append(_apply_prior(lin, ymin01[i]))
    A1, A2 = TAGV01
    p1, p2 = [A1[3], A1[7], A1[11]], [A2[3], A2[7], A2[11]]
    y1 = [A1[1], A1[5], A1[9]]
    d12 = [p2[k] - p1[k] for k in range(3)]
    nd = _cross(y1, d12)
    nn = math.sqrt((nd[0] * nd[0] + nd[1] * nd[1]) + nd[2] * nd[2])
    nd = [v / nn for v in nd]
    ed12 = [cp[1][k] - cp[0][k] for k in range(3)]
    dir1 = cp[0][3:]
    en = _cross(dir1, ed12)
    ne = math.sqrt((en[0] * en[0] + en[1] * en[1]) + en[2] * en[2])
    en = [v / ne for v in en]
    c1, c2 = _cross(dir1, en), _cross(y1, nd)
    Ac, Bc = [dir1, en, c1], [y1, nd, c2]
    Bt = [Bc[r][c] for r in range(3) for c in range(3)]
    At = [Ac[r][c] for r in range(3) for c in range(3)]
    for c in range(3):                                    # R = A / B: Gaussian elimination on B' R' = A'
        pv = c
        for r in range(c + 1, 3):
            if abs(Bt[r * 3 + c]) > abs(Bt[pv * 3 + c]):
                pv = r
        if pv != c:
            for k in range(3):
                Bt[c * 3 + k], Bt[pv * 3 + k] = Bt[pv * 3 + k], Bt[c * 3 + k]
                At[c * 3 + k], At[pv * 3 + k] = At[pv * 3 + k], At[c * 3 + k]
        for r in range(c + 1, 3):
            f = Bt[r * 3 + c] / Bt[c * 3 + c]
            for k in range(c, 3):
                Bt[r * 3 + k] = Bt[r * 3 + k] - f * Bt[c * 3 + k]
            for k in range(3):
                At[r * 3 + k] = At[r * 3 + k] - f * At[c * 3 + k]
    Rt = [0.0] * 9
    for k in range(3):
        for r in (2, 1, 0):
            s = At[r * 3 + k]
            for q in range(r + 1, 3):
                s = s - Bt[r * 3 + q] * Rt[q * 3 + k]
            Rt[r * 3 + k] = s / Bt[r * 3 + r]
    T0 = [0.0] * 16
    for r in range(3):
        for c in range(3):
            T0[r * 4 + c] = Rt[c * 3 + r]
    for r in range(3):
        s = (T0[r * 4] * p1[0] + T0[r * 4 + 1] * p1[1]) + T0[r * 4 + 2] * p1[2]
        T0[r * 4 + 3] = cp[0][r] - s
    T0[15] = 1.0
    return T2vec(T0)


def _eps(x):
    x = abs(x)
    if x < 2.2250738585072014e-308:
        return 5e-324
    m, e = math.frexp(x)
    return math.ldexp(1.0, e - 53)


def nelder_mead6(fobj, x0, tolx=1e-5, tolf=1e-5, maxiter=100000, maxfun=100000):
    """MATLAB fminsearch.m, n = 6 (same order of operations as oracle/src/orc_fit.c::nelder_mead6_fn)"""
    N = 6
    v = [list(x0)]
    fv = [fobj(v[0])]
    for j in range(N):
        y = list(x0)
        y[j] = (1 + 0.05) * y[j] if y[j] != 0 else 0.00025
        v.append(y)
        fv.append(fobj(y))

    def sort_simplex():
        order = sorted(range(N + 1), key=lambda k: fv[k])     # Python's sort is stable, as MATLAB's
        return [v[k] for k in order], [fv[k] for k in order]

    v, fv = sort_simplex()
    func_evals, itercount = N + 1, 1
    while func_evals < maxfun and itercount < maxiter:
        df = max(abs(fv[0] - fv[j]) for j in range(1, N + 1))
        dx = max(abs(v[j][k] - v[0][k]) for j in range(1, N + 1) for k in range(N))
        if df <= max(tolf, 10 * _eps(fv[0])) and dx <= max(tolx, 10 * _eps(max(v[0]))):
            break
        xbar = []
        for k in range(N):
            s = v[0][k]
            for j in range(1, N):
                s = s + v[j][k]
            xbar.append(s / N)
        xr = [2.0 * xbar[k] - 1.0 * v[N][k] for k in range(N)]
        fxr = fobj(xr); func_evals += 1
        shrink = False
        if fxr < fv[0]:
            xe = [3.0 * xbar[k] - 2.0 * v[N][k] for k in range(N)]
            fxe = fobj(xe); func_evals += 1
            if fxe < fxr:
                v[N], fv[N] = xe, fxe
            else:
                v[N], fv[N] = xr, fxr
        elif fxr < fv[N - 1]:
            v[N], fv[N] = xr, fxr
        elif fxr < fv[N]:
            xc = [1.5 * xbar[k] - 0.5 * v[N][k] for k in range(N)]
            fxc = fobj(xc); func_evals += 1
            if fxc <= fxr:
                v[N], fv[N] = xc, fxc
            else:
                shrink = True
        else:
            xcc = [0.5 * xbar[k] + 0.5 * v[N][k] for k in range(N)]
            fxcc = fobj(xcc); func_evals += 1
            if fxcc < fv[N]:
                v[N], fv[N] = xcc, fxcc
            else:
                shrink = True
        if shrink:
            for j in range(1, N + 1):
                v[j] = [v[0][k] + 0.5 * (v[j][k] - v[0][k]) for k in range(N)]
                fv[j] = fobj(v[j])
            func_evals += N
        v, fv = sort_simplex()
        itercount += 1
    return v[0], fv[0], itercount, func_evals


class MultiFrameObjective:
    """v(agvPose) with the per-frame terms computed on the GPU"""

    def __init__(self, pts3, cnt, TAGV, radius):
        self.L = _lib.load()
        self.pts3, self.cnt, self.radius = pts3.contiguous(), cnt.contiguous(), float(radius)
        self.F = cnt.shape[0]
        self.TAGV = torch.tensor(TAGV, dtype=torch.float64, device=pts3.device).reshape(self.F, 16).contiguous()
        self.terms = torch.zeros(self.F, dtype=torch.float64, device=pts3.device)
        self.Tdev = torch.zeros(16, dtype=torch.float64, device=pts3.device)

    def __call__(self, x):
        self.Tdev.copy_(torch.tensor(vec2T(x), dtype=torch.float64))
        _lib.check(self.L.cpe_multi_frame_terms(self.pts3.data_ptr(), self.cnt.data_ptr(), self.F, self.TAGV.data_ptr(),
                                                self.Tdev.data_ptr(), self.radius, self.terms.data_ptr(),
                                                torch.cuda.current_stream().cuda_stream), 'cpe_multi_frame_terms')
        v = 0.0
        for t in self.terms.tolist():                      # v = v + (vi*vi')/length(vi), in frame order
            v = v + t
        return v


def fit_multi_frame(pts3, cnt, cyl_raw, angles, radius):
    """[T, fval] = fitCylinderWPts3sAngs(Pts3s, angs, cylRadius)
    pts3 f64[F,MAXP,3] / cnt i32[F] / cyl_raw f64[F,2,6] as returned by fit_cylinder_batch (fitCylinderWPts3 per frame),
    angles: F x 2 (pan, tilt) in rad  ->  dict(T 4x4 row-major list, x, x0, fvals [f0, f], iters, evals)"""
    F = cnt.shape[0]
    assert F >= 2 and len(angles) == F
    TAGV = [get_TAGVcyl(float(a[0]), float(a[1])) for a in angles]
    raw01 = cyl_raw[:2].cpu().tolist()
    ymin01 = [float(pts3[i, :int(cnt[i]), 1].min()) for i in range(2)]
    x0 = initial_pose(raw01, ymin01, TAGV[:2])
    obj = MultiFrameObjective(pts3, cnt, [v for T in TAGV for v in T], radius)
    f0 = obj(x0)
    x, f, iters, evals = nelder_mead6(obj, x0)
    return dict(T=vec2T(x), x=x, x0=x0, fvals=[f0, f], iters=iters, evals=evals, TAGV=TAGV)


def _tol_params(tol_x=1e-5, tol_f=1e-5, max_iter=100000, max_fun_evals=100000):
    return _lib.CpeFitParams(tol_x, tol_f, max_iter, max_fun_evals, 0, 0)


def _frame_tables(pts3, cnt, cyl_raw, angles, frame_ok, group_start):
    """the frame tables of the resident multi-frame calls as the C ABI takes them: checked, contiguous, on the points' device
    -> pts3, cnt, cyl_raw, TAGV f64[n,16], frame_ok (i32[n] or None), group_start i32[G+1], G"""
    dev, n = pts3.device, cnt.shape[0]
    pts3, cnt, cyl_raw = pts3.contiguous(), cnt.contiguous(), cyl_raw.contiguous()
    assert pts3.dtype == torch.float64 and cyl_raw.dtype == torch.float64 and cnt.dtype == torch.int32
    assert pts3.shape == (n, _lib.MAXP, 3) and cyl_raw.shape == (n, 2, 6)
    if torch.is_tensor(angles):
        TAGV = angles.to(device=dev, dtype=torch.float64).contiguous()
        assert TAGV.shape == (n, 16), 'a tensor of angles is the [n,16] table of getTAGVcyl matrices'
    else:
        assert len(angles) == n
        TAGV = torch.tensor([get_TAGVcyl(float(a[0]), float(a[1])) for a in angles], dtype=torch.float64).reshape(n, 16).to(dev)
    if group_start is None:
        group_start = [0, n]
    if not torch.is_tensor(group_start):
        group_start = torch.tensor(list(group_start), dtype=torch.int32)
    gs = group_start.to(device=dev, dtype=torch.int32).contiguous()
    G = gs.numel() - 1
    assert G >= 0
    if frame_ok is not None:
        frame_ok = frame_ok.to(device=dev, dtype=torch.int32).contiguous()
        assert frame_ok.shape == (n,)
    return pts3, cnt, cyl_raw, TAGV, frame_ok, gs, G


def fit_multi_frame_gpu(pts3, cnt, cyl_raw, angles, radius, frame_ok=None, group_start=None, x0=None, method='nm', **tol):
    """fitCylinderWPts3sAngs for G groups of frames in one resident call (cpe_multi_frame_fit_batch): nothing is read back
    and the launch is queued on the current stream.  Arguments given on the host -- angles as pan / tilt pairs, a list for
    group_start or x0 -- are made into tensors here and copied to the device from pageable memory; only the form with
    device tensors for all of them (angles as the [n,16] table) is free of host copies and graph-capturable.
    pts3 f64[n,MAXP,3] / cnt i32[n] / cyl_raw f64[n,2,6] as fit_multi_frame takes them (device tensors)
    angles       n x 2 (pan, tilt) in rad on the host, or a device tensor f64[n,16] of row-major getTAGVcyl matrices
    frame_ok     None, or i32[n] on the device: a frame with 0 is left out of its group
    group_start  None = one group of all n frames; G+1 ascending frame offsets (list, or i32 device tensor)
    x0           None = the initial pose of fitCylinderWPts3sAngs.m:40-69, or f64[G,6] (device tensor or nested list)
    method       'nm' = the reference's fminsearch (cpe_multi_frame_fit_batch); 'lm' = the build-defined fast mode
                 (cpe_multi_frame_fit_lm_batch): Levenberg-Marquardt on the same objective, and with x0 None an initial pose made
                 of all usable frames instead of :40-69 (see include/cpe.h)
    tol          tol_x, tol_f, max_iter, max_fun_evals (default: the reference's 1e-5 / 1e-5 / 1e5 / 1e5)
    -> dict of device tensors: x0, x f64[G,6]; T f64[G,16] row-major vec2T(x); fvals f64[G,2] = [f0, f]; iters i32[G,2] =
       [iterations, evaluations]; n_used i32[G]; status i32[G] (0 = fitted; see include/cpe.h); TAGV f64[n,16]; with 'lm' also
       frame_terms f64[n]: the term of every kept frame of a fitted group at the returned pose, NaN for every other frame.
       group_result(res, g) is the host view of one group with the keys of fit_multi_frame."""
    assert method in ('nm', 'lm')
    L = _lib.load()
    dev, n = pts3.device, cnt.shape[0]
    pts3, cnt, cyl_raw, TAGV, frame_ok, gs, G = _frame_tables(pts3, cnt, cyl_raw, angles, frame_ok, group_start)
    if x0 is not None:
        x0 = torch.as_tensor(x0, dtype=torch.float64).to(dev).reshape(G, 6).contiguous()
    params = _tol_params(**tol)
    if method == 'lm':
        params.mode = _lib.const.FIT_LM
    out = dict(x0=torch.empty((G, 6), dtype=torch.float64, device=dev), x=torch.empty((G, 6), dtype=torch.float64, device=dev),
               T=torch.empty((G, 16), dtype=torch.float64, device=dev), fvals=torch.empty((G, 2), dtype=torch.float64, device=dev),
               iters=torch.empty((G, 2), dtype=torch.int32, device=dev), n_used=torch.empty(G, dtype=torch.int32, device=dev),
               status=torch.empty(G, dtype=torch.int32, device=dev), TAGV=TAGV)
    args = (pts3.data_ptr(), cnt.data_ptr(), TAGV.data_ptr(), cyl_raw.data_ptr(), frame_ok.data_ptr() if frame_ok is not None else None,
            gs.data_ptr(), G, n, float(radius), ctypes.addressof(params), x0.data_ptr() if x0 is not None else None,
            out['x0'].data_ptr(), out['x'].data_ptr(), out['T'].data_ptr(), out['fvals'].data_ptr(), out['iters'].data_ptr(),
            out['n_used'].data_ptr(), out['status'].data_ptr())
    stream = torch.cuda.current_stream().cuda_stream
    if method == 'lm':
        out['frame_terms'] = torch.full((n,), float('nan'), dtype=torch.float64, device=dev)
        _lib.check(L.cpe_multi_frame_fit_lm_batch(*args, out['frame_terms'].data_ptr(), stream), 'cpe_multi_frame_fit_lm_batch')
    else:
        _lib.check(L.cpe_multi_frame_fit_batch(*args, stream), 'cpe_multi_frame_fit_batch')
    return out


def fit_multi_frame_consensus_gpu(pts3, cnt, cyl_raw, angles, radius, frame_ok=None, group_start=None, tau=0.5, max_hyp=2048,
                                  max_rounds=4, min_inliers=3, **tol):
    """Build-defined (cpe_multi_frame_consensus_batch; the rule is numbered in include/cpe.h): the LM form of the multi-frame fit
    for experiments that hold frames with status 0 and a wrong cylinder.  Poses made of two usable frames each are scored by
    the kept frames whose term at them lies below tau^2 (the rms of dist - radius below tau); the best pose's frames are fitted
    by the LM loop of method='lm', the inliers are taken again, up to max_rounds times.  Two launches on the current stream,
    nothing is read back.
    pts3, cnt, cyl_raw, angles, radius, frame_ok, group_start, tol: as fit_multi_frame_gpu takes them
    tau          in the unit of the points (> 0); max_hyp 1..4096 hypotheses per group; max_rounds 0..16; min_inliers >= 2: a
                 consensus of fewer frames is refused (status 5)
    -> dict of device tensors: x0, x, T, fvals, iters, n_used, status, TAGV as fit_multi_frame_gpu(method='lm') -- x0 the
       winning hypothesis, fvals = [the objective of x0 over its inliers, of x over the frames x was fitted to], iters summed
       over the rounds -- and n_inliers i32[G] (frames x was fitted to), info i32[G,4] = [winning hypothesis, its two frames,
       rounds done], flags i32[G] (lib.CONSENSUS_CONVERGED | lib.CONSENSUS_SHRUNK), inlier i32[n] (1 / 0 for the kept frames of a
       fitted group, -1 for every other frame), frame_terms f64[n] (the term of every kept frame of a fitted group at x,
       outliers included; NaN for every other frame).  A majority of frames that are wrong in the same way wins; one tau per
       call; a frame is in or out whole."""
    L = _lib.load()
    dev, n = pts3.device, cnt.shape[0]
    pts3, cnt, cyl_raw, TAGV, frame_ok, gs, G = _frame_tables(pts3, cnt, cyl_raw, angles, frame_ok, group_start)
    params = _tol_params(**tol)
    params.mode = _lib.const.FIT_LM
    cons = _lib.CpeConsensusParams(float(tau), int(max_hyp), int(max_rounds), int(min_inliers))
    ws = torch.empty(max(1, L.cpe_multi_frame_consensus_workspace_bytes(G, cons.max_hyp)), dtype=torch.uint8, device=dev)
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    out = dict(x0=f64(G, 6), x=f64(G, 6), T=f64(G, 16), fvals=f64(G, 2), iters=i32(G, 2), n_used=i32(G), n_inliers=i32(G),
               info=i32(G, 4), flags=i32(G), status=i32(G), inlier=torch.full((n,), -1, dtype=torch.int32, device=dev),
               frame_terms=torch.full((n,), float('nan'), dtype=torch.float64, device=dev), TAGV=TAGV)
    _lib.check(L.cpe_multi_frame_consensus_batch(
        pts3.data_ptr(), cnt.data_ptr(), TAGV.data_ptr(), cyl_raw.data_ptr(), frame_ok.data_ptr() if frame_ok is not None else None,
        gs.data_ptr(), G, n, float(radius), ctypes.addressof(params), ctypes.addressof(cons), ws.data_ptr(), ws.numel(),
        *(out[k].data_ptr() for k in ('x0', 'x', 'T', 'fvals', 'iters', 'n_used', 'n_inliers', 'info', 'flags', 'status', 'inlier',
                                      'frame_terms')), torch.cuda.current_stream().cuda_stream), 'cpe_multi_frame_consensus_batch')
    return out


def _pixels_inputs(what, cam1, cam2, x0, radius, K1, K2, T21, laser_table, frame_ok, group_start, sel_cos, min_cos, tol_x, tol_f, max_iter):
    """what the two pixel-space multi-frame calls share: the arguments checked, and everything but the angles as the C ABI takes it
    -> dev, n, tabs ((xy, id, cnt) per camera, None for an absent one), frame_ok, group_start i32[G+1], G, x0 f64[G,6], K1, K2, T21,
    P, line_status, centre"""
    from . import fit as _fit
    for c in (cam1, cam2):
        if any(t is None for t in c) and not all(t is None for t in c):
            raise ValueError(f'{what}: a camera is given by all three of xy, id, cnt or by none')
    if cam1[0] is None and cam2[0] is None:
        raise ValueError(f'{what}: both cameras are absent')
    if not laser_table.has_centre():
        raise ValueError(f'{what}: the table has no projector centre (centre_status is not ST_OK)')
    if not (0 < min_cos < 1 and min_cos <= sel_cos < 1 and tol_x > 0 and tol_f > 0 and int(max_iter) >= 1 and radius > 0):
        raise ValueError(f'{what}: 0 < min_cos <= sel_cos < 1, tol_x, tol_f, radius > 0 and max_iter >= 1, got {min_cos}, {sel_cos}, '
                         f'{tol_x}, {tol_f}, {radius}, {max_iter}')
    if x0 is None:
        raise ValueError(f'{what}: x0 is required (there is no closed-form start in pixel space)')
    some = cam1[2] if cam1[2] is not None else cam2[2]
    dev, n = some.device, some.shape[0]
    tabs = []
    for name, c in (('camera 1 ', cam1), ('camera 2 ', cam2)):
        if c[0] is None:
            tabs.append((None, None, None))
            continue
        gp = _fit.GridTables(c[0].contiguous(), c[1].contiguous(), c[2].contiguous())
        _fit._check_tables(what, gp, n, name, dev)
        tabs.append((gp.xy, gp.id, gp.cnt))
    if group_start is None:
        group_start = [0, n]
    if not torch.is_tensor(group_start):
        group_start = torch.tensor(list(group_start), dtype=torch.int32)
    gs = group_start.to(device=dev, dtype=torch.int32).contiguous()
    G = gs.numel() - 1
    assert G >= 0
    if frame_ok is not None:
        frame_ok = frame_ok.to(device=dev, dtype=torch.int32).contiguous()
        assert frame_ok.shape == (n,)
    x0 = torch.as_tensor(x0, dtype=torch.float64).to(dev).reshape(G, 6).contiguous()
    K1, K2, T21 = _fit._cameras(K1, K2, T21, dev)
    P, st, centre = _fit._table_on(laser_table, dev, centre=True)
    return dev, n, tabs, frame_ok, gs, G, x0, K1, K2, T21, P, st, centre


def fit_multi_frame_pixels_gpu(xy1, id1, cnt1, xy2, id2, cnt2, angles, x0, radius, K1, K2, T21, laser_table, frame_ok=None,
                               group_start=None, sel_cos=0.35, min_cos=0.1, gate_px=0.0, tol_x=1e-9, tol_f=1e-9, max_iter=100,
                               want_res=False):
    """Build-defined, opt-in (cpe_multi_frame_fit_pixels_batch; the rule is numbered in include/cpe.h):
    T_Cam_AGV fitted to the pixels of every kept frame of a group at once, from a start that a point-based multi-frame fit gave.
    One launch on the current stream, nothing is read back.
    xy1 f64[n,MAXP,2], id1 i32[n,MAXP,2], cnt1 i32[n]: camera 1's tables (device tensors); xy2, id2, cnt2: camera 2's.  Either
                 camera's three may all be None: that camera is absent
    angles, frame_ok, group_start: as fit_multi_frame_gpu takes them (the ranges of two groups may not share a frame here)
    x0           f64[G,6] (device tensor or nested list), required: e.g. fit_multi_frame_gpu(..., method='lm')['x']
    K1, K2, T21, laser_table: the cameras and a fit.LaserTable (ids are (col, row)), as fit.fit_cylinder_pixels_batch takes them;
                 the table must have a projector centre and be rigid with camera 1 across the frames
    sel_cos      the grazing gate for membership of the used set (min_cos <= sel_cos < 1); min_cos: the gate of every evaluation;
                 gate_px <= 0: no residual gate
    -> dict of device tensors: x f64[G,6], T f64[G,16], fvals f64[G,2], iters i32[G,2], n_used i32[G], counts i32[G,4], stats
       f64[G,4], status i32[G], N f64[G,21], cov f64[G,6,6] = F / (2 |S| - 6) inverse(J'J) in the step's coordinates (dw, dt), NaN
       where the status is not 0; pt_state i32[n,2,MAXP]; frame_cyl f64[n,6] and frame_stats f64[n,4] (NaN for every frame that is
       not a kept frame of a fitted group); res f64[n,2,MAXP,2] with want_res (zero for those frames), else None; TAGV f64[n,16]"""
    what = 'fit_multi_frame_pixels_gpu'
    L = _lib.load()
    dev, n, tabs, frame_ok, gs, G, x0, K1, K2, T21, P, st, centre = _pixels_inputs(
        what, (xy1, id1, cnt1), (xy2, id2, cnt2), x0, radius, K1, K2, T21, laser_table, frame_ok, group_start, sel_cos, min_cos, tol_x, tol_f,
        max_iter)
    if torch.is_tensor(angles):
        TAGV = angles.to(device=dev, dtype=torch.float64).contiguous()
        assert TAGV.shape == (n, 16), 'a tensor of angles is the [n,16] table of getTAGVcyl matrices'
    else:
        assert len(angles) == n
        TAGV = torch.tensor([get_TAGVcyl(float(a[0]), float(a[1])) for a in angles], dtype=torch.float64).reshape(n, 16).to(dev)
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    nan = float('nan')
    out = dict(x=f64(G, 6), T=f64(G, 16), fvals=f64(G, 2), iters=i32(G, 2), n_used=i32(G), counts=i32(G, 4), stats=f64(G, 4),
               status=i32(G), N=f64(G, 21), pt_state=torch.full((n, 2, _lib.MAXP), -1, dtype=torch.int32, device=dev),
               frame_cyl=torch.full((n, 6), nan, dtype=torch.float64, device=dev),
               frame_stats=torch.full((n, 4), nan, dtype=torch.float64, device=dev),
               res=torch.zeros((n, 2, _lib.MAXP, 2), dtype=torch.float64, device=dev) if want_res else None)
    from .fit import _ptr as p
    if G and n:
        _lib.check(L.cpe_multi_frame_fit_pixels_batch(
            *(p(t) for t in tabs[0]), *(p(t) for t in tabs[1]), TAGV.data_ptr(), p(frame_ok), gs.data_ptr(), G, n, x0.data_ptr(),
            float(radius), K1.data_ptr(), K2.data_ptr(), T21.data_ptr(), P.data_ptr(), st.data_ptr(), laser_table.lo, laser_table.hi,
            centre.data_ptr(), laser_table.swap_for('col_row'), float(min_cos), float(sel_cos), float(gate_px), float(tol_x),
            float(tol_f), int(max_iter), *(p(out[k]) for k in ('x', 'T', 'fvals', 'iters', 'n_used', 'counts', 'stats', 'status', 'N',
                                                               'pt_state', 'frame_cyl', 'frame_stats', 'res')),
            torch.cuda.current_stream().cuda_stream), 'cpe_multi_frame_fit_pixels_batch')
    elif G:                                                    # groups of no frames: what the call would have written
        for k in ('x', 'T', 'fvals', 'iters', 'n_used', 'counts', 'stats', 'N'):
            out[k].zero_()
        out['status'].fill_(_lib.const.ST_FEW_POINTS)
    out['cov'] = _pixels_covariance(out)
    out['TAGV'] = TAGV
    return out


def _pixels_covariance(out):
    """F / (2 |S| - 6) inverse(N) per group -> f64[G,6,6], NaN where the status is not 0 or N cannot be inverted"""
    G, dev = out['status'].shape[0], out['status'].device
    iu = torch.triu_indices(6, 6, device=dev)
    Nf = torch.zeros((G, 6, 6), dtype=torch.float64, device=dev)
    Nf[:, iu[0], iu[1]] = out['N']
    Nf = Nf + torch.triu(Nf, 1).transpose(1, 2)
    ok = out['status'] == 0
    eye = torch.eye(6, dtype=torch.float64, device=dev)
    inv, info = torch.linalg.inv_ex(torch.where(ok[:, None, None], Nf, eye))
    dof = (2 * out['counts'][:, :2].sum(1) - 6).to(torch.float64)
    ok = ok & (info == 0) & (dof > 0)
    cov = inv * (out['fvals'][:, 1] / torch.where(dof > 0, dof, torch.ones_like(dof)))[:, None, None]
    return torch.where(ok[:, None, None], cov, torch.full_like(cov, float('nan')))


def fit_multi_frame_pixels_angles_gpu(xy1, id1, cnt1, xy2, id2, cnt2, angles, x0, radius, K1, K2, T21, laser_table, frame_ok=None,
                                      group_start=None, sigma_px=0.25, sigma_angle=0.002, w_pan=None, w_tilt=None, sel_cos=0.35,
                                      min_cos=0.1, gate_px=0.0, tol_x=1e-9, tol_f=1e-9, max_iter=100, want_res=False):
    """Build-defined, opt-in (cpe_multi_frame_fit_pixels_angles_batch; the rule is numbered in include/cpe.h):
    T_Cam_AGV and the pan and tilt of every kept frame fitted jointly to the pixels of a group, each angle held at its nominal value
    by a Gaussian prior.  For heads whose angles are not exact; with exact angles fit_multi_frame_pixels_gpu is 2 - 15 x nearer.
    One launch on the current stream, nothing is read back.
    xy1 .. cnt2, x0, radius, K1, K2, T21, laser_table, frame_ok, group_start, sel_cos, min_cos, gate_px, tol_x, tol_f, max_iter,
                 want_res: as fit_multi_frame_pixels_gpu takes them; a group may hold at most lib.const.MFJOINT_MAXF kept frames
    angles       the nominal (pan, tilt) in rad: n x 2 on the host, or a device tensor f64[n,2]
    sigma_px, sigma_angle: the weight of the prior is sigma_px / sigma_angle pixels per radian for both angles; w_pan, w_tilt
                 given explicitly override it
    -> the dict of fit_multi_frame_pixels_gpu (fvals holds the prior's part, stats[:, 2] does not; N is the reduced matrix with the
       angles eliminated and cov = F / (2 |S| - 6) inverse(N) the covariance of (dw, dt) with the angles marginalised; TAGV is the
       chain at the NOMINAL angles), and angles0 f64[n,2], angles f64[n,2] the fitted ones, frame_N f64[n,17] = V | W | g of every
       frame's block, angle_sigma f64[n,2] the standard errors of the fitted angles (the last three NaN for every frame that is not
       a kept frame of a fitted group)"""
    from .fit import _ptr as p
    what = 'fit_multi_frame_pixels_angles_gpu'
    L = _lib.load()
    w_pan = float(sigma_px) / float(sigma_angle) if w_pan is None else float(w_pan)
    w_tilt = float(sigma_px) / float(sigma_angle) if w_tilt is None else float(w_tilt)
    if not (0 < w_pan < math.inf and 0 < w_tilt < math.inf):
        raise ValueError(f'{what}: the prior weights must be positive and finite, got {w_pan}, {w_tilt}')
    dev, n, tabs, frame_ok, gs, G, x0, K1, K2, T21, P, st, centre = _pixels_inputs(
        what, (xy1, id1, cnt1), (xy2, id2, cnt2), x0, radius, K1, K2, T21, laser_table, frame_ok, group_start, sel_cos, min_cos, tol_x, tol_f,
        max_iter)
    angles0 = torch.as_tensor(angles, dtype=torch.float64).to(dev).reshape(n, 2).contiguous()
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    nans = lambda *shape: torch.full(shape, float('nan'), dtype=torch.float64, device=dev)
    out = dict(x=f64(G, 6), T=f64(G, 16), fvals=f64(G, 2), iters=i32(G, 2), n_used=i32(G), counts=i32(G, 4), stats=f64(G, 4),
               status=i32(G), N=f64(G, 21), pt_state=torch.full((n, 2, _lib.MAXP), -1, dtype=torch.int32, device=dev),
               frame_cyl=nans(n, 6), frame_stats=nans(n, 4),
               res=torch.zeros((n, 2, _lib.MAXP, 2), dtype=torch.float64, device=dev) if want_res else None,
               angles=nans(n, 2), frame_N=nans(n, 17))
    if G and n:
        _lib.check(L.cpe_multi_frame_fit_pixels_angles_batch(
            *(p(t) for t in tabs[0]), *(p(t) for t in tabs[1]), angles0.data_ptr(), p(frame_ok), gs.data_ptr(), G, n, x0.data_ptr(),
            w_pan, w_tilt, float(radius), K1.data_ptr(), K2.data_ptr(), T21.data_ptr(), P.data_ptr(), st.data_ptr(), laser_table.lo,
            laser_table.hi, centre.data_ptr(), laser_table.swap_for('col_row'), float(min_cos), float(sel_cos), float(gate_px),
            float(tol_x), float(tol_f), int(max_iter),
            *(p(out[k]) for k in ('x', 'T', 'fvals', 'iters', 'n_used', 'counts', 'stats', 'status', 'N', 'pt_state', 'frame_cyl',
                                  'frame_stats', 'res', 'angles', 'frame_N')),
            torch.cuda.current_stream().cuda_stream), 'cpe_multi_frame_fit_pixels_angles_batch')
    elif G:                                                    # groups of no frames: what the call would have written
        for k in ('x', 'T', 'fvals', 'iters', 'n_used', 'counts', 'stats', 'N'):
            out[k].zero_()
        out['status'].fill_(_lib.const.ST_FEW_POINTS)
    out['cov'] = _pixels_covariance(out)
    out['angle_sigma'] = _angle_sigma(out, gs)
    out['angles0'] = angles0
    out['TAGV'] = agv_chain_batch(angles0) if n else f64(0, 16)
    return out


def _angle_sigma(out, gs):
    """the standard errors of the fitted angles: with s2 = F / (2 |S| - 6), C = cov of the frame's group and B = inverse(V) W',
    cov(q_i) = s2 inverse(V_i) + B C B' -> the square roots of its diagonal f64[n,2]; NaN where frame_N or cov is.  Device only."""
    fN, G = out['frame_N'], out['status'].shape[0]
    n, dev = fN.shape[0], fN.device
    if n == 0 or G == 0:
        return torch.full((n, 2), float('nan'), dtype=torch.float64, device=dev)
    grp = torch.bucketize(torch.arange(n, device=dev, dtype=torch.int32), gs[1:].contiguous(), right=True).clamp(max=G - 1)
    dof = (2 * out['counts'][:, :2].sum(1) - 6).to(torch.float64)
    s2 = (out['fvals'][:, 1] / dof)[grp]
    C = out['cov'][grp]
    v0, v1, v2 = fN[:, 0], fN[:, 1], fN[:, 2]
    det = v0 * v2 - v1 * v1
    Vi = torch.stack([v2, -v1, -v1, v0], 1).reshape(n, 2, 2) / det[:, None, None]
    B = Vi @ fN[:, 3:15].reshape(n, 6, 2).transpose(1, 2)
    cq = s2[:, None, None] * Vi + B @ C @ B.transpose(1, 2)
    return torch.sqrt(torch.diagonal(cq, dim1=1, dim2=2))


def group_result(res, g=0):
    """one group of fit_multi_frame_gpu's result on the host (this synchronises), with the keys of fit_multi_frame --
    T (flat row-major 4x4), x, x0, fvals [f0, f], iters, evals, TAGV (all frames' matrices) -- plus n_used and status, and
    frame_terms (all frames') where the result has them (method='lm'); of fit_multi_frame_consensus_gpu's result also
    n_inliers, info [hypothesis, frame, frame, rounds], flags and inlier (all frames')"""
    it = res['iters'][g].tolist()
    out = dict(T=res['T'][g].tolist(), x=res['x'][g].tolist(), x0=res['x0'][g].tolist(), fvals=res['fvals'][g].tolist(),
               iters=it[0], evals=it[1], TAGV=res['TAGV'].tolist(), n_used=int(res['n_used'][g]), status=int(res['status'][g]))
    if 'frame_terms' in res:
        out['frame_terms'] = res['frame_terms'].tolist()
    if 'inlier' in res:
        out.update(n_inliers=int(res['n_inliers'][g]), info=res['info'][g].tolist(), flags=int(res['flags'][g]),
                   inlier=res['inlier'].tolist())
    return out


def vec2T_batch(x):
    """vec2T.m on the device: x f64[n,6] -> T f64[n,16] row-major (cpe_pose_vec2T_batch; asynchronous)"""
    x = x.contiguous()
    assert x.dtype == torch.float64 and x.dim() == 2 and x.shape[1] == 6
    T = torch.empty((x.shape[0], 16), dtype=torch.float64, device=x.device)
    _lib.check(_lib.load().cpe_pose_vec2T_batch(x.data_ptr(), x.shape[0], T.data_ptr(), torch.cuda.current_stream().cuda_stream),
               'cpe_pose_vec2T_batch')
    return T


def T2vec_batch(T):
    """T2vec.m on the device: T f64[n,16] (or [n,4,4]) row-major -> x f64[n,6] (cpe_pose_T2vec_batch; asynchronous)"""
    T = T.reshape(T.shape[0], 16).contiguous()
    assert T.dtype == torch.float64
    x = torch.empty((T.shape[0], 6), dtype=torch.float64, device=T.device)
    _lib.check(_lib.load().cpe_pose_T2vec_batch(T.data_ptr(), T.shape[0], x.data_ptr(), torch.cuda.current_stream().cuda_stream),
               'cpe_pose_T2vec_batch')
    return x


def agv_chain_batch(angles):
    """getTAGVcyl.m on the device: angles f64[n,2] (pan, tilt) in rad -> f64[n,16] row-major (cpe_agv_chain_batch; asynchronous).
    get_TAGVcyl's operations with the device math library's sin / cos / tan."""
    angles = angles.contiguous()
    assert angles.dtype == torch.float64 and angles.dim() == 2 and angles.shape[1] == 2
    A = torch.empty((angles.shape[0], 16), dtype=torch.float64, device=angles.device)
    _lib.check(_lib.load().cpe_agv_chain_batch(angles.data_ptr(), angles.shape[0], A.data_ptr(), torch.cuda.current_stream().cuda_stream),
               'cpe_agv_chain_batch')
    return A


def estimate_frame_angles_gpu(pts3, cnt, cyl_raw, T, radius, pose_index=None, a0=None, **tol):
    """Build-defined (nothing like it in the reference): pan and tilt of every frame from a calibrated camera-AGV pose, the
    inverse of exp_gridDetection.m:90-93 (cpe_frame_angles_lm_batch, one wavefront per frame).  Nothing is read back and the
    launch is queued on the current stream; arguments given on the host (T, pose_index, a0 as lists or arrays) are made into
    tensors here and copied to the device.
    pts3 f64[n,MAXP,3] / cnt i32[n] / cyl_raw f64[n,2,6] as fit_cylinder_batch returns them (device tensors); cyl_raw may be
                 None when a0 is given
    T            the pose(s) T_Cam_AGV: 16 or G x 16 (or G x 4 x 4) row-major values, e.g. fit_multi_frame_gpu(...)['T']
    pose_index   None = every frame uses T[0]; i32[n]: the pose of every frame
    a0           None = the closed-form start from the frame's fitted axis cyl_raw[f,1,3:6] (assumes |pan| < pi/2; a missing
                 start never means zero: see include/cpe.h); f64[n,2] (pan, tilt) in rad, e.g. the nominal angles
    tol          tol_x, tol_f, max_iter (default 1e-5 / 1e-5 / 1e5)
    -> dict of device tensors: angles0, angles f64[n,2]; fvals f64[n,2] = [f(a0), f(a)]; iters i32[n,2] = [iterations,
       evaluations]; TAGV f64[n,16] getTAGVcyl at the result; Tcyl f64[n,16] = T * TAGV (exp_gridDetection.m:91); status i32[n]
       (0 = estimated; 5 = too few points / no usable start / not finite; 6 = pose_index out of range; every other output of
       such a frame is zero)"""
    L = _lib.load()
    dev, n = pts3.device, cnt.shape[0]
    pts3, cnt = pts3.contiguous(), cnt.contiguous()
    assert pts3.dtype == torch.float64 and cnt.dtype == torch.int32 and pts3.shape == (n, _lib.MAXP, 3)
    if cyl_raw is not None:
        cyl_raw = cyl_raw.contiguous()
        assert cyl_raw.dtype == torch.float64 and cyl_raw.shape == (n, 2, 6)
    T = torch.as_tensor(T, dtype=torch.float64).to(dev).reshape(-1, 16).contiguous()
    G = T.shape[0]
    if pose_index is not None:
        pose_index = torch.as_tensor(pose_index).to(device=dev, dtype=torch.int32).contiguous()
        assert pose_index.shape == (n,)
    if a0 is not None:
        a0 = torch.as_tensor(a0, dtype=torch.float64).to(dev).reshape(n, 2).contiguous()
    params = _tol_params(**tol)
    params.mode = _lib.const.FIT_LM
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    out = dict(angles0=f64(n, 2), angles=f64(n, 2), fvals=f64(n, 2), iters=torch.empty((n, 2), dtype=torch.int32, device=dev),
               TAGV=f64(n, 16), Tcyl=f64(n, 16), status=torch.empty(n, dtype=torch.int32, device=dev))
    _lib.check(L.cpe_frame_angles_lm_batch(pts3.data_ptr(), cnt.data_ptr(), cyl_raw.data_ptr() if cyl_raw is not None else None,
                                           T.data_ptr(), pose_index.data_ptr() if pose_index is not None else None, G, n,
                                           float(radius), ctypes.addressof(params), a0.data_ptr() if a0 is not None else None,
                                           out['angles0'].data_ptr(), out['angles'].data_ptr(), out['fvals'].data_ptr(),
                                           out['iters'].data_ptr(), out['TAGV'].data_ptr(), out['Tcyl'].data_ptr(),
                                           out['status'].data_ptr(), torch.cuda.current_stream().cuda_stream),
               'cpe_frame_angles_lm_batch')
    return out
