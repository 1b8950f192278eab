"""Host-side mirror of utils/fitSingleCylinder.m for a batch of stereo frames.

    [pts3, cylT, fvals, meanError] = fitSingleCylinder(i, gridPtsPair, cylRadius, ..., stereoParams, draw)

becomes fit_single_cylinder_batch(tables_left, tables_right, K1, K2, T_C2_C1, radius): all frames at
once, everything resident on the GPU, one wavefront per frame (csrc/fit.hip)."""
import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional

import torch

from . import lib as _lib

_c = _lib.const     # every constant below is the header's CPE_<name> (include/cpe.h), under the name callers know
MAXP = _c.MAXP
SEL_CHOOSE_IDX, SEL_THRESHOLD, SEL_JOIN = _c.SEL_CHOOSE_IDX, _c.SEL_THRESHOLD, _c.SEL_JOIN
FLAG_FALLBACK, FLAG_OVERFLOW = _c.FIT_FLAG_FALLBACK, _c.FIT_FLAG_OVERFLOW
ST_OK, ST_FEW_POINTS, ST_OVERFLOW = _c.ST_OK, _c.ST_FEW_POINTS, _c.ST_OVERFLOW      # the statuses of the fit
FIT_MIN_POINTS = _c.FIT_MIN_POINTS


@dataclass
class GridTables:
    """padded grid-point tables of n images: the reference's N x 4 [x y colIdx rowIdx] matrices"""
    xy: torch.Tensor    # f64 [n, MAXP, 2]
    id: torch.Tensor    # i32 [n, MAXP, 2]  (col, row)
    cnt: torch.Tensor   # i32 [n]

    @staticmethod
    def from_lists(mats, device):
        """mats: list of (N_i x 4) arrays [x y col row] (makePyGridPts.m:41)"""
        import numpy as np
        n = len(mats)
        xy = np.zeros((n, MAXP, 2)); ids = np.zeros((n, MAXP, 2), np.int32); cnt = np.zeros(n, np.int32)
        for i, m in enumerate(mats):
            m = np.asarray(m, dtype=np.float64).reshape(-1, 4)
            if len(m) > MAXP:
                raise ValueError(f'table {i} has {len(m)} points > MAXP={MAXP}')
            xy[i, :len(m)] = m[:, :2]; ids[i, :len(m)] = m[:, 2:4].astype(np.int32); cnt[i] = len(m)
        return GridTables(torch.from_numpy(xy).to(device), torch.from_numpy(ids).to(device),
                          torch.from_numpy(cnt).to(device))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev3(a, device, shape):
    t = torch.as_tensor(a, dtype=torch.float64).reshape(shape).contiguous()
    return t.to(device)


# ---- call plumbing shared by the wrappers below (none of it loads the library) ----

def _check_tables(what, gp, n=None, prefix='', dev=None):
    """the dtype / shape / device check of a GridTables: n images (default: as many as gp.cnt holds) on dev (default: gp.xy's)"""
    n = gp.cnt.shape[0] if n is None else n
    dev = gp.xy.device if dev is None else dev
    for name, t, dt, shape in (('xy', gp.xy, torch.float64, (n, MAXP, 2)), ('id', gp.id, torch.int32, (n, MAXP, 2)),
                               ('cnt', gp.cnt, torch.int32, (n,))):
        if t.dtype != dt or tuple(t.shape) != shape or t.device != dev:
            raise TypeError(f'{what}: {prefix}{name} must be {dt} {list(shape)} on {dev}, got {t.dtype} {list(t.shape)} on {t.device}')


def _line_count(what, lo, hi):
    """L = hi - lo + 1 grid-line indices, which must be 1..MAXL"""
    nl = int(hi) - int(lo) + 1
    if not 1 <= nl <= _lib.MAXL:
        raise ValueError(f'{what}: {nl} indices in [{lo}, {hi}], must be 1..{_lib.MAXL}')
    return nl


def _cameras(K1, K2, T21, dev):
    return _dev3(K1, dev, (9,)), _dev3(K2, dev, (9,)), _dev3(T21, dev, (16,))


def _table_on(table, dev, centre=False):
    """(P, status[, centre]) of a LaserTable as the kernels read them on dev"""
    out = (table.P.to(device=dev, dtype=torch.float64).contiguous(), table.status.to(device=dev, dtype=torch.int32).contiguous())
    return out + (table.centre.to(device=dev, dtype=torch.float64).contiguous(),) if centre else out


def _ptr(t):
    """the address the library gets: NULL for None and for a tensor without elements"""
    return None if t is None or t.numel() == 0 else t.data_ptr()


def _slab(dev, dtype, zero, n, fields):
    """one allocation (torch.zeros if zero, else torch.empty) carved into contiguous views that lie in the listed order, touch
    and fill it: fields = [(name, shape)], every view is [n, *shape] (n None: shape as it stands) -> dict name -> view"""
    shapes = [(() if n is None else (n,)) + tuple(shape) for _, shape in fields]
    sizes = [math.prod(s) for s in shapes]
    buf = (torch.zeros if zero else torch.empty)(sum(sizes), dtype=dtype, device=dev)
    return {name: t.view(s) for (name, _), s, t in zip(fields, shapes, buf.split(sizes))}


def select_triangulate_batch(gp1: GridTables, gp2: GridTables, K1, K2, T21, selector=SEL_CHOOSE_IDX, patch=3, th=0.3):
    """chooseIdx / triangulateWithThreshold / findGridCorrespondences + triangulate (fitSingleCylinder.m:10-17)"""
    L = _lib.load()
    dev = gp1.xy.device
    n = gp1.cnt.shape[0]
    K1, K2, T21 = _cameras(K1, K2, T21, dev)
    ws_bytes = L.cpe_fit_workspace_bytes(n)
    ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=dev)
    p1 = torch.zeros((n, MAXP, 2), dtype=torch.float64, device=dev); p2 = torch.zeros_like(p1)
    idx = torch.zeros((n, MAXP, 2), dtype=torch.int32, device=dev)
    X = torch.zeros((n, MAXP, 3), dtype=torch.float64, device=dev)
    err = torch.zeros((n, MAXP), dtype=torch.float64, device=dev)
    m = torch.zeros(n, dtype=torch.int32, device=dev); me = torch.zeros(n, dtype=torch.float64, device=dev)
    flags = torch.zeros(n, dtype=torch.int32, device=dev)
    _lib.check(L.cpe_select_triangulate_batch(gp1.xy.data_ptr(), gp1.id.data_ptr(), gp1.cnt.data_ptr(),
                                              gp2.xy.data_ptr(), gp2.id.data_ptr(), gp2.cnt.data_ptr(), n,
                                              K1.data_ptr(), K2.data_ptr(), T21.data_ptr(), selector, patch, th,
                                              ws.data_ptr(), ws_bytes, p1.data_ptr(), p2.data_ptr(), idx.data_ptr(),
                                              X.data_ptr(), err.data_ptr(), m.data_ptr(), me.data_ptr(),
                                              flags.data_ptr(), _stream()), 'cpe_select_triangulate_batch')
    return dict(p1=p1, p2=p2, idx=idx, pts3=X, err=err, m=m, mean_err=me, flags=flags, _ws=ws)


def choose_idx_batch(gp1: GridTables, gp2: GridTables, K1, K2, T21, patch=3, th=0.3):
    """[cgp1, cgp2] = chooseIdx(gp1, gp2, imgInfo, stereoParams, patch, th) (chooseIdx.m; fitSingleCylinder.m:12) for a batch:
    dict(p1, p2 f64[n,MAXP,2], idx i32[n,MAXP,2], m i32[n], flags i32[n])"""
    L = _lib.load()
    dev = gp1.xy.device
    n = gp1.cnt.shape[0]
    K1, K2, T21 = _cameras(K1, K2, T21, dev)
    ws_bytes = L.cpe_fit_workspace_bytes(n)
    ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=dev)
    p1 = torch.zeros((n, MAXP, 2), dtype=torch.float64, device=dev); p2 = torch.zeros_like(p1)
    idx = torch.zeros((n, MAXP, 2), dtype=torch.int32, device=dev)
    m = torch.zeros(n, dtype=torch.int32, device=dev); flags = torch.zeros(n, dtype=torch.int32, device=dev)
    _lib.check(L.cpe_choose_idx_batch(gp1.xy.data_ptr(), gp1.id.data_ptr(), gp1.cnt.data_ptr(), gp2.xy.data_ptr(), gp2.id.data_ptr(),
                                      gp2.cnt.data_ptr(), n, K1.data_ptr(), K2.data_ptr(), T21.data_ptr(), patch, th, ws.data_ptr(),
                                      ws_bytes, p1.data_ptr(), p2.data_ptr(), idx.data_ptr(), m.data_ptr(), flags.data_ptr(), _stream()),
               'cpe_choose_idx_batch')
    return dict(p1=p1, p2=p2, idx=idx, m=m, flags=flags, _ws=ws)


def triangulate_batch(p1, p2, cnt, K1, K2, T21):
    """[worldPoints, reprojectionErrors] = triangulate(cgp1, cgp2, stereoParams) + meanError (fitSingleCylinder.m:15-17):
    p1, p2 f64[n,MAXP,2], cnt i32[n] -> dict(pts3 f64[n,MAXP,3], err f64[n,MAXP], mean_err f64[n])"""
    L = _lib.load()
    dev = p1.device
    n = cnt.shape[0]
    K1, K2, T21 = _cameras(K1, K2, T21, dev)
    X = torch.zeros((n, MAXP, 3), dtype=torch.float64, device=dev)
    err = torch.zeros((n, MAXP), dtype=torch.float64, device=dev); me = torch.zeros(n, dtype=torch.float64, device=dev)
    _lib.check(L.cpe_triangulate_batch(p1.contiguous().data_ptr(), p2.contiguous().data_ptr(), cnt.data_ptr(), n, K1.data_ptr(),
                                       K2.data_ptr(), T21.data_ptr(), X.data_ptr(), err.data_ptr(), me.data_ptr(), _stream()),
               'cpe_triangulate_batch')
    return dict(pts3=X, err=err, mean_err=me)


FIT_NELDER_MEAD, FIT_LM = _c.FIT_NELDER_MEAD, _c.FIT_LM


def _fit_outputs(n, dev):
    """cyl_raw, cyl f64[n,2,6], T f64[n,4,4], fvals f64[n,2], iters i32[n,2], status i32[n]: zeroed, every one its own tensor"""
    z = lambda dt, *shape: torch.zeros((n,) + shape, dtype=dt, device=dev)
    return z(torch.float64, 2, 6), z(torch.float64, 2, 6), z(torch.float64, 4, 4), z(torch.float64, 2), z(torch.int32, 2), z(torch.int32)


def fit_cylinder_batch(pts3, cnt, radius, tol_x=1e-5, tol_f=1e-5, max_iter=100000, max_fun_evals=100000, mode=FIT_NELDER_MEAD):
    """fitCylinderWPts3 + applyCylParamsPrior + cylParams2T (fitSingleCylinder.m:20-25)"""
    L = _lib.load()
    dev = pts3.device
    n = cnt.shape[0]
    raw, cyl, T, fv, it, st = _fit_outputs(n, dev)
    prm = _lib.CpeFitParams(tol_x, tol_f, max_iter, max_fun_evals, mode, 0)
    _lib.check(L.cpe_fit_cylinder_batch(pts3.data_ptr(), cnt.data_ptr(), n, float(radius), C.addressof(prm),
                                        raw.data_ptr(), cyl.data_ptr(), T.data_ptr(), fv.data_ptr(), it.data_ptr(),
                                        st.data_ptr(), _stream()), 'cpe_fit_cylinder_batch')
    return dict(cyl_raw=raw, cyl=cyl, T=T, fvals=fv, iters=it, status=st)


def fit_cylinder_ransac_batch(pts3, cnt, radius, hypotheses=64, sample=12, tau=0.5, seed=0, frame0=0, hyp_iters=8, tol_x=1e-5,
                              tol_f=1e-5, max_iter=100000, max_fun_evals=100000, mode=FIT_LM):
    """BUILD-DEFINED (BASELINE config 5; the reference has no RANSAC): the fit wrapped in a consensus search, see
    include/cpe.h cpe_fit_cylinder_ransac_batch.  Extra outputs: n_inliers i32[n], inlier_mask u8[n,MAXP]."""
    L = _lib.load()
    dev = pts3.device
    n = cnt.shape[0]
    raw, cyl, T, fv, it, st = _fit_outputs(n, dev)
    ninl = torch.zeros(n, dtype=torch.int32, device=dev); mask = torch.zeros((n, _lib.MAXP), dtype=torch.uint8, device=dev)
    prm = _lib.CpeFitParams(tol_x, tol_f, max_iter, max_fun_evals, mode, 0)
    rp = _lib.CpeRansacParams(hypotheses, sample, tau, seed, frame0, hyp_iters, 0)
    _lib.check(L.cpe_fit_cylinder_ransac_batch(pts3.data_ptr(), cnt.data_ptr(), n, float(radius), C.addressof(prm), C.addressof(rp),
                                               raw.data_ptr(), cyl.data_ptr(), T.data_ptr(), fv.data_ptr(), it.data_ptr(),
                                               st.data_ptr(), ninl.data_ptr(), mask.data_ptr(), _stream()),
               'cpe_fit_cylinder_ransac_batch')
    return dict(cyl_raw=raw, cyl=cyl, T=T, fvals=fv, iters=it, status=st, n_inliers=ninl, inlier_mask=mask)


MATCH_MAX_WIN = _c.MATCH_MAX_WIN
MATCH_SHIFTED, MATCH_WEAK, MATCH_EDGE, MATCH_OVERFLOW = (_c.MATCH_FLAG_SHIFTED, _c.MATCH_FLAG_WEAK, _c.MATCH_FLAG_EDGE,
                                                         _c.MATCH_FLAG_OVERFLOW)


def match_offset_batch(gp1: GridTables, gp2: GridTables, K1, K2, T21, radius, win_c=4, win_r=4, th=0.3, tau=0.5, hyp_iters=8,
                       min_score=8, want_scores=True):
    """BUILD-DEFINED (the reference has nothing like it): the (dc, dr) to add to the (col,row) indices of table 1 so that the
    index join pairs the same grid points in both images, found by scoring every shift of the window with the fixed-radius
    cylinder; see include/cpe.h cpe_match_offset_batch.
    -> dict(offset i32[n,2], score i32[n,4] (best, runner-up, at (0,0), pairs kept at the winner), scores i32[n,ncand] (None
            without want_scores), flags i32[n] (MATCH_*), id1 i32[n,MAXP,2] = gp1.id + offset, tables = gp1 with that id)"""
    L = _lib.load()
    dev = gp1.xy.device
    n = gp1.cnt.shape[0]
    if not (0 <= win_c <= MATCH_MAX_WIN and 0 <= win_r <= MATCH_MAX_WIN):
        raise ValueError(f'match_offset_batch: window {win_c} x {win_r} outside 0..{MATCH_MAX_WIN}')
    K1, K2, T21 = _cameras(K1, K2, T21, dev)
    ncand = (2 * win_c + 1) * (2 * win_r + 1)
    ws_bytes = L.cpe_match_offset_workspace_bytes(n, win_c, win_r)
    ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=dev)
    offset = torch.zeros((n, 2), dtype=torch.int32, device=dev); score = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    scores = torch.zeros((n, ncand), dtype=torch.int32, device=dev) if want_scores else None
    flags = torch.zeros(n, dtype=torch.int32, device=dev); id1 = torch.zeros((n, MAXP, 2), dtype=torch.int32, device=dev)
    prm = _lib.CpeMatchParams(win_c, win_r, th, tau, hyp_iters, min_score)
    _lib.check(L.cpe_match_offset_batch(gp1.xy.data_ptr(), gp1.id.data_ptr(), gp1.cnt.data_ptr(), gp2.xy.data_ptr(), gp2.id.data_ptr(),
                                        gp2.cnt.data_ptr(), n, K1.data_ptr(), K2.data_ptr(), T21.data_ptr(), float(radius),
                                        C.addressof(prm), ws.data_ptr(), ws_bytes, offset.data_ptr(), score.data_ptr(),
                                        scores.data_ptr() if want_scores else None, flags.data_ptr(), id1.data_ptr(), _stream()),
               'cpe_match_offset_batch')
    return dict(offset=offset, score=score, scores=scores, flags=flags, id1=id1, tables=GridTables(gp1.xy, id1, gp1.cnt), _ws=ws)


def _fit_points(pts3, m, radius, ransac, overflow=None, **kw):
    """fit_cylinder_batch, or fit_cylinder_ransac_batch with the keywords of the dict `ransac`, on m points per frame.  overflow:
    the flags i32[n] of whatever made the points; a frame it skipped with FLAG_OVERFLOW because its indices do not fit the dense
    table has m = 0, and is reported as the ST_OVERFLOW it is"""
    fit = fit_cylinder_batch(pts3, m, radius, **kw) if ransac is None else fit_cylinder_ransac_batch(pts3, m, radius, **ransac, **kw)
    if overflow is not None:
        fit['status'].masked_fill_((overflow & FLAG_OVERFLOW) != 0, ST_OVERFLOW)
    return fit


def fit_single_cylinder_batch(gp1: GridTables, gp2: GridTables, K1, K2, T21, radius, selector=SEL_CHOOSE_IDX,
                              patch=3, th=0.3, ransac=None, match=None, **fit_kw):
    """[pts3, cylT, fvals, meanError] = fitSingleCylinder(...) for every frame of the batch.
    status: the fit's (ST_OK / ST_FEW_POINTS), or ST_OVERFLOW where the selector set FLAG_OVERFLOW (all outputs zero).
    ransac: None (reference behaviour) or a dict of fit_cylinder_ransac_batch keywords (build-defined config 5).
    match: None (reference behaviour: equal indices are the same grid point) or a dict of match_offset_batch keywords
    (build-defined; {} = its defaults): the index shift between the two tables is searched first, and the selector and the fit
    get table 1 with the shift applied (`idx` is then in the numbering of image 2).  The result always holds offset i32[n,2],
    match_score i32[n,4] and match_flags i32[n]; all zeros when the search is off."""
    n, dev = gp1.cnt.shape[0], gp1.xy.device
    if match is not None:
        mo = match_offset_batch(gp1, gp2, K1, K2, T21, radius, **dict(match, want_scores=False))
        gp1 = mo['tables']
        extra = dict(offset=mo['offset'], match_score=mo['score'], match_flags=mo['flags'], _match_ws=mo['_ws'])
    else:
        z = torch.zeros((n, 7), dtype=torch.int32, device=dev)       # (one fill: this is the path of every call without the search)
        extra = dict(offset=z[:, 0:2], match_score=z[:, 2:6], match_flags=z[:, 6])
    sel = select_triangulate_batch(gp1, gp2, K1, K2, T21, selector, patch, th)
    return dict(sel, **_fit_points(sel['pts3'], sel['m'], radius, ransac, sel['flags'], **fit_kw), **extra)


CURV_REFERENCE, CURV_INTERCEPT, CURV_MAXK = _c.CURV_REFERENCE, _c.CURV_INTERCEPT, _c.CURV_MAXK
_CURV_UNKNOWNS = {CURV_REFERENCE: 5, CURV_INTERCEPT: 6}
_CURV_FIELDS = (('Kdir', torch.float64, (MAXP, 2, 3)), ('L', torch.float64, (MAXP, 2)), ('normal', torch.float64, (MAXP, 3)),
                ('pt_status', torch.uint8, (MAXP,)))


def _check_points(what, pts3, cnt):
    """the dtype / shape / device check of a point table: pts3 f64[n,MAXP,3] and cnt i32[n] on one device -> n"""
    if not isinstance(cnt, torch.Tensor) or cnt.dim() != 1:
        raise TypeError(f'{what}: cnt must be a torch.int32 tensor [n]')
    n, dev = cnt.shape[0], pts3.device
    for name, t, dt, shape in (('pts3', pts3, torch.float64, (n, MAXP, 3)), ('cnt', cnt, torch.int32, (n,))):
        if t.dtype != dt or tuple(t.shape) != shape or t.device != dev:
            raise TypeError(f'{what}: {name} must be {dt} {list(shape)} on {dev}, got {t.dtype} {list(t.shape)} on {t.device}')
    return n


def _check_curv_args(what, k, mode):
    if mode not in _CURV_UNKNOWNS:
        raise ValueError(f'{what}: mode {mode} must be CURV_REFERENCE ({CURV_REFERENCE}) or CURV_INTERCEPT ({CURV_INTERCEPT})')
    if int(k) != k or not _CURV_UNKNOWNS[mode] <= k <= CURV_MAXK:
        raise ValueError(f'{what}: k {k} must be {_CURV_UNKNOWNS[mode]}..{CURV_MAXK} in mode {mode}')


def est_curvatures_batch(pts3, cnt, k=_c.CURV_K, mode=CURV_REFERENCE, want_neighbours=False):
    """[K, L] = estCurvatures(Pts3) for every point of every frame, see include/cpe.h cpe_est_curvatures_batch.  pts3
    f64[n,MAXP,3], cnt i32[n] as select_triangulate_batch returns them; mode CURV_REFERENCE (the reference's arithmetic) or
    CURV_INTERCEPT (build-defined: unit frame, quadric with a constant term).
    -> dict(Kdir f64[n,MAXP,2,3], L f64[n,MAXP,2] (ascending), normal f64[n,MAXP,3], nbr i32[n,MAXP,k] (None without
            want_neighbours), pt_status u8[n,MAXP], status i32[n], k, mode)"""
    n = _check_points('est_curvatures_batch', pts3, cnt)
    _check_curv_args('est_curvatures_batch', k, mode)
    L = _lib.load()
    dev = pts3.device
    pts3, cnt = pts3.contiguous(), cnt.contiguous()
    # (the kernel writes every slot of every output: no fills)
    Kd, Lm, nrm = _slab(dev, torch.float64, False, n, [(name, shape) for name, dt, shape in _CURV_FIELDS if dt == torch.float64]).values()
    pt = torch.empty((n, MAXP), dtype=torch.uint8, device=dev)
    st = torch.empty(n, dtype=torch.int32, device=dev)
    nbr = torch.empty((n, MAXP, int(k)), dtype=torch.int32, device=dev) if want_neighbours else None
    _lib.check(L.cpe_est_curvatures_batch(_ptr(pts3), _ptr(cnt), n, int(k), int(mode), _ptr(Kd), _ptr(Lm), _ptr(nrm), _ptr(nbr), _ptr(pt),
                                          _ptr(st), _stream()), 'cpe_est_curvatures_batch')
    return dict(Kdir=Kd, L=Lm, normal=nrm, nbr=nbr, pt_status=pt, status=st, k=int(k), mode=int(mode))


def curvature_consensus_batch(pts3, cnt, curv, rho_max=0.25, r_min=0.0, r_max=math.inf):
    """BUILD-DEFINED: what a frame's curvatures say together, see include/cpe.h cpe_curvature_consensus_batch.  curv: the dict of
    est_curvatures_batch on the same pts3 and cnt.  A point is gated in when its |lambda|min / |lambda|max <= rho_max and
    r_min < 1 / |lambda|max < r_max.
    -> dict(axis f64[n,8] (origin, direction, radius = lower median of 1 / |lambda|max, spread = rms distance of the centres of
            curvature from the axis), n_gated i32[n], gate u8[n,MAXP], status i32[n] (ST_FEW_POINTS: fewer than 3 gated))"""
    what = 'curvature_consensus_batch'
    n = _check_points(what, pts3, cnt)
    dev = pts3.device
    for name, dt, shape in _CURV_FIELDS:
        t = curv[name]
        if t.dtype != dt or tuple(t.shape) != (n,) + shape or t.device != dev:
            raise TypeError(f'{what}: curv[{name!r}] must be {dt} {[n] + list(shape)} on {dev}, got {t.dtype} {list(t.shape)} on {t.device}')
    rho_max, r_min, r_max = float(rho_max), float(r_min), float(r_max)
    if not (rho_max >= 0 and r_min >= 0 and r_max > r_min):
        raise ValueError(f'{what}: rho_max {rho_max} must be >= 0 and 0 <= r_min {r_min} < r_max {r_max}')
    L = _lib.load()
    c = lambda t: t.contiguous()
    axis = torch.empty((n, 8), dtype=torch.float64, device=dev)
    ng, st = _slab(dev, torch.int32, False, None, [('n_gated', (n,)), ('status', (n,))]).values()
    gate = torch.empty((n, MAXP), dtype=torch.uint8, device=dev)
    Kd, Lm, nrm, pt = (c(curv[name]) for name, _, _ in _CURV_FIELDS)
    _lib.check(L.cpe_curvature_consensus_batch(_ptr(c(pts3)), _ptr(c(cnt)), n, _ptr(Kd), _ptr(Lm), _ptr(nrm), _ptr(pt), rho_max, r_min, r_max,
                                               _ptr(axis), _ptr(ng), _ptr(gate), _ptr(st), _stream()), 'cpe_curvature_consensus_batch')
    return dict(axis=axis, n_gated=ng, gate=gate, status=st)


def _curvature_options(what, curvature, radius):
    """(k, mode, rho_max, r_min, r_max) of a `curvature` dict: mode CURV_INTERCEPT, k 20, rho_max 0.25 and the band
    radius (1 -/+ band), band = 1/3, unless the dict says otherwise (radius None: no band, r_min 0 and r_max inf)"""
    o = dict(curvature or {})
    k, mode, rho_max, band = o.pop('k', 20), o.pop('mode', CURV_INTERCEPT), o.pop('rho_max', 0.25), o.pop('band', 1.0 / 3.0)
    r_min = o.pop('r_min', 0.0 if radius is None else radius * (1.0 - band))
    r_max = o.pop('r_max', math.inf if radius is None else radius * (1.0 + band))
    if o:
        raise ValueError(f'{what}: unknown curvature options {sorted(o)}')
    _check_curv_args(what, k, mode)
    return k, mode, rho_max, r_min, r_max


def compact_gated(pts3, gate):
    """the gated points of every frame moved to the front in table order (torch only, no host synchronisation):
    pts3 f64[n,MAXP,3], gate u8[n,MAXP] -> (f64[n,MAXP,3] with zeros behind the kept points, i32[n] how many were kept)"""
    keep = gate != 0
    n, P = keep.shape
    at = torch.cumsum(keep, 1) - 1                                          # a kept point's place: the kept points before it
    at = torch.where(keep, at, torch.full_like(at, P))                      # everything else goes to one spare slot behind the table
    out = torch.zeros((n, P + 1, 3), dtype=pts3.dtype, device=pts3.device)
    out.scatter_(1, at[:, :, None].expand(-1, -1, 3), pts3)
    return out[:, :P].contiguous(), keep.sum(1, dtype=torch.int32)


def fit_single_cylinder_gated_batch(gp1: GridTables, gp2: GridTables, K1, K2, T21, radius, curvature=None, selector=SEL_CHOOSE_IDX,
                                    patch=3, th=0.3, ransac=None, **fit_kw):
    """BUILD-DEFINED, fit_single_cylinder_batch behind the curvature gate: select_triangulate_batch, est_curvatures_batch and
    curvature_consensus_batch on its points, then the fit on the gated points alone (compacted in table order on the device).
    curvature: None or a dict of k, mode (default CURV_INTERCEPT), rho_max, band (default 1/3: r_min, r_max = radius (1 -/+
    band)), r_min, r_max.  -> everything fit_single_cylinder_batch returns (pts3 and m are the selector's, before the gate)
    beside gate u8[n,MAXP], n_gated i32[n], curv_axis f64[n,8], curv_status i32[n], pts3_gated f64[n,MAXP,3].  A frame that keeps
    fewer than FIT_MIN_POINTS points ends in ST_FEW_POINTS like any other."""
    k, mode, rho_max, r_min, r_max = _curvature_options('fit_single_cylinder_gated_batch', curvature, float(radius))
    n, dev = gp1.cnt.shape[0], gp1.xy.device
    sel = select_triangulate_batch(gp1, gp2, K1, K2, T21, selector, patch, th)
    curv = est_curvatures_batch(sel['pts3'], sel['m'], k=k, mode=mode)
    con = curvature_consensus_batch(sel['pts3'], sel['m'], curv, rho_max=rho_max, r_min=r_min, r_max=r_max)
    kept, m = compact_gated(sel['pts3'], con['gate'])
    z = torch.zeros((n, 7), dtype=torch.int32, device=dev)
    return dict(sel, **_fit_points(kept, m, radius, ransac, sel['flags'], **fit_kw), offset=z[:, 0:2], match_score=z[:, 2:6],
                match_flags=z[:, 6], gate=con['gate'], n_gated=con['n_gated'], curv_axis=con['axis'], curv_status=con['status'],
                pts3_gated=kept)


PLANE_NO_GRID, PLANE_ORIGIN_POINT = _c.PLANEFIT_NO_GRID, _c.PLANEFIT_ORIGIN_POINT


def _point_tables(what, pts3, idx, cnt, use=None):
    """the tables as the kernels read them: contiguous f64[n,MAXP,3], i32[n,MAXP,2], i32[n], u8[n,MAXP] on one device"""
    n = cnt.shape[0]
    for name, t, dt, shape in (('pts3', pts3, torch.float64, (n, MAXP, 3)), ('idx', idx, torch.int32, (n, MAXP, 2)),
                               ('cnt', cnt, torch.int32, (n,)), ('use', use, torch.uint8, (n, MAXP))):
        if t is None:
            continue
        if t.dtype != dt or tuple(t.shape) != shape or t.device != pts3.device:
            raise TypeError(f'{what}: {name} must be {dt} {list(shape)} on {pts3.device}, got {t.dtype} {list(t.shape)} on {t.device}')
    c = lambda t: None if t is None else t.contiguous()
    return c(pts3), c(idx), c(cnt), c(use)


def fit_plane_batch(pts3, idx, cnt, tau=0.0, max_rounds=4):
    """BUILD-DEFINED, the planar target's fit (fitplane.m with an optional trimming loop, the grid map, the board pose), see
    include/cpe.h cpe_fit_plane_batch.  pts3 f64[n,MAXP,3], idx i32[n,MAXP,2], cnt i32[n] as select_triangulate_batch returns them
    -> dict(P f64[n,4], T f64[n,4,4], grid f64[n,3,3] (O, U, V), stats f64[n,8] (plane rms, max |r|, 3 eigenvalues, grid rms,
            refits, 0), n_inliers i32[n], inlier_mask u8[n,MAXP], plane_flags i32[n] (PLANE_*), status i32[n])"""
    L = _lib.load()
    pts3, idx, cnt, _ = _point_tables('fit_plane_batch', pts3, idx, cnt)
    dev = pts3.device
    n = cnt.shape[0]
    # (the kernel writes every slot of every output: no fills)
    P, T, grid, stats = _slab(dev, torch.float64, False, n, [('P', (4,)), ('T', (4, 4)), ('grid', (3, 3)), ('stats', (8,))]).values()
    ninl, flags, st = _slab(dev, torch.int32, False, None, [('n_inliers', (n,)), ('plane_flags', (n,)), ('status', (n,))]).values()
    mask = torch.empty((n, MAXP), dtype=torch.uint8, device=dev)
    prm = _lib.CpePlaneFitParams(float(tau), int(max_rounds), 0)
    _lib.check(L.cpe_fit_plane_batch(pts3.data_ptr(), idx.data_ptr(), cnt.data_ptr(), n, C.addressof(prm), P.data_ptr(), T.data_ptr(),
                                     grid.data_ptr(), stats.data_ptr(), ninl.data_ptr(), mask.data_ptr(), flags.data_ptr(),
                                     st.data_ptr(), _stream()), 'cpe_fit_plane_batch')
    return dict(P=P, T=T, grid=grid, stats=stats, n_inliers=ninl, inlier_mask=mask, plane_flags=flags, status=st)


def index_planes_batch(pts3, idx, cnt, lo, hi, use=None, frame_ok=None, min_spread=1e-4):
    """BUILD-DEFINED: the plane of light of every grid-line index lo..hi of both index components over the frames of the batch
    (several board poses), and the point nearest to all of them: the projector's centre.  See include/cpe.h
    cpe_index_planes_batch.  use u8[n,MAXP] (e.g. fit_plane_batch's inlier_mask) and frame_ok i32[n] are optional.
    -> dict(P f64[2,L,4], stats f64[2,L,4] (rms, max |r|, lambda_mid / lambda_max, 0), count, frames, status i32[2,L],
            centre f64[4] (C, rms), centre_status i32[1], lo, hi)"""
    L = _lib.load()
    pts3, idx, cnt, use = _point_tables('index_planes_batch', pts3, idx, cnt, use)
    dev = pts3.device
    n = cnt.shape[0]
    nl = _line_count('index_planes_batch', lo, hi)
    if frame_ok is not None:
        if frame_ok.shape != (n,) or frame_ok.device != dev:
            raise TypeError(f'index_planes_batch: frame_ok must hold {n} values on {dev}')
        frame_ok = frame_ok.to(torch.int32).contiguous()
    # (the kernels write every slot of every output: no fills)
    P, stats, centre = _slab(dev, torch.float64, False, None, [('P', (2, nl, 4)), ('stats', (2, nl, 4)), ('centre', (4,))]).values()
    count, frames, st, cst = _slab(dev, torch.int32, False, None, [('count', (2, nl)), ('frames', (2, nl)), ('status', (2, nl)),
                                                                   ('centre_status', (1,))]).values()
    _lib.check(L.cpe_index_planes_batch(pts3.data_ptr(), idx.data_ptr(), cnt.data_ptr(), n, None if use is None else use.data_ptr(),
                                        None if frame_ok is None else frame_ok.data_ptr(), int(lo), int(hi), float(min_spread),
                                        P.data_ptr(), stats.data_ptr(), count.data_ptr(), frames.data_ptr(), st.data_ptr(),
                                        centre.data_ptr(), cst.data_ptr(), _stream()), 'cpe_index_planes_batch')
    return dict(P=P, stats=stats, count=count, frames=frames, status=st, centre=centre, centre_status=cst, lo=int(lo), hi=int(hi))


# (RELABEL_FEW_LINES << c for id component c)
RELABEL_NO_CENTRE, RELABEL_OVERFLOW, RELABEL_FEW_LINES = _c.RELABEL_FLAG_NO_CENTRE, _c.RELABEL_FLAG_OVERFLOW, _c.RELABEL_FLAG_FEW_LINES
LINE_KEPT, LINE_UNSUPPORTED, LINE_PHANTOM = _c.RELABEL_LINE_KEPT, _c.RELABEL_LINE_UNSUPPORTED, _c.RELABEL_LINE_PHANTOM


def grid_relabel_batch(tables: GridTables, center, swap=0, min_pts=3, merge_frac=0.65, dir=(1, 1)):
    """BUILD-DEFINED: the planar detector's tables with their grid lines re-labelled from the geometry, per image -- the labels'
    grouping is kept, their values are replaced by the lines' order across the centre stepped by the measured pitch, phantom
    lines and their points are dropped.  See include/cpe.h cpe_grid_relabel_batch.  center f64[n,2] (x, y) as
    api.detect_grid_batch returns it; swap 0: id component 0 is positioned in y (the planar detector's (row, col)).
    -> dict(tables (GridTables, compacted; slots from cnt on hold zeros), src i32[n,MAXP] (the slot every written slot came
            from), lines dict(label, index, points, state i32[n,2,MAXL], p f64[n,2,MAXL]; per line slot = the labels seen,
            ascending; zeros from counts[..., 0] on), pitch f64[n,2], counts i32[n,2,4] (labels seen, supported, phantoms, kept),
            flags i32[n] (RELABEL_*))"""
    L = _lib.load()
    n = tables.cnt.shape[0]
    dev = tables.xy.device
    _check_tables('grid_relabel_batch', tables)
    if center.dtype != torch.float64 or tuple(center.shape) != (n, 2) or center.device != dev:
        raise TypeError(f'grid_relabel_batch: center must be torch.float64 [{n}, 2] on {dev}, got {center.dtype} {list(center.shape)} '
                        f'on {center.device}')
    dir = tuple(int(d) for d in dir)
    if len(dir) != 2 or not all(d in (1, -1) for d in dir):
        raise ValueError(f'grid_relabel_batch: dir {dir} must be two of +1, -1')
    if int(swap) not in (0, 1) or int(min_pts) < 2 or not 0.0 < float(merge_frac) < 1.0:
        raise ValueError(f'grid_relabel_batch: swap {swap} must be 0 or 1, min_pts {min_pts} >= 2, merge_frac {merge_frac} in (0, 1)')
    xy, ids, cnt, center = tables.xy.contiguous(), tables.id.contiguous(), tables.cnt.contiguous(), center.contiguous()
    ML = _lib.MAXL
    xy_o = torch.zeros((n, MAXP, 2), dtype=torch.float64, device=dev)
    id_o, src, lines, counts, cnt_o, flags = _slab(dev, torch.int32, True, n, [('id', (MAXP, 2)), ('src', (MAXP,)), ('lines', (2, ML, 4)),
                                                                               ('counts', (2, 4)), ('cnt', ()), ('flags', ())]).values()
    line_p, pitch = _slab(dev, torch.float64, True, n, [('p', (2, ML)), ('pitch', (2,))]).values()
    prm = _lib.CpeRelabelParams(int(swap), int(min_pts), float(merge_frac), (C.c_int32 * 2)(*dir))
    _lib.check(L.cpe_grid_relabel_batch(xy.data_ptr(), ids.data_ptr(), cnt.data_ptr(), center.data_ptr(), n, C.addressof(prm),
                                        xy_o.data_ptr(), id_o.data_ptr(), cnt_o.data_ptr(), src.data_ptr(), lines.data_ptr(),
                                        line_p.data_ptr(), pitch.data_ptr(), counts.data_ptr(), flags.data_ptr(), _stream()),
               'cpe_grid_relabel_batch')
    return dict(tables=GridTables(xy_o, id_o, cnt_o), src=src,
                lines=dict(label=lines[..., 0], index=lines[..., 1], points=lines[..., 2], state=lines[..., 3], p=line_p),
                pitch=pitch, counts=counts, flags=flags)


def _cat_tables(g1: GridTables, g2: GridTables):
    return GridTables(torch.cat([g1.xy, g2.xy]), torch.cat([g1.id, g2.id]), torch.cat([g1.cnt, g2.cnt]))


def fit_single_plane_batch(gp1: GridTables, gp2: GridTables, K1, K2, T21, selector=SEL_CHOOSE_IDX, patch=3, th=0.3, tau=0.0,
                           max_rounds=4, relabel=None, center1=None, center2=None):
    """the planar counterpart of fit_single_cylinder_batch: select_triangulate_batch, then fit_plane_batch on its points and
    indices.  Returns the selector's outputs beside the fit's; status is the fit's, or ST_OVERFLOW where the selector set
    FLAG_OVERFLOW (such a frame has m = 0, so all its fit outputs are zero).
    relabel (BUILD-DEFINED): None, or a dict of grid_relabel_batch keywords ({} = its defaults): both images' tables are
    re-labelled in one call (center1, center2 f64[n,2]: the two images' centres as the detect call returns them) before the
    selector reads them; the result gains relabel_counts i32[n,2,2,4] and relabel_flags i32[n,2] (frame, image, ...)."""
    rl = None
    if relabel is not None:
        if center1 is None or center2 is None:
            raise ValueError('fit_single_plane_batch: relabel needs center1 and center2, the centres of both images')
        n = gp1.cnt.shape[0]
        rl = grid_relabel_batch(_cat_tables(gp1, gp2), torch.cat([center1, center2]), **relabel)
        t = rl['tables']
        gp1, gp2 = GridTables(t.xy[:n], t.id[:n], t.cnt[:n]), GridTables(t.xy[n:], t.id[n:], t.cnt[n:])
    sel = select_triangulate_batch(gp1, gp2, K1, K2, T21, selector, patch, th)
    fit = fit_plane_batch(sel['pts3'], sel['idx'], sel['m'], tau=tau, max_rounds=max_rounds)
    fit['status'].masked_fill_((sel['flags'] & FLAG_OVERFLOW) != 0, ST_OVERFLOW)
    out = dict(sel)
    out.update(fit)
    if rl is not None:
        n = gp1.cnt.shape[0]
        out['relabel_counts'] = torch.stack([rl['counts'][:n], rl['counts'][n:]], 1)
        out['relabel_flags'] = torch.stack([rl['flags'][:n], rl['flags'][n:]], 1)
    return out


@dataclass
class LaserTable:
    """BUILD-DEFINED: the laser-plane table of a calibrated projector, what index_planes_batch fits over several board poses.
    P f64[2,L,4] (unit normal, offset; camera-1 coordinates), status i32[2,L] (ST_OK = the line has a plane), lo, hi (the grid
    indices the L = hi - lo + 1 lines stand for), centre f64[4] (the projector's centre, rms), centre_status i32[1], and
    family0: which grid index family 0 of the table holds, 'col' or 'row'.  The planar detector writes its ids as (row, col),
    so a table from boards has family0 = 'row'; the cylinder's detector writes (col, row) (GridTables.id)."""
    P: torch.Tensor
    status: torch.Tensor
    lo: int
    hi: int
    centre: torch.Tensor
    centre_status: torch.Tensor
    family0: str = 'col'
    # centre_status == ST_OK as a host value, for the calls that need the centre (grid_predict_batch): set by whoever knows it
    # without asking the device (load does; to carries it on); None = not known yet, read from the device once by has_centre()
    centre_ok: Optional[bool] = None

    def has_centre(self):
        """is centre_status ST_OK?  Answered from centre_ok; while that is None the word is read from the device (one wait) and
        kept.  Whoever rewrites centre_status in place sets centre_ok (or None) with it."""
        if self.centre_ok is None:
            self.centre_ok = bool((self.centre_status.reshape(-1)[:1] == ST_OK).all().item())
        return self.centre_ok

    def __post_init__(self):
        if self.family0 not in ('col', 'row'):
            raise ValueError("LaserTable.family0 is 'col' or 'row'")
        self.lo, self.hi = int(self.lo), int(self.hi)
        nl = _line_count('LaserTable', self.lo, self.hi)
        if tuple(self.P.shape) != (2, nl, 4) or tuple(self.status.shape) != (2, nl):
            raise ValueError(f'LaserTable: P must be [2,{nl},4] and status [2,{nl}], got {list(self.P.shape)} and {list(self.status.shape)}')

    @staticmethod
    def from_index_planes(out, lo=None, hi=None, family0='col'):
        """out: the dict of index_planes_batch (lo, hi default to the ones it holds)"""
        return LaserTable(out['P'], out['status'], out['lo'] if lo is None else lo, out['hi'] if hi is None else hi, out['centre'],
                          out['centre_status'], family0)

    def swap_for(self, ids='col_row'):
        """CpeTableTriParams.swap for tables whose id is (col, row) ('col_row', GridTables) or (row, col) ('row_col')"""
        if ids not in ('col_row', 'row_col'):
            raise ValueError("ids is 'col_row' or 'row_col'")
        return int((self.family0 == 'col') != (ids == 'col_row'))

    def to(self, device):
        return LaserTable(self.P.to(device), self.status.to(device), self.lo, self.hi, self.centre.to(device),
                          self.centre_status.to(device), self.family0, self.centre_ok)

    def save(self, path):
        """one .npz file (numpy appends the suffix to a path without it)"""
        import numpy as np
        np.savez(path, P=self.P.cpu().numpy(), status=self.status.cpu().numpy(), lo=np.int64(self.lo), hi=np.int64(self.hi),
                 centre=self.centre.cpu().numpy(), centre_status=self.centre_status.cpu().numpy(), family0=np.array(self.family0))

    @staticmethod
    def load(path, device='cpu'):
        import numpy as np
        with np.load(path, allow_pickle=False) as z:
            t = lambda k, dt: torch.from_numpy(np.ascontiguousarray(z[k])).to(dt).to(device)
            return LaserTable(t('P', torch.float64), t('status', torch.int32), int(z['lo']), int(z['hi']), t('centre', torch.float64),
                              t('centre_status', torch.int32), str(z['family0']), bool((np.asarray(z['centre_status']).reshape(-1)[:1] == ST_OK).all()))


def fit_projector_model(pts3, idx, cnt, lo, hi, use=None, frame_ok=None, tau=0.0, max_rounds=4, min_spread=1e-4, tolx=1e-9, tolf=1e-9,
                        maxiter=100, x0=None):
    """BUILD-DEFINED: the projector as two pencils of planes n = a_k + v b_k through one centre C, fitted to the points and
    indices of many frames (board poses, or the cylinder experiment's own stereo points), with an optional trimming band tau
    that drops the residuals of mis-numbered frames.  See include/cpe.h cpe_fit_projector_model.  Inputs as index_planes_batch;
    x0 f64[15] is an optional start.
    -> dict(model f64[16] (C, a_0, b_0, a_1, b_1, objective), info i32[8] (status, refits, LM iterations, evaluations, kept
            residuals per family, 0, 0), moments f64[2,L,12], count, frames i32[2,L], inlier_mask u8[2,n,MAXP],
            frame_counts i32[n,4] (kept, trimmed of family 0; kept, trimmed of family 1), lo, hi)"""
    L = _lib.load()
    pts3, idx, cnt, use = _point_tables('fit_projector_model', pts3, idx, cnt, use)
    dev = pts3.device
    n = cnt.shape[0]
    nl = _line_count('fit_projector_model', lo, hi)
    if frame_ok is not None:
        if frame_ok.shape != (n,) or frame_ok.device != dev:
            raise TypeError(f'fit_projector_model: frame_ok must hold {n} values on {dev}')
        frame_ok = frame_ok.to(torch.int32).contiguous()
    if x0 is not None:
        x0 = _dev3(x0, dev, (15,))
    # (the kernels write every slot of every output, the mask after the call's own fill: no fills here)
    model, moments = _slab(dev, torch.float64, False, None, [('model', (16,)), ('moments', (2, nl, 12))]).values()
    info, count, frames, fc = _slab(dev, torch.int32, False, None, [('info', (8,)), ('count', (2, nl)), ('frames', (2, nl)),
                                                                    ('frame_counts', (n, 4))]).values()
    mask = torch.empty((2, n, MAXP), dtype=torch.uint8, device=dev)
    prm = _lib.CpeProjectorModelParams(float(tau), int(max_rounds), int(maxiter), float(min_spread), float(tolx), float(tolf))
    _lib.check(L.cpe_fit_projector_model(_ptr(pts3), _ptr(idx), _ptr(cnt), n, _ptr(use), _ptr(frame_ok), int(lo), int(hi), C.addressof(prm),
                                         _ptr(x0), model.data_ptr(), info.data_ptr(), moments.data_ptr(), count.data_ptr(),
                                         frames.data_ptr(), _ptr(mask), _ptr(fc), _stream()), 'cpe_fit_projector_model')
    return dict(model=model, info=info, moments=moments, count=count, frames=frames, inlier_mask=mask, frame_counts=fc, lo=int(lo),
                hi=int(hi))


@dataclass
class ProjectorModel:
    """BUILD-DEFINED: a fitted projector (fit_projector_model).  C f64[3] the centre, a, b f64[2,3]: the plane of index v of
    family k has the normal a[k] + v b[k] and holds C (camera-1 coordinates); rms: sqrt of the mean squared residual of the fit;
    family0 as LaserTable's; model f64[16] and info i32[8] are the call's own outputs, which table() reads."""
    model: torch.Tensor
    info: torch.Tensor
    family0: str = 'col'

    def __post_init__(self):
        if self.family0 not in ('col', 'row'):
            raise ValueError("ProjectorModel.family0 is 'col' or 'row'")
        if tuple(self.model.shape) != (16,) or tuple(self.info.shape) != (8,):
            raise ValueError(f'ProjectorModel: model must be [16] and info [8], got {list(self.model.shape)} and {list(self.info.shape)}')

    @staticmethod
    def from_fit(out, family0='col'):
        """out: the dict of fit_projector_model"""
        return ProjectorModel(out['model'], out['info'], family0)

    @property
    def status(self):
        return int(self.info[0])

    @property
    def C(self):
        return self.model[:3]

    @property
    def a(self):
        return self.model[3:15].view(2, 2, 3)[:, 0]

    @property
    def b(self):
        return self.model[3:15].view(2, 2, 3)[:, 1]

    @property
    def rms(self):
        kept = int(self.info[4]) + int(self.info[5])
        return float(self.model[15].clamp(min=0) / kept) ** 0.5 if kept > 0 else 0.0

    def table(self, lo, hi):
        """the laser-plane table of the indices lo..hi, any range of at most MAXL: also indices no frame showed"""
        L = _lib.load()
        nl = _line_count('ProjectorModel.table', lo, hi)
        dev = self.model.device
        model, info = self.model.to(torch.float64).contiguous(), self.info.to(device=dev, dtype=torch.int32).contiguous()
        P, centre = _slab(dev, torch.float64, False, None, [('P', (2, nl, 4)), ('centre', (4,))]).values()
        st, cst = _slab(dev, torch.int32, False, None, [('status', (2, nl)), ('centre_status', (1,))]).values()
        _lib.check(L.cpe_projector_model_table(model.data_ptr(), info.data_ptr(), int(lo), int(hi), P.data_ptr(), st.data_ptr(),
                                               centre.data_ptr(), cst.data_ptr(), _stream()), 'cpe_projector_model_table')
        return LaserTable(P, st, lo, hi, centre, cst, self.family0)

    def to(self, device):
        return ProjectorModel(self.model.to(device), self.info.to(device), self.family0)

    def save(self, path):
        """one .npz file (numpy appends the suffix to a path without it)"""
        import numpy as np
        np.savez(path, model=self.model.cpu().numpy(), info=self.info.cpu().numpy(), family0=np.array(self.family0))

    @staticmethod
    def load(path, device='cpu'):
        import numpy as np
        with np.load(path, allow_pickle=False) as z:
            return ProjectorModel(torch.from_numpy(np.ascontiguousarray(z['model'])).to(torch.float64).to(device),
                                  torch.from_numpy(np.ascontiguousarray(z['info'])).to(torch.int32).to(device), str(z['family0']))


def table_triangulate_batch(gp: GridTables, K, Tc, table: LaserTable, need_both=False, min_sin=0.01, max_res=0.0, ids='col_row'):
    """BUILD-DEFINED: 3-D points of one camera's grid tables from the laser-plane table, see include/cpe.h
    cpe_table_triangulate_batch.  K: that camera's intrinsics; Tc: camera-1 coordinates -> that camera's (None = camera 1, T21
    for camera 2).  gp.id is (col, row) as GridTables says (ids='row_col' for the planar detector's tables); which family of
    the table either component addresses follows from table.family0.
    -> dict(pts3 f64[n,MAXP,3], idx i32[n,MAXP,2], res f64[n,MAXP,2] (mm off either plane), src i32[n,MAXP,2] (planes used as
            bits, source slot), m i32[n], counts i32[n,4] (m, with both planes, refused before / after the cut), stats f64[n,2]
            (rms and max |res|)); slots from m on hold zeros"""
    L = _lib.load()
    dev = gp.xy.device
    n = gp.cnt.shape[0]
    _check_tables('table_triangulate_batch', gp)
    K = _dev3(K, dev, (9,))
    Tc = None if Tc is None else _dev3(Tc, dev, (16,))
    P, st = _table_on(table, dev)
    X, res, stats = _slab(dev, torch.float64, True, n, [('pts3', (MAXP, 3)), ('res', (MAXP, 2)), ('stats', (2,))]).values()
    idx, src, m, counts = _slab(dev, torch.int32, True, n, [('idx', (MAXP, 2)), ('src', (MAXP, 2)), ('m', ()), ('counts', (4,))]).values()
    prm = _lib.CpeTableTriParams(table.swap_for(ids), int(bool(need_both)), float(min_sin), float(max_res))
    _lib.check(L.cpe_table_triangulate_batch(gp.xy.contiguous().data_ptr(), gp.id.contiguous().data_ptr(), gp.cnt.contiguous().data_ptr(), n,
                                             K.data_ptr(), None if Tc is None else Tc.data_ptr(), P.data_ptr(), st.data_ptr(), table.lo,
                                             table.hi, C.addressof(prm), X.data_ptr(), idx.data_ptr(), res.data_ptr(), src.data_ptr(),
                                             m.data_ptr(), counts.data_ptr(), stats.data_ptr(), _stream()), 'cpe_table_triangulate_batch')
    return dict(pts3=X, idx=idx, res=res, src=src, m=m, counts=counts, stats=stats)


FUSED_TRUNCATED = _c.FUSED_FLAG_TRUNCATED                            # (beside FLAG_OVERFLOW)
FUSED_RAY1, FUSED_RAY2, FUSED_PLANE0, FUSED_PLANE1 = 1, 2, 4, 8     # bits of src[..., 0]


def fused_triangulate_batch(gp1: GridTables, gp2: GridTables, K1, K2, T21, table: LaserTable, need_both=False, min_sin=0.01,
                            sigma_px=0.25, sigma_mm=0.02, max_res=0.0, max_px=0.0, ids='col_row'):
    """BUILD-DEFINED: 3-D points from both cameras' rays AND the laser-plane table in one weighted solve per point, see
    include/cpe.h cpe_fused_triangulate_batch.  Every grid point of either table is a candidate: pairs (two rays and up to two
    planes), then the points only one camera found (one ray and its planes, exactly table_triangulate_batch's point).
    need_both, min_sin: for one-ray candidates; sigma_px, sigma_mm: the weights of a pair; max_res (mm), max_px (px): gates.
    -> dict(pts3 f64[n,MAXP,3], idx i32[n,MAXP,2], res f64[n,MAXP,4] (px off ray 1, ray 2; mm off the plane of component 0, 1),
            src i32[n,MAXP,3] (FUSED_* bits, slot in table 1 or -1, slot in table 2 or -1), m i32[n], counts i32[n,6] (m, pairs,
            left-only, right-only, refused, truncated), stats f64[n,4] (rms, max ray residual in px; rms, max plane residual in
            mm), flags i32[n] (FLAG_OVERFLOW, FUSED_TRUNCATED)); slots from m on hold zeros"""
    L = _lib.load()
    dev = gp1.xy.device
    n = gp1.cnt.shape[0]
    _check_tables('fused_triangulate_batch', gp1, n, 'gp1.', dev)
    _check_tables('fused_triangulate_batch', gp2, n, 'gp2.', dev)
    if not (sigma_px > 0 and sigma_mm > 0):
        raise ValueError(f'fused_triangulate_batch: sigma_px and sigma_mm must be > 0, got {sigma_px} and {sigma_mm}')
    K1, K2, T21 = _cameras(K1, K2, T21, dev)
    P, st = _table_on(table, dev)
    X, res, stats = _slab(dev, torch.float64, True, n, [('pts3', (MAXP, 3)), ('res', (MAXP, 4)), ('stats', (4,))]).values()
    idx, src, m, flags, counts = _slab(dev, torch.int32, True, n, [('idx', (MAXP, 2)), ('src', (MAXP, 3)), ('m', ()), ('flags', ()),
                                                                   ('counts', (6,))]).values()
    prm = _lib.CpeFusedTriParams(table.swap_for(ids), int(bool(need_both)), float(min_sin), float(sigma_px), float(sigma_mm),
                                 float(max_res), float(max_px))
    c = lambda t: t.contiguous()
    x1, d1, c1, x2, d2, c2 = c(gp1.xy), c(gp1.id), c(gp1.cnt), c(gp2.xy), c(gp2.id), c(gp2.cnt)
    _lib.check(L.cpe_fused_triangulate_batch(x1.data_ptr(), d1.data_ptr(), c1.data_ptr(), x2.data_ptr(), d2.data_ptr(), c2.data_ptr(), n,
                                             K1.data_ptr(), K2.data_ptr(), T21.data_ptr(), P.data_ptr(), st.data_ptr(), table.lo, table.hi,
                                             C.addressof(prm), X.data_ptr(), idx.data_ptr(), res.data_ptr(), src.data_ptr(), m.data_ptr(),
                                             counts.data_ptr(), stats.data_ptr(), flags.data_ptr(), _stream()),
               'cpe_fused_triangulate_batch')
    return dict(pts3=X, idx=idx, res=res, src=src, m=m, counts=counts, stats=stats, flags=flags)


def fit_single_cylinder_fused_batch(gp1: GridTables, gp2: GridTables, K1, K2, T21, table: LaserTable, radius, ransac=None,
                                    mode=FIT_NELDER_MEAD, need_both=False, min_sin=0.01, sigma_px=0.25, sigma_mm=0.02, max_res=0.0,
                                    max_px=0.0, **fit_kw):
    """BUILD-DEFINED, fit_single_cylinder_batch on fused points: fused_triangulate_batch, then fit_cylinder_batch (ransac: a dict
    of fit_cylinder_ransac_batch keywords) on its points with cnt = m.
    -> the fit's keys (cyl_raw, cyl, T, fvals, iters, status[, n_inliers, inlier_mask]) beside pts3, idx, m, counts, res, src,
    stats, flags and mean_err f64[n] = stats[:, 0], the rms ray residual of the pairs in pixels.  status is ST_OVERFLOW where the
    join set FLAG_OVERFLOW."""
    tri = fused_triangulate_batch(gp1, gp2, K1, K2, T21, table, need_both=need_both, min_sin=min_sin, sigma_px=sigma_px,
                                  sigma_mm=sigma_mm, max_res=max_res, max_px=max_px)
    return dict(tri, **_fit_points(tri['pts3'], tri['m'], radius, ransac, tri['flags'], mode=mode, **fit_kw), mean_err=tri['stats'][:, 0])


PRED_MAXN = _c.PRED_MAXN
PRED_OK, PRED_NO_FRAME, PRED_NO_PLANE, PRED_PARALLEL, PRED_MISS, PRED_GRAZING = (
    _c.PRED_OK, _c.PRED_NO_FRAME, _c.PRED_NO_PLANE, _c.PRED_PARALLEL, _c.PRED_MISS, _c.PRED_GRAZING)


def grid_predict_batch(cyl, radius, K1, K2, T21, table: LaserTable, use=None, window=None, min_cos=0.1, image_size=None):
    """BUILD-DEFINED: where the grid nodes of `table` fall on the cylinder of every frame's pose and in both images, see
    include/cpe.h cpe_grid_predict_batch.  cyl f64[n,6] (a point on the axis, the axis direction; camera-1 coordinates), e.g.
    fit_cylinder_batch(...)['cyl'][:, 1]; use: bool / u8 [n] or None; window ((lo0, hi0), (lo1, hi1)): the node indices of table
    family 0 and 1, default the whole table, which must then hold at most PRED_MAXN nodes; image_size (h, w) or None: no bound.
    A table whose centre_status is not ST_OK is refused (LaserTable.has_centre: answered from table.centre_ok, which load() sets
    and to() carries on; a table built without it costs one read from the device, the only wait for the GPU here).
    -> dict(X f64[n,N,3], px f64[n,2,N,2], state i32[n,N] (PRED_*), vis i32[n,N] (bit 0 camera 1, bit 1 camera 2),
            counts i32[n,4] (OK, visible in 1, in 2, in both), window, Nu, Nv, family0)"""
    L = _lib.load()
    if not table.has_centre():
        raise ValueError('grid_predict_batch: the table has no projector centre (centre_status is not ST_OK)')
    if window is None:
        window = ((table.lo, table.hi), (table.lo, table.hi))
    (lo0, hi0), (lo1, hi1) = ((int(a), int(b)) for a, b in window)
    Nu, Nv = hi0 - lo0 + 1, hi1 - lo1 + 1
    if not (table.lo <= lo0 <= hi0 <= table.hi and table.lo <= lo1 <= hi1 <= table.hi):
        raise ValueError(f'grid_predict_batch: window {window} outside the table [{table.lo}, {table.hi}]')
    if Nu * Nv > PRED_MAXN:
        raise ValueError(f'grid_predict_batch: {Nu} x {Nv} nodes, at most {PRED_MAXN}: give a smaller window')
    if not 0 < min_cos < 1:
        raise ValueError(f'grid_predict_batch: min_cos must lie in (0, 1), got {min_cos}')
    if cyl.dtype != torch.float64 or cyl.dim() != 2 or cyl.shape[1] != 6:
        raise TypeError(f'grid_predict_batch: cyl must be float64 [n,6], got {cyl.dtype} {list(cyl.shape)}')
    dev = cyl.device
    n, N = cyl.shape[0], Nu * Nv
    cyl = cyl.contiguous()
    if use is not None:
        use = use.to(device=dev, dtype=torch.uint8).contiguous()
        if tuple(use.shape) != (n,):
            raise TypeError(f'grid_predict_batch: use must be [{n}], got {list(use.shape)}')
    K1, K2, T21 = _cameras(K1, K2, T21, dev)
    P, st, centre = _table_on(table, dev, centre=True)
    # (the kernels write every slot)
    X, px = _slab(dev, torch.float64, False, n, [('X', (N, 3)), ('px', (2, N, 2))]).values()
    state, vis, counts = _slab(dev, torch.int32, False, n, [('state', (N,)), ('vis', (N,)), ('counts', (4,))]).values()
    h, w = (0, 0) if image_size is None else (int(image_size[0]), int(image_size[1]))
    prm = _lib.CpeGridPredictParams((C.c_int32 * 2)(lo0, lo1), (C.c_int32 * 2)(hi0, hi1), float(min_cos), w, h)
    _lib.check(L.cpe_grid_predict_batch(_ptr(cyl), _ptr(use), n, float(radius), K1.data_ptr(), K2.data_ptr(), T21.data_ptr(), P.data_ptr(),
                                        st.data_ptr(), table.lo, table.hi, centre.data_ptr(), C.addressof(prm), _ptr(X), _ptr(px), _ptr(state),
                                        _ptr(vis), _ptr(counts), _stream()), 'cpe_grid_predict_batch')
    return dict(X=X, px=px, state=state, vis=vis, counts=counts, window=((lo0, hi0), (lo1, hi1)), Nu=Nu, Nv=Nv, family0=table.family0)


def grid_assign_batch(gp: GridTables, pred, cam, tau_px=4.0, ratio=0.5, ids='col_row'):
    """BUILD-DEFINED: one camera's grid tables re-numbered by the nearest predicted node, see include/cpe.h
    cpe_grid_assign_batch.  pred: the dict of grid_predict_batch for the same n frames; cam 1 or 2: whose images gp holds;
    ids: what gp.id holds ('col_row' as GridTables, 'row_col' as the planar detector writes).
    -> dict(tables (GridTables of the kept points: xy, the new id, cnt = m), src i32[n,MAXP] (input slot), dist f64[n,MAXP] (px),
            m i32[n], counts i32[n,8] (m, kept unchanged, kept re-numbered, no node, far, ambiguous, conflict, 0), stats f64[n,2]
            (rms, max of dist), node_slot i32[n,N] (the kept point's input slot per node, or -1)); slots from m on hold zeros"""
    L = _lib.load()
    if cam not in (1, 2):
        raise ValueError('grid_assign_batch: cam is 1 or 2')
    if ids not in ('col_row', 'row_col'):
        raise ValueError("ids is 'col_row' or 'row_col'")
    if not (tau_px > 0 and 0 < ratio <= 1):
        raise ValueError(f'grid_assign_batch: tau_px must be > 0 and ratio in (0, 1], got {tau_px} and {ratio}')
    dev = gp.xy.device
    n = gp.cnt.shape[0]
    _check_tables('grid_assign_batch', gp)
    Nu, Nv = pred['Nu'], pred['Nv']
    N = Nu * Nv
    px, vis = pred['px'], pred['vis']
    if tuple(px.shape) != (n, 2, N, 2) or tuple(vis.shape) != (n, N) or px.device != dev or not px.is_contiguous() or not vis.is_contiguous():
        raise TypeError(f'grid_assign_batch: pred must hold contiguous px [{n},2,{N},2] and vis [{n},{N}] on {dev}')
    swap = int((pred['family0'] == 'col') != (ids == 'col_row'))
    xy_out, dist, stats = _slab(dev, torch.float64, True, n, [('xy', (MAXP, 2)), ('dist', (MAXP,)), ('stats', (2,))]).values()
    id_out, src, m, counts, node_slot = _slab(dev, torch.int32, True, n, [('id', (MAXP, 2)), ('src', (MAXP,)), ('m', ()), ('counts', (8,)),
                                                                          ('node_slot', (N,))]).values()
    prm = _lib.CpeGridAssignParams(float(tau_px), float(ratio), swap, 0)
    c = lambda t: t.contiguous()
    x, d, k = c(gp.xy), c(gp.id), c(gp.cnt)
    _lib.check(L.cpe_grid_assign_batch(_ptr(x), _ptr(d), _ptr(k), n, None if n == 0 else px.data_ptr() + 16 * N * (cam - 1), 4 * N, _ptr(vis),
                                       cam - 1, pred['window'][0][0], pred['window'][1][0], Nu, Nv, C.addressof(prm), _ptr(xy_out),
                                       _ptr(id_out), _ptr(src), _ptr(dist), _ptr(m), _ptr(counts), _ptr(stats), _ptr(node_slot), _stream()),
               'cpe_grid_assign_batch')
    return dict(tables=GridTables(xy_out, id_out, m), src=src, dist=dist, m=m, counts=counts, stats=stats, node_slot=node_slot)


_REFINE_KEYS = ('cyl_raw', 'cyl', 'T', 'fvals', 'iters', 'status', 'pts3', 'idx', 'm', 'mean_err')


def fit_single_cylinder_refined_batch(gp1: GridTables, gp2: GridTables, K1, K2, T21, table: LaserTable, radius, rounds=2, first=None,
                                      tau_px=4.0, ratio=0.5, window=None, min_cos=0.1, image_size=None, fused=None, mode=FIT_LM,
                                      pixels=None, **fit_kw):
    """BUILD-DEFINED, opt-in: fit_single_cylinder_batch, then `rounds` rounds that re-number every grid point against the grid
    the frame's own fitted cylinder predicts and fit again on fused points.
    First fit_single_cylinder_batch(gp1, gp2, K1, K2, T21, radius, **first) (first: its keywords, match= included; None = the
    reference's).  Then per round, for the frames whose current status is ST_OK: grid_predict_batch from the current cyl[:, 1]
    (window, min_cos, image_size), grid_assign_batch of both images' detections (tau_px, ratio; with match= table 1 carries the
    shift), fused_triangulate_batch on the re-numbered tables (fused: its keywords) and fit_cylinder_batch (mode, fit_kw).  A frame
    takes a round's result only when that round's fit has status ST_OK; the choice is a torch.where on the device, and nothing
    here waits for the GPU beyond grid_predict_batch's one look at a new table's centre_status.
    -> dict(cyl_raw, cyl, T, fvals, iters, status, pts3, idx, m, mean_err (the first call's reprojection error, or a round's rms
            ray residual; pixels either way): of the result each frame ended with; tables1, tables2: the
            GridTables that result was made from (the re-numbered ones where a round was taken); round_taken i32[n]: the last
            round taken, 0 = the first fit stands; renumbered i32[n,2]: points of image 1, 2 whose index that round changed;
            rounds: per round dict(counts i32[n,2,8], stats f64[n,2,2] of grid_assign_batch per image, status i32[n] of the
            round's fit, taken bool[n]); first: the first call's dict)
    pixels: None, or a dict of fit_cylinder_pixels_batch keywords ({} = its defaults): the result is polished on tables1, tables2 by
    polish_with_pixels, whose keys the dict gains; without it nothing here changes."""
    rounds = int(rounds)
    if rounds < 0:
        raise ValueError('fit_single_cylinder_refined_batch: rounds < 0')
    n, dev = gp1.cnt.shape[0], gp1.xy.device
    first_out = fit_single_cylinder_batch(gp1, gp2, K1, K2, T21, radius, **(first or {}))
    if first and first.get('match') is not None:
        gp1 = GridTables(gp1.xy, gp1.id + first_out['offset'][:, None, :], gp1.cnt)
    cur = {k: first_out[k] for k in _REFINE_KEYS}
    t1, t2 = gp1, gp2
    taken_round = torch.zeros(n, dtype=torch.int32, device=dev)
    renum = torch.zeros((n, 2), dtype=torch.int32, device=dev)
    per_round = []
    for r in range(1, rounds + 1):
        use = cur['status'] == ST_OK
        pred = grid_predict_batch(cur['cyl'][:, 1], radius, K1, K2, T21, table, use=use, window=window, min_cos=min_cos,
                                  image_size=image_size)
        a1 = grid_assign_batch(gp1, pred, 1, tau_px=tau_px, ratio=ratio)
        a2 = grid_assign_batch(gp2, pred, 2, tau_px=tau_px, ratio=ratio)
        tri = fused_triangulate_batch(a1['tables'], a2['tables'], K1, K2, T21, table, **(fused or {}))
        fit = _fit_points(tri['pts3'], tri['m'], radius, None, tri['flags'], mode=mode, **fit_kw)
        take = use & (fit['status'] == ST_OK)
        new = dict(fit, pts3=tri['pts3'], idx=tri['idx'], m=tri['m'], mean_err=tri['stats'][:, 0])
        pick = lambda a, b: torch.where(take.view((n,) + (1,) * (a.dim() - 1)), a, b)
        cur = {k: pick(new[k], cur[k]) for k in _REFINE_KEYS}
        t1 = GridTables(pick(a1['tables'].xy, t1.xy), pick(a1['tables'].id, t1.id), pick(a1['tables'].cnt, t1.cnt))
        t2 = GridTables(pick(a2['tables'].xy, t2.xy), pick(a2['tables'].id, t2.id), pick(a2['tables'].cnt, t2.cnt))
        taken_round = torch.where(take, torch.full_like(taken_round, r), taken_round)
        renum = pick(torch.stack([a1['counts'][:, 2], a2['counts'][:, 2]], 1), renum)
        per_round.append(dict(counts=torch.stack([a1['counts'], a2['counts']], 1), stats=torch.stack([a1['stats'], a2['stats']], 1),
                              status=fit['status'], taken=take))
    out = dict(cur)
    out.update(tables1=t1, tables2=t2, round_taken=taken_round, renumbered=renum, rounds=per_round, first=first_out)
    if pixels is not None:
        out = polish_with_pixels(out, t1, t2, K1, K2, T21, table, radius, pixels)
    return out


SHIFT_MAX_WIN = _c.SHIFT_MAX_WIN
SHIFT_SHIFTED, SHIFT_WEAK, SHIFT_EDGE = _c.SHIFT_FLAG_SHIFTED, _c.SHIFT_FLAG_WEAK, _c.SHIFT_FLAG_EDGE


def index_shift_batch(pts3, idx, cnt, table: LaserTable, use=None, win=(4, 4), tau=1.0, min_score=8, ids='col_row'):
    """BUILD-DEFINED: the shift to add to the grid indices of every STEREO frame so that its points lie on the planes of `table`
    that its indices name, searched per index component over d in [-win[c], win[c]]; see include/cpe.h cpe_index_shift_batch.
    pts3, idx, cnt, use as index_planes_batch; ids says what idx holds ('col_row' as GridTables, 'row_col' as the planar
    detector), which family of the table either component addresses follows from table.family0.
    -> dict(shift i32[n,2], score i32[n,2,4] (best, runner-up, at d = 0, usable points), scores i32[n, 2 win[0] + 2 win[1] + 2]
            (every candidate, component 0 first, d ascending), rms f64[n,2,2] (at the applied shift, at d = 0), flags i32[n,2]
            (SHIFT_*), idx i32[n,MAXP,2] = idx + shift below the count, zeros past it)"""
    L = _lib.load()
    pts3, idx, cnt, use = _point_tables('index_shift_batch', pts3, idx, cnt, use)
    dev = pts3.device
    n = cnt.shape[0]
    win = tuple(int(w) for w in win)
    if len(win) != 2 or not all(0 <= w <= SHIFT_MAX_WIN for w in win):
        raise ValueError(f'index_shift_batch: window {win} outside 0..{SHIFT_MAX_WIN}')
    if not tau > 0:
        raise ValueError(f'index_shift_batch: tau must be > 0, got {tau}')
    P, st = _table_on(table, dev)
    ncand = 2 * win[0] + 1 + 2 * win[1] + 1
    # (the kernel writes every slot of every output but idx past the count)
    shift, score, scores, flags = _slab(dev, torch.int32, False, n, [('shift', (2,)), ('score', (2, 4)), ('scores', (ncand,)),
                                                                     ('flags', (2,))]).values()
    rms = torch.empty((n, 2, 2), dtype=torch.float64, device=dev)
    out = torch.zeros((n, MAXP, 2), dtype=torch.int32, device=dev)
    prm = _lib.CpeIndexShiftParams((C.c_int32 * 2)(*win), float(tau), int(min_score), table.swap_for(ids))
    _lib.check(L.cpe_index_shift_batch(_ptr(pts3), _ptr(idx), _ptr(cnt), n, _ptr(use), P.data_ptr(), st.data_ptr(), table.lo, table.hi,
                                       C.addressof(prm), _ptr(shift), _ptr(score), _ptr(scores), _ptr(rms), _ptr(flags), _ptr(out), _stream()),
               'cpe_index_shift_batch')
    return dict(shift=shift, score=score, scores=scores, rms=rms, flags=flags, idx=out)


def fit_projector_model_renumbered(pts3, idx, cnt, lo, hi, use=None, frame_ok=None, win=(4, 4), shift_tau=None, shift_min_score=8,
                                   family0='col', **fit_kw):
    """BUILD-DEFINED: fit_projector_model that brings back the frames it would only trim.  Four steps, all enqueued, no host
    synchronisation: the model on [lo, hi] with the trimming band fit_kw['tau'] > 0; its table for [lo - w, hi + w], w = max(win);
    index_shift_batch of every frame against that table (shift_tau defaults to the fit's tau); the model again on
    [lo - w, hi + w] with the re-numbered indices, started from the first model.  idx is (col, row) for family0 'col' and (row,
    col) for 'row': component c is family c either way.  A frame the caller leaves out with frame_ok is searched all the same and
    fitted in neither call.
    -> dict(first (the first fit's dict), table (its LaserTable), shift (index_shift_batch's dict, shift['idx'] the indices the
            refit read), fit (the refit's dict), lo, hi (the refit's range))"""
    tau = fit_kw.get('tau', 0.0)
    if not tau > 0:
        raise ValueError('fit_projector_model_renumbered: tau must be > 0 (an untrimmed first model is spoiled by the frames it is '
                         'meant to repair)')
    w = max(int(x) for x in win)
    lo2, hi2 = int(lo) - w, int(hi) + w
    if hi2 - lo2 + 1 > _lib.MAXL:
        raise ValueError(f'fit_projector_model_renumbered: {hi2 - lo2 + 1} indices in [{lo}, {hi}] widened by {w}, must be 1..{_lib.MAXL}')
    first = fit_projector_model(pts3, idx, cnt, lo, hi, use=use, frame_ok=frame_ok, **fit_kw)
    table = ProjectorModel.from_fit(first, family0).table(lo2, hi2)
    shift = index_shift_batch(pts3, idx, cnt, table, use=use, win=win, tau=tau if shift_tau is None else shift_tau,
                              min_score=shift_min_score, ids='col_row' if family0 == 'col' else 'row_col')
    refit = fit_projector_model(pts3, shift['idx'], cnt, lo2, hi2, use=use, frame_ok=frame_ok, **dict(fit_kw, x0=first['model'][:15]))
    return dict(first=first, table=table, shift=shift, fit=refit, lo=lo2, hi=hi2)


def fit_single_cylinder_mono_batch(gp: GridTables, K, Tc, table: LaserTable, radius, ransac=None, mode=FIT_NELDER_MEAD, need_both=False,
                                   min_sin=0.01, max_res=0.0, pixels=None, **fit_kw):
    """BUILD-DEFINED, fit_single_cylinder_batch from one camera: table_triangulate_batch, then fit_cylinder_batch (ransac: a
    dict of fit_cylinder_ransac_batch keywords) on its points with cnt = m.
    -> the fit's keys (cyl_raw, cyl, T, fvals, iters, status[, n_inliers, inlier_mask]) beside pts3, idx, m, counts, res, src,
    stats and mean_err f64[n] = stats[:, 0]: NOT a reprojection error in pixels as in the stereo call, but the rms distance in mm
    of the points from the planes that made them (0 for points cut with one plane only).
    pixels: None, or a dict of fit_cylinder_pixels_batch keywords ({} = its defaults): the result is polished on gp by
    polish_with_pixels (this camera alone), whose keys the dict gains; without it nothing here changes."""
    tri = table_triangulate_batch(gp, K, Tc, table, need_both=need_both, min_sin=min_sin, max_res=max_res)
    out = dict(tri, **_fit_points(tri['pts3'], tri['m'], radius, ransac, mode=mode, **fit_kw), mean_err=tri['stats'][:, 0])
    if pixels is not None:
        out = polish_mono_with_pixels(out, gp, K, Tc, table, radius, pixels)
    return out


MONO_SHIFT_MAX_TOP_K = 8


def mono_shift_batch(gp: GridTables, K, Tc, table: LaserTable, win=(4, 4), tau=0.1, min_score=8, min_sin=0.01, top_k=4, ids='col_row'):
    """BUILD-DEFINED: the grid-index shift of ONE camera's frames against the laser-plane table, searched over |d_c| <= win[c] by
    the two plane residuals of every point (one ray, two planes: over-determined by one); see include/cpe.h cpe_mono_shift_batch.
    gp, K, Tc, table, ids as table_triangulate_batch.  The call reports and applies nothing.
    -> dict(scores i32[n, (2 win[0] + 1)(2 win[1] + 1)] (every candidate, d0-major, ascending), cand i32[n,top_k,2] and cand_score
            i32[n,top_k] (the best top_k candidates in rank order; (0, 0) and -1 past the candidate count), score i32[n,4] (best,
            runner-up, at (0, 0), usable points), rms f64[n,2] (mm, at the best candidate, at (0, 0)), flags i32[n] (SHIFT_EDGE,
            SHIFT_WEAK), win)"""
    L = _lib.load()
    dev = gp.xy.device
    n = gp.cnt.shape[0]
    _check_tables('mono_shift_batch', gp)
    win = tuple(int(w) for w in win)
    if len(win) != 2 or not all(0 <= w <= SHIFT_MAX_WIN for w in win):
        raise ValueError(f'mono_shift_batch: window {win} outside 0..{SHIFT_MAX_WIN}')
    if not tau > 0:
        raise ValueError(f'mono_shift_batch: tau must be > 0, got {tau}')
    if not 1 <= int(top_k) <= MONO_SHIFT_MAX_TOP_K:
        raise ValueError(f'mono_shift_batch: top_k {top_k} outside 1..{MONO_SHIFT_MAX_TOP_K}')
    if not (min_sin >= 0 and int(min_score) >= 0):
        raise ValueError(f'mono_shift_batch: min_sin and min_score must be >= 0, got {min_sin} and {min_score}')
    top_k = int(top_k)
    K = _dev3(K, dev, (9,))
    Tc = None if Tc is None else _dev3(Tc, dev, (16,))
    P, st = _table_on(table, dev)
    ncand = (2 * win[0] + 1) * (2 * win[1] + 1)
    # (the kernels write every slot of every output)
    scores, cand, cand_score, score, flags = _slab(dev, torch.int32, False, n, [('scores', (ncand,)), ('cand', (top_k, 2)),
                                                                                ('cand_score', (top_k,)), ('score', (4,)),
                                                                                ('flags', ())]).values()
    rms = torch.empty((n, 2), dtype=torch.float64, device=dev)
    c = lambda t: t.contiguous()
    x, d, k = c(gp.xy), c(gp.id), c(gp.cnt)
    _lib.check(L.cpe_mono_shift_batch(_ptr(x), _ptr(d), _ptr(k), n, K.data_ptr(), None if Tc is None else Tc.data_ptr(), P.data_ptr(),
                                      st.data_ptr(), table.lo, table.hi, win[0], win[1], float(tau), float(min_sin), int(min_score),
                                      table.swap_for(ids), top_k, _ptr(scores), _ptr(cand), _ptr(cand_score),
                                      _ptr(score), _ptr(rms), _ptr(flags), _stream()), 'cpe_mono_shift_batch')
    return dict(scores=scores, cand=cand, cand_score=cand_score, score=score, rms=rms, flags=flags, win=win)


_MONO_KEYS = ('cyl_raw', 'cyl', 'T', 'fvals', 'iters', 'status', 'pts3', 'idx', 'm', 'counts', 'res', 'src', 'stats', 'mean_err')


def _fit_rms(fit, m):
    """sqrt(final objective / points) in mm, +inf where the fit is not ST_OK"""
    rms = torch.sqrt(fit['fvals'][:, 1] / m.clamp(min=1).to(torch.float64))
    return torch.where((fit['status'] == ST_OK) & torch.isfinite(rms), rms, torch.full_like(rms, math.inf))


def fit_single_cylinder_mono_repaired_batch(gp: GridTables, cam, K1, K2, T21, table: LaserTable, radius, shift=None, rounds=1,
                                            max_res=0.25, vote_frac=0.5, rms_ratio=1.5, tau_px=4.0, ratio=0.5, window=None, min_cos=0.1,
                                            image_size=None, mode=FIT_LM, **fit_kw):
    """BUILD-DEFINED, opt-in: fit_single_cylinder_mono_batch with the two repairs a one-camera frame can have (DESIGN.md section
    3.7): the frame-wide index shift, then `rounds` rounds that re-number every grid point against the grid the frame's own fitted
    cylinder predicts.  cam 1 or 2: whose tables gp holds (camera 2 reads K2 and T21).  Every triangulation here needs both planes
    and gates them with max_res; every fit is fit_cylinder_batch(mode, **fit_kw).
    first = fit_single_cylinder_mono_batch(gp, K, Tc, table, radius, mode=mode, need_both=True, max_res=max_res, **fit_kw); with
    shift=None and rounds=0 its outputs are the result, bit for bit.
    shift: None (skip), or a dict of mono_shift_batch keywords ({} = its defaults).  The votes leave top_k candidates; each is
    applied to a copy of gp.id, triangulated and fitted (top_k pairs of calls on all n frames).  A candidate is eligible when
    cand_score >= max(min_score, vote_frac * best) and its fit is ST_OK; the eligible candidate with the smallest
    fit rms = sqrt(fvals[:, 1] / m) is chosen (the better-ranked one on a tie), and trusted when it is the only eligible one or
    rms_ratio * its rms <= the next smallest rms.  Otherwise SHIFT_WEAK, the shift is (0, 0) and the frame goes on as `first`.
    Rounds, for the frames whose current status is ST_OK: grid_predict_batch from the current cyl[:, 1] (window, min_cos,
    image_size), grid_assign_batch of gp with the shift applied (tau_px, ratio), table_triangulate_batch and the fit.  A frame takes a
    round only when that round's fit is ST_OK.  Every choice is a torch.where on the device; nothing here waits for the GPU beyond
    grid_predict_batch's one look at a new table's centre_status.
    -> the keys of fit_single_cylinder_mono_batch (src[..., 1] is the slot in `tables`), of the result each frame ended with, and
       shift i32[n,2] (applied), shift_flags i32[n] (SHIFT_SHIFTED: a non-zero shift was applied; SHIFT_WEAK: no trusted choice;
       SHIFT_EDGE: the applied shift lies on the window's border), vote_flags i32[n] (mono_shift_batch's own), shift_score i32[n,4],
       cand i32[n,top_k,2], cand_score i32[n,top_k], cand_rms f64[n,top_k] (mm; +inf where the candidate's fit is not ST_OK),
       tables (the GridTables the result was made from), round_taken i32[n] (0: none), renumbered i32[n] (points whose index that
       round changed), rounds: per round dict(counts i32[n,8], stats f64[n,2] of grid_assign_batch, status i32[n], taken bool[n]),
       first.  With shift=None: one candidate (0, 0) with cand_score -1 and the rms of `first`."""
    rounds = int(rounds)
    if rounds < 0:
        raise ValueError('fit_single_cylinder_mono_repaired_batch: rounds < 0')
    if cam not in (1, 2):
        raise ValueError('fit_single_cylinder_mono_repaired_batch: cam is 1 or 2')
    for k in ('need_both', 'min_sin', 'ransac'):
        if k in fit_kw:
            raise ValueError(f'fit_single_cylinder_mono_repaired_batch: {k} does not apply (both planes are always needed, every fit '
                             'is fit_cylinder_batch)')
    if not (vote_frac >= 0 and rms_ratio >= 1):
        raise ValueError(f'fit_single_cylinder_mono_repaired_batch: vote_frac >= 0 and rms_ratio >= 1, got {vote_frac} and {rms_ratio}')
    n, dev = gp.cnt.shape[0], gp.xy.device
    K, Tc = (K1, None) if cam == 1 else (K2, T21)

    def solve(tables):
        tri = table_triangulate_batch(tables, K, Tc, table, need_both=True, max_res=max_res)
        return dict(tri, **fit_cylinder_batch(tri['pts3'], tri['m'], radius, mode=mode, **fit_kw), mean_err=tri['stats'][:, 0])

    first = solve(gp)
    cur = {k: first[k] for k in _MONO_KEYS}
    pick = lambda take, a, b: torch.where(take.view((n,) + (1,) * (a.dim() - 1)), a, b)
    applied = torch.zeros((n, 2), dtype=torch.int32, device=dev)
    if shift is None:
        z = torch.zeros((n, 6), dtype=torch.int32, device=dev)
        flags, vote_flags, shift_score = z[:, 0], z[:, 1], z[:, 2:6]
        cand = torch.zeros((n, 1, 2), dtype=torch.int32, device=dev)
        cand_score = torch.full((n, 1), -1, dtype=torch.int32, device=dev)
        cand_rms = _fit_rms(first, first['m'])[:, None]
    else:
        ms = mono_shift_batch(gp, K, Tc, table, **shift)
        cand, cand_score, shift_score, vote_flags = ms['cand'], ms['cand_score'], ms['score'], ms['flags']
        top_k = cand.shape[1]
        sols = [solve(GridTables(gp.xy, gp.id + cand[:, k, None, :], gp.cnt)) for k in range(top_k)]
        cand_rms = torch.stack([_fit_rms(s, s['m']) for s in sols], 1)
        need = torch.clamp(vote_frac * shift_score[:, 0].to(torch.float64), min=float(shift.get('min_score', 8)))
        eligible = (cand_score.to(torch.float64) >= need[:, None]) & torch.isfinite(cand_rms)
        r_sorted, order = torch.sort(torch.where(eligible, cand_rms, torch.full_like(cand_rms, math.inf)), dim=1, stable=True)
        n_elig = eligible.sum(1)
        trusted = (n_elig == 1)
        if top_k > 1:
            trusted = trusted | ((n_elig >= 2) & (rms_ratio * r_sorted[:, 0] <= r_sorted[:, 1]))
        chosen = order[:, 0]
        for k in range(top_k):
            take = trusted & (chosen == k)
            cur = {key: pick(take, sols[k][key], cur[key]) for key in _MONO_KEYS}
            applied = pick(take, cand[:, k], applied)
        win = torch.tensor(ms['win'], dtype=torch.int32, device=dev)
        edge = ((applied.abs() == win) & (win > 0)).any(1)
        flags = (torch.where(trusted, 0, SHIFT_WEAK) | torch.where((applied != 0).any(1), SHIFT_SHIFTED, 0) |
                 torch.where(edge, SHIFT_EDGE, 0)).to(torch.int32)
    shifted = GridTables(gp.xy, gp.id + applied[:, None, :], gp.cnt)
    tables = shifted
    taken_round = torch.zeros(n, dtype=torch.int32, device=dev)
    renum = torch.zeros(n, dtype=torch.int32, device=dev)
    per_round = []
    for r in range(1, rounds + 1):
        use = cur['status'] == ST_OK
        pred = grid_predict_batch(cur['cyl'][:, 1], radius, K1, K2, T21, table, use=use, window=window, min_cos=min_cos,
                                  image_size=image_size)
        a = grid_assign_batch(shifted, pred, cam, tau_px=tau_px, ratio=ratio)
        new = solve(a['tables'])
        take = use & (new['status'] == ST_OK)
        cur = {k: pick(take, new[k], cur[k]) for k in _MONO_KEYS}
        tables = GridTables(pick(take, a['tables'].xy, tables.xy), pick(take, a['tables'].id, tables.id), pick(take, a['tables'].cnt, tables.cnt))
        taken_round = torch.where(take, torch.full_like(taken_round, r), taken_round)
        renum = pick(take, a['counts'][:, 2], renum)
        per_round.append(dict(counts=a['counts'], stats=a['stats'], status=new['status'], taken=take))
    out = dict(cur)
    out.update(shift=applied, shift_flags=flags, vote_flags=vote_flags, shift_score=shift_score, cand=cand, cand_score=cand_score,
               cand_rms=cand_rms, tables=tables, round_taken=taken_round, renumbered=renum, rounds=per_round, first=first)
    return out


PIXFIT_MIN_PTS = _c.PIXFIT_MIN_PTS
_PIX_WANT = ('res', 'pt_state', 'X')


def fit_cylinder_pixels_batch(gp1: Optional[GridTables], gp2: Optional[GridTables], cyl0, radius, K1, K2, T21, table: LaserTable, use=None,
                              gate_px=0.0, min_cos=0.1, ids='col_row', want=('res',), tol_x=1e-9, tol_f=1e-9, max_iter=100):
    """BUILD-DEFINED, opt-in: the cylinder pose that minimises the pixel distance between every detection and the predicted pixel of
    its own grid node, in both images at once; see include/cpe.h cpe_fit_cylinder_pixels_batch.  gp1, gp2:
    the two cameras' tables, either may be None (that camera is absent); cyl0 f64[n,6]: the start, e.g. fit_cylinder_batch(...)
    ['cyl'][:, 1]; use: bool / u8 [n] or None; gate_px <= 0: no gate; ids as table_triangulate_batch; want: which of the optional
    per-detection outputs 'res', 'pt_state', 'X' to make.  The indices are trusted: re-number first (grid_assign_batch).  A table
    without a projector centre is refused, as grid_predict_batch does.
    -> dict(cyl f64[n,6] (raw: no prior applied), fvals f64[n,2] (F at the start, at the end; px^2), iters i32[n,2], counts i32[n,4]
            (used of camera 1, of camera 2, refused, gated), stats f64[n,4] (rms of camera 1, of camera 2, of both, largest
            residual; px), status i32[n], res f64[n,2,MAXP,2], pt_state i32[n,2,MAXP], X f64[n,2,MAXP,3] (None unless wanted))"""
    what = 'fit_cylinder_pixels_batch'
    L = _lib.load()
    if gp1 is None and gp2 is None:
        raise ValueError(f'{what}: both cameras are absent')
    if not table.has_centre():
        raise ValueError(f'{what}: the table has no projector centre (centre_status is not ST_OK)')
    want = (want,) if isinstance(want, str) else tuple(want)
    if any(w not in _PIX_WANT for w in want):
        raise ValueError(f'{what}: want holds {want}, known: {_PIX_WANT}')
    if cyl0.dtype != torch.float64 or cyl0.dim() != 2 or cyl0.shape[1] != 6:
        raise TypeError(f'{what}: cyl0 must be float64 [n,6], got {cyl0.dtype} {list(cyl0.shape)}')
    if not (0 < min_cos < 1 and tol_x > 0 and tol_f > 0 and int(max_iter) >= 1 and radius > 0):
        raise ValueError(f'{what}: min_cos in (0, 1), tol_x, tol_f, radius > 0 and max_iter >= 1, got {min_cos}, {tol_x}, {tol_f}, {radius}, '
                         f'{max_iter}')
    dev, n = cyl0.device, cyl0.shape[0]
    cyl0 = cyl0.contiguous()
    for name, gp in (('gp1.', gp1), ('gp2.', gp2)):
        if gp is not None:
            _check_tables(what, gp, n, name, dev)
    if use is not None:
        use = use.to(device=dev, dtype=torch.uint8).contiguous()
        if tuple(use.shape) != (n,):
            raise TypeError(f'{what}: use must be [{n}], got {list(use.shape)}')
    K1, K2, T21 = _cameras(K1, K2, T21, dev)
    P, st, centre = _table_on(table, dev, centre=True)
    # (the kernel writes every slot of every output: no fills)
    cyl, fvals, stats = _slab(dev, torch.float64, False, n, [('cyl', (6,)), ('fvals', (2,)), ('stats', (4,))]).values()
    iters, counts, status = _slab(dev, torch.int32, False, n, [('iters', (2,)), ('counts', (4,)), ('status', ())]).values()
    res = torch.empty((n, 2, MAXP, 2), dtype=torch.float64, device=dev) if 'res' in want else None
    pt = torch.empty((n, 2, MAXP), dtype=torch.int32, device=dev) if 'pt_state' in want else None
    X = torch.empty((n, 2, MAXP, 3), dtype=torch.float64, device=dev) if 'X' in want else None
    c = lambda gp: (None, None, None) if gp is None or n == 0 else (gp.xy.contiguous(), gp.id.contiguous(), gp.cnt.contiguous())
    t1, t2 = c(gp1), c(gp2)
    if n:
        _lib.check(L.cpe_fit_cylinder_pixels_batch(*(_ptr(t) for t in t1), *(_ptr(t) for t in t2), _ptr(cyl0), _ptr(use), n, float(radius),
                                                   K1.data_ptr(), K2.data_ptr(), T21.data_ptr(), P.data_ptr(), st.data_ptr(), table.lo, table.hi,
                                                   centre.data_ptr(), table.swap_for(ids), float(min_cos), float(gate_px), float(tol_x),
                                                   float(tol_f), int(max_iter), _ptr(cyl), _ptr(fvals), _ptr(iters), _ptr(counts), _ptr(stats),
                                                   _ptr(status), _ptr(res), _ptr(pt), _ptr(X), _stream()), 'cpe_fit_cylinder_pixels_batch')
    return dict(cyl=cyl, fvals=fvals, iters=iters, counts=counts, stats=stats, status=status, res=res, pt_state=pt, X=X)


def _prior_rows(rows, ymin):
    """applyCylParamsPrior.m on rows f64[n,k,6] with the points' smallest y, ymin f64[n]: the direction with d_y >= 0 and the axis
    point at that y (the arithmetic of cpe_fit_cylinder_batch's epilogue) -> f64[n,k,6]"""
    o, d = rows[..., :3], rows[..., 3:]
    d = torch.where(d[..., 1:2] < 0, -d, d)
    dy = d[..., 1]
    flat = dy.abs() < torch.finfo(torch.float64).eps
    t = torch.where(flat, torch.zeros_like(dy), (ymin[:, None] - o[..., 1]) / torch.where(flat, torch.ones_like(dy), dy))
    return torch.cat([o + t[..., None] * d, d], -1)


def _cyl_to_T(cyl):
    """cylParams2T.m on cyl f64[n,6] -> f64[n,4,4]: y along the axis, z = (1, 0, 0) x y, x = y x z, the origin at the axis point"""
    y = cyl[:, 3:] / cyl[:, 3:].norm(dim=1, keepdim=True)
    z = torch.stack([torch.zeros_like(y[:, 0]), -y[:, 2], y[:, 1]], 1)
    z = z / z.norm(dim=1, keepdim=True)
    x = torch.linalg.cross(y, z)
    x = x / x.norm(dim=1, keepdim=True)
    T = torch.zeros((cyl.shape[0], 4, 4), dtype=cyl.dtype, device=cyl.device)
    T[:, :3, 0], T[:, :3, 1], T[:, :3, 2], T[:, :3, 3], T[:, 3, 3] = x, y, z, cyl[:, :3], 1.0
    return T


def _pixels_options(what, pixels):
    o = dict(pixels or {})
    if 'want' in o or 'use' in o:
        raise ValueError(f"{what}: pixels may not set 'want' or 'use' (the polish needs the nodes' points and runs on the ST_OK frames)")
    return o


def fit_single_cylinder_pixels_batch(gp1: Optional[GridTables], gp2: Optional[GridTables], K1, K2, T21, table: LaserTable, radius,
                                     start=None, **pixels):
    """BUILD-DEFINED, opt-in: a start, then fit_cylinder_pixels_batch from it on the frames whose start is ST_OK.
    start: None = fit_single_cylinder_fused_batch(gp1, gp2, K1, K2, T21, table, radius, mode=FIT_LM) (both cameras needed), or the
    caller's dict with cyl, cyl_raw f64[n,2,6], T f64[n,4,4] and status i32[n] (any fit of this module).  pixels: keywords of
    fit_cylinder_pixels_batch (gate_px, min_cos, ids, tol_x, tol_f, max_iter).  The pixel fit starts at start['cyl'][:, 1].  Its
    result gets the conventions of fit_cylinder_batch: cyl_raw = [the start pose; the fitted pose], cyl = applyCylParamsPrior on
    both rows with the nodes' 3-D points X of the used detections as the points (in torch, on the device), T = cylParams2T of the
    final row.  A frame keeps the start's cyl_raw, cyl and T when the pixel fit is not ST_OK: a torch.where, nothing waits.
    -> dict(cyl_raw, cyl f64[n,2,6], T f64[n,4,4], status i32[n] (the start's), taken bool[n] (the pixel fit's result stands),
            start (its dict), pixels (fit_cylinder_pixels_batch's dict, want = res, pt_state, X))"""
    what = 'fit_single_cylinder_pixels_batch'
    opts = _pixels_options(what, pixels)
    if start is None:
        if gp1 is None or gp2 is None:
            raise ValueError(f'{what}: the default start is the fused fit of both cameras; give start= for one camera')
        start = fit_single_cylinder_fused_batch(gp1, gp2, K1, K2, T21, table, radius, mode=FIT_LM)
    ok0 = start['status'] == ST_OK
    cyl0 = start['cyl'][:, 1].contiguous()
    px = fit_cylinder_pixels_batch(gp1, gp2, cyl0, radius, K1, K2, T21, table, use=ok0, want=_PIX_WANT, **opts)
    taken = ok0 & (px['status'] == ST_OK)
    n = cyl0.shape[0]
    used = px['pt_state'].reshape(n, -1) == 0
    ymin = torch.where(used, px['X'].reshape(n, -1, 3)[..., 1], torch.full((), math.inf, dtype=torch.float64, device=cyl0.device)).amin(1)
    ymin = torch.where(taken, ymin, torch.zeros_like(ymin))
    raw = torch.stack([cyl0, px['cyl']], 1)
    cyl = _prior_rows(raw, ymin)
    T = _cyl_to_T(torch.where(taken[:, None], cyl[:, 1], start['cyl'][:, 1]))
    pick = lambda a, b: torch.where(taken.view((n,) + (1,) * (a.dim() - 1)), a, b)
    return dict(cyl_raw=pick(raw, start['cyl_raw']), cyl=pick(cyl, start['cyl']), T=pick(T, start['T']), status=start['status'], taken=taken,
                start=start, pixels=px)


def polish_with_pixels(out, gp1: Optional[GridTables], gp2: Optional[GridTables], K1, K2, T21, table: LaserTable, radius, pixels):
    """BUILD-DEFINED, opt-in: the result `out` of any cylinder fit of this module (cyl, cyl_raw, T, status) polished by
    fit_single_cylinder_pixels_batch(gp1, gp2, ..., start=out, **pixels) -> a copy of out whose cyl_raw, cyl and T are the pixel
    fit's where that is ST_OK (every other key stays: fvals, iters and mean_err describe the 3-D fit), beside pixels (the dict of
    fit_cylinder_pixels_batch) and, flat for FramePipeline.run_raw, pixels_taken bool[n], pixels_fvals f64[n,2], pixels_stats
    f64[n,4], pixels_counts i32[n,4], pixels_status i32[n]"""
    pol = fit_single_cylinder_pixels_batch(gp1, gp2, K1, K2, T21, table, radius, start=out, **pixels)
    px = pol['pixels']
    return dict(out, cyl_raw=pol['cyl_raw'], cyl=pol['cyl'], T=pol['T'], pixels=px, pixels_taken=pol['taken'], pixels_fvals=px['fvals'],
                pixels_stats=px['stats'], pixels_counts=px['counts'], pixels_status=px['status'])


def polish_mono_with_pixels(out, gp: GridTables, K, Tc, table: LaserTable, radius, pixels):
    """polish_with_pixels for ONE camera's tables, with K, Tc as table_triangulate_batch takes them (Tc None: camera 1)"""
    eye = torch.eye(4, dtype=torch.float64)
    if Tc is None:
        return polish_with_pixels(out, gp, None, K, K, eye, table, radius, pixels)
    return polish_with_pixels(out, None, gp, K, K, Tc, table, radius, pixels)
