"""Cases and a numpy reference for the index-shift search of stereo frames against a laser-plane table (include/cpe.h
cpe_index_shift_batch).

ref_index_shift restates the header's numbered rule in float64, one frame and one component at a time, with every candidate's
residuals as one array.  Beside the outputs of the call it reports

    margin    the smallest | |r| - tau | / tau over the residuals of all usable points and all candidates whose line is in
              range and OK: as long as it is far above the rounding of r (a few eps (|X| + |P4|) / tau ~ 1e-13), the kernel
              and the reference count the same points, and every integer output can be compared exactly;
    rms_tol   64 eps max(|X| + |P4|) over the points that count at the applied shift or at d = 0: a residual is three products
              and three sums of terms bounded by |X| and |P4|, and the root of a mean of squares moves by no more than its terms.

Cases are generated so that every margin is > 1e-6 (tests/test_index_shift_cases_cpu.py asserts it).

Measured on this reference: tests/proj_model_cases.py::shifted_frames(seed) for the seeds 0, 1, 2 (12 cylinder frames of 225
points, frames 3 and 7 numbered one column up) against the table -16..16 of ref_projector_model(tau = 1) on the same frames,
tau 1 mm, window 4: every frame and family scores 225 at the right shift and 0 at every other candidate; frames 3 and 7 get
(-1, 0), all others (0, 0)."""
import functools
import math

import numpy as np

import plane_fit_cases as PC
import proj_model_cases as M
import table_tri_cases as TC

MAXP, MAXL = PC.MAXP, PC.MAXL
EPS = PC.EPS
ST_OK = 0
MAX_WIN = 8
SHIFTED, WEAK, EDGE = 1, 2, 4
DEFAULTS = dict(win=(4, 4), tau=1.0, min_score=8, swap=0)


def ref_index_shift(X, I, cnt, P, status, lo, hi, use=None, win=(4, 4), tau=1.0, min_score=8, swap=0):
    """-> dict(shift (n,2), score (n,2,4), scores (n, 2 win0 + 2 win1 + 2), rms (n,2,2), flags (n,2), idx (n,MAXP,2): I with
    the shift added below the clamped count (int32 wrap), untouched past it; count (n,) the clamped counts; margin, rms_tol)"""
    X = np.asarray(X, np.float64).reshape(-1, MAXP, 3)
    I = np.asarray(I, np.int32).reshape(-1, MAXP, 2)
    cnt = np.asarray(cnt).reshape(-1)
    P, status = np.asarray(P, np.float64), np.asarray(status)
    n = len(cnt)
    ncand = 2 * win[0] + 1 + 2 * win[1] + 1
    out = dict(shift=np.zeros((n, 2), np.int32), score=np.zeros((n, 2, 4), np.int32), scores=np.zeros((n, ncand), np.int32),
               rms=np.zeros((n, 2, 2)), flags=np.zeros((n, 2), np.int32), idx=I.copy(), count=np.zeros(n, np.int32))
    margin, scale = math.inf, 0.0
    for f in range(n):
        c_ = min(max(int(cnt[f]), 0), MAXP)
        out['count'][f] = c_
        ok = np.isfinite(X[f, :c_]).all(1)
        if use is not None:
            ok &= np.asarray(use).reshape(-1, MAXP)[f, :c_] != 0
        pts = X[f, :c_][ok]
        for c in range(2):
            k, w = c ^ swap, win[c]
            iv = I[f, :c_, c][ok].astype(np.int64)
            near = (iv >= lo - w) & (iv <= hi + w)
            sc, res = {}, {}
            for d in range(-w, w + 1):
                v = iv + d
                can = near & (v >= lo) & (v <= hi)
                can[can] = status[k, v[can] - lo] == ST_OK
                pl = P[k, v[can] - lo]
                r = (pl[:, 0] * pts[can, 0] + pl[:, 1] * pts[can, 1]) + pl[:, 2] * pts[can, 2] + pl[:, 3]
                if len(r):
                    margin = min(margin, float(np.abs(np.abs(r) - tau).min() / tau))
                hit = np.abs(r) < tau
                sc[d] = int(hit.sum())
                res[d] = (r[hit], (np.linalg.norm(pts[can][hit], axis=1) + np.abs(pl[hit, 3])))
            best_d = min(sc, key=lambda d: (-sc[d], abs(d), d))
            ranked = sorted(sc.values(), reverse=True)
            best, second = ranked[0], ranked[1] if len(ranked) > 1 else 0
            flags, d_app = 0, best_d
            if not (best >= min_score and best >= 2 * second):
                flags |= WEAK
                d_app = 0
            if w > 0 and abs(best_d) == w:
                flags |= EDGE
            if d_app != 0:
                flags |= SHIFTED
            out['shift'][f, c], out['flags'][f, c] = d_app, flags
            out['score'][f, c] = [best, second, sc[0], len(pts)]
            out['scores'][f, (2 * win[0] + 1 if c else 0):(2 * win[0] + 1 if c else 0) + 2 * w + 1] = [sc[d] for d in range(-w, w + 1)]
            for j, d in enumerate((d_app, 0)):
                r, s = res[d]
                if len(r):
                    out['rms'][f, c, j] = math.sqrt(float((r * r).mean()))
                    scale = max(scale, float(s.max()))
            out['idx'][f, :c_, c] = (I[f, :c_, c].astype(np.int64) + d_app).astype(np.int32)     # (wraps like the kernel's sum)
    out.update(margin=margin, rms_tol=64 * EPS * scale)
    return out


# ------------------------------------------------------------------------------------------------------ cases
def _shift(frames, shifts):
    """copies of the frames with (d0, d1) added to the indices of frame i"""
    out = []
    for fr, s in zip(frames, shifts):
        out.append(dict(fr, idx=(fr['idx'] + np.asarray(s, np.int32)).astype(np.int32)))
    return out


def _plain(frames):
    return [dict(X=f['X'], idx=f['idx']) for f in frames]


def table_of_model(x, lo, hi):
    """cpe_projector_model_table of a model x[15] of proj_model_cases: dict(P, status, lo, hi), every line OK"""
    v = np.arange(lo, hi + 1)
    nrm = np.stack([np.stack([PC._orient_big(n) for n in M.normals(np.asarray(x, np.float64), k, v)[0]]) for k in range(2)])
    return TC.table_from_normals(nrm, np.asarray(x[:3], np.float64), lo, hi)


@functools.lru_cache(maxsize=None)
def model_table(seed):
    """the table -16..16 of the reference's projector model (tau = 1) of shifted_frames(seed): what the pipeline searches against"""
    X, I, cnt = PC.pack(M.shifted_frames(seed))
    ref = M.ref_projector_model(X, I, cnt, -12, 12, tau=M.TAU)
    assert ref['status'] == 0
    return table_of_model(ref['x'], -16, 16)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(frames, table[, use, win, tau, min_score, swap])"""
    rig = TC.rig_table(-16, 16)
    cy = _plain(M.cylinder_frames(0))
    sh = M.shifted_frames(0)
    mp = _plain(PC.multi_pose(0))
    c = {}
    for seed in (0, 1, 2):
        c[f'shifted model table {seed}'] = dict(frames=M.shifted_frames(seed), table=model_table(seed))
    c['shifted rig table'] = dict(frames=sh, table=rig)
    c['shifted noisy table'] = dict(frames=sh, table=dict(TC.noisy_table(0)))
    for tau in (0.5, 2.0):
        c[f'shifted tau {tau}'] = dict(frames=sh, table=rig, tau=tau)
    # batches of 1, 3, 65; shifts of +-1 and +-3 in either or both families
    moves = [(-1, 0), (3, -3), (0, 1), (-3, 0), (1, 1), (0, -3), (3, 3), (0, 0)]
    c['one frame'] = dict(frames=_shift(cy[:1], [(0, -1)]), table=rig)
    three = _shift(cy[:3], moves[:3])
    c['three frames'] = dict(frames=three, table=rig)
    c['eight shifts'] = dict(frames=_shift(cy[:8], moves), table=rig)
    small = _plain(PC.multi_pose(7, 65, 0.25, 2, 3))             # 65 boards of 9 x 9 points
    c['65 frames'] = dict(frames=_shift(small, [(i % 7 - 3, i % 5 - 2) for i in range(65)]), table=rig)
    # windows; (1, 1) puts the shift of 1 on the border (EDGE) and the shifts of 3 outside
    for win in ((0, 0), (1, 1), (8, 8), (2, 5)):
        c[f'window {win[0]} {win[1]}'] = dict(frames=three, table=rig, win=win)
    # counts -1, 0, 1, 63, 64, 65 on one board numbered a column up; 2048 and 3000 on a near board of 46 x 46 indices
    order = np.random.default_rng(5).permutation(len(mp[3]['X']))
    sub = lambda k, **kw: dict(X=mp[3]['X'][order][:k], idx=mp[3]['idx'][order][:k] + np.array([1, 0], np.int32), **kw)
    c['counts'] = dict(frames=[sub(10, cnt=-1), sub(10, cnt=0), sub(1), sub(63), sub(64), sub(65)], table=rig)
    big = []
    for i, (tx, ty, z) in enumerate(((-9.0, 14.0, 190.0), (11.0, -8.0, 205.0))):
        bi, bX, _ = PC.board_table(*PC.board(tx, ty, z), cols=range(-20, 26), rows=range(-10, 36), seed=11 + i)
        big.append(dict(X=bX[:MAXP], idx=(bi[:MAXP] + np.array([0, -1 - i], np.int32)).astype(np.int32), cnt=(MAXP, 3000)[i]))
    c['counts 2048 3000'] = dict(frames=big, table=TC.rig_table(-24, 40), tau=0.25)
    # L = 1: only the 25 points of the one line can count; L = 256
    c['L 1'] = dict(frames=_shift(cy[:2], [(0, 0), (-2, 0)]), table=TC.rig_table(2, 2))
    c['L 256'] = dict(frames=three, table=TC.rig_table(-128, 127))
    # NaN / Inf coordinates and a use mask
    nanf = dict(X=three[1]['X'].copy(), idx=three[1]['idx'])
    nanf['X'][::17, 2] = np.nan
    nanf['X'][5::29, 0] = np.inf
    c['nan points'] = dict(frames=[three[0], nanf, three[2]], table=rig)
    use = (np.random.default_rng(9).random((3, MAXP)) < 0.7).astype(np.uint8)
    use[2] = 0
    c['use'] = dict(frames=three, table=rig, use=use)
    # garbage indices: INT32_MIN, INT32_MAX and the values next to [lo - win, hi + win] on either side, in a frame that is shifted
    g = dict(X=three[0]['X'], idx=three[0]['idx'].copy())
    g['idx'][0] = [-2 ** 31, 2 ** 31 - 1]
    g['idx'][1] = [2 ** 31 - 1, -2 ** 31]
    g['idx'][2] = [-21, 21]
    g['idx'][3] = [21, -21]
    g['idx'][4] = [-20, 20]
    g['idx'][5] = [20, -20]
    c['garbage indices'] = dict(frames=[g, three[1]], table=rig)
    # refused lines: some of the winner's; all of the winner's (the columns 5 and 6, numbered one up, need the lines 5 and 6)
    c['refused lines'] = dict(frames=three, table=TC.with_status(rig, (3, 7), (-4, 7)))
    two = (cy[0]['idx'][:, 0] >= 5) & (cy[0]['idx'][:, 0] <= 6)
    c['winner refused'] = dict(frames=_shift([dict(X=cy[0]['X'][two], idx=cy[0]['idx'][two])], [(1, 0)]), table=TC.with_status(rig, (5, 6)))
    # the families exchanged in the table, and swap
    c['transposed swap 1'] = dict(frames=three, table=TC.transposed(rig), swap=1)
    c['swap 1'] = dict(frames=three, table=rig, swap=1)
    # WEAK: by min_score; by the lead rule with a band that takes in the neighbouring planes
    c['min_score 226'] = dict(frames=three, table=rig, min_score=226)
    c['min_score 0 empty'] = dict(frames=[dict(X=cy[0]['X'], idx=cy[0]['idx'], cnt=0)], table=rig, min_score=0)
    for tau in (3.0, 4.5, 6.0):
        c[f'wide band {tau}'] = dict(frames=three, table=rig, tau=tau)
    # a frame in parts: the first a points numbered d_a columns off, the next b points d_b columns off.  100 + 100: an exact tie
    # (with 0 in it, 0 wins; between -1 and +1, -1 wins and is not trusted); 120 + 80: a lead below 2; 120 + 60: a lead of exactly 2
    def parts(a, da, b, db):
        idx = cy[0]['idx'][:a + b].copy()
        idx[:a, 0] += da
        idx[a:, 0] += db
        return dict(X=cy[0]['X'][:a + b], idx=idx)
    c['ties and leads'] = dict(frames=[parts(100, 1, 100, 0), parts(100, 1, 100, -1), parts(120, 1, 80, 0), parts(120, 1, 60, 0),
                                       parts(100, -2, 100, 2)], table=rig)
    return c


def params(case):
    return {k: case.get(k, d) for k, d in DEFAULTS.items()}


def arrays(case, poison=None):
    X, I, cnt = PC.pack(case['frames'], poison)
    return X, I, cnt, case.get('use')


@functools.lru_cache(maxsize=None)
def reference(name):
    case = cases()[name]
    X, I, cnt, use = arrays(case)
    t = case['table']
    return ref_index_shift(X, I, cnt, t['P'], t['status'], t['lo'], t['hi'], use, **params(case))
