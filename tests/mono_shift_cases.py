"""Cases and numpy references for the grid-index shift of one-camera frames (include/cpe.h cpe_mono_shift_batch; DESIGN.md
section 3.7) and for the repaired one-camera fit built on it (cpe_amd.fit.fit_single_cylinder_mono_repaired_batch).  The rig, the
tables and the cylinder frame are those of tests/table_tri_cases.py, the scenarios those of tests/grid_predict_cases.py.

ref_mono_shift restates the numbered rule of the header in float64 numpy, one frame at a time, every operation written out in
the header's order (no dot products of a library: a sum of three products is (a0 b0 + a1 b1) + a2 b2 on both sides).  Beside the
outputs of the call it reports

    margin    the smallest relative distance of a decision from its gate over every usable point and every candidate whose two
              planes are usable: | max(|res0|, |res1|) / tau - 1 |, den against min_sin^2 and s against 0 (|sum a b| / sum |a b|,
              as tests/table_tri_cases.py measures it).  While it is far above the rounding of a residual (a few eps (|X| + |P4|)
              / tau, about 1e-12) kernel and reference count the same points, and scores, cand, cand_score, score, flags and the
              order are compared exactly.  Cases are generated so that every margin is above 1e-6
              (tests/test_mono_shift_cases_cpu.py asserts it);
    rms_tol   (2 m + 18) eps rms per entry, m the counting points of that candidate.  rms = sqrt(S / m), S the sum of the 2 m
              squares res0^2 + res1^2.  A square carries twice its residual's relative error (allowed: 16 eps) and its own
              rounding; a sum of 2 m non-negative terms, added in ANY order (the kernel adds a pair, then per lane, then by a
              butterfly; numpy pairwise), is within (2 m - 1) eps of the exact sum, relatively.  So either side's S is within
              (2 m + 16) eps of the exact one, the two differ by at most twice that, the root halves it, and the division and the
              root add a rounding each.  (The derivation of tests/grid_predict_cases.py for its stats[0], with 2 m terms for m.)

The chain (ref_repair_chain below) restates fit_single_cylinder_mono_repaired_batch with the references alone:
ref_mono_shift -> per candidate table_tri_cases.ref_table_triangulate(need_both, max_res) and oracle.fit_cylinder(mode=1) -> the
eligibility and rms rules -> per round grid_predict_cases.ref_grid_predict, ref_grid_assign, ref_table_triangulate and the fit.

Measured with this chain and the oracle's LM (mode 1) on table_tri_cases.cylinder_frame(0.25,
seed), seeds 0..4, 424 points, both cameras, on rig_table(-16, 16) and noisy_table(seed), window 4, tau 0.1 mm, max_res 0.25 mm,
one round; scenarios of grid_predict_cases.scenario applied to the one image, plus `frame_shift`: every index numbered (+2, -1)
off, and `frame_shift_w8`: the same searched with window 8 on rig_table(-24, 24), where the epipolar alias of the true shift lies
inside the window.  MONO_REPAIR_BOUNDS are twice the worst seed's axis error of the last round, either table, the practice of
grid_predict_cases.REFINE_BOUNDS.

tests/test_mono_shift_cases_cpu.py measures these again, prints them and holds them to the figures of MEASURED below: per
scenario and table the fewest points kept after the round, the worst axis error of the last round in degrees and mm, and the smallest ratio of the runner-up's fit rms to the chosen
candidate's where two candidates were eligible (None: one was)

  scenario         table   first fit     shift step                                round 1                       axis, worst seed
  off_by_one       either  382 points    (0, 0): 382 votes, no other eligible      418-423 kept, 40-42 re-numb.  0.0915 deg, 0.0450 mm
  column_shift     either  249 points    (0, 0) 249 and (-1, 0) 175 votes, fit     418-423 kept, 175 re-numb.    0.0915 deg, 0.0450 mm
                                         rms 0.14-0.15 and 0.16-0.18 mm: ratio
                                         1.001-1.171 < 1.5, so WEAK and (0, 0)
  third_missing    either  283 points    (0, 0): 283 votes                         278-283 kept                  0.1043 deg, 0.0553 mm
  frame_shift      either  0 points      (-2, 1): 424 votes; (3, -1) 91-147,       418-423 kept                  0.0915 deg, 0.0450 mm
                                         not eligible
  frame_shift_w8   rig     0 points      (-2, 1) 424 votes, rms 0.150-0.169 mm;    418-423 kept                  0.0915 deg, 0.0437 mm
                                         the alias, (-7, 3) for camera 1 with
                                         310-329 votes and (5, 4) for camera 2
                                         with 423-424: rms 0.409-0.539 mm,
                                         ratio 2.498-3.426 against the gate 1.5

No kept point carries a wrong index in any of the 90 runs.  NOT covered, and a limit of the rule (README): frame_shift_w8 on
noisy_table(seed), whose lines end at +-12, so that the alias (-7, 3) keeps only the 276 points of a strip 100 mm nearer to the
camera: it gets 210-224 votes, fits with 0.087-0.110 mm against the true shift's 0.153-0.166 mm, and where it is eligible
(camera 1, seeds 1-4; 213-224 >= 212 votes) the rms rule trusts it.  The window must stay inside what the table covers."""
import functools
import math

import numpy as np

import grid_predict_cases as GC
import plane_fit_cases as PC
import table_tri_cases as TC

MAXP, MAXL, EPS, ST_OK = PC.MAXP, PC.MAXL, PC.EPS, PC.ST_OK
MAX_WIN, MAX_TOP_K = 8, 8
SHIFTED, WEAK, EDGE = 1, 2, 4
RADIUS = TC.RADIUS
DEFAULTS = dict(win=(4, 4), tau=0.1, min_sin=0.01, min_score=8, swap=0, top_k=4)
INT_KEYS = ('scores', 'cand', 'cand_score', 'score', 'flags')


# ------------------------------------------------------------------------------------------------------ the reference
def _dot3(n, v):
    return (n[..., 0] * v[..., 0] + n[..., 1] * v[..., 1]) + n[..., 2] * v[..., 2]


def ref_mono_shift(xy, ids, cnt, K, Tc, P, status, lo, hi, win=(4, 4), tau=0.1, min_sin=0.01, min_score=8, swap=0, top_k=4):
    """one frame.  xy (>=cnt,2), ids (>=cnt,2), K (3,3), Tc (4,4) or None, P (2,L,4), status (2,L) -> dict(scores (C,), cand
    (top_k,2), cand_score (top_k,), score (4,), rms (2,), flags, rms_tol (2,), counting (2,): the points behind either rms, margin)"""
    n = min(max(int(cnt), 0), MAXP)
    xy = np.asarray(xy, np.float64).reshape(-1, 2)[:n]
    ids = np.asarray(ids).reshape(-1, 2)[:n].astype(np.int64)
    K = np.asarray(K, np.float64).reshape(3, 3)
    T = np.eye(4) if Tc is None else np.asarray(Tc, np.float64).reshape(4, 4)
    R, t = T[:3, :3], T[:3, 3]
    P, status = np.asarray(P, np.float64), np.asarray(status)
    L = hi - lo + 1
    assert P.shape == (2, L, 4) and status.shape == (2, L)
    o = np.array([-((R[0, a] * t[0] + R[1, a] * t[1]) + R[2, a] * t[2]) for a in range(3)])
    fin = np.isfinite(xy).all(1)
    near = fin.copy()
    for c in (0, 1):
        near &= (ids[:, c] >= lo - win[c]) & (ids[:, c] <= hi + win[c])          # before any addition
    x, y, iv = xy[near, 0], xy[near, 1], ids[near]
    m = len(x)
    margin = math.inf
    cands = [(d0, d1) for d0 in range(-win[0], win[0] + 1) for d1 in range(-win[1], win[1] + 1)]
    sc, sq = {}, {}
    with np.errstate(all='ignore'):
        vy = (y - K[1, 2]) / K[1, 1]
        vx = ((x - K[0, 2]) - K[0, 1] * vy) / K[0, 0]
        d = np.stack([(R[0, a] * vx + R[1, a] * vy) + R[2, a] for a in range(3)], 1).reshape(m, 3)
        d = d / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])[:, None]
        side = [{}, {}]                                                           # per component and d_c: usable, plane, a, b
        for c in (0, 1):
            fam = c ^ swap
            for dc in range(-win[c], win[c] + 1):
                v = iv[:, c] + dc
                use = (v >= lo) & (v <= hi)
                line = np.where(use, v - lo, 0)
                use &= status[fam, line] == ST_OK
                pl = P[fam, line]
                side[c][dc] = (use, pl, _dot3(pl, d), _dot3(pl, o[None, :]) + pl[:, 3])
        for d0, d1 in cands:
            (u0, p0, a0, b0), (u1, p1, a1, b1) = side[0][d0], side[1][d1]
            both = u0 & u1
            den = a0 * a0 + a1 * a1
            if min_sin > 0:
                margin = GC._min_margin(margin, np.abs(den / (min_sin * min_sin) - 1), both)
            ok = both & (den >= min_sin * min_sin) & np.isfinite(den)
            sab = a0 * b0 + a1 * b1
            s = -sab / den
            margin = GC._min_margin(margin, np.abs(sab) / (np.abs(a0 * b0) + np.abs(a1 * b1)), ok & np.isfinite(s))
            ok &= (s > 0) & np.isfinite(s)
            X = o[None, :] + s[:, None] * d
            r0, r1 = _dot3(p0, X) + p0[:, 3], _dot3(p1, X) + p1[:, 3]
            margin = GC._min_margin(margin, np.abs(np.maximum(np.abs(r0), np.abs(r1)) / tau - 1), ok)
            hit = ok & (np.abs(r0) < tau) & (np.abs(r1) < tau)
            sc[d0, d1] = int(hit.sum())
            sq[d0, d1] = float((r0[hit] * r0[hit] + r1[hit] * r1[hit]).sum())
    order = sorted(cands, key=lambda q: (-sc[q], abs(q[0]) + abs(q[1]), abs(q[0]), q[0], q[1]))
    best_d = order[0]
    best, second = sc[best_d], sc[order[1]] if len(order) > 1 else 0
    cand, cand_score = np.zeros((top_k, 2), np.int32), np.full(top_k, -1, np.int32)
    for k, q in enumerate(order[:top_k]):
        cand[k], cand_score[k] = q, sc[q]
    flags = 0
    if any(win[c] > 0 and abs(best_d[c]) == win[c] for c in (0, 1)):
        flags |= EDGE
    if best < min_score or best < 2 * second:
        flags |= WEAK
    counting = np.array([sc[best_d], sc[0, 0]])
    rms = np.array([math.sqrt(sq[q] / sc[q]) if sc[q] else 0.0 for q in (best_d, (0, 0))])
    return dict(scores=np.array([sc[q] for q in cands], np.int32), cand=cand, cand_score=cand_score,
                score=np.array([best, second, sc[0, 0], int(fin.sum())], np.int32), rms=rms, flags=np.int32(flags),
                rms_tol=(2 * counting + 18) * EPS * rms, counting=counting, margin=margin)


def compare_frame(got, ref, what=''):
    """got: dict(scores, cand, cand_score, score, rms, flags) of one frame against ref_mono_shift's -> the rms error over its
    tolerance (0 when both are 0)"""
    for k in INT_KEYS:
        assert np.array_equal(np.asarray(got[k]), ref[k]), f'{what}: {k}\n{np.asarray(got[k])}\n{ref[k]}'
    g = np.asarray(got['rms'], np.float64)
    assert np.isfinite(g).all(), f'{what}: rms not finite'
    e = np.abs(g - ref['rms'])
    assert (e <= ref['rms_tol']).all(), f'{what}: rms {g} != {ref["rms"]} within {ref["rms_tol"]}'
    return float(np.max(e / np.where(ref['rms_tol'] > 0, ref['rms_tol'], 1.0)))


# ------------------------------------------------------------------------------------------------------ cases
LO, HI = TC.LO, TC.HI
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def _frame(cam=1, seed=0, shift=(0, 0), keep=None):
    """the cylinder frame of the seed as camera `cam` sees it with id = true index - shift, so that `shift` is what the search has to
    find; keep: the slots kept, in that order"""
    idx, _, uv1, uv2 = TC.cylinder_frame(0.25, seed)
    uv = uv1 if cam == 1 else uv2
    keep = np.arange(len(idx)) if keep is None else keep
    return dict(xy=uv[keep], id=(idx[keep] - np.asarray(shift, np.int32)).astype(np.int32))


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(frames: list of dict(xy, id[, cnt]), cam, table, params): one call each.  Counts -1, 0, 1, 63, 64, 65 and 2048;
    windows (0, 0), (0, 4), (4, 0), (4, 4), (8, 8); both cameras; a transposed table with swap; refused lines; indices INT32_MIN /
    INT32_MAX and just outside [lo - win, hi + win]; NaN / inf pixels; a winner on the window's edge; tau 0.5, where the alias ties
    the winner for camera 1; a natural frame; min_score 0 with an empty frame; batches of 1, 3 and 65; top_k 1 and 8"""
    rig, main = TC.rig_table(LO, HI), TC.main_table()
    idx = TC.cylinder_frame(0.25, 0)[0]
    order = np.random.default_rng(5).permutation(len(idx))
    c = {}
    c['natural'] = dict(frames=[_frame()], cam=1, table=rig, params={})
    counts = [dict(_frame(shift=(1, -2), keep=order[:k])) for k in (1, 63, 64, 65)]
    counts += [dict(_frame(keep=order[:10]), cnt=-1), dict(_frame(keep=order[:10]), cnt=0)]
    c['counts'] = dict(frames=counts, cam=1, table=rig, params=dict(min_score=0))
    big = TC.frame_cases()['count 2048']
    c['count 2048'] = dict(frames=[dict(xy=big['xy'], id=(big['id'] - np.int32([0, 1])).astype(np.int32)),
                                   dict(xy=big['xy'], id=big['id'], cnt=3000)], cam=1, table=rig, params={})
    for w in ((0, 0), (0, 4), (4, 0), (4, 4), (8, 8)):
        c[f'window {w}'] = dict(frames=[_frame(shift=(0, 0)), _frame(shift=(0, 3)), _frame(shift=(-2, 0))], cam=1, table=rig,
                                params=dict(win=w))
    c['camera 2'] = dict(frames=[_frame(2), _frame(2, 1, (2, -1)), _frame(2, 2, (-1, 1), order[:70])], cam=2, table=main, params={})
    c['transposed swap 1'] = dict(frames=[_frame(shift=(2, -1)), _frame(1, 3, (0, 1))], cam=1, table=TC.transposed(main),
                                  params=dict(swap=1))
    c['refused lines'] = dict(frames=[_frame(shift=(1, 0)), _frame(shift=(0, -1)), _frame()], cam=1, table=main, params={})
    wild = _frame(shift=(1, 1))
    wid = wild['id'].copy()
    wid[0] = [INT_MIN, 0]; wid[1] = [0, INT_MAX]; wid[2] = [INT_MAX, INT_MIN]; wid[3, 0] = LO - 5; wid[4, 1] = HI + 5
    wid[5, 0] = LO - 4; wid[6, 1] = HI + 4; wid[70] = [INT_MAX - 3, INT_MAX]; wid[130] = [INT_MIN + 2, 7]
    c['wild indices'] = dict(frames=[dict(xy=wild['xy'], id=wid)], cam=1, table=rig, params={})
    nx = _frame(shift=(-1, 0))
    nxy = nx['xy'].copy()
    nxy[5, 0] = np.nan; nxy[63, 1] = np.inf; nxy[64] = -np.inf; nxy[139, 1] = np.nan; nxy[200, 0] = 1e300
    c['nan pixels'] = dict(frames=[dict(xy=nxy, id=nx['id'])], cam=1, table=rig, params={})
    c['edge winner'] = dict(frames=[_frame(shift=(4, 0)), _frame(shift=(1, -4)), _frame(shift=(-2, 2)), _frame(shift=(5, 0))], cam=1,
                            table=rig, params={})
    third = np.sort(np.random.default_rng(8000).permutation(len(idx))[:len(idx) - len(idx) // 3])
    c['alias ties at tau 0.5'] = dict(frames=[_frame(shift=(2, -1), keep=third)], cam=1, table=rig, params=dict(tau=0.5))
    c['alias loses at tau 0.1'] = dict(frames=[_frame(shift=(2, -1), keep=third)], cam=1, table=rig, params={})
    c['empty frame, min_score 0'] = dict(frames=[dict(xy=np.zeros((0, 2)), id=np.zeros((0, 2), np.int32)), _frame()], cam=1, table=rig,
                                         params=dict(min_score=0))
    c['empty frame, min_score 8'] = dict(c['empty frame, min_score 0'], params={})
    c['top_k 1'] = dict(frames=[_frame(shift=(2, -1)), _frame()], cam=1, table=rig, params=dict(top_k=1))
    c['top_k 8'] = dict(frames=[_frame(shift=(2, -1)), _frame()], cam=1, table=rig, params=dict(top_k=8))
    c['top_k 8, window (0, 1)'] = dict(frames=[_frame(shift=(0, 1)), _frame()], cam=1, table=rig, params=dict(top_k=8, win=(0, 1)))
    c['noisy table'] = dict(frames=[_frame(1, 0, (1, 1)), _frame(1, 0)], cam=1, table=TC.noisy_table(0), params={})
    c['L 1'] = dict(frames=[_frame()], cam=1, table=TC.rig_table(0, 0), params=dict(min_score=0))
    c['L 256'] = dict(frames=[_frame(shift=(0, 2))], cam=1, table=TC.rig_table(-128, 127), params={})
    pool = [_frame(1, s, sh, kp) for s, sh, kp in ((0, (0, 0), None), (1, (1, 0), None), (2, (0, -2), order[:200]), (3, (3, 3), None),
                                                   (4, (-4, 1), order[:65]), (0, (0, 0), order[:0]), (1, (-1, -1), order[:64]))]
    c['one frame'] = dict(frames=pool[1:2], cam=1, table=rig, params={})
    c['three frames'] = dict(frames=pool[2:5], cam=1, table=rig, params={})
    c['65 frames'] = dict(frames=[pool[i % len(pool)] for i in range(65)], cam=1, table=rig, params={})
    return c


def params(case):
    return dict(DEFAULTS, **case['params'])


def arrays(case, poison=None):
    """-> xy f64[n,MAXP,2], id i32[n,MAXP,2], cnt i32[n] (table_tri_cases.pack: poison fills the slots past every frame's points)"""
    return TC.pack(case['frames'], poison)


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> list of ref_mono_shift results, one per frame of the call (equal frames of a batch share one)"""
    case = cases()[name]
    K, Tc = TC.camera(case['cam'])
    t = case['table']
    done, out = {}, []
    for f in case['frames']:
        if id(f) not in done:
            done[id(f)] = ref_mono_shift(f['xy'], f['id'], f.get('cnt', len(f['xy'])), K, Tc, t['P'], t['status'], t['lo'], t['hi'],
                                         **params(case))
        out.append(done[id(f)])
    return out


# name -> (table range or None for the main one, keywords of the call): every one is CPE_ERR_ARG
REFUSED_CALLS = {
    'win 9, 0': (None, dict(win=(9, 0))), 'win 0, 9': (None, dict(win=(0, 9))), 'win -1': (None, dict(win=(-1, 4))),
    'tau 0': (None, dict(tau=0.0)), 'tau < 0': (None, dict(tau=-0.1)), 'tau nan': (None, dict(tau=float('nan'))),
    'top_k 0': (None, dict(top_k=0)), 'top_k 9': (None, dict(top_k=9)), 'min_score -1': (None, dict(min_score=-1)),
    'min_sin -1': (None, dict(min_sin=-1.0)), 'swap 2': (None, dict(swap=2)), 'L 257': ((0, 256), {}), 'L 0': ((3, 2), {}),
}


# ------------------------------------------------------------------------------------------------------ the repair chain
SCENARIOS = GC.SCENARIOS + ('frame_shift',)
FRAME_SHIFT = (2, -1)


@functools.lru_cache(maxsize=None)
def scenario(name, seed, cam):
    """-> dict(gp (m,4) [x y col row] of camera `cam` as the detector would hand it over, true (m,2) the true indices, shift: the
    frame-wide shift the search has to find).  The scenarios of grid_predict_cases act on the one image (column_shift is its
    right image's, so it is applied to whichever camera is asked for); frame_shift numbers the whole frame FRAME_SHIFT off"""
    if name.startswith('frame_shift'):
        idx, _, uv1, uv2 = TC.cylinder_frame(0.25, seed)
        uv = uv1 if cam == 1 else uv2
        return dict(gp=np.concatenate([uv, idx + np.asarray(FRAME_SHIFT)], 1), true=idx, shift=(-FRAME_SHIFT[0], -FRAME_SHIFT[1]))
    s = GC.scenario(name, seed)
    if name == 'column_shift':
        gp = s['gp2'].copy()
        if cam == 1:
            gp[:, :2] = TC.cylinder_frame(0.25, seed)[2]
        return dict(gp=gp, true=s['true2'], shift=(0, 0))
    return dict(gp=s[f'gp{cam}'], true=s[f'true{cam}'], shift=(0, 0))


def chain_table(which, seed, lo=LO, hi=HI):
    return TC.rig_table(lo, hi) if which == 'rig' else TC.noisy_table(seed)


def _solve(xy, ids, K, Tc, table, max_res, radius, mode):
    import oracle
    tri = TC.ref_table_triangulate(xy, ids, len(xy), K, Tc, table['P'], table['status'], table['lo'], table['hi'], need_both=1,
                                   max_res=max_res)
    out = dict(tri=tri, status=PC.ST_FEW_POINTS, cyl=None, rms=math.inf, margin=tri['margin'])
    if tri['m'] >= 5:
        fit = oracle.fit_cylinder(tri['X'], radius, mode=mode)
        out.update(status=fit['status'], cyl=oracle.apply_prior(fit['cyl'], tri['X']))
        if fit['status'] == ST_OK and np.isfinite(fit['fvals'][1]):
            out['rms'] = math.sqrt(fit['fvals'][1] / tri['m'])
    return out


def ref_repair_chain(gp, cam, table, shift=None, rounds=1, max_res=0.25, vote_frac=0.5, rms_ratio=1.5, tau_px=4.0, ratio=0.5,
                     image_size=None, radius=RADIUS, mode=1, cams=None, centre=None):
    """fit_single_cylinder_mono_repaired_batch on one frame with the references alone -> dict(shift, flags, trusted, vote (the
    ref_mono_shift result or None), cand_rms, eligible, first, cur (the solve the frame ended with), ids (the indices behind it),
    src (their slots in gp), rounds: list of dict(assign, solve, taken), round_taken, renumbered, margin)"""
    import oracle
    oracle.build()
    K1, K2, T21 = PC.rig()[:3] if cams is None else cams
    centre = PC.rig()[5] if centre is None else centre
    K, Tc = (K1, None) if cam == 1 else (K2, T21)
    xy, ids = np.ascontiguousarray(gp[:, :2]), gp[:, 2:].astype(np.int32)
    first = _solve(xy, ids, K, Tc, table, max_res, radius, mode)
    out = dict(first=first, vote=None, shift=(0, 0), flags=0, trusted=True, cand_rms=None, eligible=None, margin=first['margin'])
    cur = first
    if shift is not None:
        prm = dict(DEFAULTS, **shift)
        prm.pop('swap')
        vote = ref_mono_shift(xy, ids, len(xy), K, Tc, table['P'], table['status'], table['lo'], table['hi'], **prm)
        sols = [_solve(xy, ids + vote['cand'][k], K, Tc, table, max_res, radius, mode) for k in range(prm['top_k'])]
        need = max(float(prm['min_score']), vote_frac * float(vote['score'][0]))
        rms = np.array([s['rms'] for s in sols])
        eligible = (vote['cand_score'] >= need) & np.isfinite(rms)
        ranked = sorted(np.nonzero(eligible)[0], key=lambda k: (rms[k], k))
        trusted = len(ranked) == 1 or (len(ranked) >= 2 and rms_ratio * rms[ranked[0]] <= rms[ranked[1]])
        applied = tuple(int(v) for v in vote['cand'][ranked[0]]) if trusted else (0, 0)
        if trusted:
            cur = sols[ranked[0]]
        flags = (0 if trusted else WEAK) | (SHIFTED if applied != (0, 0) else 0)
        if any(prm['win'][c] > 0 and abs(applied[c]) == prm['win'][c] for c in (0, 1)):
            flags |= EDGE
        # how far the rms decision is from its gate, and every candidate's own gates
        gate = math.inf
        if len(ranked) >= 2:
            gate = abs(rms_ratio * rms[ranked[0]] / rms[ranked[1]] - 1)
        out.update(vote=vote, shift=applied, flags=flags, trusted=trusted, cand_rms=rms, eligible=eligible, rms_gate=gate,
                   ratio=rms[ranked[1]] / rms[ranked[0]] if len(ranked) >= 2 else math.inf,
                   margin=min([out['margin'], vote['margin']] + [s['margin'] for s in sols]))
    ids = (ids + np.asarray(out['shift'], np.int32)).astype(np.int32)
    cur_ids, cur_src = ids[cur['tri']['src'][:, 1]], cur['tri']['src'][:, 1]
    iw, ih = (0, 0) if image_size is None else (image_size[1], image_size[0])
    out.update(rounds=[], round_taken=0, renumbered=0)
    for r in range(1, rounds + 1):
        if cur['status'] != ST_OK:
            break
        pr = GC.ref_grid_predict(cur['cyl'], True, radius, K1, K2, T21, table['P'], table['status'], table['lo'], table['hi'], centre,
                                 img_w=iw, img_h=ih)
        a = GC.ref_grid_assign(xy, ids, len(xy), pr['px'][cam - 1], pr['vis'], cam - 1, (table['lo'], table['lo']), pr['Nu'], pr['Nv'],
                               tau_px, ratio)
        new = _solve(a['xy'], a['id'], K, Tc, table, max_res, radius, mode)
        taken = new['status'] == ST_OK
        out['rounds'].append(dict(assign=a, solve=new, taken=taken))
        out['margin'] = min(out['margin'], new['margin'], a['margin'], pr['margin'])
        if taken:
            cur, out['round_taken'], out['renumbered'] = new, r, int(a['counts'][2])
            cur_ids, cur_src = a['id'][new['tri']['src'][:, 1]], a['src'][new['tri']['src'][:, 1]]
    out.update(cur=cur, ids=cur_ids, src=cur_src)
    return out


@functools.lru_cache(maxsize=None)
def chain_reference(name, seed, cam, which):
    """the chain on scenario(name, seed, cam) with the table `which` ('rig' / 'noisy'), window 4 (frame_shift_w8: window 8 on
    rig_table(-24, 24), the noisy table as it is), one round"""
    s = scenario(name, seed, cam)
    if name == 'frame_shift_w8':
        return ref_repair_chain(s['gp'], cam, chain_table(which, seed, -24, 24), shift=dict(win=(8, 8)), rounds=1)
    return ref_repair_chain(s['gp'], cam, chain_table(which, seed), shift={}, rounds=1)


def chain_errors(r, true):
    """-> dict(kept, wrong: kept points whose index is not the true one, axis_deg, axis_mm)"""
    deg, mm = TC.axis_errors(r['cur']['cyl']) if r['cur']['cyl'] is not None else (math.inf, math.inf)
    return dict(kept=len(r['ids']), wrong=int((r['ids'] != true[r['src']]).any(1).sum()), axis_deg=deg, axis_mm=mm)


# the figures of the module docstring's table
MEASURED = {
    ('off_by_one', 'rig'): dict(kept=418, axis_deg=0.0915, axis_mm=0.0437, ratio=None),
    ('off_by_one', 'noisy'): dict(kept=418, axis_deg=0.0832, axis_mm=0.0450, ratio=None),
    ('column_shift', 'rig'): dict(kept=418, axis_deg=0.0915, axis_mm=0.0437, ratio=1.001),
    ('column_shift', 'noisy'): dict(kept=418, axis_deg=0.0832, axis_mm=0.0450, ratio=1.006),
    ('third_missing', 'rig'): dict(kept=278, axis_deg=0.1043, axis_mm=0.0553, ratio=None),
    ('third_missing', 'noisy'): dict(kept=278, axis_deg=0.0974, axis_mm=0.0532, ratio=None),
    ('frame_shift', 'rig'): dict(kept=418, axis_deg=0.0915, axis_mm=0.0437, ratio=None),
    ('frame_shift', 'noisy'): dict(kept=418, axis_deg=0.0832, axis_mm=0.0450, ratio=None),
    ('frame_shift_w8', 'rig'): dict(kept=418, axis_deg=0.0915, axis_mm=0.0437, ratio=2.498),
}
# twice the worst seed's axis error of the last round, either camera, either table (the practice of grid_predict_cases.REFINE_BOUNDS)
MONO_REPAIR_BOUNDS = {name: dict(axis_deg=2 * max(v['axis_deg'] for (n_, _), v in MEASURED.items() if n_ == name),
                                 axis_mm=2 * max(v['axis_mm'] for (n_, _), v in MEASURED.items() if n_ == name))
                      for name in SCENARIOS + ('frame_shift_w8',)}
# what the chain decides per scenario: the shift step's choice is trusted, or SHIFT_WEAK with the frame's own indices kept
TRUSTED = dict(off_by_one=True, column_shift=False, third_missing=True, frame_shift=True, frame_shift_w8=True)
