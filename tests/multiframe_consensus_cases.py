"""The consensus over frames in front of the multi-frame LM fit (include/cpe.h cpe_multi_frame_consensus_batch, DESIGN.md
section 3.7), restated in numpy on top of multiframe_lm_cases -- Problem, initial_pose on the two-frame sub-problem, lm -- with the
scenes and the case table of its tests.

Nothing here is bit-exact with the kernels (multiframe_lm_cases says why), so every DECISION the rule takes has to be far from
its threshold for a case to be comparable at all.  ref_consensus returns two margins:

    inlier_margin  the smallest |sqrt(term) / tau - 1| over every inlier decision taken: every kept frame with a point at every
                   hypothesis that is not void (the winner's x0 among them) and at every x_r
    key_gap        (sum of the runner-up - sum of the winner) / sum of the winner, the runner-up being the next key with the
                   winner's inlier count (inf without one)

test_multiframe_consensus_cpu.py requires inlier_margin > 1e-3 and key_gap > 1e-6 of every case: the terms of the restatement and
of the kernels agree to about 1e-12 relative.  A case that misses is replaced, not excused."""
import math

import numpy as np

import multiframe_cases as mc
import multiframe_lm_cases as lc

RADIUS = mc.RADIUS
MAXF = 1024
MAX_HYP = 4096
ST_OK, ST_FEW, ST_OVERFLOW = 0, 5, 6
CONVERGED, SHRUNK = 1, 2
DEFAULTS = dict(tau=0.5, max_hyp=2048, max_rounds=4, min_inliers=3)

# Twice the worst errors of ref_consensus against Ttrue over make_scene(24, seed, 0.1, npts=200), seeds 0-9, 3 and 8 frames
# displaced (test_multiframe_consensus_cpu.py::test_reference_rejects_the_displaced_frames prints them; per-frame fits by
# oracle.fit_cylinder(mode=1)): MEASURED_WORST.  The practice of plane_fit_cases.NOISY_BOUNDS.
MEASURED_WORST = dict(rot_deg=0.0096, tr_mm=0.0433)     # 0.009595 deg (8 displaced, seed 0), 0.043275 mm (8 displaced, seed 6)
NOISY_CONSENSUS_BOUNDS = dict(rot_deg=2 * MEASURED_WORST['rot_deg'], tr_mm=2 * MEASURED_WORST['tr_mm'])


# ------------------------------------------------------------------------------------------------------------ the pairs
def plan(u, max_hyp):
    """-> R offsets per frame, H hypotheses, dense (every unordered pair occurs) for u >= 2 usable frames"""
    R = max(1, max_hyp // u)
    dense = R >= u // 2
    if dense:
        R = u // 2
    return R, min(R * u, max_hyp), dense


def pairs(u, max_hyp):
    """hypothesis h -> (a, b, first): places in the usable list; first False = the pair occurred before as (b, a) (the offset
    u/2 of an even u), the hypothesis is void"""
    R, H, dense = plan(u, max_hyp)
    out = []
    for h in range(H):
        k, a = divmod(h, u)
        off = 1 + k if dense else 1 + ((2 * k + 1) * (u // 2 - 1)) // (2 * R)
        out.append((a, (a + off) % u, not (2 * off == u and a >= off)))
    return out


# ------------------------------------------------------------------------------------------------------- the reference
def key_before(k1, k2):
    """keys (count, sum, h): more inliers first, then the smaller sum, then the smaller h"""
    if k1[0] != k2[0]:
        return k1[0] > k2[0]
    if k1[1] != k2[1]:
        return k1[1] < k2[1]
    return k1[2] < k2[2]


def ref_consensus(P, cnt, TAGV, raw, keep=None, tau=0.5, max_hyp=2048, max_rounds=4, min_inliers=3, radius=RADIUS, tolx=1e-5,
                  tolf=1e-5, maxiter=100000):
    """the rule of cpe_multi_frame_consensus_batch for ONE group: the frames with keep != 0 (None: all).  -> dict(status, and with
    status 0: x0, x, T, fvals, iters [iterations, evaluations], n_used, n_inliers, info [h, frame, frame, rounds], flags,
    inlier i32[F] (-1: not kept), frame_terms f64[F] (NaN: not kept), fitted (frames x was fitted to), inlier_margin, key_gap)"""
    F = len(cnt)
    cnt = np.minimum(np.maximum(np.asarray(cnt), 0), mc.MAXP)
    TAGV = np.asarray(TAGV, dtype=np.float64).reshape(F, 16)
    kept = [f for f in range(F) if keep is None or keep[f]]
    m = len(kept)
    fail = lambda st, **kw: dict(dict(status=st, n_used=0, n_inliers=0, info=[0, 0, 0, 0], flags=0, inlier_margin=math.inf,
                                      key_gap=math.inf), **kw)
    if m > MAXF:
        return fail(ST_OVERFLOW)
    if m < 2:
        return fail(ST_FEW)
    K = np.array(kept)
    usable = [kept[i] for i in lc.usable_frames(cnt[K], raw[K])]
    u = len(usable)
    if u < 2:
        return fail(ST_FEW)
    live = np.array([k for k in range(m) if cnt[kept[k]] >= 1])      # kept places with a point: the others have the term 0
    full = lc.Problem(P[K[live]], cnt[K[live]], TAGV[K[live]], radius)
    tau2 = tau * tau

    def terms_at(x):
        t = np.zeros(m)
        t[live] = full.frame_terms(x)
        return t

    def inliers(t):
        return [k for k in live.tolist() if t[k] < tau2]

    def ordered_sum(t, places):
        v = 0.0
        for k in places:
            v = v + float(t[k])
        return v

    def margin(t):
        return float(np.nanmin(np.abs(np.sqrt(t[live]) / tau - 1)))       # (a term that is not finite is no inlier by any margin)

    hyps = []                                                        # (key, x, terms) of the hypotheses that are not void
    for h, (a, b, first) in enumerate(pairs(u, max_hyp)):
        if not first:
            continue
        two = [usable[a], usable[b]]
        pair = lc.Problem(P[two], cnt[two], TAGV[two], radius)
        x = lc.initial_pose(pair, raw[two])
        if x is None or not (np.isfinite(x).all() and np.isfinite(pair.f(x))):
            continue
        t = terms_at(x)
        S = inliers(t)
        hyps.append(((len(S), ordered_sum(t, S), h), x, t))
    if not hyps:
        return fail(ST_FEW)
    best = hyps[0]
    for c in hyps[1:]:
        if key_before(c[0], best[0]):
            best = c
    (count, s0, h), x0, t = best
    rivals = sorted(c[0][1] for c in hyps if c[0][0] == count and c[0][2] != h)
    key_gap = (rivals[0] - s0) / s0 if rivals and s0 > 0 else math.inf
    inlier_margin = min(margin(c[2]) for c in hyps)
    if count < min_inliers:
        return fail(ST_FEW, inlier_margin=inlier_margin, best_count=count)
    S = inliers(t)
    x, fx, fitted = np.array(x0), s0, S
    iters = evals = rounds = flags = 0
    for r in range(1, max_rounds + 1):
        sub = [kept[k] for k in S]
        x, fx, it, ev = lc.lm(lc.Problem(P[sub], cnt[sub], TAGV[sub], radius), x, tolx, tolf, maxiter)
        iters, evals, rounds, fitted = iters + it, evals + ev, r, S
        t = terms_at(x)
        inlier_margin = min(inlier_margin, margin(t))
        Sn = inliers(t)
        if Sn == S:
            flags |= CONVERGED
            break
        if len(Sn) < min_inliers:
            flags |= SHRUNK
            break
        S = Sn
    inl = np.full(F, -1, np.int32)
    inl[K] = 0
    inl[[kept[k] for k in fitted]] = 1
    ft = np.full(F, np.nan)
    ft[K] = t
    a, b, _ = pairs(u, max_hyp)[h]
    return dict(status=ST_OK, x0=np.array(x0), x=np.array(x), T=lc.vec2T(x), fvals=[s0, fx], iters=[iters, evals], n_used=m,
                n_inliers=len(fitted), info=[h, usable[a], usable[b], rounds], flags=flags, inlier=inl, frame_terms=ft,
                fitted=[kept[k] for k in fitted], inlier_margin=inlier_margin, key_gap=key_gap)


# -------------------------------------------------------------------------------------------------------------- scenes
def displace(P, cnt, frames, rng):
    """-> a copy of P in which every frame of `frames` is a perfect cylinder of the right radius in the wrong place: its points
    rotated by 5-30 degrees about a random axis through their centroid and shifted by up to 30 mm per component"""
    P = P.copy()
    for f in frames:
        n = int(cnt[f])
        axis = rng.standard_normal(3)
        w = axis / np.linalg.norm(axis) * math.radians(rng.uniform(5.0, 30.0))
        shift = rng.uniform(-30.0, 30.0, 3)
        c = P[f, :n].mean(0)
        P[f, :n] = (P[f, :n] - c) @ lc.rot_exp(w).T + c + shift
    return P


def displaced_scene(F, seed, n_bad, noise=0.1, npts=200, start=0):
    """make_scene with n_bad frames displaced; frame choice, rotations and shifts from default_rng(100 + seed).
    -> P, cnt, angles, Ttrue, the displaced frames (ascending)"""
    P, cnt, angles, Ttrue = mc.make_scene(F, seed, noise, start=start, npts=npts)
    rng = np.random.default_rng(100 + seed)
    bad = sorted(rng.choice(F, n_bad, replace=False).tolist()) if n_bad else []
    return displace(P, cnt, bad, rng), cnt, angles, Ttrue, bad


def per_frame_fits(orc, P, cnt):
    """[cylParams0; cylParams] of every frame with a point by the oracle's LM (fit_cylinder(mode=1)); zero rows for the others"""
    raw = np.zeros((len(cnt), 2, 6))
    for i in range(len(cnt)):
        if cnt[i] >= 1:
            r = orc.fit_cylinder(P[i, :cnt[i]], RADIUS, mode=1)
            raw[i, 0], raw[i, 1] = r['cyl0'], r['cyl']
    return raw


# The case table.  F frames of make_scene(F, seed, noise 0.1) with `bad` of them displaced; npts None = the points per frame cycle
# through COUNT_CYCLE from `start`; cons = the options that differ from DEFAULTS.  expect: 'bad' (default) = status 0 and exactly the
# displaced frames (and those named by `also_out`) rejected; 'few' = CPE_ST_FEW_POINTS.  edit = what is done to the tables after
# the per-frame fits (see build()).
CASES = {
    # groups of 2, 3, 4, 5 kept frames
    'F2': dict(F=2, seed=3, bad=0, npts=None, start=4, cons=dict(min_inliers=2)),
    'F3_1bad_min3': dict(F=3, seed=1, bad=1, npts=None, start=1, expect='few'),
    'F3_1bad_min2': dict(F=3, seed=1, bad=1, npts=None, start=1, cons=dict(min_inliers=2)),
    'F4_1bad': dict(F=4, seed=0, bad=1, npts=None, start=2),
    'F5_1bad': dict(F=5, seed=2, bad=1, npts=None, start=1),
    # 24 frames of 200 points, the scenes NOISY_CONSENSUS_BOUNDS were measured on; rounds 0, 1, 4
    'F24_clean': dict(F=24, seed=0, bad=0, npts=200),
    'F24_3bad': dict(F=24, seed=1, bad=3, npts=200),
    'F24_3bad_r0': dict(F=24, seed=1, bad=3, npts=200, cons=dict(max_rounds=0)),
    'F24_3bad_r1': dict(F=24, seed=1, bad=3, npts=200, cons=dict(max_rounds=1)),
    'F24_8bad': dict(F=24, seed=2, bad=8, npts=200),
    'F24_clean_h1': dict(F=24, seed=0, bad=0, npts=200, cons=dict(max_hyp=1)),
    'F24_8bad_h23': dict(F=24, seed=2, bad=8, npts=200, cons=dict(max_hyp=23)),
    'F24_8bad_h24': dict(F=24, seed=2, bad=8, npts=200, cons=dict(max_hyp=24)),
    'F12_all_bad': dict(F=12, seed=0, bad=12, npts=64, expect='few'),
    # the experiment's size with every pair (990 hypotheses), all point counts of COUNT_CYCLE
    'F45_5bad': dict(F=45, seed=22, bad=5, npts=None, start=0),
    # more usable frames than hypotheses: spread offsets
    'F65_10bad_h65': dict(F=65, seed=5, bad=10, npts=None, start=3, cons=dict(max_hyp=65)),
    'F65_30bad_h130': dict(F=65, seed=6, bad=30, npts=64, cons=dict(max_hyp=130)),
    'F130_30bad_h130': dict(F=130, seed=12, bad=30, npts=63, cons=dict(max_hyp=130)),
    'F130_30bad_h129': dict(F=130, seed=12, bad=30, npts=63, cons=dict(max_hyp=129)),
    # kept but unusable: a frame without points (never an inlier), a NaN row and a zero direction (inliers all the same)
    'F9_unusable': dict(F=9, seed=8, bad=2, npts=65, edit='unusable', also_out=[4]),
    # frame_ok holes: frames 0, 5 and 11 are not kept
    'F14_holes': dict(F=14, seed=9, bad=3, npts=160, edit='holes'),
    # a tight tau: the two-frame pose x0 leaves one good frame just outside, the refit on the other seven takes it in, and the
    # second round returns its list (rounds = 2)
    'two_rounds': dict(F=10, seed=53, bad=2, npts=65, cons=dict(tau=0.115)),
}


def build(name, orc):
    """-> dict(P, cnt, angles, TAGV, raw, keep (None or i32[F]), Ttrue, bad, cons (all four options), expect, ref)"""
    c = CASES[name]
    P, cnt, angles, Ttrue, bad = displaced_scene(c['F'], c['seed'], c['bad'], npts=c.get('npts'), start=c.get('start', 0),
                                                 noise=c.get('noise', 0.1))
    keep = None
    if c.get('edit') == 'unusable':
        cnt = cnt.copy()
        cnt[4] = 0
    raw = per_frame_fits(orc, P, cnt)
    if c.get('edit') == 'unusable':
        raw[1, 1, 2] = np.nan
        raw[6, 1, 3:] = 0.0
    if c.get('edit') == 'holes':
        keep = np.ones(c['F'], np.int32)
        keep[[0, 5, 11]] = 0
    TAGV = np.stack([mc.get_TAGVcyl(*a).ravel() for a in angles])
    cons = dict(DEFAULTS, **c.get('cons', {}))
    ref = ref_consensus(P, cnt, TAGV, raw, keep, **cons)
    out = [f for f in sorted(set(bad) | set(c.get('also_out', []))) if keep is None or keep[f]]
    return dict(name=name, P=P, cnt=cnt, angles=angles, TAGV=TAGV, raw=raw, keep=keep, Ttrue=Ttrue, bad=bad, out=out, cons=cons,
                expect=c.get('expect', 'bad'), ref=ref)


def pose_errors(T, Ttrue):
    """-> rotation error in degrees, translation error in the unit of the points"""
    T = np.asarray(T).reshape(4, 4)
    return lc.rotation_error_deg(T, Ttrue), float(np.linalg.norm(T[:3, 3] - Ttrue[:3, 3]))
