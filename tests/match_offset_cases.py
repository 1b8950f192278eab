"""Cases and a Python reference for the index-shift search (include/cpe.h cpe_match_offset_batch).

The reference restates the rule of the header from what the oracle already exports -- find_correspondences, triangulate,
fit_cylinder(mode=1, maxiter=hyp_iters), dist_pts3_to_line -- so the kernel is compared at tolerance 0.

Cases: ground-truth tables of cpe_amd.synth (no rendering) with seeded 0.25 px noise, the right table's indices shifted by a
known amount; and hand-made tables (a lattice on a cylinder projected through the same rig) at the counts and index ranges
where the kernels take another path: empty tables, 4 / 5 kept pairs (CPE_FIT_MIN_POINTS), 63 / 64 / 65 points (the wave
tail), 256 / 257 and 1024 / 1025 points (the LDS size classes of the scoring kernel), a full 2048-point table, a count
above CPE_MAXP, duplicate indices, a window of 0, a table-2 span of 127 / 128, an index beyond +-9999, garbage."""
import functools

import numpy as np

MAXP = 2048
TBL = 128
FIT_MIN_POINTS = 5
SHIFTED, WEAK, EDGE, OVERFLOW = 1, 2, 4, 8
DEFAULTS = dict(win_c=4, win_r=4, th=0.3, tau=0.5, hyp_iters=8, min_score=8)
R = 45.0


# ------------------------------------------------------------------------------------------------------ the reference
def candidates(win_c, win_r):
    """dc the outer index, dr the inner, both ascending"""
    return [(dc, dr) for dc in range(-win_c, win_c + 1) for dr in range(-win_r, win_r + 1)]


def pick_winner(cands, scores):
    """index of the smallest key (-score, |dc|+|dr|, |dc|, dc, dr)"""
    return min(range(len(cands)), key=lambda k: (-scores[k], abs(cands[k][0]) + abs(cands[k][1]), abs(cands[k][0]), cands[k][0], cands[k][1]))


def score_candidate(orc, a, b, dc, dr, K1, K2, T21, radius, th, tau, hyp_iters):
    """-> (score, pairs kept) of one candidate; a, b: (N,4) [x y col row]"""
    s = a.copy()
    s[:, 2] += dc
    s[:, 3] += dr
    c1, c2, _ = orc.find_correspondences(s, b)
    if len(c1) == 0:
        return 0, 0
    X, err = orc.triangulate(c1, c2, K1, K2, T21)
    P = np.ascontiguousarray(X[err < th])
    if len(P) < FIT_MIN_POINTS:
        return 0, len(P)
    fit = orc.fit_cylinder(P, radius, tolx=1e-5, tolf=1e-5, maxiter=hyp_iters, mode=1)
    if fit['status'] != 0:
        return 0, len(P)
    x = fit['cyl']
    d = orc.dist_pts3_to_line(P, x[:3], x[:3] + x[3:])
    return int((np.abs(d - radius) < tau).sum()), len(P)


def reference(orc, t1, cnt1, t2, cnt2, K1, K2, T21, radius=R, win_c=4, win_r=4, th=0.3, tau=0.5, hyp_iters=8, min_score=8):
    """one frame -> dict(offset (2,), score (4,), scores (ncand,), flags, id1_out (n1,2)); counts are clamped to [0, MAXP]"""
    n1, n2 = min(max(int(cnt1), 0), MAXP), min(max(int(cnt2), 0), MAXP)
    a = np.asarray(t1, np.float64).reshape(-1, 4)[:n1]
    b = np.asarray(t2, np.float64).reshape(-1, 4)[:n2]
    cands = candidates(win_c, win_r)
    scores, kept = np.zeros(len(cands), np.int32), np.zeros(len(cands), np.int32)
    overflow = False
    if n1 > 0 and n2 > 0:
        span = b[:, 2:4].max(0) - b[:, 2:4].min(0)
        ids = np.concatenate([a[:, 2:4], b[:, 2:4]])
        overflow = bool((span >= TBL).any() or ids.min() < -9999 or ids.max() > 9999)
        if not overflow:
            for k, (dc, dr) in enumerate(cands):
                scores[k], kept[k] = score_candidate(orc, a, b, dc, dr, K1, K2, T21, radius, th, tau, hyp_iters)
    w = pick_winner(cands, scores)
    wdc, wdr = cands[w]
    flags, off = 0, (wdc, wdr)
    if overflow:
        flags |= OVERFLOW
    if scores[w] < min_score:
        flags |= WEAK
        off = (0, 0)
    if (win_c > 0 and abs(wdc) == win_c) or (win_r > 0 and abs(wdr) == win_r):
        flags |= EDGE
    if off != (0, 0):
        flags |= SHIFTED
    rest = np.delete(scores, w)
    return dict(offset=np.array(off, np.int32),
                score=np.array([scores[w], rest.max() if len(rest) else 0, scores[cands.index((0, 0))], kept[w]], np.int32),
                scores=scores, flags=flags, id1_out=a[:, 2:4].astype(np.int32) + np.array(off, np.int32))


# ------------------------------------------------------------------------------------------------------------- tables
@functools.lru_cache(maxsize=None)
def rig(h, w):
    from cpe_amd import synth
    scene = synth.Scene(h=h, w=w)
    K1, K2, T21, Tp = synth.make_rig(scene)
    return scene, K1, K2, T21, Tp


def gt_tables(h, w, seed, frame, shift, noise=0.25):
    """tables of frame `frame` of the seed's scene parameters from synth.ground_truth: pixel noise on both sides, the right
    table's indices moved by `shift` (so `shift` is what has to be added to the left table)"""
    from cpe_amd import synth
    scene, K1, K2, T21, Tp = rig(h, w)
    fp = synth._frame_params(scene, frame + 1, seed)
    gt = synth.ground_truth(scene, K1, K2, T21, Tp, fp, scene.pitch_px / scene.focal)[frame]
    rng = np.random.default_rng(7919 * seed + 131 * frame + 17)
    t1 = np.concatenate([gt['uv1'] + noise * rng.standard_normal(gt['uv1'].shape), gt['idx']], 1)
    t2 = np.concatenate([gt['uv2'] + noise * rng.standard_normal(gt['uv2'].shape), gt['idx'] + np.array(shift)], 1)
    return t1, t2


def lattice_tables(nc, nr, seed=0, noise=0.0, n=None, shift=(0, 0)):
    """nc x nr points on a cylinder of radius R in front of the 640x480 rig, index (col,row) = lattice position, projected
    into both cameras (tables only: nothing has to be visible); the first n in a seeded order"""
    _, K1, K2, T21, _ = rig(480, 640)
    rng = np.random.default_rng(seed)
    ang = np.linspace(-0.9, 0.9, nc) + np.pi
    yy = (np.arange(nr) - (nr - 1) / 2) * (120.0 / max(nr - 1, 1))
    A, Y = np.meshgrid(ang, yy, indexing='ij')
    C, Rw = np.meshgrid(np.arange(nc), np.arange(nr), indexing='ij')
    X = np.stack([27.0 + R * np.sin(A.ravel()), Y.ravel(), 365.0 + R * np.cos(A.ravel())], 1)
    X2 = X @ T21[:3, :3].T + T21[:3, 3]
    p1 = X @ K1.T
    p2 = X2 @ K2.T
    uv1, uv2 = p1[:, :2] / p1[:, 2:3], p2[:, :2] / p2[:, 2:3]
    idx = np.stack([C.ravel(), Rw.ravel()], 1).astype(np.float64)
    order = rng.permutation(len(X))[:n]
    t1 = np.concatenate([uv1 + noise * rng.standard_normal(uv1.shape), idx], 1)[order]
    t2 = np.concatenate([uv2 + noise * rng.standard_normal(uv2.shape), idx + np.array(shift)], 1)[order]
    return t1, t2


def _case(name, t1, t2, size=(480, 640), cnt1=None, cnt2=None, expect_offset=None, expect_flags=None, **params):
    return dict(name=name, t1=t1, t2=t2, size=size, cnt1=len(t1) if cnt1 is None else cnt1, cnt2=len(t2) if cnt2 is None else cnt2,
                expect_offset=expect_offset, expect_flags=expect_flags, params=dict(DEFAULTS, **params))


SHIFTS = [(0, 0), (1, 0), (-2, 1), (0, -3), (4, 4), (-4, 2)]


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    # ground-truth tables, the right table shifted: the shift has to come back, SHIFTED exactly when it is not (0,0); a shift
    # with a component of 4 lies on the border of the default window, which is what EDGE says
    for k, s in enumerate(SHIFTS):
        t1, t2 = gt_tables(480, 640, seed=k % 2 * 3, frame=k, shift=s)
        fl = (SHIFTED if s != (0, 0) else 0) | (EDGE if 4 in (abs(s[0]), abs(s[1])) else 0)
        out.append(_case(f'gt640_shift{s[0]}_{s[1]}', t1, t2, expect_offset=s, expect_flags=fl))
    t1, t2 = gt_tables(1200, 1920, seed=11, frame=0, shift=(-2, 1))
    out.append(_case('gt1920_shift-2_1', t1, t2, size=(1200, 1920), expect_offset=(-2, 1), expect_flags=SHIFTED))
    # the true shift outside the window: whatever wins, the flags say that the window was too small
    t1, t2 = gt_tables(480, 640, seed=0, frame=1, shift=(5, 0))
    out.append(_case('gt640_shift5_0_window4', t1, t2, expect_flags='edge'))
    # hand-made
    e = np.zeros((0, 4))
    t1, t2 = lattice_tables(6, 8, seed=1)
    out.append(_case('empty_left', e, t2, expect_offset=(0, 0), expect_flags=WEAK))
    out.append(_case('empty_right', t1, e, expect_offset=(0, 0), expect_flags=WEAK))
    out.append(_case('empty_both', e, e, expect_offset=(0, 0), expect_flags=WEAK))
    out.append(_case('negative_count', t1, t2, cnt1=-3, expect_offset=(0, 0), expect_flags=WEAK))
    for n in (4, 5):          # noise-free, so every pair is kept: 4 is below CPE_FIT_MIN_POINTS, 5 is fitted
        a, b = lattice_tables(6, 8, seed=2, n=n)
        out.append(_case(f'kept{n}', a, b, expect_offset=(0, 0), expect_flags=WEAK))
    for n in (63, 64, 65, 256, 257, 1024, 1025):
        a, b = lattice_tables(30, 40, seed=n, noise=0.1, n=n, shift=(1, -1))
        out.append(_case(f'lattice{n}', a, b, expect_offset=(1, -1), expect_flags=SHIFTED))
    a, b = lattice_tables(32, 64, seed=5, noise=0.1, shift=(-1, 0))
    out.append(_case('full2048', a, b, expect_offset=(-1, 0), expect_flags=SHIFTED, win_c=2, win_r=1))
    out.append(_case('count_above_maxp', a, b, cnt1=3000, cnt2=MAXP + 1, expect_offset=(-1, 0), expect_flags=SHIFTED | EDGE, win_c=1,
                     win_r=1))
    # duplicates: rows of table 2 repeated behind the originals with other pixels (never looked up), rows of table 1
    # repeated (each finds the same partner: more pairs than table 2 has points)
    a, b = lattice_tables(7, 9, seed=6, noise=0.1, shift=(0, 2))
    b2 = np.concatenate([b, b[:20] + np.array([3.0, -2.0, 0, 0])])
    a2 = np.concatenate([a, a[5:40], a[5:40]])
    out.append(_case('duplicates', a2, b2, expect_offset=(0, 2), expect_flags=SHIFTED))
    a, b = lattice_tables(8, 10, seed=7, noise=0.1)
    out.append(_case('window0', a, b, expect_offset=(0, 0), expect_flags=0, win_c=0, win_r=0))
    out.append(_case('window0_shifted_tables', *lattice_tables(8, 10, seed=7, noise=0.1, shift=(1, 0)), expect_offset=(0, 0), expect_flags=WEAK,
                     win_c=0, win_r=0))
    out.append(_case('window_c_only', *lattice_tables(8, 10, seed=8, noise=0.1, shift=(3, 0)), expect_offset=(3, 0), expect_flags=SHIFTED | EDGE,
                     win_c=3, win_r=0))
    # the dense table of image 2: a span of 127 fits, 128 does not; an index beyond +-9999 in either table does not
    for span, fl in ((127, 0), (128, OVERFLOW | WEAK)):
        far = b[:1].copy()
        far[0, 2] = b[:, 2].min() + span
        out.append(_case(f'span{span}', a, np.concatenate([b, far]), expect_offset=(0, 0), expect_flags=fl))
        far = b[:1].copy()
        far[0, 3] = b[:, 3].max() - span
        out.append(_case(f'span{span}_rows', a, np.concatenate([b, far]), expect_offset=(0, 0), expect_flags=fl))
    far = a[:1].copy()
    far[0, 2] = a[:, 2].min() + 300         # table 1 alone may span anything: its far point finds no partner
    out.append(_case('span300_left_only', np.concatenate([a, far]), b, expect_offset=(0, 0), expect_flags=0))
    for side in (0, 1):
        for v in (10000, -10000):
            far = (a, b)[side][:1].copy()
            far[0, 3] = v
            tabs = [a, b]
            tabs[side] = np.concatenate([tabs[side], far])
            out.append(_case(f'index{v}_table{side + 1}', tabs[0], tabs[1], expect_offset=(0, 0), expect_flags=OVERFLOW | WEAK))
    far = b[:1].copy()
    far[0, 2] = 9999
    out.append(_case('index9999_left_only', np.concatenate([a, far]), b, expect_offset=(0, 0), expect_flags=0))
    # garbage: 10 points with random pixels under the indices of a 2 x 5 block
    rng = np.random.default_rng(99)
    ids = np.stack(np.meshgrid(np.arange(2), np.arange(5), indexing='ij'), -1).reshape(-1, 2).astype(np.float64)
    g1 = np.concatenate([rng.uniform(50, 590, (10, 1)), rng.uniform(50, 430, (10, 1)), ids], 1)
    g2 = np.concatenate([rng.uniform(50, 590, (10, 1)), rng.uniform(50, 430, (10, 1)), ids], 1)
    out.append(_case('garbage10', g1, g2, expect_offset=(0, 0), expect_flags='weak'))
    return out


def case_rig(case):
    _, K1, K2, T21, _ = rig(*case['size'])
    return K1, K2, T21


@functools.lru_cache(maxsize=None)
def references():
    """name -> reference result, computed once per process"""
    import oracle
    oracle.build()
    out = {}
    for c in cases():
        K1, K2, T21 = case_rig(c)
        out[c['name']] = reference(oracle, c['t1'], c['cnt1'], c['t2'], c['cnt2'], K1, K2, T21, R, **c['params'])
    return out


def pack(group, poison=True):
    """cases -> xy1, id1, cnt1, xy2, id2, cnt2 numpy arrays; slots past a table's rows are NaN pixels and 9999 / -9999
    indices (poison) or zero"""
    n = len(group)
    arrs = []
    for t, ck in (('t1', 'cnt1'), ('t2', 'cnt2')):
        xy = np.full((n, MAXP, 2), np.nan if poison else 0.0)
        ids = np.full((n, MAXP, 2), 9999 if poison else 0, np.int32)
        if poison:
            ids[:, :, 1] = -9999
        cnt = np.zeros(n, np.int32)
        for i, c in enumerate(group):
            m = min(len(c[t]), MAXP)
            xy[i, :m] = c[t][:m, :2]
            ids[i, :m] = c[t][:m, 2:4].astype(np.int32)
            cnt[i] = c[ck]
        arrs += [xy, ids, cnt]
    return arrs
