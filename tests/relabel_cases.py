"""Cases and a numpy reference for the per-image re-labelling of the planar target's grid lines (include/cpe.h
cpe_grid_relabel_batch).

ref_grid_relabel restates the header's numbered rule in float64, one image and one id component at a time, every sum taken
sequentially in slot order as the header says.  Beside the outputs of the call it reports

    tol       per image and component, for the positions p and for pitch: the largest over the lines that have a position of
              64 eps N S (1 + sum|t - tm| |t_centre - tm| / Stt), S = max |xy| + |center| of the image.  The means are sums of N
              terms bounded by S (relative error N eps); the slope Stu / Stt carries the errors of the centred coordinates, each
              a few eps S, weighted by |t - tm| / Stt, and is multiplied by the lever t_centre - tm.  pitch is a difference of
              two positions (or the mean of two such differences): 2 tol;
    margin    the smallest relative distance of any decision from its threshold: two neighbouring positions of the sorted
              lists (gap / max |p|), a neighbour's gap against merge_frac pitch0, g / pitch against the rounding boundary
              k + 1/2 that decides inc, and the two nearest anchor candidates ((d2 - d1) / d2).  While it is far above tol / pitch
              the kernel and the reference take the same decisions and every integer output can be compared exactly.

Cases are generated so that every margin is > 1e-6 and every tol <= 1e-6 px (tests/test_relabel_cases_cpu.py asserts both).

Board cases are analytic (plane_fit_cases.board / board_hits / project_pair: rays of the rig's projector cut with a board of up
to 30 deg tilt, projected into camera 1 or 2 with 0.25 px noise); their true indices are then hidden behind the label patterns
measured on the detector (module docstring of tests/test_relabel_cases_cpu.py).  Lattice cases are synthetic grids of a given
pitch with a shear and noise, for the sizes no board reaches: 256 lines per component, 2048 points, labels at the ends of int32.
ids are (row, col) as the planar detector writes them: component 0 is positioned in y (swap 0)."""
import functools
import math

import numpy as np

import plane_fit_cases as PC

MAXP, MAXL = PC.MAXP, PC.MAXL
EPS = PC.EPS
NO_CENTRE, OVERFLOW, FEW_LINES = 1, 2, 4
KEPT, UNSUPPORTED, PHANTOM = 0, 1, 2
MAX_INC = 1 << 20
DEFAULTS = dict(swap=0, min_pts=3, merge_frac=0.65, dir=(1, 1))
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
DROPPED = 10 ** 6      # the `true` index of a point that the rule must drop (a phantom, a fragment, a non-finite pixel)


def _mid(sorted_vals):
    m = len(sorted_vals)
    return (sorted_vals[(m - 1) // 2] + sorted_vals[m // 2]) / np.float64(2.0)


def ref_grid_relabel(xy, ids, cnt, center, swap=0, min_pts=3, merge_frac=0.65, dir=(1, 1)):
    """-> dict(xy, id, cnt, src: the compacted tables (zeros from cnt on), label, index, points, state (n,2,MAXL) and p: the line
    table (zeros from counts[..., 0] on), pitch (n,2), counts (n,2,4), flags (n,), tol (n,2), margin)"""
    xy = np.asarray(xy, np.float64).reshape(-1, MAXP, 2)
    ids = np.asarray(ids, np.int32).reshape(-1, MAXP, 2)
    cnt = np.asarray(cnt).reshape(-1)
    center = np.asarray(center, np.float64).reshape(-1, 2)
    n = len(cnt)
    out = dict(xy=np.zeros((n, MAXP, 2)), id=np.zeros((n, MAXP, 2), np.int32), cnt=np.zeros(n, np.int32), src=np.zeros((n, MAXP), np.int32),
               label=np.zeros((n, 2, MAXL), np.int32), index=np.zeros((n, 2, MAXL), np.int32), points=np.zeros((n, 2, MAXL), np.int32),
               state=np.zeros((n, 2, MAXL), np.int32), p=np.zeros((n, 2, MAXL)), pitch=np.zeros((n, 2)),
               counts=np.zeros((n, 2, 4), np.int32), flags=np.zeros(n, np.int32), tol=np.zeros((n, 2)))
    margin = math.inf
    with np.errstate(all='ignore'):
        for f in range(n):
            c_ = min(max(int(cnt[f]), 0), MAXP)
            slots = np.nonzero(np.isfinite(xy[f, :c_]).all(1))[0]                                   # rule 1
            flags = 0 if np.isfinite(center[f]).all() else NO_CENTRE
            for c in range(2):                                                                      # rule 2
                lab = ids[f, slots, c].astype(np.int64)
                if len(lab) and int(lab.max()) - int(lab.min()) >= MAXL:
                    flags |= OVERFLOW
            if flags:
                out['flags'][f] = flags
                continue
            S = (np.abs(xy[f, slots]).max() if len(slots) else 0.0) + np.abs(center[f]).max()
            new_of = []                                                                             # per component: label -> new index
            for c in range(2):
                iu = 1 if (c ^ swap) == 0 else 0
                it = 1 - iu
                tc, uc = center[f, it], center[f, iu]
                lab = ids[f, slots, c].astype(np.int64)
                labels = sorted(set(lab.tolist()))
                P, N_, sup = [], [], []
                for L in labels:                                                                    # rule 3
                    sl = slots[lab == L]
                    N = len(sl)
                    st = su = np.float64(0.0)
                    for k in sl:
                        st = st + xy[f, k, it]; su = su + xy[f, k, iu]
                    tm, um = st / np.float64(N), su / np.float64(N)
                    Stt = Stu = np.float64(0.0)
                    for k in sl:
                        dt, du = xy[f, k, it] - tm, xy[f, k, iu] - um
                        Stt = Stt + dt * dt; Stu = Stu + dt * du
                    p = um + (Stu / Stt) * (tc - tm)
                    has_p = bool(Stt > 0.0) and bool(np.isfinite(p))
                    P.append(p if has_p else np.float64(0.0)); N_.append(N); sup.append(has_p and N >= min_pts)
                    if has_p:
                        lever = np.abs(xy[f, sl, it] - tm).sum() * abs(tc - tm) / Stt
                        out['tol'][f, c] = max(out['tol'][f, c], 64 * EPS * N * S * (1.0 + lever))
                nl = len(labels)
                state = [KEPT if s else UNSUPPORTED for s in sup]
                index = [0] * nl
                order = sorted((i for i in range(nl) if sup[i]), key=lambda i: (P[i], labels[i]))   # rule 4
                ns = len(order)
                gaps = [P[order[i + 1]] - P[order[i]] for i in range(ns - 1)]
                for i, g in enumerate(gaps):
                    margin = min(margin, float(g / max(abs(P[order[i]]), abs(P[order[i + 1]]), 1.0)))
                pitch0 = _mid(sorted(gaps)) if gaps else np.float64(0.0)
                thr = np.float64(merge_frac) * pitch0
                if thr > 0:
                    for g in gaps:
                        margin = min(margin, float(abs(g - thr) / thr))
                rem = []
                for i, ls in enumerate(order):                                                      # rule 5
                    ph = (i > 0 and gaps[i - 1] < thr and N_[order[i - 1]] >= N_[ls]) or \
                         (i < ns - 1 and gaps[i] < thr and N_[order[i + 1]] > N_[ls])
                    if ph:
                        state[ls] = PHANTOM
                    else:
                        rem.append(ls)
                nr = len(rem)
                if nr:
                    g2 = [P[rem[i + 1]] - P[rem[i]] for i in range(nr - 1)]                        # rule 6
                    ng = len(g2)
                    med_all = _mid(sorted(g2)) if g2 else np.float64(0.0)
                    pre = [0]
                    for i, g in enumerate(g2):
                        v = sorted(g2[k] for k in (i - 2, i - 1, i + 1, i + 2) if 0 <= k < ng)
                        pi = med_all if len(v) < 2 else _mid(v)
                        inc = 1
                        if pi > 0.0:
                            q = g / pi
                            r = np.floor(q + np.float64(0.5))
                            if r >= MAX_INC:
                                inc = MAX_INC
                            elif r > 1.0:
                                inc = int(r)
                            if np.isfinite(q):
                                b = max(inc, 1) + 0.5                                               # the boundaries around q
                                margin = min(margin, float(min(abs(q - b) / b, abs(q - (b - 1.0)) / (b - 1.0) if b > 1.5 else math.inf)))
                        pre.append(pre[-1] + inc)
                    d = [abs(P[ls] - uc) for ls in rem]                                             # rule 7
                    a = min(range(nr), key=lambda i: (d[i], i))
                    if nr > 1:
                        d2 = sorted(d)
                        margin = min(margin, float((d2[1] - d2[0]) / d2[1]) if d2[1] > 0 else 0.0)
                    for i, ls in enumerate(rem):
                        index[ls] = int(dir[c]) * (pre[i] - pre[a])
                else:
                    out['flags'][f] |= FEW_LINES << c
                out['label'][f, c, :nl] = np.asarray(labels, np.int64).astype(np.int32)
                out['index'][f, c, :nl], out['points'][f, c, :nl], out['state'][f, c, :nl] = index, N_, state
                out['p'][f, c, :nl] = P
                out['pitch'][f, c] = pitch0
                out['counts'][f, c] = nl, ns, ns - nr, nr
                new_of.append({L: (index[i], state[i]) for i, L in enumerate(labels)})
            m = 0
            for k in slots:                                                                          # rule 8
                (i0, s0), (i1, s1) = new_of[0][int(ids[f, k, 0])], new_of[1][int(ids[f, k, 1])]
                if s0 == KEPT and s1 == KEPT:
                    out['xy'][f, m], out['id'][f, m], out['src'][f, m] = xy[f, k], (i0, i1), k
                    m += 1
            out['cnt'][f] = m
    out['margin'] = margin
    return out


# ------------------------------------------------------------------------------------------------------ tables
def pack(tables, counts=None, poison=None):
    """tables: list of (m,4) [x y id0 id1] -> xy f64[n,MAXP,2], id i32[n,MAXP,2], cnt i32[n] (counts: the declared counts, default
    m).  Slots from min(m, MAXP) on hold zeros, or with poison=seed NaN / Inf / huge pixels and garbage labels"""
    n = len(tables)
    xy, ids, cnt = np.zeros((n, MAXP, 2)), np.zeros((n, MAXP, 2), np.int32), np.zeros(n, np.int32)
    if poison is not None:
        rng = np.random.default_rng(poison)
        xy[:] = rng.choice([np.nan, np.inf, -1e300, 1e9, 12.5], size=xy.shape)
        ids[:] = rng.choice([0, 1, I32_MIN, I32_MAX, 3], size=ids.shape)
    for f, t in enumerate(tables):
        t = np.asarray(t, np.float64).reshape(-1, 4)[:MAXP]
        xy[f, :len(t)], ids[f, :len(t)] = t[:, :2], t[:, 2:].astype(np.int64).astype(np.int32)
        cnt[f] = len(t) if counts is None else counts[f]
        assert min(max(int(cnt[f]), 0), MAXP) <= len(t), 'a declared count may not uncover unfilled slots'
    return xy, ids, cnt


def board_image(tilt_x, tilt_y, depth, rows, cols, cam=0, noise=0.25, seed=0, shift=(0.0, 0.0)):
    """one image of a board -> (m,4) [x y row col] with the TRUE indices (col-major slot order), centre (2,) = the exact pixel of
    the grid point (0, 0)"""
    n, P4 = PC.board(tilt_x, tilt_y, depth, shift)
    idx, X = PC.board_hits(n, P4, cols, rows)
    uv = PC.project_pair(X, noise, np.random.default_rng(seed))[cam]
    ctr = PC.project_pair(PC.board_hits(n, P4, [0], [0])[1], 0.0, None)[cam][0]
    return np.concatenate([uv, idx[:, ::-1].astype(np.float64)], 1), ctr


@functools.lru_cache(maxsize=None)
def true_dir():
    """the sign with which the true (row, col) indices grow with (y, x) in the rig's images"""
    t, _ = board_image(0, 0, 360, range(-3, 4), range(-3, 4), noise=0.0)
    return int(np.sign(np.polyfit(t[:, 2], t[:, 1], 1)[0])), int(np.sign(np.polyfit(t[:, 3], t[:, 0], 1)[0]))


def lattice(nr, nc, pitch=(31.0, 29.0), keep=None, noise=0.05, seed=0, origin=(900.0, 600.0), shear=(0.04, -0.03), anchor=None,
            shuffle=True):
    """a synthetic grid of nr x nc lines: point (i, j) at origin + (j px + shear_x i py, i py + shear_y j px) + noise, true ids
    (i - ia, j - ja) with (ia, ja) = anchor (default the middle); keep(i, j) selects the points -> (m,4) [x y row col], centre
    (0.2 pitch off the anchor point, so that no two lines are as near)"""
    rng = np.random.default_rng(seed)
    ia, ja = (nr // 2, nc // 2) if anchor is None else anchor
    ii, jj = np.meshgrid(np.arange(nr), np.arange(nc), indexing='ij')
    ii, jj = ii.ravel(), jj.ravel()
    if keep is not None:
        sel = keep(ii, jj)
        ii, jj = ii[sel], jj[sel]
    px, py = pitch
    pos = lambda i, j: np.stack([origin[0] + j * px + shear[0] * i * py, origin[1] + i * py + shear[1] * j * px], -1)
    xy = pos(ii, jj) + rng.normal(0, noise, (len(ii), 2))
    t = np.concatenate([xy, np.stack([ii - ia, jj - ja], 1).astype(np.float64)], 1)
    if shuffle:
        t = t[rng.permutation(len(t))]
    return t, pos(ia, ja) + np.array([0.2 * px, 0.2 * py])


def relabel(t, comp, mapping):
    """the table with the true index v of component comp replaced by mapping(v) (a dict or a function)"""
    t = t.copy()
    fn = (lambda v: mapping[v]) if isinstance(mapping, dict) else mapping
    t[:, 2 + comp] = [fn(int(v)) for v in t[:, 2 + comp]]
    return t


def measured_pattern(tilt=(20.0, -12.0), cam=0, seed=5):
    """what the oracle's detector was seen to write on rendered boards (the issue's measurements): rows -5..6 x cols -3..3; row
    labels -6..-2 for the true -5..-1 and 2..7 for 1..6, and labels -1, +1 for two phantom lines of 4 points each 0.4 pitch either
    side of row 0 (the rim of the centre spot); column labels -3..3 for the true -2, -3, -1, 0, 2, 1, 3 and label 4 for a 3-point
    fragment of column 0 -> labelled table, true table (the phantom points with true row DROPPED), centre"""
    rows, cols = range(-5, 7), range(-3, 4)
    t, ctr = board_image(tilt[0], tilt[1], 365.0, rows, cols, cam=cam, seed=seed)
    colmap = {-2: -3, -3: -2, -1: -1, 0: 0, 2: 1, 1: 2, 3: 3}
    lab = relabel(relabel(t, 0, lambda v: v - 1 if v < 0 else v + 1 if v > 0 else 0), 1, colmap)
    frag = np.nonzero((t[:, 3] == 0) & (t[:, 2] >= 4))[0][:3]
    lab[frag, 3] = 4
    true = t.copy()
    true[frag, 2] = DROPPED                                             # dropped with the fragment
    # the phantoms: points of the columns -2, -1, 1, 2 at 0.4 of the local row pitch either side of row 0
    r0 = {int(c): t[(t[:, 2] == 0) & (t[:, 3] == c)][0] for c in (-2, -1, 1, 2)}
    r1 = {int(c): t[(t[:, 2] == 1) & (t[:, 3] == c)][0] for c in (-2, -1, 1, 2)}
    extra = []
    for s in (-1, 1):
        for c in (-2, -1, 1, 2):
            q = r0[c][:2] + s * 0.4 * (r1[c][:2] - r0[c][:2])
            extra.append([q[0], q[1], s, colmap[c]])
    lab = np.concatenate([lab, np.asarray(extra)])
    true = np.concatenate([true, np.asarray([[e[0], e[1], DROPPED, DROPPED] for e in extra])])
    return lab, true, ctr


# ------------------------------------------------------------------------------------------------------ cases
@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(tables [(m,4) labelled], true [(m,4) or None], center (n,2), counts or None, params, expect: what the case is
    for)"""
    C = {}

    def add(name, tables, true, center, counts=None, sign=None, **params):
        # sign: how the true ids of components 0, 1 grow with the position (boards: the rig's; lattices: +1)
        C[name] = dict(tables=tables, true=true, center=np.asarray(center, np.float64).reshape(-1, 2), counts=counts,
                       sign=true_dir() if sign is None else sign, params=dict(DEFAULTS, **params))

    rows, cols = range(-6, 7), range(-4, 5)
    base = [board_image(tx, ty, d, rows, cols, cam=cam, seed=s) for tx, ty, d, cam, s in
            ((4, -3, 350, 0, 1), (20, 10, 370, 1, 2), (-30, 25, 340, 0, 3), (30, -30, 390, 1, 4))]
    T = [b[0] for b in base]
    ctr = [b[1] for b in base]
    rng = np.random.default_rng(11)
    add('identity', T, T, ctr)
    add('reflection', [relabel(relabel(t, 0, lambda v: -v), 1, lambda v: -v) for t in T], T, ctr)
    perm_r, perm_c = (dict(zip(r, rng.permutation(list(r)).tolist())) for r in (rows, cols))
    add('permutation', [relabel(relabel(t, 0, perm_r), 1, perm_c) for t in T], T, ctr)
    add('offset', [relabel(relabel(t, 0, lambda v: v + 1000), 1, lambda v: v - 77) for t in T], T, ctr)
    add('int32 ends', [relabel(relabel(t, 0, lambda v: I32_MIN + 6 + v), 1, lambda v: I32_MAX - 4 + v) for t in T[:3]], T[:3], ctr[:3])
    pat = [measured_pattern(tl, cam, s) for tl, cam, s in (((20.0, -12.0), 0, 5), ((4.0, 3.0), 1, 6), ((-30.0, 18.0), 0, 7))]
    add('measured pattern', [p[0] for p in pat], [p[1] for p in pat], [p[2] for p in pat])
    gone = lambda t, comp, vals: t[~np.isin(t[:, 2 + comp], vals)]
    add('one line removed', [gone(T[0], 0, [2]), gone(T[1], 1, [-2]), gone(T[2], 0, [-3])],
        [gone(T[0], 0, [2]), gone(T[1], 1, [-2]), gone(T[2], 0, [-3])], ctr[:3])
    add('two lines removed', [gone(T[0], 0, [2, 3]), gone(T[3], 1, [1, 2]), gone(gone(T[2], 0, [-3, -2]), 1, [2, 3])],
        [gone(T[0], 0, [2, 3]), gone(T[3], 1, [1, 2]), gone(gone(T[2], 0, [-3, -2]), 1, [2, 3])], ctr[:1] + ctr[3:] + ctr[2:3])
    one = [t[t[:, 2] == 0] for t in T[:2]] + [T[2][T[2][:, 3] == 0]]
    add('single line', one, one, ctr[:3])
    diag = [t[t[:, 2] == t[:, 3]] for t in T[:2]]
    add('single point per line', diag, diag, ctr[:2])
    two = [t[np.isin(t[:, 2], [0, 1])] for t in T[:2]]
    add('two rows min_pts 2', two, two, ctr[:2], min_pts=2)
    add('min_pts 5', [t[np.abs(t[:, 3]) <= 2] for t in T[:3]], [t[np.abs(t[:, 3]) <= 2] for t in T[:3]], ctr[:3], min_pts=5)
    add('dir -1', T[:3], T[:3], ctr[:3], dir=(-1, 1))
    add('dir -1 -1', T[:1], T[:1], ctr[:1], dir=(-1, -1))
    add('swap 1 transposed', [t[:, [0, 1, 3, 2]] for t in T[:3]], [t[:, [0, 1, 3, 2]] for t in T[:3]], ctr[:3], sign=true_dir()[::-1], swap=1)
    bad = [T[0].copy(), T[1].copy(), T[2].copy()]
    bad[0][[3, 40, 77], 0] = np.nan
    bad[1][[0, 5], 1] = np.inf
    bad[1][9, 0] = -np.inf
    tb = [b.copy() for b in bad]
    for b in tb:
        b[~np.isfinite(b[:, :2]).all(1), 2:] = DROPPED
    add('nan inf pixels', bad, tb, ctr[:3])
    add('nan centre', T[:3], None, [ctr[0], [np.nan, 5.0], [7.0, np.inf]])

    # lattices: line counts 1, 2, 3, 64, 65, 256 per component, counts -1 .. 3000, batches of 1, 3 and 65
    lat = lattice
    for nlines in (1, 2, 3):
        t, c = lat(nlines, 5, seed=nlines)
        t2, c2 = lat(5, nlines, seed=10 + nlines)
        add(f'{nlines} lines', [t, t2], [t, t2], [c, c2], sign=(1, 1))
    band = lambda w: (lambda i, j: (j - i) % w == 0)
    for nlines, w, pitch in ((64, 16, (9.0, 8.0)), (65, 13, (9.0, 8.0)), (256, 32, (7.0, 6.0))):
        t, c = lat(nlines, nlines, keep=band(w), pitch=pitch, seed=nlines, origin=(50.0, 40.0), shear=(0.002, -0.001), noise=0.02)
        add(f'{nlines} lines', [t], [t], [c], sign=(1, 1))
    t256, c256 = lat(256, 256, keep=band(32), pitch=(7.0, 6.0), seed=3, origin=(50.0, 40.0), shear=(0.002, -0.001), noise=0.02)
    assert len(t256) == MAXP
    add('span 255', [relabel(t256, 0, lambda v: v + 5000)], [t256], [c256], sign=(1, 1))
    wide = t256.copy()
    wide[wide[:, 2] == wide[:, 2].max(), 2] += 1                  # the last row's label one further: span 256
    add('span 256', [wide, T[0]], None, [c256, ctr[0]])
    wide1 = t256.copy()
    wide1[wide1[:, 3] == wide1[:, 3].min(), 3] -= 1
    add('span 256 component 1', [wide1], None, [c256])
    t9, c9 = lat(9, 9, seed=21)
    big, cb = lat(46, 45, keep=lambda i, j: i * 45 + j < MAXP + 7, pitch=(12.0, 11.0), seed=22, shuffle=False, origin=(100.0, 50.0))
    assert len(big) > MAXP
    cl = [-1, 0, 1, 2, 63, 64, 65]
    add('counts', [t9] * len(cl) + [big[:MAXP], big[:MAXP]], None, [c9] * len(cl) + [cb, cb], counts=cl + [2048, 3000])
    many, mc = [], []
    for i in range(65):
        t, c = lat(4 + i % 5, 3 + i % 7, seed=100 + i, pitch=(20.0 + i % 3, 17.0 + i % 4))
        many.append(t); mc.append(c)
    add('65 images', many, many, mc, sign=(1, 1))
    return C


def arrays(case, poison=None):
    xy, ids, cnt = pack(case['tables'], case['counts'], poison)
    return xy, ids, cnt, case['center']


@functools.lru_cache(maxsize=None)
def reference(name):
    case = cases()[name]
    return ref_grid_relabel(*arrays(case), **case['params'])


def check_true(case, ref):
    """every written point carries dir * true_dir * its true index; every point of a true line that kept min_pts points and is
    not marked DROPPED is written -> the number of written points"""
    sign = np.asarray(case['params']['dir']) * np.asarray(case['sign'])
    total = 0
    for f, true in enumerate(case['true']):
        m = int(ref['cnt'][f])
        want = true[ref['src'][f, :m], 2:].astype(np.int64)
        assert not (want == DROPPED).any(), f'image {f}: a phantom point was written'
        assert np.array_equal(ref['id'][f, :m], want * sign), f'image {f}: indices differ from the true ones'
        total += m
    return total


# ------------------------------------------------------------------------------------------------------ rendered boards
H, W = 480, 640
# the free table of 8 boards (30 deg, seed 7) against the scene's true planes, measured with the numpy chain (board_table; module
# docstring of tests/test_relabel_cases_cpu.py); the bounds are twice these, this project's custom for one seed's figures
TABLE_MEASURED = dict(worst_deg=0.1683, median_deg=0.0347, centre_rms_mm=0.2503, centre_mm=1.1313)
TABLE_BOUNDS = {k: 2 * v for k, v in TABLE_MEASURED.items()}
RENDERED = tuple((t, s) for t in (4.0, 20.0, 30.0) for s in (2, 4, 7))      # tilt_deg, seed: 4 frames each, the measured 36


@functools.lru_cache(maxsize=None)
def boards(tilt, seed, n=4):
    from cpe_amd import synth
    return synth.render_batch(n, H, W, seed=seed, scene=synth.Scene(h=H, w=W, target='plane', tilt_deg=tilt))


def joined(xy1, id1, xy2, id2):
    """the pairs of equal ids, in the first table's order -> p1 (m,2), p2 (m,2), idx (m,2)"""
    at = {tuple(i): k for k, i in reversed(list(enumerate(np.asarray(id2).tolist())))}
    pairs = [(k, at[tuple(i)]) for k, i in enumerate(np.asarray(id1).tolist()) if tuple(i) in at]
    a, b = [p[0] for p in pairs], [p[1] for p in pairs]
    return np.asarray(xy1)[a].reshape(-1, 2), np.asarray(xy2)[b].reshape(-1, 2), np.asarray(id1)[a].reshape(-1, 2)


@functools.lru_cache(maxsize=None)
def oracle_frames(tilt, seed, n=4, **params):
    """per frame of boards(tilt, seed, n): the oracle's planar detections of both images and ref_grid_relabel of the two ->
    list of dict(det (left, right), ref, tables: the relabelled (xy, id) of left and right)"""
    import oracle
    from oracle import stages as S
    oracle.build()
    b = boards(tilt, seed, n)
    out = []
    for i in range(n):
        det = [S.detect_grid_plane(b[k][i].numpy()) for k in ('left', 'right')]
        assert det[0]['status'] == 0 and det[1]['status'] == 0
        xy, ids, cnt = pack([np.concatenate([d['xy'], d['id']], 1) for d in det])
        ref = ref_grid_relabel(xy, ids, cnt, np.stack([d['center'] for d in det]), **dict(DEFAULTS, **dict(params)))
        out.append(dict(det=det, ref=ref, tables=[(ref['xy'][k, :ref['cnt'][k]], ref['id'][k, :ref['cnt'][k]]) for k in range(2)]))
    return out


def off_board(b, i, t1, t2):
    """the joined pairs of two (xy, id) tables of frame i, triangulated -> distances to the true board (mm), idx, X, err (px)"""
    import oracle
    p1, p2, idx = joined(*t1, *t2)
    if not len(p1):
        return np.zeros(0), idx, np.zeros((0, 3)), np.zeros(0)
    X, err = oracle.triangulate(p1, p2, b['K1'], b['K2'], b['T21'])
    return X @ b['plane_n'][i] - b['plane_d'][i], idx, X, err


def table_figures(P, status, centre, lo, scene):
    """a free table of row / col planes (family 0 = row, as the planar detector's ids) against table_tri_cases.true_table(scene)
    -> dict(worst_deg, median_deg, lines, centre_mm): plane angles over the lines with status 0, the centre's distance"""
    import table_tri_cases as TC
    from cpe_amd import synth
    t = TC.true_table(scene)
    ang = []
    for k in range(2):
        for j in np.nonzero(status[k] == 0)[0]:
            v = lo + int(j)
            if t['lo'] <= v <= t['hi']:
                a = PC.angle(P[k, j, :3], t['P'][1 - k, v - t['lo'], :3])
                ang.append(math.degrees(min(a, math.pi - a)))
    Tp = synth.make_rig(scene)[3]
    return dict(worst_deg=max(ang), median_deg=float(np.median(ang)), lines=len(ang),
                centre_mm=float(np.linalg.norm(centre[:3] + Tp[:3, :3].T @ Tp[:3, 3])))


def board_table(tilt, seed, n=8, relabelled=True, err_px=1.0, band_mm=1.0):
    """the free laser-plane table of n rendered boards, all in numpy: the joined pairs with a reprojection error below err_px,
    plane_fit_cases.ref_fit_plane with a band of band_mm per frame, ref_index_planes over the inliers -> dict(table, lo, hi,
    figures (table_figures), frames: per frame (pairs used, inliers))"""
    b = boards(tilt, seed, n)
    fr = oracle_frames(tilt, seed, n)
    frames, per = [], []
    for i, f in enumerate(fr):
        tabs = f['tables'] if relabelled else [(d['xy'], d['id']) for d in f['det']]
        _, idx, X, err = off_board(b, i, *tabs)
        ok = err < err_px
        fit = PC.ref_fit_plane(X[ok], idx[ok], int(ok.sum()), band_mm, 4)
        frames.append(dict(X=X[ok], idx=idx[ok], use=fit['mask'], ok=int(fit['status'] == 0)))
        per.append((int(ok.sum()), int(fit['n_inliers'])))
    X, I, cnt = PC.pack(frames)
    use = np.stack([f['use'] for f in frames])
    ok = np.asarray([f['ok'] for f in frames], np.int32)
    sel = (use != 0) & (ok != 0)[:, None]
    lo, hi = int(I[sel].min()), int(I[sel].max())
    tab = PC.ref_index_planes(X, I, cnt, lo, hi, use, ok)
    return dict(table=tab, lo=lo, hi=hi, frames=per, figures=table_figures(tab['P'], tab['status'], tab['centre'], lo, b['scene']))
