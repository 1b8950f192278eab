"""The stereo selectors (k_select_triangulate in csrc/fit.hip: chooseIdx.m, triangulateWithThreshold.m,
findGridCorrespondences.m) at every patch size and on grids with holes: the cases, and the reference restated plainly.

plain_choose_idx is chooseIdx.m:19-104 read line by line into Python -- a dict as the containers.Map, sorted() on the strings
f'{c}_{r}' as its key order -- with oracle.triangulate for the reprojection errors (the oracle's triangulation has the kernel's
bits, tests/test_fit_shapes_gpu.py).  tests/test_selector_cases_cpu.py compares it with the C oracle, which the GPU tests
(tests/test_selectors_gpu.py) then compare the kernel with; no GPU is needed here.

Every threshold in use is computed from the means (or errors) the restatement gives, half way between two that differ, so no
decision sits near its threshold by accident; the boundary cases sit on it on purpose."""
import collections
import functools

import numpy as np

import oracle
from test_fit_shapes_gpu import _grid, _rig

PATCHES = tuple(range(1, 9))
TH_FIXED = 0.3              # fitSingleCylinder.m:12


@functools.lru_cache(maxsize=None)
def rig():
    oracle.build()
    return _rig()


# ------------------------------------------------------------------------------------------ the plain restatement
def _first_rows(t):
    """ismember(..., 'rows') / find(): the lowest row index of every (col,row)"""
    first = {}
    for i, row in enumerate(t):
        first.setdefault((int(row[2]), int(row[3])), i)
    return first


Window = collections.namedtuple('Window', 'at cand complete loc1 loc2 err mean')
Chosen = collections.namedtuple('Chosen', 'keys rows1 rows2 means complete fallback windows')


def plain_windows(t1, t2, rig_, patch):
    """chooseIdx.m:22-62: every window of patch x patch unique values of image 1, its candidates in the order :37-41 builds
    them, whether both tables hold all of them, and then the errors of triangulate and their mean (the sum in candidate order)"""
    K1, K2, T21 = rig_
    ux = sorted(set(int(v) for v in t1[:, 2]))                       # :22-23
    uy = sorted(set(int(v) for v in t1[:, 3]))
    f1, f2 = _first_rows(t1), _first_rows(t2)
    out = []
    for ix in range(len(ux) - patch + 1):                            # :29-30
        for iy in range(len(uy) - patch + 1):
            cand = [(c, r) for c in ux[ix:ix + patch] for r in uy[iy:iy + patch]]         # :32-41
            if not all(k in f1 for k in cand) or not all(k in f2 for k in cand):          # :44-49
                out.append(Window((ix, iy), cand, False, None, None, None, float('nan')))
                continue
            loc1 = [f1[k] for k in cand]
            loc2 = [f2[k] for k in cand]
            _, err = oracle.triangulate(t1[loc1, :2], t2[loc2, :2], K1, K2, T21)          # :52-57
            s = 0.0
            for e in err:
                s = s + float(e)
            out.append(Window((ix, iy), cand, True, loc1, loc2, [float(e) for e in err], s / (patch * patch)))
    return out


def plain_join(t1, t2):
    """findGridCorrespondences.m: every row of table 1 that table 2 has, in table-1 order, with the first such row of table 2
    -> keys, rows in table 1, rows in table 2"""
    keys, rows1, rows2 = [], [], []
    for i in range(len(t1)):
        hit = np.flatnonzero((t2[:, 2:4] == t1[i, 2:4]).all(1))     # :15
        if len(hit) == 0:
            continue
        keys.append((int(t1[i, 2]), int(t1[i, 3]))); rows1.append(i); rows2.append(int(hit[0]))
    return keys, rows1, rows2


def plain_choose_idx(t1, t2, rig_, patch, th, windows=None):
    """chooseIdx.m:19-104 -> Chosen(keys, rows in table 1, rows in table 2, the mean of every window (NaN where incomplete),
    which windows were complete, whether the join of :101-104 was used, the windows themselves)"""
    windows = plain_windows(t1, t2, rig_, patch) if windows is None else windows
    point_map = {}                                                   # :19
    for w in windows:
        if not w.complete or not w.mean < th:                        # :65
            continue
        for k, e, a, b in zip(w.cand, w.err, w.loc1, w.loc2):        # :67-83
            if k in point_map:
                if e < point_map[k][0]:
                    point_map[k] = (e, a, b)
            else:
                point_map[k] = (e, a, b)
    means, complete = [w.mean for w in windows], [w.complete for w in windows]
    if not point_map:                                                # :101-104
        return Chosen(*plain_join(t1, t2), means, complete, True, windows)
    keys = sorted(point_map, key=lambda k: f'{k[0]}_{k[1]}')          # :89, the order of a containers.Map with char keys
    return Chosen(keys, [point_map[k][1] for k in keys], [point_map[k][2] for k in keys], means, complete, False, windows)


def plain_pair_errors(t1, t2, rig_):
    """the join and the reprojection error of each of its pairs (triangulateWithThreshold.m:16-28)"""
    keys, rows1, rows2 = plain_join(t1, t2)
    if not keys:
        return keys, rows1, rows2, []
    _, err = oracle.triangulate(t1[rows1, :2], t2[rows2, :2], *rig_)
    return keys, rows1, rows2, [float(e) for e in err]


def plain_threshold(t1, t2, rig_, th):
    """triangulateWithThreshold.m:16-43 -> keys, rows in table 1, rows in table 2, the errors of all joined pairs, fallback"""
    keys, rows1, rows2, err = plain_pair_errors(t1, t2, rig_)
    valid = [i for i, e in enumerate(err) if e < th]                 # :31
    if not valid:                                                    # :40-43 (and :19-24: nothing joined, nothing returned)
        return keys, rows1, rows2, err, bool(keys)
    return [keys[i] for i in valid], [rows1[i] for i in valid], [rows2[i] for i in valid], err, False


# ----------------------------------------------------------------------------------------------------- the cases
Case = collections.namedtuple('Case', 'name t1 t2 reaches fixed_th')


def _perm(t, seed):
    return t[np.random.default_rng(seed).permutation(len(t))]


def _thin_out(t, fraction, seed):
    """t without round(fraction * len(t)) of its rows, the rest in an order of its own"""
    order = np.random.default_rng(seed).permutation(len(t))
    return t[order[int(round(fraction * len(t))):]]


def _without_cols(t, cols):
    return t[~np.isin(t[:, 2], list(cols))]


def _moved(t, rows, dxy):
    t = t.copy()
    t[rows, :2] += np.asarray(dxy, np.float64)
    return t


MOVE = (0.0, 5.0)           # 5 px across the epipolar lines (along them a move changes the depth, not the error): error ~2.5 px
OUTLIER = (5, 6)            # interior: every neighbour has a window of any patch size that leaves this node out


@functools.lru_cache(maxsize=None)
def cases():
    r = rig()
    out = []

    def add(name, t1, t2, reaches, fixed=False):
        out.append(Case(name, np.ascontiguousarray(t1), np.ascontiguousarray(t2), tuple(reaches), fixed))

    a, b = _grid(r, range(0, 12), range(0, 12), 101)
    add('full', _perm(a, 1), _perm(b, 2), ['mixed', 'shared'])
    for name, frac, seed in (('holes10', 0.10, 110), ('holes30', 0.30, 130)):
        a, b = _grid(r, range(-9, 17), range(-4, 18), seed)          # 26 x 22
        add(name, _thin_out(a, frac, seed + 1), _thin_out(b, frac, seed + 2), ['mixed', 'incomplete', 'shared'])
    a, b = _grid(r, range(0, 14), range(0, 12), 140)
    add('col_gone', _perm(_without_cols(a, [5]), 3), _perm(_without_cols(b, [5]), 4), ['mixed', 'gap'])
    a, b = _grid(r, range(0, 14), range(0, 12), 141)
    add('col_only_in_1', _perm(a, 5), _perm(_without_cols(b, [5]), 6), ['mixed', 'incomplete', 'dead_column'])
    a, b = _grid(r, range(-2, 14), range(0, 12), 142)                # table 2 alone has columns 5 and -2, -1 (below the range
    add('col_only_in_2', _perm(_without_cols(a, [5, -2, -1]), 7), _perm(b, 8), ['mixed', 'gap'])    # of image 1)
    a, b = _grid(r, range(3, 5), range(0, 12), 150)
    add('thin', _perm(a, 9), _perm(b, 10), ['thin'], fixed=True)
    for p in PATCHES:
        a, b = _grid(r, range(-1, p - 1), range(2, 2 + p), 160 + p)
        add(f'exact_{p}', _perm(a, 11), _perm(b, 12), [f'exact:{p}'], fixed=True)
    for want, nx, ny in ((63, 9, 11), (64, 10, 10), (65, 7, 15)):
        a, b = _grid(r, range(0, nx), range(-3, ny - 3), 170 + want)
        add(f'tail{want}', _perm(a, 13), _perm(b, 14), ['mixed', f'windows:{want}'])
    a, b = _grid(r, range(0, 12), range(0, 12), 180)
    bad = np.flatnonzero((b[:, 2] == OUTLIER[0]) & (b[:, 3] == OUTLIER[1]))
    add('outlier', _perm(a, 15), _perm(_moved(b, bad, MOVE), 16), ['rescue'], fixed=True)
    a, b = _grid(r, range(0, 12), range(0, 12), 181)
    add('all_bad', _perm(a, 17), _perm(_moved(b, slice(None), MOVE), 18), ['all_bad'], fixed=True)
    a, b = _grid(r, [-12, -11, -10, -9, -2, -1, 0, 1, 2, 9, 10, 11, 99, 100, 101], [-100, -99, -10, -9, -1, 0, 1, 9, 10, 11], 190)
    add('digits', _perm(a, 19), _perm(b, 20), ['mixed', 'digits'])
    # the `duplicates` construction of test_fit_shapes_gpu._sel_cases on a grid with 10 % holes: a (col,row) twice in a table,
    # with different pixels, is found through its first row
    s1, s2 = _grid(r, range(0, 12), range(0, 12), 200)
    d1, d2 = _grid(r, range(0, 12), range(0, 12), 201)
    s1, s2 = _thin_out(s1, 0.10, 202), _thin_out(s2, 0.10, 203)
    dup = np.random.default_rng(204).permutation(144)[:40]
    t1 = np.concatenate([s1, d1[dup]])
    add('dups', _perm(t1, 205), np.concatenate([d2[dup[::-1]], s2]), ['mixed', 'incomplete', 'duplicates'])
    assert all(max(len(c.t1), len(c.t2)) <= 600 for c in out)
    return tuple(out)


def case(name):
    return {c.name: c for c in cases()}[name]


CASE_NAMES = ('full', 'holes10', 'holes30', 'col_gone', 'col_only_in_1', 'col_only_in_2', 'thin') + tuple(
    f'exact_{p}' for p in PATCHES) + ('tail63', 'tail64', 'tail65', 'outlier', 'all_bad', 'digits', 'dups')


@functools.lru_cache(maxsize=None)
def windows(name, patch):
    c = case(name)
    return tuple(plain_windows(c.t1, c.t2, rig(), patch))


@functools.lru_cache(maxsize=None)
def pair_errors(name):
    c = case(name)
    return plain_pair_errors(c.t1, c.t2, rig())


def _midpoint_near_median(values):
    """the midpoint of the two adjacent sorted values nearest the median whose relative distance is above 1e-6; None when no two
    values are that far apart"""
    v = sorted(values)
    gaps = [i for i in range(len(v) - 1) if v[i + 1] - v[i] > 1e-6 * v[i + 1]]
    if not gaps:
        return None
    mid = (len(v) - 2) / 2.0                                         # the gap that splits the values in halves
    i = min(gaps, key=lambda g: (abs(g - mid), g))
    return v[i] + (v[i + 1] - v[i]) / 2.0


def threshold(name, patch=None):
    """the th a case is run with: for chooseIdx at `patch`, from the means of its complete windows; patch None: for
    triangulateWithThreshold, from the errors of its joined pairs.  TH_FIXED for the cases whose claim depends on that value, and
    where fewer than two distinct values exist to put a threshold between."""
    if case(name).fixed_th:
        return TH_FIXED
    values = pair_errors(name)[3] if patch is None else [w.mean for w in windows(name, patch) if w.complete]
    th = _midpoint_near_median(values)
    return TH_FIXED if th is None else th


@functools.lru_cache(maxsize=None)
def chosen(name, patch, th=None):
    c = case(name)
    return plain_choose_idx(c.t1, c.t2, rig(), patch, threshold(name, patch) if th is None else th, windows(name, patch))


def providers(name, patch, th):
    """key -> the windows (at) with mean < th that hold it"""
    out = collections.defaultdict(list)
    for w in windows(name, patch):
        if w.complete and w.mean < th:
            for k in w.cand:
                out[k].append(w.at)
    return out


BOUNDARY = tuple((f'exact_{p}', p) for p in PATCHES) + (('full', 3),)


@functools.lru_cache(maxsize=None)
def boundary(name, patch):
    """(th_equal, th_above, window): th_equal is the double the restatement computes for the mean of `window` = (ix, iy),
    th_above the next double.  With th_equal the window is rejected, with th_above it is accepted -- and the result shows it: the
    window is then the only accepted one that holds at least one of its keys (boundary_keys).  Of the windows that qualify, the
    one whose mean is nearest the median."""
    ws = [w for w in windows(name, patch) if w.complete]
    order = sorted(ws, key=lambda w: w.mean)
    rank = {w.at: i for i, w in enumerate(order)}
    best = None
    for w in ws:
        th_above = float(np.nextafter(w.mean, np.inf))
        prov = providers(name, patch, th_above)
        if any(prov[k] == [w.at] for k in w.cand):
            score = abs(rank[w.at] - (len(ws) - 1) / 2.0)
            if best is None or score < best[0]:
                best = (score, w)
    w = best[1]
    return w.mean, float(np.nextafter(w.mean, np.inf)), w.at


def boundary_keys(name, patch):
    """the keys that only the boundary window offers once it is accepted"""
    _, th_above, at = boundary(name, patch)
    return sorted(k for k, ws in providers(name, patch, th_above).items() if ws == [at])


BOUNDARY_PAIR = 'full'


@functools.lru_cache(maxsize=None)
def boundary_pair(name=BOUNDARY_PAIR):
    """(th_equal, th_above, key) for triangulateWithThreshold: the joined pair whose error is the median one, and that error"""
    keys, _, _, err = pair_errors(name)
    i = sorted(range(len(err)), key=lambda j: err[j])[len(err) // 2]
    return err[i], float(np.nextafter(err[i], np.inf)), keys[i]
