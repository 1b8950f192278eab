"""Inputs for LAB-L + CLAHE(4.5, 4 x 4) on its own (cpe_debug_clahe_planes, cpe_debug_clahe_planes_bgr, include/cpe.h): one idea
per generator, the smallest frames that reach each path.  A case is dict(gray u8 [h,w], tiles: per CLAHE tile (kind, order),
resid: per tile the clipped excess modulo 256 the tile was built for, or None).  Histograms are stated over L values (the bins
CLAHE clips) and lifted to grey values through the oracle's LAB-L table; where two grey values share an L value the count is
split between them.  A frame whose size is no multiple of 4 is drawn on CLAHE's padded canvas and cropped, so its edge tiles
hold what reflect-101 makes of them.  The oracle's view (`ref`), the numpy restatement and the checks that every generator
reaches the rule it is named for live in tests/test_clahe_generators_cpu.py; tests/test_clahe_stage_gpu.py runs the cases
through the kernels."""
import numpy as np

NTHR = 17
RESIDUALS = (0, 1, 2, 85, 86, 127, 128, 129, 255)      # step 256 // r: -, 256, 128, 3, 2, 2, 2, 1, 1
ORDERS = ('sorted', 'shuffled', 'first0', 'first_nz', 'sorted_desc')

_LAB = None


def lab_table():
    """the oracle's LAB-L table, u8[256]"""
    global _LAB
    if _LAB is None:
        from oracle import stages as S
        _LAB = S.lab_l(np.arange(256, dtype=np.uint8)[None])[0].copy()
    return _LAB


def geom(h, w, clip=4.5):
    """CLAHE's padded canvas, tile size and clip limit (clahe.cpp: both sides grow when either is no multiple of 4)"""
    eh, ew = (h, w) if h % 4 == 0 and w % 4 == 0 else (h + 4 - h % 4, w + 4 - w % 4)
    th, tw = eh // 4, ew // 4
    return dict(eh=eh, ew=ew, th=th, tw=tw, total=th * tw, clip=max(int(clip * (th * tw) / 256), 1))


# ---------------------------------------------------------------- one tile from an exact list of per-value counts
def fill_tile(counts, th, tw, order, seed=0):
    """u8 [th,tw] holding counts[v] pixels of value v in raster order: sorted (long runs that cross dwords, rows and the 256
    thread stride), sorted_desc (the same, first pixel the largest value), shuffled (runs of 1 where the histogram allows),
    first0 / first_nz (shuffled, first pixel 0 / not 0: the start state of the run a thread carries)"""
    counts = np.asarray(counts, np.int64)
    assert counts.shape == (256,) and counts.min() >= 0 and counts.sum() == th * tw, (counts.sum(), th * tw)
    px = np.repeat(np.arange(256, dtype=np.uint8), counts)
    if order == 'sorted_desc':
        px = px[::-1]
    elif order != 'sorted':
        px = np.random.default_rng(seed).permutation(px)
        if order in ('first0', 'first_nz'):
            want = (px == 0) if order == 'first0' else (px != 0)
            if want.any() and not want[0]:
                k = int(np.argmax(want))
                px[0], px[k] = px[k], px[0]
        else:
            assert order == 'shuffled', order
    return np.ascontiguousarray(px.reshape(th, tw))


def lift(hl, seed=0):
    """grey-value counts whose LAB-L histogram is hl (counts over L values; L values the table never gives must be 0)"""
    lab = lab_table()
    hl = np.asarray(hl, np.int64)
    out = np.zeros(256, np.int64)
    for L in np.nonzero(hl)[0]:
        pre = np.nonzero(lab == L)[0]
        assert len(pre), f'L value {L} has no grey value'
        if len(pre) == 1:
            out[pre[0]] = hl[L]
        else:     # grey values that share an L value: both hold a part
            a = hl[L] // 2 if seed % 2 else (hl[L] + 1) // 2
            out[pre[0]], out[pre[1]] = a, hl[L] - a
    return out


def _spread(rest, bins, cap, rng):
    """rest pixels over the given bins, at most cap each, at least one bin exactly at cap when rest allows"""
    out = np.zeros(256, np.int64)
    bins = np.asarray(bins)
    assert 0 <= rest <= len(bins) * cap, (rest, len(bins), cap)
    if rest == 0:
        return out
    if rest >= cap:
        out[bins[rng.integers(len(bins))]] = cap
        rest -= cap
    free = bins[out[bins] == 0]
    if len(free) * cap <= 2_000_000:
        slots = np.repeat(free, cap)
        out += np.bincount(rng.choice(slots, size=rest, replace=False), minlength=256)
    else:
        wgt = rng.random(len(free)) + 0.05
        c = np.minimum((wgt / wgt.sum() * rest).astype(np.int64), cap)
        k = 0
        left = rest - int(c.sum())
        while left > 0:
            room = min(cap - int(c[k % len(free)]), left)
            c[k % len(free)] += room
            left -= room
            k += 1
        out[free] += c
    return out


def hist_resid(total, clip, r, variant, seed):
    """L histogram of a tile whose clipped excess is r modulo 256: 1 .. 3 heavy bins (variant picks how many and whether the
    first or the last L value is one of them) above the clip limit, every other bin at or below it.  None if the tile is too
    small for it."""
    rng = np.random.default_rng(seed)
    lvals = np.unique(lab_table())
    m = max(0, (total // 3 - r) // 256)
    if variant % 3 == 2 and r == 0:
        m = 0                               # nothing clipped at all
    E = r + 256 * m
    nh = 0 if E == 0 else min(1 + variant % 3, E)
    while nh > 1 and nh * clip + E > total:
        nh -= 1
    if nh * clip + E > total:
        m = max(0, (total - clip - r) // 256)
        E = r + 256 * m
        if E == 0 or clip + E > total:
            return None
        nh = 1
    ends = [lvals[0], lvals[-1]]
    heavy = list(rng.choice(lvals[1:-1], size=nh, replace=False))
    if nh and variant % 2 == 0:
        heavy[0] = ends[(variant // 2) % 2]
    hl = np.zeros(256, np.int64)
    if nh:
        cuts = np.sort(rng.choice(np.arange(1, E), size=nh - 1, replace=False)) if nh > 1 else np.zeros(0, np.int64)
        parts = np.diff(np.concatenate([[0], cuts, [E]]))
        for b, e in zip(heavy, parts):
            hl[b] = clip + e
    light = np.array([v for v in lvals if v not in heavy])
    rest = total - int(hl.sum())
    if rest > len(light) * clip:
        return None
    hl += _spread(rest, light, clip, rng)
    return hl


def residual_of(hl, clip):
    """(clipped excess, residual, step) of an L histogram"""
    ex = int(np.maximum(np.asarray(hl, np.int64) - clip, 0).sum())
    r = ex % 256
    return ex, r, (max(256 // r, 1) if r else 0)


# ---------------------------------------------------------------- histogram kinds of the patchworks
def _kind_hist(kind, total, clip, seed):
    """grey-value counts of one tile"""
    rng = np.random.default_rng(seed)
    lab = lab_table()
    lvals = np.unique(lab)
    g = np.zeros(256, np.int64)
    if kind == 'flat':                         # one bin holds the tile
        g[int(rng.integers(1, 255))] = total
    elif kind == 'all0':
        g[0] = total
    elif kind == 'all255':
        g[255] = total
    elif kind == 'dark':                       # flat dark: a few low values
        g[:4] = np.bincount(rng.integers(0, 4, total), minlength=4)
    elif kind == 'unclipped':                  # every L bin at or below the clip limit, some exactly at it
        g = lift(_spread(total, lvals, clip, rng), seed)
    elif kind == 'lutties':
        # nothing clipped, and the cumulative sums pass through every sum s at which f32(s) * f32(255 / total) is k + 0.5 with k
        # even (rint and half-up rounding of the table differ there), where the tile size has such sums
        v = np.arange(total + 1).astype(np.float32) * (np.float32(255) / np.float32(total))
        ties = [int(s) for s in np.nonzero((v - np.floor(v) == 0.5) & (np.floor(v) % 2 == 0))[0]] + [total]
        hl = np.zeros(256, np.int64)
        cum, k = 0, int(rng.integers(0, 40))
        while cum < total:
            target = min(s for s in ties if s > cum)
            hl[lvals[k]] = min(max(clip - k % 2, 1), target - cum)
            cum += int(hl[lvals[k]])
            k += 1
        g = lift(hl, seed)
    elif kind == 'noise':
        g = np.bincount(rng.integers(0, 256, total), minlength=256).astype(np.int64)
    elif kind == 'pairs':
        # grey values that share an L value (75 / 76 -> 82, 110 / 111 -> 119, ...), each below the clip limit, together above
        # it; next to them pairs that do not share (77 / 78, 112 / 113) with the same counts
        shared = [(a, a + 1) for a in range(255) if lab[a] == lab[a + 1]]
        shared = ([p for p in shared if p[0] in (75, 110)] + [p for p in shared if p[0] not in (75, 110)])[:6]
        used = []
        each = clip // 2 + 1
        for a, b in shared:
            for v in (a, b, b + 1, b + 2):
                if g[v] == 0 and g.sum() + each <= total:
                    g[v] = each
                    used.append(v)
        rest = total - int(g.sum())
        others = np.array([v for v in range(256) if v not in used and not any(lab[v] == lab[u] for u in used)])
        others = others[np.unique(lab[others], return_index=True)[1]]      # one grey value per L bin
        k = int(min(len(others), max(1, -(-rest // max(clip * 3, 1)))))
        pick = rng.choice(others, size=k, replace=False)
        g[pick] += np.bincount(rng.integers(0, k, rest), minlength=k)
    else:
        raise KeyError(kind)
    assert g.sum() == total
    return g


def _ramp_tile(th, tw, seed):
    x = (np.arange(tw) * 255 // max(tw - 1, 1)).astype(np.uint8)
    t = np.repeat(x[None], th, 0)
    return np.ascontiguousarray(t if seed % 2 == 0 else t[:, ::-1])


# neighbours differ strongly: interpolated values cross .5 at many weights
PATCH_A = ('dark', 'noise', 'ramp', 'flat',
           'noise', 'all255', 'dark', 'pairs',
           'ramp', 'all0', 'unclipped', 'noise',
           'pairs', 'noise', 'flat', 'dark')
PATCH_B = ('noise', 'all0', 'pairs', 'ramp',
           'all255', 'unclipped', 'noise', 'dark',
           'flat', 'lutties', 'dark', 'all255',
           'ramp', 'pairs', 'all0', 'noise')


def _assemble(h, w, make_tile):
    G = geom(h, w)
    canvas = np.zeros((G['eh'], G['ew']), np.uint8)
    for t in range(16):
        ty, tx = divmod(t, 4)
        canvas[ty * G['th']:(ty + 1) * G['th'], tx * G['tw']:(tx + 1) * G['tw']] = make_tile(t, G)
    return np.ascontiguousarray(canvas[:h, :w])


def gen_patch(h, w, layout, seed):
    tiles = []

    def tile(t, G):
        kind, order = layout[t], ORDERS[(t + seed) % len(ORDERS)]
        tiles.append((kind, order))
        if kind == 'ramp':
            return _ramp_tile(G['th'], G['tw'], t + seed)
        return fill_tile(_kind_hist(kind, G['total'], G['clip'], 1000 * seed + t), G['th'], G['tw'], order, 77 * seed + t)
    return dict(gray=_assemble(h, w, tile), tiles=tiles, resid=[None] * 16)


def gen_resid(h, w, seed=0):
    """tile t has the clipped excess RESIDUALS[t % 9] modulo 256 (a residual the tile is too small for falls back to the next
    one that fits), in every pixel order"""
    tiles, resid = [], []

    def tile(t, G):
        for k in range(len(RESIDUALS)):
            r = RESIDUALS[(t + seed + k) % len(RESIDUALS)]
            hl = hist_resid(G['total'], G['clip'], r, t + seed, 31 * seed + t)
            if hl is not None:
                break
        order = ORDERS[(t // 2 + seed) % len(ORDERS)]
        tiles.append(('resid', order)); resid.append(r)
        return fill_tile(lift(hl, t), G['th'], G['tw'], order, 13 * seed + t)
    return dict(gray=_assemble(h, w, tile), tiles=tiles, resid=resid)


def gen_uniform(h, w, v):
    return dict(gray=np.full((h, w), v, np.uint8), tiles=[('const', 'sorted')] * 16, resid=[None] * 16)


# ---------------------------------------------------------------- sizes and named cases
SMALL = ((64, 64), (68, 68), (64, 72), (72, 80), (65, 67), (66, 64), (64, 66))
MID = ((320, 512), (316, 512), (320, 496), (317, 512), (328, 528), (512, 512))
LONG = ((64, 4096), (4096, 64))
PRODUCT = (1200, 1920)
HUGE = (4096, 4096)


def _build():
    c = {}
    for h, w in SMALL + MID:
        s = f'{h}x{w}'
        if h % 4 == 0 and w % 4 == 0:      # a padded frame's edge tiles are not what the generator filled
            c[f'resid_{s}'] = (gen_resid, (h, w, 0))
            c[f'resid2_{s}'] = (gen_resid, (h, w, 5))
        c[f'patchA_{s}'] = (gen_patch, (h, w, PATCH_A, 1))
        c[f'patchB_{s}'] = (gen_patch, (h, w, PATCH_B, 2))
    c['zeros_64x64'] = (gen_uniform, (64, 64, 0))
    c['full_64x64'] = (gen_uniform, (64, 64, 255))
    c['zeros_65x67'] = (gen_uniform, (65, 67, 0))
    c['full_320x512'] = (gen_uniform, (320, 512, 255))
    for h, w in LONG:
        c[f'resid_{h}x{w}'] = (gen_resid, (h, w, 3))
        c[f'patchA_{h}x{w}'] = (gen_patch, (h, w, PATCH_A, 3))
    c['resid_1200x1920'] = (gen_resid, (1200, 1920, 7))
    c['patchB_1200x1920'] = (gen_patch, (1200, 1920, PATCH_B, 4))
    c['patchA_4096x4096'] = (gen_patch, (4096, 4096, PATCH_A, 6))
    return c


CASES = _build()
_MADE = {}
_REF = {}


def size_of(name):
    h, w = name.rsplit('_', 1)[1].split('x')
    return int(h), int(w)


def names(sizes=None):
    return [n for n in CASES if sizes is None or size_of(n) in sizes]


def sizes():
    out = []
    for n in CASES:
        if size_of(n) not in out:
            out.append(size_of(n))
    return out


def get(name):
    if name not in _MADE:
        f, a = CASES[name]
        c = f(*a)
        c['gray'].setflags(write=False)
        _MADE[name] = c
    return _MADE[name]


def tile_hists(L):
    """i64 [16,256]: the histograms CLAHE takes of an L plane (reflect-101 padding included)"""
    h, w = L.shape
    G = geom(h, w)
    ext = np.pad(L, ((0, G['eh'] - h), (0, G['ew'] - w)), mode='reflect')
    t = ext.reshape(4, G['th'], 4, G['tw']).transpose(0, 2, 1, 3).reshape(16, -1)
    return np.stack([np.bincount(r, minlength=256) for r in t]).astype(np.int64)


# ---------------------------------------------------------------- true-colour versions of grey cases
COLOUR_CASES = ('patchA_64x64', 'patchB_65x67', 'patchA_320x512', 'patchB_317x512', 'resid_328x528')


def bgr_of(gray, variant):
    """a colour frame from a grey one: channels permuted and scaled (a red, a green or a blue dominant), a little texture of
    their own, so that the L channel is not LAB-L of the luma"""
    g = gray.astype(np.float64)
    rng = np.random.default_rng(100 + variant)
    scales = [(0.18, 0.35, 1.0), (1.0, 0.22, 0.45), (0.3, 1.0, 0.12)][variant % 3]
    ch = [g * s + rng.integers(0, 5, gray.shape) for s in scales]
    return np.ascontiguousarray(np.clip(np.stack(ch, 2), 0, 255).astype(np.uint8))


# ---------------------------------------------------------------- the oracle's view of a case, computed once
def expected(cl):
    """planes, bucket sizes and box as a CLAHE image [n,h,w] defines them: planes[t] = cl > 50 + 10 t in the 64 x 8 tile
    layout with its zero tile columns and zero rows below the frame, pixels per grey-level bucket, box of the pixels > 50"""
    n, h, w = cl.shape
    th8, chunks = (h + 7) // 8, (w + 63) // 64
    planes = np.zeros((n, NTHR, th8, chunks + 2, 8), np.uint64)
    pad = np.zeros((n, th8 * 8, chunks * 64), np.uint8)
    pad[:, :h, :w] = cl
    for t in range(NTHR):
        bits = (pad > 50 + 10 * t).reshape(n, th8, 8, chunks, 64)
        words = np.packbits(bits, axis=-1, bitorder='little').view('<u8')[..., 0]   # (n, th8, 8, chunks)
        planes[:, t, :, 1:chunks + 1, :] = words.transpose(0, 1, 3, 2)
    buckets = np.zeros((n, NTHR + 1), np.int32)
    box = np.zeros((n, 4), np.int32)
    for f in range(n):
        v = cl[f].astype(np.int32)
        lev = np.where(v <= 50, 0, np.minimum((v - 41) // 10, 17))
        buckets[f, 1:] = np.bincount(lev.ravel(), minlength=NTHR + 1)[1:]
        ys, xs = np.nonzero(v > 50)
        box[f] = [xs.min(), ys.min(), xs.max(), ys.max()] if len(xs) else [2 ** 31 - 1, 2 ** 31 - 1, -1, -1]
    return planes, buckets, box


def ref(name, colour=None):
    """dict(L, cl, planes, buckets, box) of the oracle for a grey case, or for its colour version bgr_of(gray, colour)"""
    key = (name, colour)
    if key not in _REF:
        from oracle import stages as S
        g = get(name)['gray']
        if colour is None:
            r = dict(L=S.lab_l(g))
        else:
            bgr = bgr_of(g, colour)
            r = dict(bgr=bgr, L=S.lab_l_bgr(bgr))
        r['cl'] = S.clahe(r['L'])
        pl, bk, bx = expected(r['cl'][None])
        r['planes'], r['buckets'], r['box'] = pl[0], bk[0], bx[0]
        for v in r.values():
            v.setflags(write=False)
        _REF[key] = r
    return _REF[key]
