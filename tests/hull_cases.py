"""Inputs for the hull stage on its own (cpe_debug_region_hull, include/cpe.h): largest external contour -> convex hull ->
filled polygon -> boundingRect.  One idea per case, on the smallest frame that still reaches the path the case is named for;
tests/test_hull_generators_cpu.py proves with the oracle alone that every case does what its name says.

A case is a boolean mask.  Mode 0 (the cylinder target's tail) is given mask * 255; mode 1 (the planar target's region stage,
threshold 127) is given grey_of(mask): 128 on every set pixel that has a background neighbour, 127 on every background pixel
that has a set neighbour, so every mask with a border puts 127 next to 128 all along it (`grey_127_128` is the case named
for it); inside, the set runs through 128 .. 255 and the background through 0 .. 127.

Mode 0 has the product's precondition: a mask with exactly ONE component gives that component a contour of positive area (the
kernel does not trace a lone component).  MODE0[name] is False for the few masks that break it; they run in mode 1 only.

What no valid mask can put in front of the kernels:
  - a region rectangle one row high: a contour of positive area spans two rows, and the planar target's second round sees a
    set that is at least 11 rows high.  The one-row sets are here as zero-area contours (status 1);
  - edges of slope 1/3 or 5/7 that run 3000 rows in a frame 96 columns wide (1/3 needs 1000 columns).  The 4096 x 96 frame has
    edges of slope 1/33, -1/33 and 5/231 over about 3000 rows, which pass through a pixel centre every 33 / 231 rows, and the
    2048 x 2048 frame has edges of slope 1/3, -1/3 and 5/7 over 1980 / 1960 rows."""
import functools

import numpy as np

G = (200, 336)            # the general frame: w % 16 == 0, w % 64 != 0, h % 32 != 0
TALL = (4096, 96)
WIDE = (96, 1104)
HR_ROWS = 64              # csrc/region.hip: rows per band of k_hull_rows
LDS_W = 2048              # csrc/region.hip: HULL_LDS_W
AREA_TURN = 64 * 64       # components one turn of k_region_area's grid takes: frame_waves(n, 8, 64) = 64 workgroups of 64 lanes per
                          # frame in a call of n <= 256 frames (fewer in larger calls, never more)
MAXROOTS = 262144         # csrc/cpe_dev.h
OVF_ROOTS = 1             # csrc/cpe_dev.h FrameState::overflow bit

REGISTRY = {}             # name -> (h, w, function -> bool mask, claims)
MODE0 = {}


def case(name, shape, claims=None, mode0=True):
    def deco(fn):
        assert name not in REGISTRY, name
        REGISTRY[name] = (shape[0], shape[1], fn, dict(claims or {}))
        MODE0[name] = mode0
        return fn
    return deco


def add(name, shape, fn, claims=None, mode0=True):
    case(name, shape, claims, mode0)(fn)


@functools.lru_cache(maxsize=None)
def _mask_small(name):
    h, w, fn, _ = REGISTRY[name]
    m = np.ascontiguousarray(fn(), bool)
    assert m.shape == (h, w), (name, m.shape)
    m.setflags(write=False)
    return m


def mask(name):
    h, w, fn, _ = REGISTRY[name]
    if h * w > (1 << 21):          # the large frames are made when asked for, not kept
        m = np.ascontiguousarray(fn(), bool)
        assert m.shape == (h, w), (name, m.shape)
        return m
    return _mask_small(name)


def shape_of(name):
    return REGISTRY[name][:2]


def claims(name):
    return REGISTRY[name][3]


def grey_of(m):
    """the mode-1 input (threshold 127): every set pixel with a background neighbour is 128 and every background pixel with a
    set neighbour is 127, so the set's whole border puts the two values side by side; the other set pixels run through
    128 .. 255 and the other background pixels through 0 .. 127"""
    from scipy.ndimage import binary_dilation
    h, w = m.shape
    y, x = np.ogrid[:h, :w]
    g = np.where(m, 128 + (x + y) % 128, (7 * x + 3 * y) % 128).astype(np.uint8)
    eight = np.ones((3, 3), bool)
    g[m & binary_dilation(~m, eight)] = 128
    g[~m & binary_dilation(m, eight)] = 127
    return g


def blank(shape):
    return np.zeros(shape, bool)


def columns(shape, x0, lo, hi):
    """mask with column x0 + i set from row lo[i] to row hi[i], both inclusive"""
    m = blank(shape)
    for i, (a, b) in enumerate(zip(lo, hi)):
        m[int(a):int(b) + 1, x0 + i] = True
    return m


def rect(shape, y0, x0, y1, x1):
    m = blank(shape)
    m[y0:y1 + 1, x0:x1 + 1] = True
    return m


def with_far_pixel(m):
    """the mask with one isolated pixel in the frame corner farthest from the shape (a second component of zero area): n_roots = 2"""
    h, w = m.shape
    ys, xs = np.nonzero(m)
    best = None
    for cy, cx in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):
        d = int(np.min(np.maximum(np.abs(ys - cy), np.abs(xs - cx))))
        if best is None or d > best[0]:
            best = (d, cy, cx)
    assert best[0] >= 2, 'no room for an isolated pixel'
    out = m.copy()
    out[best[1], best[2]] = True
    return out


# ---------------------------------------------------------------- polygons with exact and near collinearity
for _k, (_y0, _x0, _y1, _x1) in {'2x2': (50, 60, 51, 61), '2x3': (50, 60, 51, 62), '3x2': (50, 60, 52, 61), '17x33': (40, 100, 56, 132)}.items():
    add('rect_' + _k, G, functools.partial(rect, G, _y0, _x0, _y1, _x1), dict(comps=1, nv=4, rect=(_x0, _y0, _x1 - _x0 + 1, _y1 - _y0 + 1)))
add('full_frame', G, lambda: np.ones(G, bool), dict(comps=1, nv=4, rect=(0, 0, G[1], G[0])))


def diamond(shape, cy, cx, r):
    y, x = np.ogrid[:shape[0], :shape[1]]
    return (np.abs(x - cx) + np.abs(y - cy)) <= r


add('diamond_r1', G, functools.partial(diamond, G, 70, 90, 1), dict(comps=1, nv=4, area=2.0))
add('diamond_r20', G, functools.partial(diamond, G, 70, 90, 20), dict(comps=1, nv=4, collinear=30))
add('diamond_r99', G, functools.partial(diamond, G, 99, 168, 99), dict(comps=1, nv=4, collinear=300))


def triangle(shape, y0, x0, length, p, q, flip_x=False, flip_y=False):
    """right triangle under the edge of slope p / q: column i holds rows y0 .. y0 + floor(i * p / q); its stair corners
    (q j, p j) lie exactly on the edge"""
    i = np.arange(length + 1)
    top = i * p // q
    m = columns(shape, x0, np.full_like(i, y0), y0 + top)
    if flip_x:
        m = m[:, ::-1]
    if flip_y:
        m = m[::-1]
    return np.ascontiguousarray(m)


for _p, _q in ((1, 2), (1, 3), (5, 7)):
    _len = 20 * _q
    add(f'tri_{_p}_{_q}', G, functools.partial(triangle, G, 30, 40, _len, _p, _q), dict(comps=1, nv=3, collinear=15))
    add(f'tri_m{_p}_{_q}', G, functools.partial(triangle, G, 30, 40, _len, _p, _q, True), dict(comps=1, nv=3, collinear=15))
    add(f'tri_{_p}_{_q}_up', G, functools.partial(triangle, G, 30, 40, _len, _p, _q, False, True), dict(comps=1, nv=3, collinear=15))
    add(f'tri_m{_p}_{_q}_up', G, functools.partial(triangle, G, 30, 40, _len, _p, _q, True, True), dict(comps=1, nv=3, collinear=15))


def stair(kind, flip_y=False):
    """the slope-1/3 triangle of 30 steps; 'out': one stair corner one pixel beyond the edge (a vertex more), 'in': one corner
    one pixel short of it (the hull does not change: the corner is cut out of it)"""
    i = np.arange(91)
    top = i // 3
    if kind == 'out':
        top[45] += 1
    elif kind == 'in':
        top[45:48] -= 1
    m = columns(G, 50, np.full_like(i, 60), 60 + top)
    return np.ascontiguousarray(m[::-1]) if flip_y else m


for _fl in (False, True):
    _s = '_up' if _fl else ''
    add('stair_on' + _s, G, functools.partial(stair, 'on', _fl), dict(comps=1, nv=3, collinear=28))
    add('stair_out' + _s, G, functools.partial(stair, 'out', _fl), dict(comps=1, nv=4, one_more_than='stair_on' + _s))
    add('stair_in' + _s, G, functools.partial(stair, 'in', _fl), dict(comps=1, nv=3, same_hull_as='stair_on' + _s))


def lens():
    """between y = x (x + 1) / 2 and its point mirror, 80 columns: both chains strictly convex, every column a vertex of each"""
    x = np.arange(80)
    lo = x * (x + 1) // 2
    hi = 3160 - (79 - x) * (80 - x) // 2
    return columns(TALL, 8, 20 + lo, 20 + hi)


add('lens', TALL, lens, dict(comps=1, nv=158, rect=(8, 20, 80, 3161)))


def ends(first, last):
    """a hexagon whose first / last column holds 1 pixel, 2 pixels or a run of 21"""
    up = {1: 0, 2: 0, 21: 10}
    dn = {1: 0, 2: 1, 21: 10}
    i = np.arange(60)
    lo = 80 - np.minimum(np.minimum(up[first] + i, 14), up[last] + (59 - i))
    hi = 80 + np.minimum(np.minimum(dn[first] + i, 14), dn[last] + (59 - i))
    return columns(G, 100, lo, hi)


for _a in (1, 2, 21):
    for _b in (1, 2, 21):
        add(f'ends_{_a}_{_b}', G, functools.partial(ends, _a, _b), dict(comps=1, first_col=_a, last_col=_b))


# ---------------------------------------------------------------- concave and holed shapes
def comb():
    m = rect(G, 120, 60, 125, 200)
    for x in range(60, 201, 10):
        m[40 + (x % 30):121, x:x + 3] = True
    return m


def c_shape():
    m = rect(G, 40, 80, 140, 180)
    m[60:121, 100:181] = False
    return m


def u_shape():
    m = rect(G, 40, 80, 140, 180)
    m[40:121, 100:161] = False
    return m


def ring(cy=90, cx=170, r1=60, r0=50):
    y, x = np.ogrid[:G[0], :G[1]]
    d = (x - cx) ** 2 + (y - cy) ** 2
    return (d <= r1 * r1) & (d > r0 * r0)


def ring_block():
    """a thin square ring, a block in its hole with more pixels than the ring, and a free block outside with fewer than the nested one"""
    m = rect(G, 30, 40, 109, 119)
    m[32:108, 42:118] = False
    m[45:95, 55:105] = True
    m[140:170, 200:230] = True
    return m


add('comb', G, comb, dict(comps=1, concave=True))
add('c_shape', G, c_shape, dict(comps=1, nv=4, concave=True))
add('u_shape', G, u_shape, dict(comps=1, nv=4, concave=True))
add('ring', G, ring, dict(comps=1, holes=1))
add('ring_block', G, ring_block, dict(comps=3, nested_larger=True, rect=(40, 30, 80, 80)))


def carved(seed, k=9):
    """the oracle-filled hull of k random lattice points, with notches cut into its border and holes into its inside; the
    3 x 3 neighbourhoods of the vertex pixels and every pixel's link to the rest are kept"""
    from oracle import stages as S
    from scipy import ndimage
    rng = np.random.default_rng(seed)
    pts = np.stack([rng.integers(20, G[1] - 20, k), rng.integers(20, G[0] - 20, k)], 1).astype(np.int32)
    hull = S.convex_hull(pts)
    full = S.fill_poly(G, hull) > 0
    keep = blank(G)
    for x, y in hull:
        keep[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = True
    m = full.copy()
    for _ in range(120):
        y, x = int(rng.integers(0, G[0])), int(rng.integers(0, G[1]))
        hh, ww = int(rng.integers(3, 30)), int(rng.integers(3, 30))
        trial = m.copy()
        trial[y:y + hh, x:x + ww] = False
        trial |= keep & full
        if ndimage.label(trial, np.ones((3, 3)))[1] == 1:
            m = trial
    return m


for _seed in (1, 2, 3, 4):
    add(f'carved_{_seed}', G, functools.partial(carved, _seed), dict(comps=1, carved=True))


# ---------------------------------------------------------------- selection among components
def blocks(*items):
    """items: (y0, x0, height, width[, cut]): a filled block; cut: its top-left corner pixel removed (contour area - 0.5)"""
    m = blank(G)
    for it in items:
        y0, x0, hh, ww = it[:4]
        m[y0:y0 + hh, x0:x0 + ww] = True
        if len(it) > 4 and it[4]:
            m[y0, x0] = False
    return m


# contourArea of an a x b block of pixels is (a - 1) (b - 1): 10 x 10 -> 81 = 4 x 28 = 2 x 82
add('tie2_square_first', G, functools.partial(blocks, (20, 30, 10, 10), (60, 200, 4, 28)), dict(comps=2, tie=2, winner_rect=(200, 60, 28, 4)))
add('tie2_bar_first', G, functools.partial(blocks, (20, 200, 4, 28), (60, 30, 10, 10)), dict(comps=2, tie=2, winner_rect=(30, 60, 10, 10)))
add('tie2_same_row', G, functools.partial(blocks, (20, 30, 10, 10), (20, 200, 4, 28)), dict(comps=2, tie=2, winner_rect=(200, 20, 28, 4)))
add('tie3', G, functools.partial(blocks, (20, 30, 10, 10), (60, 200, 4, 28), (120, 100, 2, 82)), dict(comps=3, tie=3, winner_rect=(100, 120, 82, 2)))
add('half_less_later', G, functools.partial(blocks, (20, 30, 10, 10), (60, 200, 10, 10, True)), dict(comps=2, margin=0.5, winner_rect=(30, 20, 10, 10)))
add('half_more_later', G, functools.partial(blocks, (20, 30, 10, 10, True), (60, 200, 10, 10)), dict(comps=2, margin=0.5, winner_rect=(200, 60, 10, 10)))


def pixels_vs_area():
    """a one-pixel-wide square ring (316 pixels, contour area 79 x 79) and a solid block (900 pixels, area 29 x 29)"""
    m = rect(G, 20, 30, 99, 109)
    m[21:99, 31:109] = False
    m[120:150, 200:230] = True
    return m


add('pixels_vs_area', G, pixels_vs_area, dict(comps=2, fewer_pixels_wins=True, winner_rect=(30, 20, 80, 80)))


def specks(with_shape=True):
    """isolated pixels on the even lattice, more than one turn of k_region_area's grid, and one block of positive area"""
    m = blank(G)
    m[0::2, 0::2] = True
    m[80:121, 130:201] = False
    if with_shape:
        m[84:117, 134:197] = True
    return m


add('specks_and_block', G, specks, dict(min_comps=AREA_TURN + 1, winner_rect=(134, 84, 63, 33)))


def zero_area():
    """1-px lines (one of them a whole row: a region rectangle one row high if it were chosen), diagonals, isolated pixels"""
    m = blank(G)
    m[10, 20:120] = True
    m[30:90, 15] = True
    for i in range(40):
        m[100 + i, 40 + i] = True
        m[100 + i, 140 - i] = True
    m[150:180, 200] = True
    m[5, 300] = True
    m[190, 10] = True
    m[199, 150:336] = True
    return m


def l_shape():
    """a one-pixel-wide L beside a line: cv2.findContours passes the L's corner on the outside only, so its contour encloses
    half a pixel -- the smallest positive area -- and it wins over the zero-area line"""
    m = blank(G)
    m[150:180, 200] = True
    m[179, 200:240] = True
    m[20, 30:300] = True
    return m


add('zero_area_only', G, zero_area, dict(min_comps=7, status=1))
add('l_shape_half_area', G, l_shape, dict(comps=2, area=0.5, nv=3, winner_rect=(200, 150, 40, 30)))
add('empty', G, lambda: blank(G), dict(comps=0, status=1))
# mode 1's threshold: a block whose border pixels are 128 in a ring of background pixels that are 127 (grey_of)
add('grey_127_128', G, functools.partial(rect, G, 60, 100, 99, 179), dict(comps=1, nv=4, rect=(100, 60, 80, 40), grey_edge=True))
add('one_pixel', G, lambda: rect(G, 90, 170, 90, 170), dict(comps=1, status=1), mode0=False)
add('one_row', G, lambda: rect(G, 90, 20, 90, 300), dict(comps=1, status=1), mode0=False)
add('one_column', G, lambda: rect(G, 10, 170, 190, 170), dict(comps=1, status=1), mode0=False)


# ---------------------------------------------------------------- frame and band edges
def border_cases(shape, tag):
    h, w = shape
    a, b = min(20, h // 3), min(30, w // 3)
    out = {
        'top': (0, w // 2 - b // 2, a, w // 2 + b // 2), 'bottom': (h - 1 - a, w // 2 - b // 2, h - 1, w // 2 + b // 2),
        'left': (h // 2 - a // 2, 0, h // 2 + a // 2, b), 'right': (h // 2 - a // 2, w - 1 - b, h // 2 + a // 2, w - 1),
        'tl': (0, 0, a, b), 'tr': (0, w - 1 - b, a, w - 1), 'bl': (h - 1 - a, 0, h - 1, b), 'br': (h - 1 - a, w - 1 - b, h - 1, w - 1),
    }
    for k, (y0, x0, y1, x1) in out.items():
        def fn(y0=y0, x0=x0, y1=y1, x1=x1, k=k):
            m = rect(shape, y0, x0, y1, x1)
            # not a plain rectangle: the corner that does not touch a border is cut off, so the hull has a slanted edge
            yy, xx = np.ogrid[:h, :w]
            cy, cx = (y1 if y0 == 0 or k in ('left', 'right') else y0), (x1 if x0 == 0 else x0)
            if k in ('top', 'bottom'):
                cx = x1
            m &= (np.abs(yy - cy) + np.abs(xx - cx)) > 6
            return m
        add(f'touch_{k}{tag}', shape, fn, dict(comps=1, touches=k))


border_cases(G, '')


def slanted(y0, height):
    """a parallelogram `height` rows high from row y0: row r spans columns 60 + r // 2 .. 130 + r // 3"""
    m = blank(G)
    for r in range(height):
        m[y0 + r, 60 + r // 2:131 + r // 3] = True
    return m


for _hh in (2, 63, 64, 65, 128, 129):
    for _y0 in (0, 1, 63):
        add(f'rows_{_hh}_at_{_y0}', G, functools.partial(slanted, _y0, _hh), dict(comps=1, rect_y=_y0, rect_h=_hh, bands=(_hh - 1 + HR_ROWS - 1) // HR_ROWS))


def span_shape(shape, x1, x2, y0=40, rows=9):
    """rows of one span x1 .. x2, with a one-pixel-narrower row above and below (a hull of 8 vertices, spans of two lengths)"""
    m = rect(shape, y0, x1, y0 + rows - 1, x2)
    if x2 - x1 >= 2:
        m[y0 - 1, x1 + 1:x2] = True
        m[y0 + rows, x1 + 1:x2] = True
    return m


for _a in (0, 1, 15):
    for _b in (14, 15, 0):
        _x1, _x2 = 96 + _a, 224 + (_b if _b else 16)
        add(f'span_{_a}_{_b}', G, functools.partial(span_shape, G, _x1, _x2), dict(comps=1, span=(_x1, _x2), x1_mod=_a, x2_mod=_b))
for _x1, _x2 in ((97, 101), (110, 113), (127, 129), (143, 158), (144, 159), (145, 160)):
    add(f'short_span_{_x1}_{_x2}', G, functools.partial(span_shape, G, _x1, _x2), dict(comps=1, span=(_x1, _x2), short=True))
add('long_span_rect', WIDE, functools.partial(span_shape, WIDE, 20, 1090), dict(comps=1, span=(20, 1090), long=True))
add('long_span_odd', WIDE, functools.partial(span_shape, WIDE, 3, 1101), dict(comps=1, span=(3, 1101), long=True))
add('long_span_tri', WIDE, functools.partial(triangle, WIDE, 5, 10, 1079, 1, 13), dict(comps=1, nv=3, long=True))
add('long_span_full', WIDE, lambda: np.ones(WIDE, bool), dict(comps=1, nv=4, long=True, rect=(0, 0, WIDE[1], WIDE[0])))


# ---------------------------------------------------------------- widths
def hexagon(shape, y0, x0, hh, ww, cut):
    m = rect(shape, y0, x0, y0 + hh - 1, x0 + ww - 1)
    yy, xx = np.ogrid[:shape[0], :shape[1]]
    for cy, cx in ((y0, x0), (y0 + hh - 1, x0 + ww - 1)):
        m &= (np.abs(yy - cy) * 2 + np.abs(xx - cx)) > cut
    return m


for _shape, _tag in (((96, 64), '_w64'), ((96, 80), '_w80'), ((70, 83), '_w83'), ((96, 320), '_w320')):
    border_cases(_shape, _tag)
    add('full_frame' + _tag, _shape, functools.partial(np.ones, _shape, bool), dict(comps=1, nv=4, rect=(0, 0, _shape[1], _shape[0])))
    add('hexagon' + _tag, _shape, functools.partial(hexagon, _shape, 10, 7, 50, 50, 20), dict(comps=1, min_nv=6))
    add('last_columns' + _tag, _shape, functools.partial(hexagon, _shape, 5, _shape[1] - 22, 40, 22, 12), dict(comps=1, min_nv=6, touches='right'))
    add('tri_5_7' + _tag, _shape, functools.partial(triangle, _shape, 8, 6, 49, 5, 7), dict(comps=1, nv=3))
    add('two_blocks' + _tag, _shape, (lambda s=_shape: rect(s, 5, 5, 14, 14) | rect(s, 40, s[1] - 30, 43, s[1] - 3)), dict(comps=2, tie=2))
add('span_83', (70, 83), functools.partial(span_shape, (70, 83), 16, 63, 30, 5), dict(comps=1, span=(16, 63)))

for _w in (2048, 2064, 2049):
    _shape = (96, _w)
    add(f'wide_hexagon_w{_w}', _shape, functools.partial(hexagon, _shape, 6, 5, 80, 2030, 60), dict(comps=1, min_nv=6, span_over=1024))
    add(f'wide_tri_w{_w}', _shape, functools.partial(triangle, _shape, 4, 3, 1989, 2, 51), dict(comps=1, nv=3, collinear=30))
    add(f'wide_lens_w{_w}', _shape, (lambda s=_shape: columns(s, 700, 48 - np.round(np.sqrt(np.arange(1300) * (1299 - np.arange(1300.0))) / 15).astype(int),
                                                                  48 + np.round(np.sqrt(np.arange(1300) * (1299 - np.arange(1300.0))) / 16).astype(int))),
        dict(comps=1, min_nv=40))
    add(f'wide_right_w{_w}', _shape, functools.partial(hexagon, _shape, 20, _w - 40, 50, 40, 16), dict(comps=1, min_nv=6, touches='right'))
    add(f'wide_two_w{_w}', _shape, (lambda s=_shape: rect(s, 5, 100, 24, 119) | hexagon(s, 30, 1500, 40, 500, 30)), dict(comps=2))
    add(f'wide_full_w{_w}', _shape, functools.partial(np.ones, _shape, bool), dict(comps=1, nv=4, rect=(0, 0, _w, 96)))
SAME_2048_2064 = ('wide_hexagon', 'wide_tri', 'wide_lens', 'wide_two')      # shapes at the same offset in both frames


# ---------------------------------------------------------------- tall frames, many vertices
def polygon(shape, pts):
    """the pixels inside or on the convex polygon pts (x, y), by exact integer half-plane tests: its hull is pts"""
    y, x = np.ogrid[:shape[0], :shape[1]]
    x = x.astype(np.int64); y = y.astype(np.int64)
    pts = [tuple(int(v) for v in p) for p in pts]
    sign = 0
    for (ax, ay), (bx, by), (cx, cy) in zip(pts, pts[1:] + pts[:1], pts[2:] + pts[:2]):
        sign += np.sign((bx - ax) * (cy - ay) - (by - ay) * (cx - ax))
    assert abs(sign) == len(pts), 'not strictly convex'
    m = np.ones(shape, bool)
    for (ax, ay), (bx, by) in zip(pts, pts[1:] + pts[:1]):
        m &= ((bx - ax) * (y - ay) - (by - ay) * (x - ax)) * (1 if sign > 0 else -1) >= 0
    return m


# (x, y): edges of slope dx / dy = 1/33, -1/33 and 5/231 over 2970 / 3003 rows
add('tall_p1_33', TALL, functools.partial(polygon, TALL, [(3, 20), (93, 2990), (3, 2990)]), dict(comps=1, nv=3, long_edge=(90, 2970)))
add('tall_m1_33', TALL, functools.partial(polygon, TALL, [(93, 20), (3, 2990), (93, 2990)]), dict(comps=1, nv=3, long_edge=(-90, 2970)))
add('tall_5_231', TALL, functools.partial(polygon, TALL, [(10, 50), (75, 3053), (40, 3053), (10, 1000)]), dict(comps=1, nv=4, long_edge=(65, 3003)))
add('tall_sliver', TALL, functools.partial(polygon, TALL, [(50, 0), (40, 4095), (60, 4095)]), dict(comps=1, nv=3, touches='tb'))
add('tall_full', TALL, functools.partial(np.ones, TALL, bool), dict(comps=1, nv=4, rect=(0, 0, 96, 4096)))

BIG = (2048, 2048)
HUGE = (4096, 4096)


def disc(shape, r):
    c = shape[0] // 2 - 1
    y, x = np.ogrid[:shape[0], :shape[1]]
    return ((x - c) ** 2 + (y - c) ** 2) <= r * r


add('disc_1020', BIG, functools.partial(disc, BIG, 1020), dict(comps=1, min_nv=300))
add('slopes_third', BIG, functools.partial(polygon, BIG, [(1024, 20), (364, 2000), (1684, 2000)]), dict(comps=1, nv=3, long_edge=(660, 1980)))
add('slope_5_7', BIG, functools.partial(polygon, BIG, [(30, 40), (1430, 2000), (30, 2000)]), dict(comps=1, nv=3, long_edge=(1400, 1960)))
add('disc_2040', HUGE, functools.partial(disc, HUGE, 2040), dict(comps=1, min_nv=500))


# ---------------------------------------------------------------- planar extras (they run in mode 0 as well)
def near(shape, which, d, size=2):
    h, w = shape
    y0 = {'t': d, 'b': h - size - d}.get(which[0], h // 2)
    x0 = {'l': d, 'r': w - size - d}.get(which[-1], w // 2)
    return rect(shape, y0, x0, y0 + size - 1, x0 + size - 1)


for _which in ('tl', 'tr', 'bl', 'br', 't', 'b', 'l', 'r'):
    for _d in (0, 3, 5):
        _nm = {'t': 't_', 'b': 'b_', 'l': '_l', 'r': '_r'}.get(_which, _which)
        add(f'near_{_which}_{_d}', G, functools.partial(near, G, _nm, _d), dict(comps=1, nv=4, dilation_clipped=_d < 5))
claims('near_tl_0')['rect1'] = (0, 0, 7, 7)

for _d in range(-5, 6):
    add(f'tile_edges_{_d:+d}', G, functools.partial(rect, G, 32 + _d, 64 + _d, 95 + _d, 191 + _d), dict(comps=1, nv=4, tile_d=_d))


# ---------------------------------------------------------------- the second extent path: every one-component case again with a far pixel
for _name in [k for k, v in REGISTRY.items() if v[3].get('comps') == 1 and MODE0[k] and v[3].get('rect') != (0, 0, v[1], v[0]) and (v[0], v[1]) != HUGE]:
    _h, _w = shape_of(_name)
    add(_name + '+px', (_h, _w), (lambda nm=_name: with_far_pixel(mask(nm))), dict(comps=2, same_as=_name))


def names_of(shape):
    return [k for k, v in REGISTRY.items() if (v[0], v[1]) == tuple(shape)]


SHAPES = sorted({(v[0], v[1]) for v in REGISTRY.values()})


def isolated_pixels(shape=(1026, 1024)):
    """more components than the root list holds"""
    m = blank(shape)
    m[0::2, 0::2] = True
    return m


# ---------------------------------------------------------------- the reference: the oracle's primitives composed
def largest_hull(mask255, need_positive):
    """what orc_plane.c's largest_hull_mask does, from the oracle's primitives: -> dict(status, mask, rect, hull, contour,
    areas (OpenCV order), best)"""
    from oracle import stages as S
    m = np.ascontiguousarray(mask255, np.uint8)
    cs = S.find_contours(m, 'external', 'simple')
    areas = [S.contour_area(p) for p, _ in cs]
    best, ba = -1, (0.0 if need_positive else -1.0)
    for i, a in enumerate(areas):
        if a > ba:
            ba, best = a, i
    if best < 0:
        return dict(status=1, mask=np.zeros_like(m), rect=None, hull=np.zeros((0, 2), np.int32), contour=None, areas=areas, best=-1)
    pts = cs[best][0]
    hull = S.convex_hull(pts)
    return dict(status=0, mask=S.fill_poly(m.shape, hull), rect=S.bounding_rect(pts), hull=hull, contour=pts, areas=areas, best=best)


def reference(m, mode):
    """mode 0: largest_hull(mask, need_positive = 1).  mode 1: get_convex_hull(grey, 127, 5) composed: the hull of the set, dilated
    by ellipse_se(11) with scipy's binary_dilation, and the hull of that; 'round1' holds the first round"""
    from oracle import stages as S
    from scipy.ndimage import binary_dilation
    if mode == 0:
        return largest_hull(np.where(m, 255, 0), 1)
    r1 = largest_hull(np.where(grey_of(m) > 127, 255, 0), 1)
    if r1['status']:
        return dict(r1, round1=r1)
    dil = binary_dilation(r1['mask'] > 0, S.ellipse_se(11) > 0)
    return dict(largest_hull(np.where(dil, 255, 0), 0), round1=r1, dilated=dil)
