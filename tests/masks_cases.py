"""Inputs for the masks stage on its own (cpe_debug_masks, include/cpe.h): one idea per generator, small frames unless the
edge needs a big one.  A case is dict(binary, gray, mc, rect, status): the pre-process's ridge mask, the grey frame, the
region stage's mask_contour (zero outside rect), its boundingRect (x, y, w, h) and its status (0 or 1 = CPE_ST_NO_REGION).
The oracle side of every case and the checks that each generator reaches the edge it is named for live in
tests/test_masks_generators_cpu.py; tests/test_masks_stage_gpu.py runs the cases through the kernels."""
import numpy as np

MAXJ = 16384            # include/cpe.h CPE_MAXJ
MAXSEG = 2048           # csrc/cpe_dev.h: valid fragments per mask
EXP_MAXKS = 176         # csrc/masks.hip: largest expansion kernel of the cylinder script (91 + r0)
SPOT_ROWS = 1024        # csrc/masks.hip: ellipse rows kept in LDS by k_spot_ellipse
OVF_JOINTS, OVF_SEGS, OVF_KERNEL = 8, 32, 64      # csrc/cpe_dev.h FrameState::overflow bits


def case(binary, gray=None, rect=None, status=0, spot=None):
    """binary u8 [h,w] (0 / 255); gray: default a dark frame with one saturated disc (spot = (cx, cy, radius), default
    radius 12 near the bottom-right corner); rect: default the whole frame; mask_contour = rect's pixels"""
    binary = np.where(np.asarray(binary) != 0, 255, 0).astype(np.uint8)
    h, w = binary.shape
    if gray is None:
        gray = np.zeros((h, w), np.uint8)
        cx, cy, r = spot if spot is not None else (w - 24, h - 24, 12)
        disc(gray, cx, cy, r)
    if rect is None:
        rect = (0, 0, w, h)
    x, y, rw, rh = rect
    mc = np.zeros((h, w), np.uint8)
    mc[y:y + rh, x:x + rw] = 255
    return dict(binary=binary, gray=np.ascontiguousarray(gray, np.uint8), mc=mc, rect=tuple(int(v) for v in rect), status=status)


def disc(img, cx, cy, r, v=255):
    h, w = img.shape
    yy, xx = np.mgrid[:h, :w]
    img[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = v
    return img


def bar(img, x0, y0, bw, bh, chamfers=(), k=3):
    """filled bw x bh rectangle; chamfers: corners ('tl', 'tr', 'bl', 'br') cut at 45 degrees by k pixels -- each adds one
    contour vertex (CHAIN_APPROX_SIMPLE), and the 3x3 opening / closing of the masks stage keep the cut"""
    yy, xx = np.mgrid[:bh, :bw]
    m = np.ones((bh, bw), bool)
    for c in chamfers:
        dx = xx if c[1] == 'l' else bw - 1 - xx
        dy = yy if c[0] == 't' else bh - 1 - yy
        m &= dx + dy >= k
    img[y0:y0 + bh, x0:x0 + bw][m] = 255
    return img


def staircase(img, x0, y0, steps, chamfers=(), run=24, dx=4, thick=3):
    """a band falling one row every dx columns: `steps` bars of run x thick, each dx to the right of and one row below the
    last -- about four contour vertices per step; chamfers on the first / last bar ('tl', 'bl' / 'tr', 'br') add one each"""
    for i in range(steps):
        ch = tuple(c for c in chamfers if (c[1] == 'l' and i == 0) or (c[1] == 'r' and i == steps - 1))
        bar(img, x0 + dx * i, y0 + i, run, thick, ch)
    return img


def thick_line(img, x0, y0, x1, y1, t=4):
    """pixels within t / 2 of the segment (x0, y0) - (x1, y1)"""
    h, w = img.shape
    yy, xx = np.mgrid[:h, :w].astype(np.float64)
    d = np.array([x1 - x0, y1 - y0], np.float64)
    L2 = float(d @ d)
    s = np.clip(((xx - x0) * d[0] + (yy - y0) * d[1]) / L2, 0, 1)
    dist2 = (xx - x0 - s * d[0]) ** 2 + (yy - y0 - s * d[1]) ** 2
    img[dist2 <= (t / 2.0) ** 2] = 255
    return img


def mirrored(a):
    """a square image whose content lies above the diagonal (x > y): the content for the horizontal masks, its transpose for
    the vertical ones (disjoint)"""
    return np.maximum(a, a.T)


# ---------------------------------------------------------------- joints chain (k_open20_joints, k_joint_centroids)
RUN_LENS = (19, 20, 21)


def gen_runs_h(h=460, w=200):
    """horizontal runs of 19, 20, 21 pixels starting at every offset around the 64-bit word edges 64 and 128 (a run may end
    on, before or after the edge) and touching both frame edges: one run per row, 3 rows apart"""
    b = np.zeros((h, w), np.uint8)
    starts = [64 * k + d for k in (1, 2) for d in range(-22, 2)]
    row = 1
    for L in RUN_LENS:
        for x0 in starts + [0, w - L]:
            b[row, x0:x0 + L] = 255
            row += 3
    assert row < h
    return case(b)


def gen_runs_v(h=192, w=600, band=64):
    """vertical runs of 19, 20, 21 pixels starting at y = band k - 22 .. band k + 20 (ending before, on or after the band
    edge, or starting on or after it) and touching the first and last rows; h at 64 k, 64 k + 1 and 64 k + 63 for the
    64-row bands of k_open20_joints<64>, band = 32 on a frame wider than 2880 for the 32-row bands of <32>"""
    b = np.zeros((h, w), np.uint8)
    starts = [band * k + d for k in (1, 2) for d in range(-22, 21) if band * k + d + 21 <= h]
    col = 1
    for L in RUN_LENS:
        for y0 in starts + [0, h - L]:
            b[y0:y0 + L, col] = 255
            col += 2
    assert col < w - 40
    return case(b, spot=(w - 20, h // 2, 12))


def gen_widths(h, w, seed=0):
    """random horizontal and vertical segments of 15 .. 45 pixels and a few crossings (joints), any width: w = 2880 still
    uses k_open20_joints<64>, w = 2881 switches to <32> (LDS budget), whose bands are 32 rows high"""
    rng = np.random.default_rng(seed + w)
    b = np.zeros((h, w), np.uint8)
    for _ in range(max(8, h * w // 600)):
        L = int(rng.integers(15, 46)); t = int(rng.integers(1, 4))
        if rng.random() < 0.5:
            x0 = int(rng.integers(-10, w)); y0 = int(rng.integers(0, h))
            b[y0:y0 + t, max(x0, 0):max(x0 + L, 0)] = 255
        else:
            x0 = int(rng.integers(0, w)); y0 = int(rng.integers(-10, h))
            b[max(y0, 0):max(y0 + L, 0), x0:x0 + t] = 255
    for x in range(20, w - 30, 97):            # crossings: joints of a few pixels
        b[40:42, x - 15:x + 15] = 255
        b[28:58, x:x + 2] = 255
    return case(b, spot=(w // 2, h // 2, 10))


def gen_joint_shapes(h=320, w=260):
    """joints of zero contour area (one pixel, one row of 5), of one unit of area (2 x 2), joints touching the frame border,
    a joint inside the hole of a ring-shaped joint (RETR_EXTERNAL drops it) and 21 x 21 joints whose centroids lie on either
    side of each edge of rect (x, x + w - 1 in; x - 1, x + w out)"""
    rx, ry, rw, rh = 60, 40, 150, 120
    b = np.zeros((h, w), np.uint8)
    b[70, 80:120] = 255; b[50:90, 100] = 255                 # one pixel
    b[100, 80:120] = 255; b[80:120, 104:109] = 255           # one row of 5 pixels
    b[130:132, 75:115] = 255; b[110:150, 90:92] = 255        # 2 x 2
    for cx, cy in ((rx, 90), (rx - 1, 125), (rx + rw - 1, 60), (rx + rw, 140), (170, ry), (130, ry - 1), (180, ry + rh - 1),
                   (140, ry + rh)):
        b[cy - 10:cy + 11, cx - 10:cx + 11] = 255
    b[0:22, 0:22] = 255; b[h - 23:h, w - 30:w] = 255; b[90:115, 0:21] = 255    # on the frame border
    # ring: 100 x 100 with 22-pixel walls, a 22 x 22 joint in the middle of its hole
    ring = np.zeros((100, 100), np.uint8); ring[:] = 255; ring[22:78, 22:78] = 0; ring[39:61, 39:61] = 255
    b[h - 105:h - 5, 2:102] = ring                           # below rect
    return case(b, rect=(rx, ry, rw, rh), spot=(135, 100, 10))


def gen_joint_lattice(h=560, w=560):
    """a lattice of 2-pixel lines, pitch 4: 140 x 140 = 19 600 joints of area 1 inside rect, more than CPE_MAXJ"""
    b = np.zeros((h, w), np.uint8)
    for k in range(0, h, 4):
        b[k:k + 2, :] = 255
    for k in range(0, w, 4):
        b[:, k:k + 2] = 255
    return case(b)


# ---------------------------------------------------------------- spot chain (k_spot_scan, k_blur19_spot, k_spot_ellipse)
def gen_spot_tiles(h=200, w=330):
    """saturated discs centred 9 px off 64 x 32 tile corners, on the frame's corners and edges (reflect-101) and in the last
    partial tile (w = 330, h = 200), plus the largest one; the blurred plane is compared on every pixel"""
    g = np.zeros((h, w), np.uint8)
    for cx, cy in ((64 - 9, 32 - 9), (128 + 9, 64 + 9), (192 - 9, 96 + 9), (256 + 9, 32 - 9), (64 + 9, 128 - 9), (256 - 9, 160 + 9),
                   (0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w // 2, 0), (0, 100), (w - 1, 100), (324, 196)):
        disc(g, cx, cy, 11)
    disc(g, 192 + 9, 160 - 9, 16)
    return case(np.zeros((h, w), np.uint8), gray=g)


def gen_plateau(h=128, w=200, with_241=True):
    """a 240 plateau (row sums exactly 240 * 256) with single 241 and 255 pixels (row sums just above it, blurred values
    still 240) and, with_241, a 40 x 40 block of 241 (row sums exactly 241 * 256: blurred 241, the spot)"""
    g = np.full((h, w), 30, np.uint8)
    g[10:h - 10, 10:w - 10] = 240
    rng = np.random.default_rng(5)
    for _ in range(30):            # 255 only left of x = 50: the tiles of the block (x >= 128, apron 12) see no row sum above 241 * 256
        y, x = rng.integers(12, h - 12), rng.integers(12, w - 12)
        g[y, x] = 255 if x < 50 else 241
    if with_241:
        g[40:80, 140:180] = 241
    return case(np.zeros((h, w), np.uint8), gray=g)


def gen_one_pixel_spot(h=64, w=96):
    """a 240 plateau with five 247 pixels: exactly one blurred pixel exceeds 240 (contour of one point: area 0, radius 0)"""
    g = np.full((h, w), 240, np.uint8)
    g[30, 39:42] = (247, 240, 247); g[31, 39:42] = 247
    return case(np.zeros((h, w), np.uint8), gray=g)


def gen_equal_spots(h=128, w=256):
    """two identical discs: equal contour areas, the first maximum in contour order is the spot"""
    g = np.zeros((h, w), np.uint8)
    disc(g, 60, 70, 14); disc(g, 190, 50, 14)
    return case(np.zeros((h, w), np.uint8), gray=g)


# disc radius -> r0 (the oracle's circle_radius0): 27 -> 21, 28 -> 22, 29 -> 23 (cr + 40 odd for 21 and 23: a and b round half
# to even), 35 -> 29 (rad < 30: + 20), 36 -> 30 (+ 5), 90 -> 85 (kernel 176 = EXP_MAXKS), 91 -> 86 (177: OVF_KERNEL)
SPOT_R0 = {21: 27, 22: 28, 23: 29, 29: 35, 30: 36, 85: 90, 86: 91}


def gen_spot_radius(r0, h=None, w=None, fragments=False):
    """one disc whose circle_radius0 is r0; fragments: short and long thick horizontal lines and their transposes beside it,
    so that the expansion kernel runs with kernel 91 + r0"""
    R = SPOT_R0[r0]
    n = max(2 * R + 140, 200) if h is None else h
    b = np.zeros((n, n), np.uint8)
    if fragments:
        a = np.zeros((n, n), np.uint8)
        bar(a, n - 80, 6, 64, 6, ('tl', 'br')); bar(a, n - 60, 20, 30, 6, ('tl',))
        b = mirrored(a)
    g = np.zeros((n, n), np.uint8)
    disc(g, n // 2, n // 2, R)
    return case(b, gray=g)


def gen_spot_cut(h=160, w=200):
    """a disc at the left edge: the ellipse (and the circle of the planar script) is cut by the frame"""
    g = np.zeros((h, w), np.uint8)
    disc(g, 4, 60, 20)
    return case(np.zeros((h, w), np.uint8), gray=g)


def gen_spot_tall(h=2160, w=3840):
    """4K frame, disc of radius 1012: r0 = 1007, an ellipse of 1039 rows, more than SPOT_ROWS (lane 0 fills the rest)"""
    g = np.zeros((h, w), np.uint8)
    disc(g, w // 2, h // 2, 1012)
    return case(np.zeros((h, w), np.uint8), gray=g)


# ---------------------------------------------------------------- fragment chain (k_roi_base, k_seg_trace, k_seg_expand)
def gen_chamfers(n=300):
    """fragments of 4 .. 8 contour vertices (rectangles with 0 .. 4 corners cut; 4 / 5 and 7 / 8 are the two scripts' lower
    limits) and a T of 15, axis-aligned, and squares
    (sxx == syy: the c == 0 branch of the 2 x 2 eigen-solver, and its general branch with a == d), in both masks"""
    a = np.zeros((n, n), np.uint8)
    cuts = ((), ('tl',), ('tl', 'br'), ('tl', 'tr', 'br'), ('tl', 'tr', 'bl', 'br'))
    x = 100
    for i, c in enumerate(cuts):
        bar(a, x, 6 + 14 * i, 40 + 6 * i, 6, c)
    bar(a, 160, 4, 24, 24); bar(a, 200, 4, 24, 24, ('tl',)); bar(a, 240, 4, 24, 24, ('tl', 'br'), k=5)
    bar(a, 200, 40, 40, 6, ('tl', 'tr', 'bl', 'br')); bar(a, 210, 46, 24, 6, ('br',))      # a T: 15 vertices
    bar(a, 180, 70, 60, 8, ('tr',)); bar(a, 250, 110, 40, 4)
    return case(mirrored(a), spot=(40, n - 40, 12))


def staircase_vertices(steps, chamfers):
    """contour vertex count of a staircase fragment after the masks stage's openings and closing (oracle)"""
    from oracle import stages as S
    img = np.zeros((24 + steps, 40 + 4 * steps), np.uint8)
    staircase(img, 8, 8, steps, chamfers)
    base = S.close_rect(S.open_rect(S.open_rect(img, 20, 1), 3, 3), 3, 3)
    cs = S.find_contours(base, 'external', 'simple')
    assert len(cs) == 1
    return len(cs[0][0])


# (steps, chamfers) of the staircases with 199 and 200 vertices (the 5 .. 200 window of the cylinder script: 200 is in) and
# 202 (out), 699 / 700 / 702 for the 8 .. 700 window of the planar one (a staircase has 4 vertices per step, a cut of its
# first or last top corner takes one away: 4 n - 3 is not in this family, comb() below makes 201 and 701);
# tests/test_masks_generators_cpu.py checks the counts
STAIRS = {199: (50, ('tl',)), 200: (50, ()), 202: (51, ('tl', 'tr')),
          699: (175, ('tl',)), 700: (175, ()), 702: (176, ('tl', 'tr'))}


def gen_stairs(counts, n):
    """staircase fragments with the given contour vertex counts (one per 16 rows), in both masks"""
    a = np.zeros((n, n), np.uint8)
    y = 4
    for c in counts:
        steps, ch = STAIRS[c]
        staircase(a, n - 48 - 4 * steps, y, steps, ch)
        y += steps + 8
    assert y < n - 48 - 4 * max(STAIRS[c][0] for c in counts)      # above the diagonal
    return case(mirrored(a), spot=(30, n - 30, 12))


def gen_nested(n=220):
    """a fragment in the hole of another (RETR_EXTERNAL drops it) and fragments of 4 .. 6 vertices around it"""
    a = np.zeros((n, n), np.uint8)
    bar(a, 80, 4, 120, 60, ('tl', 'br'))
    a[8:60, 102:178] = 0                                      # walls: 22 wide left / right, 4 thick top / bottom
    bar(a, 120, 30, 40, 5, ('tl', 'br'))                       # inside the hole
    bar(a, 150, 80, 40, 5, ('tr',))
    return case(mirrored(a), spot=(30, n - 30, 12))


def gen_clipped(h=180, w=240):
    """fragments cut by the frame edges (end points within 7 px of them: the 15 px patch and the support are clipped) and
    by rect"""
    b = np.zeros((h, w), np.uint8)
    thick_line(b, -10, 3, 50, 6); thick_line(b, w - 60, h - 5, w + 5, h - 2); thick_line(b, w - 50, 2, w + 10, 0)
    thick_line(b, 70, 50, 140, 54); thick_line(b, 60, 100, 150, 96)
    # rect (x >= 3) clips the first line above and this one
    thick_line(b, 2, 60, 5, 120); thick_line(b, w - 3, 40, w - 6, 110); thick_line(b, 180, 40, 184, 90)
    return case(b, rect=(3, 0, w - 3, h), spot=(120, 150, 10))


def gen_fan(n=520, count=17):
    """straight thick fragments of 60 x k pixels, k = -8 .. 8 (every integer end-point direction a 20-pixel opening keeps,
    0 degrees and, from the PCA end points, 180 included), long and short ones (the 0.8 * glen test), odd or even count;
    their transposes (+-90 degrees) in the vertical mask"""
    a = np.zeros((n, n), np.uint8)
    for i, k in enumerate(range(-8, -8 + count)):
        L = 60 if i % 3 else 90
        y = 12 + 22 * i
        thick_line(a, n - 10 - L, y, n - 10, y + k)
    assert not np.tril(a).any()             # above the diagonal: the transposes do not touch
    return case(mirrored(a), spot=(n - 40, n - 40, 12))      # the ellipse cuts neither the lines nor their transposes


def gen_many_fragments(h=600, w=800):
    """2 210 identical fragments (the spot's ellipse cuts 4 of them: 2 206 valid) of 5 vertices (3 rows apart: the closing does not join them) in the horizontal mask:
    more than MAXSEG valid fragments (OVF_SEGS)"""
    b = np.zeros((h, w), np.uint8)
    for y in range(2, h - 6, 7):
        for x in range(2, w - 28, 30):
            bar(b, x, y, 26, 4, ('tl',))
    return case(b, spot=(w - 16, h - 16, 12))


def comb(img, x0, y0, teeth, chamfers=(), step=False, H=6):
    """a 6-pixel-high bar with `teeth` 20 x 3 teeth (half on top, half below, 4 px apart: the closing keeps the gaps), its
    corners cut (chamfers), and with step a 24 x 3 block on its top-left end.  Vertex count (CHAIN_APPROX_SIMPLE, after the
    masks stage's openings and closing): 4, + 3 for the step, + 6 per tooth, + 1 per cut corner"""
    top = (teeth + 1) // 2
    W = 24 * top + 60
    bar(img, x0, y0, W, H, chamfers)
    if step:
        bar(img, x0, y0 - 3, 24, 3)
    for i in range(teeth):
        bar(img, x0 + 35 + 24 * (i // 2), y0 - 3 if i % 2 == 0 else y0 + H, 20, 3)
    return img


# vertex count -> comb(teeth, chamfers, step); tests/test_masks_generators_cpu.py checks every count
COMBS = {7: (0, (), True), 8: (0, ('bl',), True), 9: (0, ('bl', 'br'), True), 199: (32, (), True), 200: (32, ('bl',), True),
         201: (32, ('bl', 'br'), True), 202: (32, ('bl', 'br', 'tr'), True), 699: (115, ('bl', 'br'), True),
         700: (116, (), False), 701: (116, ('tl',), False), 702: (116, ('tl', 'tr'), False)}


def gen_counts(counts, w):
    """one comb per vertex count, 20 rows apart: the limits of the fragments' vertex window on both sides (5 .. 200: 199,
    200, 201, 202; 8 .. 700: 7, 8, 9 and 699, 700, 701, 702)"""
    h = 20 * len(counts) + 60
    b = np.zeros((h, w), np.uint8)
    for i, c in enumerate(counts):
        teeth, ch, step = COMBS[c]
        comb(b, 8, 10 + 20 * i, teeth, ch, step)
    return case(b, spot=(w - 24, h - 20, 12))


def bump_bar(img, x0, y0, W, H):
    """a W x H bar with a centred 24 x 3 bump on top (10 vertices): its PCA end points are its corners (x0, y0) and
    (x0 + W - 1, y0 + H - 1), so the fragment's direction is (W - 1, H - 1)"""
    bar(img, x0, y0, W, H)
    bar(img, x0 + (W - 24) // 2, y0 - 3, 24, 3)
    return img


def f32_angle(dx, dy):
    """expand_line_roi's angle of an end-point difference: -np.degrees(np.arctan2(dy, dx)) in float32, as orc_masks.c"""
    import math
    at = np.float32(math.atan2(float(dy), float(dx)))
    return -np.float32(at * np.float32(180.0 / math.pi))


def f32_length(dx, dy):
    import math
    return np.float32(math.hypot(float(dx), float(dy)))


def gen_angle_tie(h=120, w=260):
    """three fragments of directions (199, 3), (41, 7) and (103, 27): their float32 angles are -0.86, -9.6888 and -14.6888,
    the median is the second, and the third lies exactly 5.0f from it (fabsf(angle - median) > 5 is false: it keeps its own
    angle).  The first is the longest; the other two are expanded"""
    b = np.zeros((h, w), np.uint8)
    bump_bar(b, 10, 10, 200, 4); bump_bar(b, 10, 34, 42, 8); bump_bar(b, 70, 34, 104, 28)
    return case(b, spot=(w - 24, h - 24, 12))


def gen_length_tie(h=96, w=128):
    """two fragments of directions (35, 5) and (28, 4): float32 lengths 35.355339 and 28.284271, and (double) 28.284271 is
    exactly 0.8 * (double) 35.355339 -- the shorter one is expanded (len > 0.8 * glen is false)"""
    b = np.zeros((h, w), np.uint8)
    bump_bar(b, 8, 10, 36, 6); bump_bar(b, 60, 10, 29, 5)
    return case(b, spot=(w - 24, h - 24, 12))


def pad(c, h, w):
    """the case inside a larger frame (zeros to the right and below; rect unchanged)"""
    out = dict(c)
    for k in ('binary', 'gray', 'mc'):
        a = np.zeros((h, w), np.uint8)
        a[:c[k].shape[0], :c[k].shape[1]] = c[k]
        out[k] = a
    return out


def fragment_table(mask):
    """(vertex count, float32 angle, float32 length) of every external contour of the expansion's base = close3x3(mask), in
    the oracle's arithmetic (orc_masks.c: PCA end points, atan2 / hypot in double rounded to float)"""
    from oracle import stages as S
    out = []
    for p, _ in S.find_contours(S.close_rect(mask, 3, 3), 'external', 'simple'):
        p1, p2 = S.pca_endpoints(p.astype(np.float32))
        if p1 is None:
            continue
        d = np.float32(p2[0] - p1[0]), np.float32(p2[1] - p1[1])
        out.append((len(p), f32_angle(*d), f32_length(*d)))
    return out


# ---------------------------------------------------------------- independent restatements (scipy) of the openings
def scipy_open20(binary, horizontal):
    """cv2.morphologyEx(MORPH_OPEN) with a 20 x 1 (1 x 20) rectangle, anchor 10: erosion and dilation over [p - 10, p + 9],
    pixels outside the image neutral"""
    from scipy import ndimage as ndi
    size = (1, 20) if horizontal else (20, 1)
    e = ndi.grey_erosion(binary, size=size, mode='constant', cval=255)      # scipy centres a window of 20 at index 10
    dorg = (0, -1) if horizontal else (-1, 0)      # grey_dilation reflects its window: origin -1 gives back [p - 10, p + 9]
    return ndi.grey_dilation(e, size=size, mode='constant', cval=0, origin=dorg)


def scipy_open3(m):
    from scipy import ndimage as ndi
    e = ndi.grey_erosion(m, size=(3, 3), mode='constant', cval=255)
    return ndi.grey_dilation(e, size=(3, 3), mode='constant', cval=0)


def spot_mask(c, spot, planar):
    """255 except the erased ellipse (circle) of mask_roi_around_center"""
    from oracle import stages as S
    cm = np.full(c['gray'].shape, 255, np.uint8)
    if planar:
        S.circle_fill(cm, spot[0], spot[1], spot[2], 0)
    else:
        S.ellipse_fill(cm, *spot, 0)
    return cm


# name -> (generator, targets, expected overflow bit)
CASES = {
    'runs_h': (gen_runs_h, ('cylinder',), 0),
    'runs_v_192': (lambda: gen_runs_v(192), ('cylinder',), 0),
    'runs_v_193': (lambda: gen_runs_v(193), ('cylinder',), 0),
    'runs_v_255': (lambda: gen_runs_v(255), ('cylinder',), 0),
    'runs_v_bands32': (lambda: gen_runs_v(128, 2881, 32), ('cylinder',), 0),
    'joint_shapes': (gen_joint_shapes, ('cylinder',), 0),
    'joint_lattice': (gen_joint_lattice, ('cylinder',), OVF_JOINTS),
    'spot_tiles': (gen_spot_tiles, ('cylinder', 'plane'), 0),
    'plateau_241': (gen_plateau, ('cylinder',), 0),
    'plateau_no_spot': (lambda: gen_plateau(with_241=False), ('cylinder',), 0),
    'one_pixel_spot': (gen_one_pixel_spot, ('cylinder', 'plane'), 0),
    'equal_spots': (gen_equal_spots, ('cylinder', 'plane'), 0),
    'r0_21': (lambda: gen_spot_radius(21), ('cylinder',), 0),
    'r0_22': (lambda: gen_spot_radius(22), ('cylinder',), 0),
    'r0_23': (lambda: gen_spot_radius(23), ('cylinder',), 0),
    'r0_29': (lambda: gen_spot_radius(29, fragments=True), ('cylinder', 'plane'), 0),
    'r0_30': (lambda: gen_spot_radius(30, fragments=True), ('cylinder', 'plane'), 0),
    'r0_85': (lambda: gen_spot_radius(85, fragments=True), ('cylinder',), 0),
    'r0_86': (lambda: gen_spot_radius(86, fragments=True), ('cylinder',), OVF_KERNEL),
    'spot_cut': (gen_spot_cut, ('cylinder', 'plane'), 0),
    'chamfers': (gen_chamfers, ('cylinder', 'plane'), 0),
    'stairs_200': (lambda: gen_stairs((199, 200, 202), 500), ('cylinder',), 0),
    'counts_200': (lambda: gen_counts((199, 200, 201, 202), 520), ('cylinder',), 0),
    'counts_plane': (lambda: gen_counts((7, 8, 9, 699, 700, 701, 702), 1500), ('plane',), 0),
    'angle_tie': (gen_angle_tie, ('cylinder', 'plane'), 0),
    'length_tie': (gen_length_tie, ('cylinder', 'plane'), 0),
    'nested': (gen_nested, ('cylinder', 'plane'), 0),
    'clipped': (gen_clipped, ('cylinder', 'plane'), 0),
    'fan_odd': (gen_fan, ('cylinder', 'plane'), 0),
    'fan_even': (lambda: gen_fan(count=16), ('cylinder',), 0),
    'many_fragments': (gen_many_fragments, ('cylinder',), OVF_SEGS),
}
WIDTHS = (64, 65, 127, 801, 1920, 2880, 2881, 4096)      # gen_widths(96, w)
# cases that need a big frame
BIG = {
    'stairs_700': (lambda: gen_stairs((699, 700, 702), 1400), ('plane',), 0),
    'spot_tall': (gen_spot_tall, ('cylinder',), 0),
}

_CACHE = {}


def get(name):
    if name not in _CACHE:
        _CACHE[name] = (CASES[name][0] if name in CASES else BIG[name][0])()
    c = _CACHE[name]
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in c.items()}


# ---------------------------------------------------------------- the oracle's view of a case
def oracle(c, target='cylinder'):
    """what the masks stage must produce for a case: oracle/stages restated in the reference's order"""
    from oracle import stages as S
    planar = target == 'plane'
    hm, vm, jall = S.extract_joints(c['binary'])
    ref = dict(hmask=hm, vmask=vm, joints_all=jall, spot_plane=S.blur19(c['gray']) > 240, status=c['status'], r0=0,
               spot=(0, 0, 0, 0))
    if c['status'] != 0:
        return ref
    st, rh, rv, r0, spot = S.mask_roi_around_center(hm, vm, c['mc'], c['gray'], planar)
    ref.update(status=st, r0=r0, spot=spot, joints=S.joints_in_rect(jall, c['rect']))
    if st != 0:
        return ref
    ref.update(roi_h=rh, roi_v=rv, blur7=S.blur7(c['gray']))
    for key, roi in (('h', rh), ('v', rv)):
        if planar:
            ref['exp_' + key], ref['seg_' + key] = S.expand_line_roi_plane(roi, c['mc'])
        else:
            ref['exp_' + key], ref['seg_' + key] = S.expand_line_roi(roi, c['mc'], 91 + r0)
    return ref
