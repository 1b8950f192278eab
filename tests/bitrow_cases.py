"""Inputs for the two bit-row kernels of the masks stage (csrc/masks.hip: k_open20_joints, k_roi_base), cut for their
decomposition: a lane owns CHUNK pixels of a row, four lanes a 64-pixel word of the one-bit planes, a wave a strip of STRIP
columns; k_open20_joints marches bands of OPEN_BAND rows, k_roi_base bands of ROI_BAND rows, and the planes leave in tile
rows of 8.  A case is the dict of tests/masks_cases.py (binary, gray, mc, rect, status); mc is any pattern inside rect here,
which puts single pixels in front of the 3x3 passes that the 20-tap openings would never let through.
tests/test_bitrow_generators_cpu.py checks that each generator reaches the edges it is named for;
tests/test_bitrow_kernels_gpu.py runs the cases through the kernels."""
import numpy as np

import masks_cases as M

CHUNK, WORD, STRIP = 16, 64, 960
OPEN_BAND, ROI_BAND, TILE_ROWS = 80, 40, 8
RUNS = (19, 20, 21)
WIDE = STRIP + WORD + CHUNK          # 1040: two strips, the last word of a row partial, rows a multiple of 16 pixels
X_EDGES = (WORD, STRIP, STRIP + CHUNK)
WIDTHS = (64, 65, 127, 128, 129, 576, 592, 801, STRIP + 1, STRIP + CHUNK, WIDE)
MIN_ROWS = 64                         # include/cpe.h: every entry refuses frames below 64 x 64
HEIGHTS = (MIN_ROWS, OPEN_BAND - 1, OPEN_BAND, OPEN_BAND + 1, 3 * ROI_BAND - 1, 3 * ROI_BAND, 3 * ROI_BAND + 1, 2 * OPEN_BAND + 1)


def bcase(binary, mc=None, rect=None, status=0, spot=None):
    """masks_cases.case with a mask_contour of the caller's: mc != 0 inside rect (default: all of rect)"""
    c = M.case(binary, rect=rect, status=status, spot=spot)
    if mc is not None:
        c['mc'] = np.where(np.asarray(mc) != 0, 255, 0).astype(np.uint8) & c['mc']
    return c


def edge_starts(edge, length):
    """first pixels of the runs of `length` that begin one pixel before, on and one after `edge`, and of those whose last
    pixel lies two before, one before and on it (the run ends before, on and after the edge)"""
    return [edge - 1, edge, edge + 1, edge - 1 - length, edge - length, edge + 1 - length]


def run_items(edges, size):
    """(kind, length, first pixel) of every run and gap of 19, 20, 21 pixels at the edges and at both ends of a line of
    `size` pixels"""
    out = []
    for kind in ('run', 'gap'):
        for L in RUNS:
            starts = [p for e in edges for p in edge_starts(e, L)] + [0, 1, size - L - 1, size - L]
            out += [(kind, L, p) for p in starts if p >= 0 and p + L <= size]
    return out


def _line(kind, L, p, size):
    a = np.zeros(size, np.uint8)
    if kind == 'run':
        a[p:p + L] = 255
    else:
        a[:] = 255
        a[p:p + L] = 0
    return a


def gen_runs_h(w=WIDE):
    """one run (or one gap in a full row) per row, two rows apart: 19, 20, 21 pixels around the word edge, the strip edge,
    the first lane edge after it and both ends of the row"""
    items = run_items([e for e in X_EDGES if e + 22 <= w], w)
    h = 2 * len(items) + 32
    b = np.zeros((h, w), np.uint8)
    for i, (kind, L, p) in enumerate(items):
        b[1 + 2 * i] = _line(kind, L, p, w)
    return bcase(b, spot=(w // 2, h - 14, 10))


def y_edges(h):
    return [e for e in (TILE_ROWS, ROI_BAND, OPEN_BAND, 2 * OPEN_BAND) if e + 22 <= h]


def gen_runs_v(h):
    """one run (or gap) per column, two columns apart: 19, 20, 21 pixels around the tile-row and band edges below h and at
    the first and last rows; then a full column, and full columns short of their first, last and a middle pixel.  (The
    entries refuse frames below MIN_ROWS rows, so a frame lower than the 20-row window cannot be put in front of the kernels;
    the CPU file holds the generator to such heights all the same.)"""
    items = run_items(y_edges(h), h)
    w = (2 * len(items) + 8 + 48 + 15) // 16 * 16
    b = np.zeros((h, w), np.uint8)
    for i, (kind, L, p) in enumerate(items):
        b[:, 1 + 2 * i] = _line(kind, L, p, h)
    x = 1 + 2 * len(items)
    b[:, x] = 255
    b[1:, x + 2] = 255
    b[:h - 1, x + 4] = 255
    b[:, x + 6] = 255; b[h // 2, x + 6] = 0
    return bcase(b, spot=(w - 20, h // 2, 10))


def gen_blobs(h, w, seed=0):
    """binary: rectangles of 21 .. 60 pixels a side (both openings keep them) and bars 1 .. 3 thick, 15 .. 50 long;
    mask_contour: rectangles of 1 .. 40 pixels a side, so mask & mask_contour has pieces of every small size"""
    rng = np.random.default_rng(1000 * seed + w + h)
    b = np.zeros((h, w), np.uint8)
    mc = np.zeros((h, w), np.uint8)
    for _ in range(max(6, h * w // 3000)):
        bw, bh = (int(v) for v in rng.integers(21, 61, 2))
        x, y = int(rng.integers(-20, w)), int(rng.integers(-20, h))
        b[max(y, 0):max(y + bh, 0), max(x, 0):max(x + bw, 0)] = 255
    for _ in range(max(6, h * w // 2000)):
        L, t = int(rng.integers(15, 51)), int(rng.integers(1, 4))
        x, y = int(rng.integers(-10, w)), int(rng.integers(-10, h))
        bw, bh = (L, t) if rng.random() < 0.5 else (t, L)
        b[max(y, 0):max(y + bh, 0), max(x, 0):max(x + bw, 0)] = 255
    for _ in range(max(12, h * w // 600)):
        bw, bh = (int(v) for v in rng.integers(1, 41, 2))
        x, y = int(rng.integers(-10, w)), int(rng.integers(-10, h))
        mc[max(y, 0):max(y + bh, 0), max(x, 0):max(x + bw, 0)] = 255
    return b, mc


def spot_for(h, w):
    return (w - 20, h - 14, 10) if h >= 40 else (w - 20, h // 2, 10)


def gen_width(w, h=96):
    """blobs at any width: rect is the frame"""
    b, mc = gen_blobs(h, w)
    return bcase(b, mc, spot=spot_for(h, w))


def gen_height(h, w=208):
    b, mc = gen_blobs(h, w, seed=3)
    return bcase(b, mc, spot=spot_for(h, w))


# the corners of the cells of k_roi_base: strip x band, word x band, lane x tile row
RECT_SHAPE = (200, WIDE)
CORNERS = [(STRIP, ROI_BAND * k) for k in (1, 2, 3, 4)] + [(WORD * j, ROI_BAND * k) for j in (1, 2, 3, 4) for k in (1, 2)] + \
          [(CHUNK * j + 400, TILE_ROWS * j + 4) for j in (1, 2, 3, 4)]


def corner_pixels():
    """one pixel at each corner, the four pixels that touch a corner in turn: (x, y)"""
    return [(x - 1 + (i & 1), y - 1 + ((i >> 1) & 1)) for i, (x, y) in enumerate(CORNERS)]


def gen_specks(holes):
    """a full binary frame, so that mask & mask_contour = mask_contour (less the spot): single pixels at the corners of the
    cells (the 3x3 opening takes them away), or a full mask_contour with single-pixel holes there (the closing fills them);
    a few 5 x 5 blocks (holes) straddle corners and stay"""
    h, w = RECT_SHAPE
    b = np.full((h, w), 255, np.uint8)
    mc = np.full((h, w), 255 if holes else 0, np.uint8)
    for x, y in corner_pixels():
        mc[y, x] = 0 if holes else 255
    for x, y in ((STRIP - 2, 3 * ROI_BAND + 18), (WORD * 5 - 2, ROI_BAND - 2), (300, 2 * ROI_BAND - 3)):
        mc[y:y + 5, x:x + 5] = 0 if holes else 255
    return bcase(b, mc, spot=(40, h - 30, 10))


# rectangles (x, y, w, h) on a RECT_SHAPE frame of blobs
RECTS = {
    'mid_word': (70, 13, 333, 101),
    'word_to_strip_edge': (WORD, ROI_BAND, STRIP - WORD, ROI_BAND),
    'from_strip_edge': (STRIP, 2 * ROI_BAND, WORD, ROI_BAND),
    'one_wide': (500, 10, 1, 150),
    'one_high': (10, 77, 1000, 1),
    'frame': (0, 0, WIDE, 200),
    'left_border': (0, 50, 30, 30),
    'right_border': (WIDE - 30, 50, 30, 30),
    'top_border': (400, 0, 50, 20),
    'bottom_border': (400, 180, 50, 20),
    'band_by_margin': (100, 10, 200, ROI_BAND - 1 - 10),            # last row 38: the band from row 40 sees only its margin
    'strip_by_margin': (700, 41, STRIP - 1 - 700, 50),              # last column 958: the strip from 960 sees only its margin
}


def gen_rect(name, full_mc=False):
    """blobs under one of RECTS; full_mc: mask_contour = every pixel of the rectangle (more survives the 3x3 passes)"""
    h, w = RECT_SHAPE
    b, mc = gen_blobs(h, w, seed=7)
    if full_mc:
        b[:] = 255
        mc[:] = 255
    sx = 40 if RECTS[name][0] > 100 else w - 40
    return bcase(b, mc, rect=RECTS[name], spot=(sx, h - 16, 10))


def with_mc_outside(c):
    """-> (the case with mask_contour set on a random half of the pixels outside rect, the case as it must be read)"""
    x, y, rw, rh = c['rect']
    rng = np.random.default_rng(99)
    noise = np.where(rng.random(c['mc'].shape) < 0.5, 255, 0).astype(np.uint8)
    noise[y:y + rh, x:x + rw] = c['mc'][y:y + rh, x:x + rw]
    return dict(c, mc=noise), c


_CACHE = {}


def get(key, fn, *args):
    if key not in _CACHE:
        _CACHE[key] = fn(*args)
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in _CACHE[key].items()}
