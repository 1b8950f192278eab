"""Sweep images (u8, what SimpleBlobDetector thresholds) for the step loop of the border followers: csrc/cpe_dev.h BitWin /
trace_border / StatVisitor and csrc/region.hip StoreVisitor.  numpy only; tests/test_trace_step_gpu.py runs them through
cpe_debug_blob_region, tests/test_trace_step_cases_cpu.py holds every generator to what its name claims with the oracle's
contours.  One idea per generator:
  chunk limits     hole and ring borders of exactly 1, 30, 31, 32, 61, 62, 63, 124, 125, 495, 496, 497 points: the chunk of
                   31 points, the quarter-wave limit of the median kernel and CH_DIRECT * 31
  revisited pixels spurs and bridges one pixel wide inside holes, staircases, diagonal one-pixel holes, a spiral, a diamond
  window edges     the tracer's 16 x 64 window starts on a multiple of 8 rows and 32 columns: holes at every x = 29 .. 35
                   (mod 32) and y = 5 .. 10 (mod 8), 3 x 400 holes along a row and a column, holes one pixel from the frame
  lockstep         1 long border among 63 short ones, 65 borders, and more borders than the chunk pool of a threshold holds
  large            4096 x 192 and 192 x 4096 frames with the holes in the last 64 columns and rows
A dark hole in a bright field is followed as a hole border (its points are stored in chunks while it is followed); a bright
ring on a dark field gives an outer border (followed a second time for its distances when it is accepted)."""
import numpy as np

CH_PTS = 31                 # csrc/region.hip: border points per chunk
LENGTHS = (1, 30, 31, 32, 61, 62, 63, 124, 125, 495, 496, 497)
MAXCH_SMALL = 8192          # csrc/workspace.h region_maxch: chunks per frame and threshold of a frame below 2 Mpixel


def canvas(h, w, bg=255, margin=6):
    """a bright field inset by a dark margin"""
    img = np.zeros((h, w), np.uint8)
    img[margin:h - margin, margin:w - margin] = bg
    return img


def hole_dims(n):
    """(rows, columns, cut) of a rectangular hole whose border has n >= 8 points: the border of an a x b hole runs through
    the 2 (a + b) field pixels beside its sides; a hole with one corner pixel left bright has one point less"""
    cut = n % 2
    half = (n + cut) // 2
    a = 3 if half <= 16 else 5 if half <= 40 else 6 if half <= 70 else 20
    return a, half - a, cut


def ring_dims(n):
    """(rows, columns, cut) of a two-pixel-wide rectangular ring whose outer border has n >= 16 points: 2 (a + b) - 4 for
    an a x b ring, one less with a corner pixel taken away"""
    cut = n % 2
    half = (n + cut + 4) // 2
    a = 5 if half <= 20 else 7 if half <= 70 else 20
    return a, half - a, cut


def gen_hole_lengths(h=136, w=264):
    """one hole per length of LENGTHS (but 1: no hole border is that short), the long ones one above the other.  The field
    is 85: the holes exist at four thresholds, so even one blob group that takes all 11 of them stays below the 48 centres a
    group holds (a long hole's radius reaches its neighbours)"""
    img = canvas(h, w, bg=85)
    x, y, rowh = 10, 9, 0
    for n in LENGTHS[1:]:
        a, b, cut = hole_dims(n)
        if x + b + 10 > w - 6:
            x, y, rowh = 10, y + rowh + 3, 0
        img[y:y + a, x:x + b] = 0
        if cut:
            img[y, x] = 85
        x += b + 4
        rowh = max(rowh, a)
    assert y + rowh < h - 8
    return img


def gen_ring_lengths(h=136, w=264):
    """one bright ring per length of LENGTHS on a dark field (its centre is dark: it is accepted); length 1 is a lone pixel.
    The rings are 65: rings and their holes are 22 blobs at two thresholds, fewer than the 48 centres a blob group holds"""
    img = np.zeros((h, w), np.uint8)
    img[4, 4] = 65
    x, y, rowh = 8, 8, 0
    for n in LENGTHS[1:]:
        a, b, cut = ring_dims(n)
        if x + b + 6 > w - 4:
            x, y, rowh = 8, y + rowh + 3, 0
        img[y:y + a, x:x + b] = 65
        img[y + 2:y + a - 2, x + 2:x + b - 2] = 0
        if cut:
            img[y, x] = 0
        x += b + 4
        rowh = max(rowh, a)
    assert y + rowh < h - 4
    return img


def gen_revisits(h=203, w=200):
    """pixels a border passes twice and borders that turn at every step"""
    img = canvas(h, w)
    # spurs: one-pixel bright lines that reach into a hole from each of its sides
    img[10:24, 10:30] = 0
    img[10:17, 14] = 255; img[18:24, 22] = 255; img[13, 10:13] = 255; img[20, 26:30] = 255
    # bridges: one-pixel bright lines across a hole, straight and diagonal (the halves are holes of their own)
    img[10:24, 36:60] = 0
    img[10:24, 44] = 255
    for i in range(14):
        img[10 + i, 46 + i] = 255
    # a hole with a lone bright pixel and a bright 2 x 2 block inside (outer borders inside a hole border)
    img[10:24, 66:86] = 0
    img[14, 70] = 255; img[17:19, 78:80] = 255
    # staircases in both directions, two pixels per step (4-connected: one hole each)
    for i in range(40):
        img[30 + i, 10 + i:12 + i] = 0
        img[30 + i, 100 - i:102 - i] = 0
    # one-pixel diagonal holes: 8-adjacent dark pixels are holes of their own whose borders share pixels
    for i in range(30):
        img[30 + i, 110 + i] = 0
        img[30 + i, 190 - i] = 0
    # a diamond: its border leaves a window through the corners
    yy, xx = np.mgrid[:h, :w]
    img[np.abs(yy - 120) + np.abs(xx - 50) <= 40] = 0
    # a square spiral, two pixels wide
    y, x, d, step = 130, 150, 0, 4
    for seg in range(18):
        dy, dx = ((0, 1), (1, 0), (0, -1), (-1, 0))[d]
        for _ in range(step):
            img[y:y + 2, x:x + 2] = 0
            y += dy; x += dx
        d = (d + 1) % 4
        if seg % 2 == 1:
            step += 5
    return img


def gen_window_phases(h=203, w=200):
    """4 x 4 holes whose first pixel lies at every x = 29 .. 35 (mod 32) and y = 5 .. 10 (mod 8)"""
    img = canvas(h, w)
    k = 0
    for dy in range(5, 11):
        for dx in range(29, 36):
            x, y = 32 * (k % 4) + dx, 8 * (1 + 2 * (k // 4)) + dy
            img[y:y + 4, x:x + 4] = 0
            k += 1
    return img


def gen_window_crossings(h=136, w=264):
    """holes wider and taller than a window at the same phases, and rectangles around every corner of the 32 x 8 lattice"""
    img = canvas(h, w)
    img[13:16, 29:229] = 0                    # through many windows along a row, starting 3 columns before a boundary
    img[21:101, 35:38] = 0                    # and down a column
    for k, (y, x) in enumerate(((30, 60), (31, 93), (38, 126), (39, 159), (46, 190))):
        img[y:y + 20, x:x + 22 + k] = 0       # 20 rows: more than a window, from every phase
    for k in range(6):                        # holes astride the corners (64 j, 8 i)
        img[78 + k:84 + k, 61 + 32 * k:67 + 32 * k] = 0
    return img


def gen_long_holes(h=430, w=437):
    """3 x 400 holes along a row and along a column (a width that is no multiple of 16)"""
    img = canvas(h, w)
    img[12:15, 20:420] = 0
    img[22:422, 9:12] = 0
    img[30:33, 29:429] = 0                    # from 3 columns before a window boundary to 2 columns before the field's end
    return img


def gen_frame_edges(h=203, w=200):
    """the field reaches the frame; holes one pixel from every edge and corner: window rows and columns outside the image"""
    img = np.full((h, w), 255, np.uint8)
    for y in (1, h // 2, h - 5):
        for x in (1, w // 2, w - 5):
            if (y, x) != (h // 2, w // 2):
                img[y:y + 4, x:x + 4] = 0
    img[1:4, 40:80] = 0; img[h - 4:h - 1, 100:160] = 0; img[60:120, 1:4] = 0; img[30:90, w - 4:w - 1] = 0
    return img


def gen_one_long(h=203, w=200):
    """64 holes: a 3 x 180 one and 63 of 3 x 4 -- one lane of the wavefront goes on alone for 340 steps.  The field is 55:
    one threshold, so the blob group of the long hole, whose radius reaches some twenty of the others, stays below 48 centres"""
    img = canvas(h, w, bg=55)
    img[10:13, 10:190] = 0
    for k in range(63):
        y, x = 20 + 8 * (k // 9), 12 + 20 * (k % 9)
        img[y:y + 3, x:x + 4] = 0
    return img


def gen_65(h=203, w=200):
    """65 holes of 3 x 4: a second turn of the wavefront with one lane"""
    img = canvas(h, w)
    for k in range(65):
        y, x = 12 + 8 * (k // 9), 12 + 20 * (k % 9)
        img[y:y + 3, x:x + 4] = 0
    return img


def gen_pool_runs_out(h=300, w=300):
    """a field of 65 with 2 x 3 holes of 55, 3 rows and 4 columns apart: they exist at threshold 60 only, every one reserves
    two chunks and there are more than MAXCH_SMALL / 2 of them.  The holes that find the pool empty are followed again for
    their distances: the blobs are the same, and no overflow is reported"""
    img = np.zeros((h, w), np.uint8)
    img[6:h - 6, 6:w - 6] = 65
    n = 0
    for y in range(8, h - 10, 3):
        for x in range(8, w - 11, 4):
            img[y:y + 2, x:x + 3] = 55
            n += 1
    assert 2 * n > MAXCH_SMALL
    return img


def gen_far_columns(h=192, w=4096):
    """a 4096-wide frame with its holes in the last 64 columns (and one long hole into them)"""
    img = np.zeros((h, w), np.uint8)
    img[6:h - 6, w - 600:w - 1] = 255
    for k in range(8):
        img[12 + 20 * k:18 + 20 * k, w - 60 + 4 * k:w - 40 + 4 * k] = 0
    img[176:179, w - 500:w - 3] = 0
    img[20:150, w - 5:w - 3] = 0
    return img


def gen_far_rows(h=4096, w=192):
    return np.ascontiguousarray(gen_far_columns(w, h).T)


# name -> generator; the frame size is the generator's default
CASES = {
    'hole_lengths': gen_hole_lengths,
    'ring_lengths': gen_ring_lengths,
    'revisits': gen_revisits,
    'window_phases': gen_window_phases,
    'window_crossings': gen_window_crossings,
    'long_holes': gen_long_holes,
    'frame_edges': gen_frame_edges,
    'one_long': gen_one_long,
    'holes_65': gen_65,
    'pool_runs_out': gen_pool_runs_out,
    'far_columns': gen_far_columns,
    'far_rows': gen_far_rows,
}

_CACHE = {}


def get(name):
    if name not in _CACHE:
        _CACHE[name] = CASES[name]()
        assert _CACHE[name].dtype == np.uint8
    return _CACHE[name].copy()
