"""Images for tests/test_sweep_outside_gpu.py: dark components of the blob sweep that reach the border of the working
rectangle (csrc/region.hip: "outside" is a terminal parent, -1, of the dark forest), one idea per generator.

Every generator returns (image u8 [h, w], facts).  facts['holes'] is the number of holes the image is built to have at each
of the 17 threshold slots; the CPU test of the module checks it against the oracle, so an image that stops reaching its
situation fails there.

Grey levels are written by bucket as in sweep_links_cases.grey: bucket b = 1 .. 17 holds 50 + 10 (b - 1) < v <= 50 + 10 b
(17: v > 210), bucket 0 is dark at every threshold.  A pixel of bucket b joins the dark forest at slot b; bucket 17 never
does.  The working rectangle is the bounding box of the pixels above 50, here always the field [m, h - m) x [m, w - m) of
bucket 17 (m = 0: the whole frame): each of its border rows and columns keeps bright pixels, the other border pixels are what
the cases place."""
import numpy as np

from sweep_links_cases import NTHR, MARGIN, grey, level  # noqa: F401  (level: used by the tests)


def _field(h, w, m):
    img = np.zeros((h, w), np.uint8)
    img[m:h - m, m:w - m] = grey(17)
    return img, (m, m, w - m - 1, h - m - 1)


def _steps(before, slot, after=0):
    """hole counts: `before` up to slot - 1, `after` from `slot` on"""
    return [before if k < slot else after for k in range(NTHR)]


# ---------------------------------------------------------------- one border pixel opens a hole
SIDES = ('top', 'bottom', 'left', 'right')
CORNERS = ('tl', 'tr', 'bl', 'br')


def gen_open(h, w, b, where, margin=MARGIN):
    """holes of bucket 0 one pixel inside the rectangle's border, each opened to it by one pixel of bucket b.  A side: a 4 x 4
    hole and one opener on the border row / column.  A corner: a 3 x 3 hole diagonal to the corner pixel; the corner's own
    4-neighbours all lie on the border, so the opener is the corner pixel with the border pixel beside it, a run of two of
    bucket b.  where: the names of the places to fill"""
    img, (x0, y0, x1, y1) = _field(h, w, margin)
    dark, opener = grey(0), grey(b)
    openers = []
    for p in where:
        if p == 'top':
            img[y0 + 1:y0 + 5, x0 + 20:x0 + 24] = dark
            openers.append((y0, x0 + 21))
        elif p == 'bottom':
            img[y1 - 4:y1, x0 + 50:x0 + 54] = dark
            openers.append((y1, x0 + 51))
        elif p == 'left':
            img[y0 + 30:y0 + 34, x0 + 1:x0 + 5] = dark
            openers.append((y0 + 31, x0))
        elif p == 'right':
            img[y0 + 60:y0 + 64, x1 - 4:x1] = dark
            openers.append((y0 + 61, x1))
        else:
            ya, yb = (y0 + 1, y0) if p[0] == 't' else (y1 - 3, y1)
            xa, xb = (x0 + 1, x0) if p[1] == 'l' else (x1 - 3, x1 - 1)
            img[ya:ya + 3, xa:xa + 3] = dark
            openers += [(yb, xb), (yb, xb + 1)]
    for y, x in openers:
        img[y, x] = opener
    return img, dict(slot=b, drop=len(where), holes=_steps(len(where), b), openers=openers, margin=margin)


# ---------------------------------------------------------------- the first labelling already reaches the border
def gen_first_labelling(h, w, margin=MARGIN):
    """dark components of bucket 0 on every side of the border, one of them with an arm deep into the rectangle that ends
    next to nothing, and three 5 x 5 holes of bucket 0 away from the border that stay holes at every threshold"""
    img, (x0, y0, x1, y1) = _field(h, w, margin)
    d = grey(0)
    img[y0:y0 + 6, x0 + 30:x0 + 41] = d                       # top
    img[y1 - 2:y1 + 1, x0 + 60:x0 + 90] = d                    # bottom
    img[y0 + 20:y0 + 23, x0:x0 + 70] = d                      # left, with an arm
    img[y0 + 23:y0 + 60, x0 + 67:x0 + 70] = d
    img[y0 + 40:y0 + 50, x1 - 1:x1 + 1] = d                    # right
    img[y1, x0] = d                                           # a single corner pixel
    holes = [(y0 + 10, x0 + 10), (y0 + 30, x0 + 40), (y0 + 70, x0 + 100)]
    for y, x in holes:
        img[y:y + 5, x:x + 5] = d
    return img, dict(slot=0, drop=0, holes=[3] * NTHR, margin=margin)


# ---------------------------------------------------------------- hand-over, then outside
def gen_handover_then_outside(h, w, j, big=False, margin=MARGIN):
    """hole B (5 x 5, raster-first) absorbs hole A (4 x 4) through a bridge of three pixels of bucket j: one hole of
    25 + 16 + 3 pixels from slot j on.  A column of bucket j + 2 leads from B to the top border: from slot j + 2 on there
    is no hole.  big: B 50 x 70 and A 30 x 50, each below the 5000 pixels up to which a hole's border is followed, and
    5003 together: a total that was not handed over shows as a border that is followed"""
    assert 1 <= j <= NTHR - 3
    img, (x0, y0, x1, y1) = _field(h, w, margin)
    yb, xb = y0 + 12, x0 + 30
    (bh, bw), (ah, aw) = ((50, 70), (30, 50)) if big else ((5, 5), (4, 4))
    img[yb:yb + bh, xb:xb + bw] = grey(0)                             # B
    img[yb + 2:yb + 2 + ah, xb + bw + 3:xb + bw + 3 + aw] = grey(0)     # A: starts two rows lower, so B's first pixel is the root
    img[yb + 3, xb + bw:xb + bw + 3] = grey(j)                         # bridge
    img[y0:yb, xb + 2] = grey(j + 2)                                  # B's way out
    holes = [2 if k < j else 1 if k < j + 2 else 0 for k in range(NTHR)]
    return img, dict(slot=j + 2, drop=1, merge_slot=j, parts=(bh * bw, ah * aw, 3), holes=holes, margin=margin)


# ---------------------------------------------------------------- a pre-linked run along the top row
RUN_LEN = 80


def gen_run_on_border(h, w, b=7, margin=MARGIN):
    """one run of 80 pixels of bucket b along the top row of the rectangle, from the rectangle's corner: it crosses a multiple
    of 64 in frame indices and one in columns counted from the rectangle's left edge, and opens two holes in one step"""
    img, (x0, y0, x1, y1) = _field(h, w, margin)
    img[y0, x0:x0 + RUN_LEN] = grey(b)
    img[y0 + 1:y0 + 5, x0 + 5:x0 + 9] = grey(0)
    img[y0 + 1:y0 + 5, x0 + 70:x0 + 74] = grey(0)
    return img, dict(slot=b, drop=2, holes=_steps(2, b), run=(y0, x0, RUN_LEN), margin=margin)


# ---------------------------------------------------------------- 4-connectivity
def gen_diagonal(h, w, margin=MARGIN):
    """two holes that touch an outside component at a corner only: one beside a block of bucket 0 on the left border, one
    beside a block of bucket 8 on the top border.  Both stay holes at every threshold"""
    img, (x0, y0, x1, y1) = _field(h, w, margin)
    img[y0 + 40:y0 + 45, x0:x0 + 5] = grey(0)
    img[y0 + 45:y0 + 49, x0 + 5:x0 + 9] = grey(0)
    img[y0:y0 + 3, x0 + 100:x0 + 103] = grey(8)
    img[y0 + 3:y0 + 7, x0 + 103:x0 + 107] = grey(0)
    return img, dict(slot=0, drop=0, holes=[2] * NTHR, margin=margin)


# ---------------------------------------------------------------- absorbed into outside
def gen_absorbed_into_outside(h, w, j=6, margin=MARGIN):
    """a block of bucket 0 on the left border, then hole H1, then hole H2 in one row of blocks, joined by two bridges of
    bucket j: at slot j H1 absorbs H2 and the outside component absorbs H1, in one step.  A third hole far away stays"""
    img, (x0, y0, x1, y1) = _field(h, w, margin)
    ya = y0 + 20
    img[ya:ya + 6, x0:x0 + 6] = grey(0)
    img[ya + 1:ya + 5, x0 + 8:x0 + 12] = grey(0)                # H1
    img[ya + 1:ya + 5, x0 + 14:x0 + 18] = grey(0)               # H2
    img[ya + 2, x0 + 6:x0 + 8] = grey(j)
    img[ya + 2, x0 + 12:x0 + 14] = grey(j)
    img[y0 + 60:y0 + 66, x0 + 80:x0 + 86] = grey(0)
    return img, dict(slot=j, drop=2, holes=_steps(3, j, 1), margin=margin)


# ---------------------------------------------------------------- degenerate frames
def gen_degenerate(h, w, kind):
    """'none_bright': no pixel above 50 (no rectangle); 'black': all zero; 'none_dark': buckets 1 .. 17 in stripes, no pixel at
    or below 50 (the first labelling finds nothing); 'white': all 255"""
    if kind == 'none_bright':
        img = np.full((h, w), 50, np.uint8)
        img[::7, ::5] = 20
    elif kind == 'black':
        img = np.zeros((h, w), np.uint8)
    elif kind == 'white':
        img = np.full((h, w), 255, np.uint8)
    else:
        img = np.empty((h, w), np.uint8)
        for x in range(w):
            img[:, x] = grey(1 + (x // 5) % 17)
    return img, dict(slot=0, drop=0, holes=None, kind=kind)


SHAPES = ((120, 176), (120, 180))       # a width that is a multiple of 16 and one that is not: both plane builders, both labelling paths
OPEN_BUCKETS = (1, 9, 16, 17)           # the first step, a middle one, the last; 17 never joins: its holes stay


def cases(h, w):
    """name -> (image, facts) of every case at one frame size"""
    out = {}
    for m, tag in ((MARGIN, ''), (0, '_frame')):            # '_frame': margin 0, the rectangle is the whole frame
        for b in OPEN_BUCKETS:
            out['open_all_%d%s' % (b, tag)] = gen_open(h, w, b, SIDES + CORNERS, m)
        for p in SIDES + CORNERS:
            for b in (1, 9, 17) if m else (9,):
                out['open_%s_%d%s' % (p, b, tag)] = gen_open(h, w, b, (p,), m)
        out['first_labelling' + tag] = gen_first_labelling(h, w, m)
        out['run_on_border' + tag] = gen_run_on_border(h, w, 7, m)
        out['absorbed_into_outside' + tag] = gen_absorbed_into_outside(h, w, 6, m)
    for j in (1, 5, 14):
        out['handover_%d' % j] = gen_handover_then_outside(h, w, j)
    out['handover_big_5'] = gen_handover_then_outside(h, w, 5, big=True)
    out['diagonal'] = gen_diagonal(h, w)
    out['diagonal_frame'] = gen_diagonal(h, w, 0)
    for kind in ('none_bright', 'black', 'none_dark', 'white'):
        out['degenerate_' + kind] = gen_degenerate(h, w, kind)
    return out
