"""Images for tests/test_sweep_links_gpu.py: the links of the blob sweep's two forests (csrc/region.hip), one idea per generator.

Every generator returns (image u8 [h, w], facts): the facts name the pixels and thresholds the image was built around, and
the CPU test of the module checks them against the oracle, so an image that stops reaching its situation fails there.

Grey levels are written by bucket (csrc/cpe_dev.h sweep_level): bucket b = 1 .. 17 holds 50 + 10 (b - 1) < v <= 50 + 10 b
(17: v > 210), bucket 0 is dark at every threshold.  A pixel of bucket b is bright at the threshold slots k < b (threshold
50 + 10 k), joins the bright forest at step 17 - b and the dark forest at slot b."""
import numpy as np

NTHR = 17
MARGIN = 6


def grey(b):
    return 20 if b == 0 else 45 + 10 * b


def level(img):
    v = img.astype(np.int32)
    return np.where(v <= 50, 0, np.minimum((v - 41) // 10, 17))


def _field(h, w, b, margin):
    img = np.zeros((h, w), np.uint8)
    img[margin:h - margin, margin:w - margin] = grey(b)
    return img


# ---------------------------------------------------------------- a run member west of a hole
RUN_LEN = 12


def gen_member_west(h, w, kind, margin=MARGIN):
    """a field of bucket 10 with two rows that hold a run of 12 pixels of one bucket (14: joins before the field; 6: after it)
    ending at the first pixel of a 4 x 4 hole.  kind: 'inside' -- no multiple of 64 among the run's frame indices;
    'cross64' -- one between the run's fifth pixel and its last but two; 'left_edge' -- the run starts in the rectangle's
    first column"""
    img = _field(h, w, 10, margin)
    runs = []
    for y, b in ((margin + 10, 14), (margin + 30, 6)):
        for a in ((margin,) if kind == 'left_edge' else range(margin + 8, w - margin - RUN_LEN - 8)):
            cut = np.flatnonzero((y * w + a + np.arange(RUN_LEN)) % 64 == 0)      # where a 64-index chunk begins inside the run
            if {'inside': len(cut) == 0, 'cross64': len(cut) == 1 and 4 <= cut[0] <= RUN_LEN - 3,
                    'left_edge': RUN_LEN - 1 not in cut}[kind]:
                break
        else:
            raise AssertionError((kind, h, w))
        img[y, a:a + RUN_LEN] = grey(b)
        img[y:y + 4, a + RUN_LEN:a + RUN_LEN + 4] = grey(0)
        runs.append(dict(y=y, x0=a, bucket=b, west=(a + RUN_LEN - 1, y)))
    return img, dict(kind=kind, runs=runs, margin=margin)


# ---------------------------------------------------------------- enclosed totals: an over-count must show
def gen_overcount(h, w, merge_bucket, margin=MARGIN):
    """a 9 x 9 ring of bucket 17 around a 5 x 5 dark centre, raster-first; beside it a frame of bucket 17 whose four dark
    panes hold fewer than 5000 pixels each and more than 5000 together; five bridge pixels of `merge_bucket` join the two at
    threshold slot merge_bucket - 1"""
    m = margin
    img = np.zeros((h, w), np.uint8)
    img[m:m + 9, m:m + 9] = grey(17)
    img[m + 2:m + 7, m + 2:m + 7] = grey(0)
    y0, x0, y1, x1 = m + 4, m + 14, h - m, w - m
    img[y0:y1, x0:x1] = grey(17)
    ym, xm = (y0 + y1) // 2, (x0 + x1) // 2
    panes = []
    for ya, yb in ((y0 + 2, ym - 1), (ym + 1, y1 - 2)):
        for xa, xb in ((x0 + 2, xm - 1), (xm + 1, x1 - 2)):
            img[ya:yb, xa:xb] = grey(0)
            panes.append((yb - ya) * (xb - xa))
    img[m + 6, m + 9:m + 14] = grey(merge_bucket)
    return img, dict(merge_slot=merge_bucket - 1, ring_centre=(m + 4.0, m + 4.0), panes=panes)


# ---------------------------------------------------------------- two absorptions in one step
def gen_two_absorptions(h, w, margin=MARGIN):
    """three blocks of bucket 17 one below the other (c, b, a in raster order), each with a hole, joined by two vertical
    connectors of bucket 12: at slot 11 b absorbs a and c absorbs b in one step"""
    m = margin
    img = np.zeros((h, w), np.uint8)
    wests = []
    for k in range(3):
        y = m + 20 * k
        img[y:y + 12, m + 20:m + 41] = grey(17)
        img[y + 4:y + 8, m + 33:m + 37] = grey(0)
        wests.append((m + 32, y + 4))
        if k:
            img[y - 8:y, m + 30] = grey(12)
    return img, dict(step_slot=11, wests=wests)


# ---------------------------------------------------------------- vertical stacks and staircases of one bucket
STACK_HEIGHTS = (8, 17, 40)
STAIR_HEIGHT = 20


def gen_stacks(h, w, dark, margin=MARGIN):
    """one-pixel-wide vertical stacks 8, 17 and 40 high and two staircases 20 high (down-right and down-left) of one bucket,
    with side pixels that join one bucket later.  dark = False: bright stacks (bucket 15, sides 14) on black, 8-connected
    stairs of single pixels; dark = True: stacks of bucket 5 (sides 6) in a field of bucket 17, 4-connected stairs of two
    pixels per row: they stay holes"""
    m = margin
    img = _field(h, w, 17, m) if dark else np.zeros((h, w), np.uint8)
    core, side = (grey(5), grey(6)) if dark else (grey(15), grey(14))
    y0 = m + 4
    cells = []
    for k, n in enumerate(STACK_HEIGHTS):
        cells.append([(y0 + i, m + 10 + 20 * k) for i in range(n)])
    wide = 2 if dark else 1
    cells.append([(y0 + i, m + 70 + i + d) for i in range(STAIR_HEIGHT) for d in range(wide)])
    cells.append([(y0 + i, m + 125 - i + d) for i in range(STAIR_HEIGHT) for d in range(wide)])
    for c in cells:
        for y, x in c:
            img[y, x - 1] = side
            img[y, x + 1] = side
    for c in cells:
        for y, x in c:
            img[y, x] = core
    return img, dict(dark=dark, slot=5 if dark else 14, heights=STACK_HEIGHTS + (STAIR_HEIGHT, STAIR_HEIGHT))


# ---------------------------------------------------------------- long runs that bridge two older components
LONG_RUN = 30


def gen_long_runs(h, w, dark, margin=MARGIN):
    """two pairs of 20 x 20 blocks 30 pixels apart, each pair bridged by a run of 30 pixels of one bucket: the first run
    touches its blocks along the row, the second lies in the row above its blocks and touches their corners only.
    dark = False: blocks of bucket 17 and runs of bucket 10 on black (8-connected: both pairs join at slot 9);
    dark = True: blocks of bucket 2 and runs of bucket 8 in a field of bucket 17 (4-connected: only the first pair joins)"""
    m = margin
    img = _field(h, w, 17, m) if dark else np.zeros((h, w), np.uint8)
    block, run = (grey(2), grey(8)) if dark else (grey(17), grey(10))
    x = m + 4
    rows = []
    for yb, yr in ((m + 6, m + 12), (m + 50, m + 49)):
        img[yb:yb + 20, x:x + 20] = block
        img[yb:yb + 20, x + 20 + LONG_RUN:x + 40 + LONG_RUN] = block
        img[yr, x + 20:x + 20 + LONG_RUN] = run
        rows.append((yr, x + 20))
    return img, dict(dark=dark, slot=8 if dark else 9, rows=rows, span=40 + LONG_RUN)


SHAPES = ((120, 176), (120, 180))       # a width that is a multiple of 16 and one that is not: both plane builders


def cases(h, w):
    """name -> (image, facts) of every case at one frame size"""
    out = {}
    for kind in ('inside', 'cross64', 'left_edge'):
        out['member_' + kind] = gen_member_west(h, w, kind)
    out['member_frame_edge'] = gen_member_west(h, w, 'left_edge', margin=0)      # the rectangle is the frame
    for b in (16, 9, 1):        # the first step that can absorb an older root, a middle one, the last
        out['overcount_%d' % b] = gen_overcount(h, w, b)
    out['two_absorptions'] = gen_two_absorptions(h, w)
    for dark in (False, True):
        out['stacks_' + ('dark' if dark else 'bright')] = gen_stacks(h, w, dark)
        out['long_runs_' + ('dark' if dark else 'bright')] = gen_long_runs(h, w, dark)
    return out
