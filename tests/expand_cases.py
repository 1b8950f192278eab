"""Inputs for the fragment expansion of the masks stage (k_roi_base's seed of exp, k_seg_expand): a mask_contour that is not
the rectangle, end points at word and frame edges, hundreds of fragments with overlapping supports, and frames that leave
nothing to find.  Cases are masks_cases.case() dicts; tests/test_expand_cases_cpu.py checks with the oracle that every
generator reaches its edge, tests/test_expand_direct_gpu.py runs them through the kernels."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import masks_cases as M  # noqa: E402


def with_contour(c, mc):
    """the case with mask_contour = mc (0 / 255) and rect = its bounding rectangle"""
    mc = np.where(mc != 0, 255, 0).astype(np.uint8)
    ys, xs = np.nonzero(mc)
    out = dict(c)
    out['mc'] = mc
    out['rect'] = (int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1))
    return out


def full_rect(c):
    """the case with mask_contour = all of its rect"""
    x, y, w, h = c['rect']
    mc = np.zeros_like(c['mc'])
    mc[y:y + h, x:x + w] = 255
    return dict(c, mc=mc)


def slit_bar(img, x0, y0, W, H, at):
    """a bump bar (10 vertices) cut by a 2-px slit `at` columns from its left end: the 3x3 opening keeps the slit, the
    closing fills it (pixels of base that are not in roi)"""
    M.bump_bar(img, x0, y0, W, H)
    img[y0 - 3:y0 + H, x0 + at:x0 + at + 2] = 0
    return img


# ---------------------------------------------------------------- 1. mask_contour is not the rectangle
POLY_N, POLY_C, POLY_R = 300, 150, 130


def polygon(n=POLY_N, c=POLY_C, r=POLY_R, sides=12):
    """a regular convex polygon (pixel centres inside all of its half planes), 0 / 255"""
    yy, xx = np.mgrid[:n, :n].astype(np.float64)
    m = np.ones((n, n), bool)
    ap = r * np.cos(np.pi / sides)
    for k in range(sides):
        th = 2 * np.pi * (k + 0.5) / sides
        m &= (xx - c) * np.cos(th) + (yy - c) * np.sin(th) <= ap
    return np.where(m, 255, 0).astype(np.uint8)


NOTCH_X = 236       # two columns of zeros in mask_contour, across the fan's fragments


def gen_polygon(notch=False, n=POLY_N):
    """fragments as in gen_fan (thick lines of every small slope, long and short) and bars with slits the closing fills, in both
    masks, under a 12-gon whose edges run through fragments, slits and expansion supports; notch: two columns (rows for the
    vertical mask: the transpose) of zeros in the polygon across the fragments -- the closing fills them in base, so base
    sticks out of mask_contour there"""
    a = np.zeros((n, n), np.uint8)
    for i, k in enumerate(range(-4, 5)):
        L = 60 if i % 3 else 90
        y = 14 + 20 * i
        M.thick_line(a, n - 12 - L, y, n - 12, y + k)
    slit_bar(a, 140, 24, 70, 5, 44)          # the polygon's edge crosses the bar left of the slit
    slit_bar(a, 130, 42, 50, 5, 24)          # inside
    assert not np.tril(a).any()
    c = M.case(M.mirrored(a), spot=(60, n - 60, 12))
    mc = polygon(n)
    if notch:
        mc[30:200, NOTCH_X:NOTCH_X + 2] = 0
        mc[NOTCH_X:NOTCH_X + 2, 30:200] = 0
    return with_contour(c, mc)


# ---------------------------------------------------------------- 2. end points at word and frame edges
RESIDUES = (0, 1, 31, 32, 62, 63)
# (first column, last column) of bump bars whose PCA end points are their top-left and bottom-right corners
WORD_BARS = ((64, 95), (129, 160), (254, 319), (384, 415), (449, 480), (510, 575))
EDGE_H = 260


def _vbar(b, x0, y0, T, L):
    """the transpose of a bump bar: T wide, L tall; its PCA end points are (x0, y0) and (x0, y0 + L - 1)"""
    cv = np.zeros((b.shape[1], b.shape[0]), np.uint8)
    M.bump_bar(cv, y0, x0, L, T)
    np.maximum(b, cv.T, out=b)


def edge_layout(w, h=EDGE_H):
    """-> (binary, horizontal end points, vertical end points): bump bars whose end points lie at columns = 0, 1, 31, 32,
    62, 63 (mod 64), within 7 px of each frame edge and in two corners; one long bar per mask so that the rest expand"""
    b = np.zeros((h, w), np.uint8)
    hp, vp = [], []

    def hbar(x0, y0, W, H=5):        # the 20-tap opening (anchor 10) moves a run one pixel on: drawn at x0 - 1
        M.bump_bar(b, x0 - 1, y0, W, H)
        hp.extend([(x0, y0), (x0 + W - 1, y0 + H - 1)])

    def vbar(x0, y0, L, T=5):
        _vbar(b, x0, y0 - 1, T, L)
        vp.extend([(x0, y0), (x0, y0 + L - 1)])

    for i, (xa, xb) in enumerate(WORD_BARS):
        hbar(xa, 30 + 14 * (i % 3), xb - xa + 1)
    hbar(2, 5, 40)                           # top-left corner
    hbar(w - 44, h - 9, 42)                  # bottom-right corner: last column w - 3, last row h - 5
    hbar(3, 120, 36)                         # left edge
    hbar(w - 40, 100, 38)                    # right edge
    hbar(200, 3, 44)                         # top edge
    hbar(120, h - 8, 40)                     # bottom edge
    hbar(60, 150, 130)                       # the longest
    for x0, y0 in ((62, 90), (127, 90), (320, 90), (575, 160)):      # columns 62, 63, 0, 63 (mod 64)
        vbar(x0, y0, 40)
    vbar(262, 3, 36)                         # top edge
    vbar(300, h - 40, 38)                    # bottom edge
    vbar(4, 60, 40)                          # left edge
    vbar(w - 8, 30, 40)                      # right edge
    vbar(440, 100, 130)                      # the longest
    return b, hp, vp


def gen_edges(w, r0, h=EDGE_H):
    """edge_layout under a saturated disc whose circle_radius0 is r0 (21, 22: kernels 112 and 113)"""
    b, _, _ = edge_layout(w, h)
    g = np.zeros((h, w), np.uint8)
    M.disc(g, 360, 150, M.SPOT_R0[r0])
    return M.case(b, gray=g)


# ---------------------------------------------------------------- 3. many jobs, overlapping supports
MANY_SHAPE = (480, 640)
MANY_L, MANY_T = 24, 4      # bars of 24 x 4: the next bar starts two columns right of and two rows below the last one's corner


def gen_many(h=MANY_SHAPE[0], w=MANY_SHAPE[1]):
    """more than 500 valid fragments per mask: 24 x 4 bars in a brick pattern whose corners lie (2, 2) apart diagonally (the
    closing does not join them, the expansion supports of neighbouring end points overlap nearly completely), with one or two
    cut corners (5 and 6 vertices), every eighth with a step (7); one long bar per mask"""
    b = np.zeros((h, w), np.uint8)
    cuts = (('tr',), ('tr', 'bl'), ('bl',), ('tr', 'bl'))      # never the corners that meet: those are the PCA end points
    px, py = 2 * (MANY_L + 1), 2 * (MANY_T + 1)

    def brick(k):
        t = np.zeros((MANY_T, MANY_L), np.uint8)
        if k % 8 == 5:
            M.bar(t, 0, 0, MANY_L, MANY_T, ('bl',))
            t[0, MANY_L - 4:] = 0             # a step: 7 vertices
        else:
            M.bar(t, 0, 0, MANY_L, MANY_T, cuts[k % 4])
        return t

    k = 0
    for y in range(2, 222, py):              # horizontal bars: rows 0 .. 221
        for x in range(2, w - px, px):
            for xx, yy in ((x, y), (x + MANY_L - 2, y + MANY_T + 1)):
                b[yy:yy + MANY_T, xx:xx + MANY_L] = brick(k); k += 1
    for x in range(2, 530, py):              # vertical bars: rows 230 .. 479, columns 0 .. 531
        for y in range(230, h - px + 1, px):
            for xx, yy in ((x, y), (x + MANY_T + 1, y + MANY_L - 2)):
                b[yy:yy + MANY_L, xx:xx + MANY_T] = brick(k).T; k += 1
    M.bump_bar(b, 560, 240, 70, 5)           # the longest of the horizontal mask
    _vbar(b, 550, 260, 5, 70)                # ... of the vertical one
    return M.case(b, spot=(600, 420, 12))


# ---------------------------------------------------------------- 4. nothing stale
STALE_SHAPE = (380, POLY_N)


def gen_busy():
    """the notched polygon frame with 80 empty rows below"""
    return M.pad(gen_polygon(True), *STALE_SHAPE)


def gen_strip():
    """the busy frame's content, but rect is a 40-row strip far below it with two fragments of its own"""
    c = gen_busy()
    b = c['binary'].copy()
    M.bump_bar(b, 100, 345, 90, 5); M.bump_bar(b, 210, 355, 30, 5)
    mc = np.zeros(STALE_SHAPE, np.uint8)
    mc[330:370, :] = 255
    return with_contour(dict(c, binary=b), mc)


def end_points(mask):
    """PCA end points (x, y) of every external contour of close3x3(mask) that has any, in the oracle's arithmetic -> list of
    ((x1, y1), (x2, y2), vertex count)"""
    from oracle import stages as S
    out = []
    for p, _ in S.find_contours(S.close_rect(mask, 3, 3), 'external', 'simple'):
        p1, p2 = S.pca_endpoints(p.astype(np.float32))
        if p1 is not None:
            out.append(((int(p1[0]), int(p1[1])), (int(p2[0]), int(p2[1])), len(p)))
    return out
