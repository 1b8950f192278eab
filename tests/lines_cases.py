"""Inputs for the lines stage on its own (cpe_debug_lines, include/cpe.h): one idea per generator, the smallest frames that
hold it.  A case is dict(exp_h, exp_v u8 [h,w] (0 / 255), joints i32 (k,2) (x, y) in the order the stage gets them, n_joints,
rect (x, y, w, h), r0, status (what the stages in front left: 0, 1 or 2), g7, gray u8 [h,w], target, subpixel (None or
(window, step))).  Components are one pixel wide unless a generator says otherwise and lie inside rect; a pitch of 2 keeps
them apart under 8-connectivity.  The oracle side of every case and the checks that each generator reaches the edge it is
named for live in tests/test_lines_generators_cpu.py; tests/test_lines_stage_gpu.py runs the cases through the kernel.

Two exits of the kernel cannot be reached by any input, and have no generator: CPE_ST_NO_LINES through `ccol < 0` (an
intersection is always entered in a row's and in a column's list, so a frame with a row point has a column point) and
CPE_ST_EMPTY (the centre column itself is kept, and it holds at least the centre point's intersection)."""
import numpy as np

MAXJ, MAXL, MAXLP, MAXP = 16384, 256, 1024, 2048      # include/cpe.h CPE_MAXJ, CPE_MAXL, CPE_MAXLP, CPE_MAXP
OVF_LINES = 2                                         # csrc/cpe_dev.h FrameState::overflow bit
GROUP_COUNTS = (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257)


def noise(h, w, seed):
    return np.random.default_rng(seed).integers(0, 200, (h, w)).astype(np.uint8)


def case(exp_h, exp_v, joints, rect=None, r0=15, status=0, g7=None, gray=None, target='cylinder', subpixel=None, n_joints=None,
         seed=1):
    exp_h = np.where(np.asarray(exp_h) != 0, 255, 0).astype(np.uint8)
    exp_v = np.where(np.asarray(exp_v) != 0, 255, 0).astype(np.uint8)
    h, w = exp_h.shape
    joints = np.ascontiguousarray(np.asarray(joints, np.int64).reshape(-1, 2).astype(np.int32))
    assert len(joints) <= MAXJ and h >= 64 and w >= 64
    g7 = noise(h, w, seed) if g7 is None else np.ascontiguousarray(g7, np.uint8)
    return dict(exp_h=exp_h, exp_v=exp_v, joints=joints, n_joints=len(joints) if n_joints is None else n_joints,
                rect=tuple(int(v) for v in (rect if rect is not None else (0, 0, w, h))), r0=int(r0), status=int(status), g7=g7,
                gray=g7 if gray is None else np.ascontiguousarray(gray, np.uint8), target=target, subpixel=subpixel)


def transposed(c):
    """the case mirrored at the diagonal: rows become columns"""
    x, y, rw, rh = c['rect']
    return dict(c, exp_h=np.ascontiguousarray(c['exp_v'].T), exp_v=np.ascontiguousarray(c['exp_h'].T),
                joints=np.ascontiguousarray(c['joints'][:, ::-1]), rect=(y, x, rh, rw), g7=np.ascontiguousarray(c['g7'].T),
                gray=np.ascontiguousarray(c['gray'].T))


def shuffled(c, seed=5):
    return dict(c, joints=np.ascontiguousarray(c['joints'][np.random.default_rng(seed).permutation(len(c['joints']))]))


def raster(joints):
    j = np.asarray(joints).reshape(-1, 2)
    return j[np.lexsort((j[:, 0], j[:, 1]))]


def lattice(h, w, xs, ys, xspan=None, yspan=None, cross=True):
    """horizontal lines at ys over xspan into exp_h, vertical lines at xs over yspan into exp_v; joints at the crossings in
    raster order (cross=False: none)"""
    eh = np.zeros((h, w), np.uint8); ev = np.zeros((h, w), np.uint8)
    x0, x1 = xspan if xspan else (min(xs), max(xs))
    y0, y1 = yspan if yspan else (min(ys), max(ys))
    for y in ys:
        eh[y, x0:x1 + 1] = 255
    for x in xs:
        ev[y0:y1 + 1, x] = 255
    j = [(x, y) for y in sorted(ys) for x in sorted(xs)] if cross else []
    return eh, ev, j


def oracle(c):
    """stages.lines_stage of a case; a frame an earlier stage ended is left alone (status kept, nothing else)"""
    from oracle import stages as S
    if c['status'] != 0:
        return dict(status=c['status'], overflow=0, center=np.zeros(2), xy=np.zeros((0, 2)), id=np.zeros((0, 2), np.int32), rows=None,
                    cols=None, n_rows=0, n_cols=0, n_groups=(0, 0))
    sp = c['subpixel']
    return S.lines_stage(c['exp_h'], c['exp_v'], c['joints'][:c['n_joints']], c['rect'], c['r0'], c['g7'], c['gray'],
                         subpixel=sp is not None, window=sp[0] if sp else 7, step=sp[1] if sp else 1.0, planar=c['target'] == 'plane')


# ---------------------------------------------------------------- group count (the ballot search: lane k owns groups k + 64 q)
def gen_groups(G, side='row', shuffle=False):
    """G short row segments of 3 joints (9 px, 10 per line of the frame, lines 2 px apart) and three columns through the
    gaps between them, so that every row meets a column whichever column remove_label takes: G label groups on the row side,
    G - 1 rows in the result; 257 groups overflow.  side='col': the transposed frame."""
    h = w = 128
    eh = np.zeros((h, w), np.uint8); ev = np.zeros((h, w), np.uint8)
    j = []
    for g in range(G):
        x0, y = 7 + 11 * (g % 10), 12 + 2 * (g // 10)
        eh[y, x0:x0 + 9] = 255
        j += [(x0, y), (x0 + 4, y), (x0 + 8, y)]
    for x in (27, 60, 104):
        ev[4:125, x] = 255
        j += [(x, 5), (x, 65), (x, 123)]
    c = case(eh, ev, raster(j), seed=G)
    if shuffle:
        c = shuffled(c, G)
    return transposed(c) if side == 'col' else c


# ---------------------------------------------------------------- joints per group (rank >= CPE_MAXLP)
def gen_group_size(N, side='row'):
    """one filled 32 x 33 block of the row mask carries N joints (its first N pixels in raster order), between a row that
    remove_label takes and two more rows; three columns"""
    h = w = 128
    eh, ev, j = lattice(h, w, (20, 60, 100), (10, 30, 110), (14, 110), (5, 120), cross=False)
    j += [(x, y) for y in (10, 30, 110) for x in (16, 50, 108)] + [(x, y) for x in (20, 60, 100) for y in (7, 51, 119)]
    eh[60:93, 40:72] = 255
    blk = [(40 + k % 32, 60 + k // 32) for k in range(N)]
    c = case(eh, ev, list(raster(j)) + blk, seed=N)
    return transposed(c) if side == 'col' else c


# ---------------------------------------------------------------- point count (total > CPE_MAXP)
def gen_points(extra=0):
    """65 x (41 + extra) lattice at pitch 4: remove_label leaves 64 rows and 40 + extra columns; the one bright window of g7
    sits on column 8, so 32 + extra columns are kept: exactly 2048 points, or 2112"""
    h = w = 320
    xs = [20 + 4 * k for k in range(41 + extra)]; ys = [20 + 4 * k for k in range(65)]
    eh, ev, j = lattice(h, w, xs, ys)
    g7 = np.zeros((h, w), np.uint8)
    g7[136:144, 48:56] = 255
    return case(eh, ev, j, g7=g7)


# ---------------------------------------------------------------- label planes (ccl_unions leaves links, k_lines follows them)
def _spiral(hh, ww):
    """a rectangular spiral from the top-left corner inwards, arms 2 px apart"""
    a = np.zeros((hh, ww), np.uint8)
    x0, y0, x1, y1 = 0, 0, ww - 1, hh - 1
    x = y = 0
    while True:
        if x1 - x < 2:
            break
        a[y, x:x1 + 1] = 1; x = x1; y0 += 2
        if y1 - y < 2:
            break
        a[y:y1 + 1, x] = 1; y = y1; x1 -= 2
        if x - x0 < 2:
            break
        a[y, x0:x + 1] = 1; x = x0; y1 -= 2
        if y - y0 < 2:
            break
        a[y0:y + 1, x] = 1; y = y0; x0 += 2
    return a


def _comb(hh, ww):
    a = np.zeros((hh, ww), np.uint8)
    a[hh - 1, :] = 1
    a[:, ::2] = 1
    return a


def _serpentine(hh, ww):
    a = np.zeros((hh, ww), np.uint8)
    for k, y in enumerate(range(0, hh, 2)):
        a[y, :] = 1
        if y + 2 < hh:
            a[y + 1, ww - 1 if k % 2 == 0 else 0] = 1
    return a


def geodesic(comp):
    """8-connected walking distance of every pixel of a component (bool [h,w]) from its raster-first pixel (-1 outside)"""
    hh, ww = comp.shape
    d = np.full((hh, ww), -1, np.int32)
    ys, xs = np.nonzero(comp)
    cur = [(int(ys[0]), int(xs[0]))]
    d[cur[0]] = 0
    k = 0
    while cur:
        k += 1
        nxt = []
        for y, x in cur:
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < hh and 0 <= xx < ww and comp[yy, xx] and d[yy, xx] < 0:
                        d[yy, xx] = k
                        nxt.append((yy, xx))
        cur = nxt
    return d


def far_joints(plane, axis, k=3):
    """per component of the plane, k pixels as far (walking distance) from its raster-first pixel as can be with pairwise
    different x (axis 0: a row's fit stays regular) or y (axis 1), farthest first; components in label order.
    -> joints, the walking distance of each component's first joint"""
    from scipy import ndimage
    lab, n = ndimage.label(plane != 0, structure=np.ones((3, 3)))
    out, dist = [], []
    for i, sl in enumerate(ndimage.find_objects(lab)):
        d = geodesic(lab[sl] == i + 1)
        ys, xs = np.nonzero(d >= 0)
        order = np.argsort(-d[ys, xs], kind='stable')
        got = []
        for q in order:
            p = (int(xs[q]) + sl[1].start, int(ys[q]) + sl[0].start)
            if all(p[axis] != g[axis] for g in got):
                got.append(p)
                if len(got) == k:
                    break
        out += got
        dist.append(int(d[got[0][1] - sl[0].start, got[0][0] - sl[1].start]))
    return out, dist


LABEL_WIDTHS = (128, 650, 801)
LABEL_RECTS = ('frame', 'tl', 'br')


def gen_labels(w, where='frame', h=64):
    """a spiral, a comb and a serpentine side by side fill rect (the frame, or a rectangle in its top-left / bottom-right
    corner) but for a short row along its top edge and a short column at its bottom edge, which remove_label takes; the
    column mask is the row mask turned by 180 degrees.  Three joints per component at its far end, where the label pass has the
    longest way to the component's first pixel.  w % 16 == 0: the word-level label passes, 650 and 801: the byte-level ones."""
    rw, rh = (w, h) if where == 'frame' else (w - 21, h - 11)
    x0, y0 = (0, 0) if where != 'br' else (w - rw, h - rh)
    ch = rh - 5
    canvas = np.zeros((ch, rw), np.uint8)
    pw = (rw - 4) // 3
    canvas[:, :pw] = _spiral(ch, pw)
    canvas[:, pw + 2:2 * pw + 2] = _comb(ch, pw)
    canvas[:, 2 * pw + 4:] = _serpentine(ch, rw - 2 * pw - 4)
    eh = np.zeros((h, w), np.uint8); ev = np.zeros((h, w), np.uint8)
    eh[y0 + 2:y0 + 2 + ch, x0:x0 + rw] = canvas
    ev[y0 + 2:y0 + 2 + ch, x0:x0 + rw] = canvas[::-1, ::-1]
    jh, dh = far_joints(eh, 0)
    jv, dv = far_joints(ev, 1)
    eh[y0, x0:x0 + 3] = 255
    ev[y0 + rh - 2:y0 + rh, x0 + 5] = 255
    j = jh + jv + [(x0, y0), (x0 + 1, y0), (x0 + 2, y0), (x0 + 5, y0 + rh - 2), (x0 + 5, y0 + rh - 1)]
    c = case(eh, ev, j, rect=(x0, y0, rw, rh), seed=w)
    c['far'] = dh + dv
    return c


# ---------------------------------------------------------------- joint lookup
def _small_lattice(h=128, w=128, pitch=16, n=6, at=16):
    p = [at + pitch * k for k in range(n)]
    return lattice(h, w, p, p)


def gen_lookup():
    """a 6 x 6 lattice whose joint list is interleaved with joints outside the frame (negative, equal to w or h, far away),
    on a row only, on a column only and on background in both masks"""
    eh, ev, j = _small_lattice()
    w = h = 128
    extra = [(-1, 20), (20, -1), (w, 32), (32, h), (-5, -5), (1 << 30, 3), (3, -(1 << 30)), (w + 7, h + 7),
             (20, 16), (24, 32), (90, 96),         # on a row, between columns
             (16, 21), (48, 70), (96, 40),         # on a column, between rows
             (21, 21), (0, 0), (127, 127), (50, 51)]   # background in both masks
    out = []
    for k, p in enumerate(j):
        out.append(p)
        if k % 2 == 0 and k // 2 < len(extra):
            out.append(extra[k // 2])
    return case(eh, ev, out)


def gen_no_joints():
    """n_joints = 0 in front of a table that still holds an earlier frame's joints"""
    eh, ev, j = _small_lattice()
    return case(eh, ev, j, n_joints=0)


def gen_all_joints():
    """n_joints = CPE_MAXJ: every pixel of the 128 x 128 frame is a joint; rows and columns every 8 pixels, so most joints
    lie on background, 128 on every line, 16 on two lines"""
    p = list(range(4, 128, 8))
    eh, ev, _ = lattice(128, 128, p, p, (0, 127), (0, 127))
    j = [(x, y) for y in range(128) for x in range(128)]
    assert len(j) == MAXJ
    return case(eh, ev, j)


# ---------------------------------------------------------------- early exits
def gen_one_row():
    eh, ev, j = lattice(128, 128, (20, 60, 100), (64,), (10, 110), (10, 110))
    return case(eh, ev, j + [(20, 12), (60, 12), (100, 12), (20, 100), (60, 100), (100, 100)])


def gen_one_col():
    return transposed(gen_one_row())


def gen_apart():
    """rows on the left, columns farther to the right than a row's domain reaches (+ 50): no intersection"""
    h, w = 128, 256
    eh = np.zeros((h, w), np.uint8); ev = np.zeros((h, w), np.uint8)
    j = []
    for y in (20, 50, 80, 110):
        eh[y, 10:41] = 255
        j += [(10, y), (25, y), (40, y)]
    for x in (200, 220, 240):
        ev[10:120, x] = 255
        j += [(x, 10), (x, 60), (x, 119)]
    return case(eh, ev, j)


def gen_tiny_groups(subpixel=None):
    """a 5 x 5 lattice, a column along x = 0, and groups of one and two joints on both sides: their equation stays [0] * 6, a
    line along the other axis with the domain [0, 0] that meets the column at x = 0 in (0, 0)"""
    eh, ev, j = _small_lattice(n=5, at=24)
    ev[0:60, 0] = 255
    j += [(0, 10), (0, 30), (0, 50)]
    eh[110, 30:40] = 255; j += [(33, 110)]
    eh[114, 30:40] = 255; j += [(31, 114), (38, 114)]
    ev[100:120, 60] = 255; j += [(60, 105)]
    ev[100:120, 70] = 255; j += [(70, 101), (70, 118)]
    return case(eh, ev, j, subpixel=subpixel, gray=noise(128, 128, 9))


def gen_status(st):
    eh, ev, j = _small_lattice()
    return case(eh, ev, j, status=st)


# ---------------------------------------------------------------- centre search (two 256-thread arg-reductions)
def _dense():
    """20 x 20 lattice at pitch 6: 19 x 19 = 361 row points, more than one per thread"""
    p = [4 + 6 * k for k in range(20)]
    return lattice(128, 128, p, p) + (p,)


def gen_constant_g7():
    eh, ev, j, _ = _dense()
    return case(eh, ev, j, g7=np.full((128, 128), 200, np.uint8))


def gen_two_maxima():
    """two windows of 255 on row points 200 (thread 200) and 260 (thread 4): the first must win the tie"""
    eh, ev, j, p = _dense()
    g7 = np.full((128, 128), 30, np.uint8)
    for q in (200, 260):
        x, y = p[q % 19], p[1 + q // 19]
        g7[y - 4:y + 4, x - 4:x + 4] = 255
    return case(eh, ev, j, g7=g7)


EDGES = ('left', 'right', 'top', 'bottom')


def gen_edge_max(edge):
    """the maximum at a point whose window the frame clips: rows at y = 2 and h - 2, columns at x = 2 and w - 2; remove_label
    takes the row at y = 0 and the short column at x = 12 (the last in min-y order)"""
    h = w = 96
    xs = [2, 22, 42, 62, 82, 94]; ys = [0, 2, 22, 42, 62, 82, 94]
    eh, ev, j = lattice(h, w, xs, ys, (0, 95), (0, 95))
    ev[50:96, 12] = 255
    j = list(raster(j + [(12, 62), (12, 82), (12, 94)]))
    x, y = dict(left=(2, 42), right=(94, 42), top=(42, 2), bottom=(42, 94))[edge]
    g7 = np.full((h, w), 50, np.uint8)
    g7[max(y - 4, 0):y + 4, max(x - 4, 0):x + 4] = 255
    c = case(eh, ev, j, g7=g7)
    c['want_center'] = (x, y)
    return c


def gen_x_equals_w():
    """a column leaning to the right meets the row y = 10 at x = w = rect.x + rect.w, the last x the rectangle test accepts,
    and that point is the centre"""
    h = w = 96
    eh, ev, j = lattice(h, w, (10, 30, 50), (2, 10, 40, 70), (4, 86), (4, 75))
    ev[80:96, 20] = 255                                  # the last column in min-y order: remove_label takes it
    j += [(20, 80), (20, 88), (20, 95)]
    for y in range(30, 71):
        ev[y, w - 1 - (y - 30 + 10) // 20] = 255
    j += [(w - 1, 30), (w - 2, 50), (w - 3, 70)]
    g7 = np.full((h, w), 50, np.uint8)
    g7[6:14, w - 4:w] = 255
    return case(eh, ev, j, g7=g7)


# ---------------------------------------------------------------- planar target
PLANE_R0 = (0, 4, 5, 9)       # half = int(r0 / 4.5) = 0, 0, 1, 2


def gen_plane_r0(r0):
    eh, ev, j = _small_lattice(n=7)
    return case(eh, ev, j, r0=r0, target='plane')


def gen_plane_two_joints():
    """every line carries two joints (none at a crossing): degree-1 fits through two points"""
    p = [20 + 16 * k for k in range(5)]
    eh, ev, _ = lattice(128, 128, p, p, (10, 110), (10, 110))
    j = [(12 + k, y) for k, y in enumerate(p)] + [(108 - k, y) for k, y in enumerate(p)]
    j += [(x, 13 + k) for k, x in enumerate(p)] + [(x, 107 - k) for k, x in enumerate(p)]
    return case(eh, ev, j, r0=9, target='plane')


def _plane_base(h=256, w=256):
    """three rows (joints away from every column) and three long columns with the smallest min y (5, 6, 7): the longest has
    the provisional domain 220 + 20 = 240 = the merge threshold"""
    eh = np.zeros((h, w), np.uint8); ev = np.zeros((h, w), np.uint8)
    j = []
    for y in (112, 152, 202):
        eh[y, 10:246] = 255
        j += [(12, y), (130, y), (244, y)]
    for k, x in enumerate((20, 120, 230)):
        ev[5 + k:226, x] = 255
        j += [(x, 5 + k), (x, 111), (x, 225)]
    return eh, ev, j


def _piece(ev, j, x, y0, y1):
    ev[y0:y1 + 1, x] = 255
    j += [(x, y0), (x, y0 + 7), (x, y1)] if y1 - y0 >= 7 else [(x, y0), (x, y1)]


def gen_plane_merge(kind):
    """the column merge of the planar script: runs of consecutive (min-y order) short columns are concatenated while their
    provisional domains (extent + 20) add up to at most the longest one (240)
      exact:  three pieces of extent 60 at x = 60: 80 + 80 + 80 = 240, one merged column
      plus1:  the same and a fourth piece (extent 3): 263 > 240, it starts a second run of its own
      n1024 / n1025: two 16-wide blocks of 512 and 512 / 513 joints merge into a list of 1024 / 1025 (overflow)
      lone:   one short column of a single joint: its run has fewer than 2 joints and is deleted"""
    eh, ev, j = _plane_base()
    if kind in ('exact', 'plus1'):
        for y0 in (20, 90, 160):
            _piece(ev, j, 60, y0, y0 + 60)
        if kind == 'plus1':
            _piece(ev, j, 170, 221, 224)
    elif kind in ('n1024', 'n1025'):
        ev[30:62, 40:56] = 255
        j += [(40 + k % 16, 30 + k // 16) for k in range(512)]
        n2 = 512 if kind == 'n1024' else 513
        ev[70:103, 80:96] = 255
        j += [(80 + k % 16, 70 + k // 16) for k in range(n2)]
    elif kind == 'lone':
        ev[30:50, 60] = 255
        j += [(60, 40)]
    return case(eh, ev, j, r0=9, target='plane')


PLANE_MERGES = ('exact', 'plus1', 'n1024', 'n1025', 'lone')


def gen_plane_first_nan():
    """the first row point has an empty window and later ones do not (the reference's max() keeps the first item when it is
    NaN): rect reaches past the right edge, and the first column in min-y order leans out of the frame where it meets the row"""
    h = w = 128
    eh = np.zeros((h, w), np.uint8); ev = np.zeros((h, w), np.uint8)
    eh[20, 10:101] = 255
    j = [(10, 20), (55, 20), (100, 20)]
    for y in range(40, 61):
        ev[y, 126 - (y - 40) // 2] = 255
    j += [(126, 40), (116, 60)]
    for x in (50, 80):
        ev[45:101, x] = 255
        j += [(x, 45), (x, 100)]
    return case(eh, ev, j, rect=(0, 0, w + 40, h), r0=5, target='plane')


# ---------------------------------------------------------------- sub-pixel refinement (cylinder target only)
SP_WINDOWS = (1, 3, 7, 13)       # 13: the largest window the API accepts (15 is refused)
SP_STEPS = (1.0, 0.5, 0.25)
SP_SHAPE = (256, 640)            # sample capacity per line: max(h, w) + 128 = 768


def _sp_gray(eh, ev, seed=3):
    """bright lines one pixel below / right of the mask's, with a soft profile, on noise"""
    base = np.maximum(np.roll(eh, 1, 0), np.roll(ev, 1, 1)).astype(np.float64)
    soft = base + 0.6 * (np.roll(base, 1, 0) + np.roll(base, -1, 0) + np.roll(base, 1, 1) + np.roll(base, -1, 1))
    g = np.clip(soft * 0.7, 0, 230) + np.random.default_rng(seed).integers(0, 20, eh.shape)
    return g.astype(np.uint8)


def gen_subpixel(window, step):
    """9 x 9 lattice of extent 80: every line is sampled over 180 px (721 samples at step 0.25, within the capacity)"""
    h, w = SP_SHAPE
    eh, ev, j = lattice(h, w, [100 + 10 * k for k in range(9)], [60 + 10 * k for k in range(9)])
    return case(eh, ev, j, gray=_sp_gray(eh, ev), subpixel=(window, step))


def gen_subpixel_long(step):
    """the same with one row of extent 400: 500 px of samples, 2001 at step 0.25 (> 768: overflow), 501 at step 1.0"""
    h, w = SP_SHAPE
    eh, ev, j = lattice(h, w, [100 + 10 * k for k in range(9)], [60 + 10 * k for k in range(9)])
    eh[150, 100:501] = 255
    j += [(100, 150), (300, 150), (500, 150)]
    return case(eh, ev, j, gray=_sp_gray(eh, ev), subpixel=(7, step))


def gen_subpixel_corner(window, side='row'):
    """a lattice against the top-left corner and a row that climbs out through the top edge: y = 10 - 0.2 x reaches -6 at the
    end of its domain (x = 80), more than window / 2 + 1 above the frame for windows up to 9 -- the reference raises there
    (status 7) and not for window 13.  Samples left of the frame (x < 0) are skipped by both.  side='col': transposed."""
    h = w = 128
    eh, ev, j = lattice(h, w, (4, 24, 44, 64), (14, 34, 54, 74), (0, 70), (0, 80))
    for x in range(10, 31):
        eh[10 - (x + 2) // 5, x] = 255
    j += [(10, 8), (20, 6), (30, 4)]
    eh[1, 40:60] = 255                       # the first row in min-y order: remove_label takes it
    j += [(40, 1), (50, 1), (59, 1)]
    c = case(eh, ev, j, gray=_sp_gray(eh, ev), subpixel=(window, 1.0))
    return transposed(c) if side == 'col' else c


def gen_subpixel_dark():
    """an all-zero grey frame: every window sums to 0 and the samples stay where they are"""
    h, w = SP_SHAPE
    eh, ev, j = lattice(h, w, [100 + 10 * k for k in range(9)], [60 + 10 * k for k in range(9)])
    return case(eh, ev, j, gray=np.zeros((h, w), np.uint8), subpixel=(7, 1.0))


# ---------------------------------------------------------------- the table of cases
def _build():
    C = {}
    for G in GROUP_COUNTS:
        for side in ('row', 'col'):
            for sh in (False, True):
                C[f'groups_{side}_{G}_{"shuffled" if sh else "raster"}'] = (gen_groups, (G, side, sh))
    for N in (1023, 1024, 1025):
        for side in ('row', 'col'):
            C[f'group_size_{side}_{N}'] = (gen_group_size, (N, side))
    C['points_2048'] = (gen_points, (0,))
    C['points_2112'] = (gen_points, (1,))
    for w in LABEL_WIDTHS:
        for where in LABEL_RECTS:
            C[f'labels_{w}_{where}'] = (gen_labels, (w, where))
    C['lookup'] = (gen_lookup, ())
    C['no_joints'] = (gen_no_joints, ())
    C['all_joints'] = (gen_all_joints, ())
    C['one_row'] = (gen_one_row, ())
    C['one_col'] = (gen_one_col, ())
    C['apart'] = (gen_apart, ())
    C['tiny_groups'] = (gen_tiny_groups, ())
    C['status_1'] = (gen_status, (1,))
    C['status_2'] = (gen_status, (2,))
    C['constant_g7'] = (gen_constant_g7, ())
    C['two_maxima'] = (gen_two_maxima, ())
    for e in EDGES:
        C[f'edge_max_{e}'] = (gen_edge_max, (e,))
    C['x_equals_w'] = (gen_x_equals_w, ())
    for r0 in PLANE_R0:
        C[f'plane_r0_{r0}'] = (gen_plane_r0, (r0,))
    C['plane_two_joints'] = (gen_plane_two_joints, ())
    for k in PLANE_MERGES:
        C[f'plane_merge_{k}'] = (gen_plane_merge, (k,))
    C['plane_first_nan'] = (gen_plane_first_nan, ())
    for win in SP_WINDOWS:
        for step in SP_STEPS:
            C[f'subpixel_w{win}_s{step}'] = (gen_subpixel, (win, step))
    for step in (1.0, 0.25):
        C[f'subpixel_long_s{step}'] = (gen_subpixel_long, (step,))
    for win in SP_WINDOWS:
        for side in ('row', 'col'):
            C[f'subpixel_corner_{side}_w{win}'] = (gen_subpixel_corner, (win, side))
    C['subpixel_dark'] = (gen_subpixel_dark, ())
    C['subpixel_tiny_groups'] = (gen_tiny_groups, ((7, 1.0),))
    return C


CASES = _build()
_MADE = {}
_REF = {}


def get(name):
    if name not in _MADE:
        f, a = CASES[name]
        _MADE[name] = f(*a)
    return _MADE[name]


def ref(name):
    """the oracle's result of a case, computed once"""
    if name not in _REF:
        _REF[name] = oracle(get(name))
    return _REF[name]


def expect_overflow(name):
    """OVF_LINES for the cases built to exceed a capacity of this stage, else 0"""
    return OVF_LINES if name in OVERFLOWS else 0


OVERFLOWS = {n for n in CASES if n.startswith(('groups_row_257', 'groups_col_257', 'group_size_row_1025', 'group_size_col_1025'))} | \
    {'points_2112', 'plane_merge_n1025', 'subpixel_long_s0.25'}


# ---------------------------------------------------------------- checks that do not go through the oracle's restatement
# The largest figures the oracle itself reaches over all the cases above (tests/test_lines_generators_cpu.py measures them and
# asserts them); the kernel, which must equal the oracle bit for bit, is allowed ten times as much against numpy.
ORACLE_FIT_DIFF = 5.1e-10       # px: fitted polynomial against numpy.polyfit of the group's joints, over the line's domain
ORACLE_RESIDUAL = 2.2e-12       # px: a reported intersection against each of its two polynomials


def lines_of(ls):
    """oracle LineSet -> [(eq[6], [(x, y), ...]), ...]"""
    return [] if ls is None else list(zip(ls.equations(), ls.points()))


def lines_of_table(d, prefix):
    """one dict of api.line_tables / FrameRecord.rows -> the same form"""
    return [(d['equations'][f'{prefix}{g + 1}'], d['points'][f'{prefix}{g + 1}']) for g in range(len(d['equations']))]


def scipy_groups(c):
    """group_points_by_label from scipy.ndimage.label (8-connected) of the masks cropped to rect: per side the joints of each
    label in order of first appearance (lists of (x, y)), without the capacities"""
    from scipy import ndimage
    x0, y0, rw, rh = c['rect']
    out = []
    for plane in (c['exp_h'], c['exp_v']):
        crop = plane[y0:y0 + rh, x0:x0 + rw]
        lab, _ = ndimage.label(crop != 0, structure=np.ones((3, 3)))
        groups, index = [], {}
        for x, y in c['joints'][:c['n_joints']].tolist():
            rx, ry = x - x0, y - y0
            if not (0 <= ry < lab.shape[0] and 0 <= rx < lab.shape[1]) or lab[ry, rx] == 0:
                continue
            k = index.setdefault(int(lab[ry, rx]), len(groups))
            if k == len(groups):
                groups.append([])
            groups[k].append((x, y))
        out.append(groups)
    return out


def _value_diff(coef_a, coef_b, ts):
    return float(np.max(np.abs(np.polyval(coef_a, ts) - np.polyval(coef_b, ts))))


def fit_diff(c, rows, cols):
    """every equation of the final lines (rows, cols as lines_of gives them) against numpy.polyfit of the joints of the label
    group it must come from -> the largest difference of the two polynomials over the line's domain (at its joints and at
    both ends), in pixels.  Raises AssertionError for a line that no group of the scipy labelling explains."""
    planar = c['target'] == 'plane'
    deg, margin, need = (1, 50.0, 2) if planar else (2, 50.0, 3)
    worst = 0.0
    for side, lines in enumerate((rows, cols)):
        groups = [np.array(g[:MAXLP], np.float64) for g in scipy_groups(c)[side][:MAXL]]
        cands = list(groups)
        if planar and side == 1:      # merged columns: runs of consecutive groups in (stable) min-y order
            order = sorted(range(len(groups)), key=lambda k: groups[k][:, 1].min())
            cands = [np.concatenate([groups[k] for k in order[a:b]])[:MAXLP] for a in range(len(order)) for b in range(a + 1, len(order) + 1)]
        kc = side                     # rows: y = f(x), cols: x = f(y)
        by_domain = {}
        for g in cands:
            if len(g) < need:
                continue
            o = np.argsort(g[:, kc], kind='stable')
            t, u = g[o, kc], g[o, 1 - kc]
            if len(np.unique(t)) > deg:
                by_domain.setdefault((t[0] - margin, t[-1] + margin), []).append((np.polyfit(t, u, deg), t))
        for eq, _ in lines:
            eq = np.asarray(eq, np.float64)
            lo, hi = (eq[2], eq[3]) if planar else (eq[3], eq[4])
            if not eq.any():
                assert any(len(g) < need for g in cands), ('an empty equation without a group too small to fit', side)
                continue
            fits = by_domain.get((float(lo), float(hi)), ())
            best = None
            if fits:
                coefs = np.array([f[0] for f in fits])
                k = int(np.argmin(np.abs(coefs - eq[:deg + 1]).max(1)))       # the group whose fit this is, if any
                best = _value_diff(eq[:deg + 1], coefs[k], np.concatenate([fits[k][1], [lo, hi]]))
            assert best is not None, ('no label group has the domain of this line', side, lo, hi)
            worst = max(worst, best)
    return worst


def residual(c, rows, cols):
    """the largest distance of a reported intersection from either of its two polynomials, in pixels"""
    deg = 1 if c['target'] == 'plane' else 2
    worst = 0.0
    for side, lines in enumerate((rows, cols)):
        for eq, pts in lines:
            for p in pts:
                worst = max(worst, abs(p[1 - side] - float(np.polyval(np.asarray(eq[:deg + 1], np.float64), p[side]))))
    return worst
