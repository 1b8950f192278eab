"""The blob stage of detect_largest_blob on its own (cpe_debug_blob_region, include/cpe.h) against the oracle, with tolerance 0.

The entry runs the library's region stage on an image of the test's choosing: the image IS what SimpleBlobDetector sweeps
(an identity table replaces LAB-L and CLAHE).  Every case is compared with oracle/stages.simple_blob_detector and
largest_blob_from_sweep on the same image:
  - blobs per threshold (CPE_PLANE_SWEEP [42+k]) and the accepted blobs (x, y, r) in f64, as sorted lists;
  - the key points as f32 bits, in order: k_blob_merge numbers the groups in creation order, as the detector does;
  - n_kp, rect and mask_contour;
  - the sweep's component counters [8+k] / [25+k] against the hole / outer contours of cv2.findContours(RETR_LIST).
The images are small generators, one idea each: the area limits and prunes of the tracers, nesting with graded grey levels,
content at the rectangle and frame edges, the three median paths, the group merge's grid search, HBM groups and ranking
paths, and the centre-pixel test at exact .5 centroids."""
import numpy as np
import pytest
import torch

NTHR = 17
OVF_GROUPS = 1024      # csrc/cpe_dev.h
MED_FAST = 496         # csrc/region.hip: CH_DIRECT * CH_PTS border points need no chunk-chain walk
SEL_CAP = 256          # csrc/region.hip: wave_select ranks at most this many candidates directly


# ---------------------------------------------------------------- image generators (u8, the sweep image itself)
def _canvas(h, w, bg=255, margin=6):
    """bright field inset by a dark margin: the working rectangle (pixels > 50) does not touch the frame"""
    img = np.zeros((h, w), np.uint8)
    img[margin:h - margin, margin:w - margin] = bg
    return img


def _polyominoes(nmax):
    """every fixed (translation-distinct) 4-connected shape of 1 .. nmax cells, as tuples of (y, x)"""
    def norm(cells):
        my = min(c[0] for c in cells); mx = min(c[1] for c in cells)
        return tuple(sorted((y - my, x - mx) for y, x in cells))
    level = {((0, 0),)}
    out = list(level)
    for _ in range(nmax - 1):
        nxt = set()
        for s in level:
            cs = set(s)
            for y, x in s:
                for dy, dx in ((1, 0), (-1, 0), (0, 1), (0, -1)):
                    c = (y + dy, x + dx)
                    if c not in cs:
                        nxt.add(norm(s + (c,)))
        level = nxt
        out += sorted(level)
    return out


def gen_small_holes(h=481, w=641):
    """every hole shape of 1 .. 6 pixels (307 of them), 16 px apart"""
    img = _canvas(h, w)
    shapes = _polyominoes(6)
    assert len(shapes) == 1 + 2 + 6 + 19 + 63 + 216
    cols = (w - 24) // 16
    for i, s in enumerate(shapes):
        y0, x0 = 12 + 16 * (i // cols), 12 + 16 * (i % cols)
        for y, x in s:
            img[y0 + y, x0 + x] = 0
    return img


def gen_area_limit_holes(h=1200, w=1920):
    """holes around the 5000 limits: compact and elongated rectangles of 4692 .. 5050 pixels (polygon area (a+1)(b+1)),
    1-pixel-wide meanders whose polygon area (about 2 n) straddles 5000, and diagonal staircases"""
    img = _canvas(h, w)
    x, y = 20, 20
    for a, b in ((68, 69), (69, 69), (70, 70), (70, 71), (71, 71), (69, 70), (50, 99), (50, 100), (40, 125), (10, 470),
                 (10, 489), (10, 490), (10, 499), (10, 500), (10, 505), (20, 227), (9, 540), (4, 1199)):
        if x + b + 10 > w - 20:
            x, y = 20, y + 140
        img[y:y + a, x:x + b] = 0
        x += b + 12
    # 1-pixel-wide meanders: rows of 200 pixels joined at alternate ends; pixel counts around 2500 (area ~ 5000) and 4900
    y += 140
    x = 20
    for n in (2480, 2490, 2495, 2499, 2500, 2505, 2510, 4900):
        px = 0
        row = 0
        while px < n:
            yy = y + 2 * row
            run = min(200, n - px)
            start = x if row % 2 == 0 else x + 200 - run
            img[yy, start:start + run] = 0
            px += run
            if px < n:
                img[yy + 1, x + (199 if row % 2 == 0 else 0)] = 0
                px += 1
            row += 1
        x += 215
        if x + 215 > w - 20:
            x, y = 20, y + 2 * row + 10
    # diagonal staircases (4-connected steps): n = 2 m pixels
    y = h - 420
    x = 20
    for m in (50, 200, 395, 400):
        for i in range(m):
            if y + i < h - 10:
                img[y + i, x + i:x + i + 2] = 0
        x += 420
    return img


def gen_bright_rings(h=481, w=641):
    """bright square rings on dark (their centroid is dark) enclosing 4970 .. 5041 hole pixels, and C shapes"""
    img = np.zeros((h, w), np.uint8)
    x, y = 10, 10
    for a, b, gap in ((70, 71, 0), (50, 100, 0), (71, 71, 0), (49, 101, 0), (70, 71, 1), (30, 40, 0), (60, 70, 1), (20, 20, 1)):
        if x + b + 6 > w - 4:
            x, y = 10, y + 110
        img[y:y + a + 4, x:x + b + 4] = 200
        img[y + 2:y + 2 + a, x + 2:x + 2 + b] = 0
        if gap:
            img[y + 2 + a // 2:y + 4 + a // 2, x:x + 2] = 0       # a C: the ring opened on its west side
        x += b + 14
    return img


def gen_nested(h=203, w=200):
    """square rings 5 levels deep with graded levels (components merge at different thresholds), plateaus at 50 + 10 k
    and +-1"""
    img = np.zeros((h, w), np.uint8)
    levels = (230, 40, 180, 95, 150, 61, 211, 49, 120)
    cy, cx = 90, 90
    for i, v in enumerate(levels):
        r = 80 - 9 * i
        img[cy - r:cy + r + 1, cx - r:cx + r + 1] = v
    for j, v in enumerate((50, 51, 59, 60, 61, 110, 111, 109, 210, 211, 209, 220)):
        img[183:195, 4 + 16 * j:14 + 16 * j] = v
        img[186:190, 7 + 16 * j:10 + 16 * j] = max(v - 30, 0)
    return img


def gen_edges(h=203, w=200):
    """content touching the frame edge, pockets open to the frame edge and to the rectangle edge, discs clipped by the
    frame"""
    img = np.zeros((h, w), np.uint8)
    img[0:60, 0:80] = 230                  # bright block in the corner: touches two frame edges
    img[10:20, 0:12] = 0                   # pocket open to the frame edge (not a hole)
    img[30:40, 30:40] = 0                  # a real hole
    img[45:52, 70:80] = 0                  # pocket open to the block's east side
    for k in range(6):                     # dots along the bottom and right edges: their discs leave the frame
        img[h - 8:h - 3, 20 + 25 * k:25 + 25 * k] = 200
        img[h - 7:h - 4, 21 + 25 * k:24 + 25 * k] = 20
        img[80 + 18 * k:85 + 18 * k, w - 6:w - 1] = 200
        img[81 + 18 * k:84 + 18 * k, w - 5:w - 2] = 20
    img[100:140, 60:100] = 160            # a bright square inside the frame with a hole at the rectangle's east edge
    img[110:130, 90:100] = 40
    return img


def gen_equal_unions(h=203, w=200):
    """two identical dot clusters: their disc unions have exactly equal area (OpenCV's contour order breaks the tie)"""
    img = np.zeros((h, w), np.uint8)
    for ox in (20, 110):
        for dy, dx in ((0, 0), (0, 22), (22, 0), (22, 22)):
            y, x = 70 + dy, ox + dx
            img[y - 6:y + 7, x - 6:x + 7] = 210
            img[y - 2:y + 3, x - 2:x + 3] = 30
    return img


def gen_median_paths(h=481, w=641):
    """hole borders of 494 .. 498 points (around MED_FAST), a disc hole and a plus whose border distances repeat, and a
    bright 2-pixel-wide spiral whose centroid falls in the dark (the bright path: second trace + histogram select)"""
    img = _canvas(h, w)
    for k, (a, b, cut) in enumerate(((20, 227, 0), (20, 228, 0), (20, 228, 1), (20, 229, 0), (20, 229, 1))):
        y, x = 10 + 26 * (k // 2), 10 + 240 * (k % 2)
        img[y:y + a, x:x + b] = 0
        if cut:
            img[y, x] = 255                      # a corner pixel less: one border point less (495, 497)
    img[90:110, 10:237] = 0
    img[90, 20] = 255                           # a bright pixel cut into the border: another border length
    yy, xx = np.mgrid[0:h, 0:w]
    img[(yy - 150) ** 2 + (xx - 80) ** 2 <= 20 ** 2] = 0
    img[(yy - 150) ** 2 + (xx - 160) ** 2 <= 10 ** 2] = 0
    img[145:156, 200:203] = 0
    img[149:152, 196:207] = 0
    # the spiral: a square spiral of a 2-pixel-wide bright line in a dark box
    img[180:460, 300:620] = 0
    cy, cx = 320, 460
    y, x, d, step = cy, cx, 0, 4
    dirs = ((0, 1), (1, 0), (0, -1), (-1, 0))
    for seg in range(26):
        dy, dx = dirs[d]
        for _ in range(step):
            if 182 <= y < 458 and 302 <= x < 618:
                img[y:y + 2, x:x + 2] = 220
            y += dy; x += dx
        d = (d + 1) % 4
        if seg % 2 == 1:
            step += 5
    img[cy - 1:cy + 3, cx - 3:cx + 1] = 0
    return img


def gen_lattice(h=481, w=641, pitch=14):
    """1500+ persistent dots (> MAXG_LDS groups), each a 3 x 3 hole: 17 centres per group"""
    img = _canvas(h, w)
    for y in range(12, h - 12, pitch):
        for x in range(12, w - 12, pitch):
            img[y - 1:y + 2, x - 1:x + 2] = 0
    return img


def gen_one_threshold_crowd(h=1200, w=1920):
    """more than MG_RANK_DIRECT blobs at one threshold: 3 x 3 holes of 55 in a field of 65 exist at threshold 60 only;
    a few persistent dots give key points"""
    img = np.zeros((h, w), np.uint8)
    img[8:h - 8, 8:w - 8] = 65
    for y in range(14, h - 14, 13):
        for x in range(14, w - 14, 13):
            img[y - 1:y + 2, x - 1:x + 2] = 55
    for k in range(8):
        y, x = 200 + 100 * k, 300 + 150 * k
        img[y - 8:y + 9, x - 8:x + 9] = 240
        img[y - 2:y + 3, x - 2:x + 3] = 0
    return img


def gen_cluster(h=203, w=200, per=2):
    """`per` holes within 10 px of each other, persistent over the 17 thresholds: the first group collects
    1 + 16 per centres (per = 2: 33 centres, more than MG_STAGE; per >= 3: more than GCAP)"""
    img = _canvas(h, w)
    offs = ((0, 0), (0, 5), (5, 0), (5, 5))[:per]
    for cy, cx in ((60, 60), (140, 140)):
        for dy, dx in offs:
            img[cy + dy - 1:cy + dy + 2, cx + dx - 1:cx + dx + 2] = 0
    img[60 - 1:60 + 2, 140 - 1:140 + 2] = 0
    return img


def gen_long_hole(h=481, w=641):
    """a 3 x 600 hole (median radius ~150 px: it joins and absorbs groups many 64 px cells away) among small dots"""
    img = _canvas(h, w)
    img[239:242, 20:620] = 0
    for k, (y, x) in enumerate(((200, 320), (280, 330), (240, 100), (240, 560), (150, 320), (330, 400), (100, 100))):
        img[y - 1:y + 2, x - 1:x + 2] = 0
        if k % 2:
            img[y - 2:y + 3, x - 2:x + 3] = 0
    return img


def gen_exact_distances(h=203, w=200):
    """hole pairs whose centroids are exactly 10 apart (not joined: dist >= minDist) and 9 apart (joined)"""
    img = _canvas(h, w)
    for k, d in enumerate((10, 9, 10, 11)):
        y, x = 30 + 40 * k, 40
        img[y - 1:y + 2, x - 1:x + 2] = 0
        img[y - 1:y + 2, x + d - 1:x + d + 2] = 0
        img[y + d - 1:y + d + 2, x + 60 - 1:x + 60 + 2] = 0
        img[y - 1:y + 2, x + 60 - 1:x + 60 + 2] = 0
    return img


def _half_centroid_shapes(seed, want):
    """22 x 22 patches with a blob whose contour centroid lies exactly on a pixel edge (.5) where floor and rint pick
    pixels of different colour, and at most 2 blobs in all (a group then collects at most 33 centres)"""
    from oracle import stages as S
    rng = np.random.default_rng(seed)
    found = []
    while len(found) < want:
        m = np.zeros((14, 14), np.uint8)
        for a, b in rng.integers(3, 11, size=(int(rng.integers(3, 7)), 2)):
            m[a:a + int(rng.integers(1, 3)), b:b + int(rng.integers(1, 4))] = 255
        hole = rng.random() < 0.5
        patch = np.zeros((22, 22), np.uint8)
        patch[4:18, 4:18] = np.where(m > 0, 0, 255) if hole else m
        for pts, is_hole in S.find_contours(patch > 127, 'list', 'none'):
            if is_hole != hole:
                continue
            m00, m10, m01 = S.contour_moments(pts)
            if not 10 <= m00 < 5000:
                continue
            cx, cy = m10 / m00, m01 / m00
            ix, iy = int(np.rint(cx)), int(np.rint(cy))
            split_x = cx % 1.0 == 0.5 and patch[iy, int(np.floor(cx))] != patch[iy, ix]
            split_y = cy % 1.0 == 0.5 and patch[int(np.floor(cy)), ix] != patch[iy, ix]
            if split_x or split_y:
                if S.simple_blob_detector(patch, cap=16, blobs=True, blob_cap=4)[1][0] <= 2:
                    found.append(patch)
                break
    return found


def gen_half_centroids(h=203, w=200):
    """blobs with centroids at exact .5 where rint and floor disagree on the centre pixel's colour, 22 px apart"""
    img = np.zeros((h, w), np.uint8)
    for i, p in enumerate(_half_centroid_shapes(5, 36)):
        y0, x0 = 2 + 22 * (i // 9), 2 + 22 * (i % 9)
        img[y0:y0 + 22, x0:x0 + 22] = p
    return img


def gen_scene(h, w, seed):
    """random dots, rings, holes and ramps at random grey levels, with noise"""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 40, size=(h, w)).astype(np.int32)
    yy, xx = np.mgrid[0:h, 0:w]
    for _ in range(max(4, h * w // 3000)):
        cy, cx = int(rng.integers(0, h)), int(rng.integers(0, w))
        r = int(rng.integers(2, max(3, min(h, w) // 8)))
        v = int(rng.integers(40, 256))
        d = np.hypot(yy - cy, xx - cx) if rng.random() < 0.5 else np.maximum(abs(yy - cy), abs(xx - cx))
        if rng.random() < 0.5:
            img[d <= r] = v
        else:
            img[(d <= r) & (d > r * 0.6)] = v
        if rng.random() < 0.5:
            img[d <= r * 0.3] = int(rng.integers(0, 60))
    img += rng.integers(-6, 7, size=(h, w))
    return np.clip(img, 0, 255).astype(np.uint8)


CASES = {
    'small_holes': (gen_small_holes, (481, 641)),
    'area_limits': (gen_area_limit_holes, (1200, 1920)),
    'bright_rings': (gen_bright_rings, (481, 641)),
    'nested': (gen_nested, (203, 200)),
    'edges': (gen_edges, (203, 200)),
    'equal_unions': (gen_equal_unions, (203, 200)),
    'median_paths': (gen_median_paths, (481, 641)),
    'lattice': (gen_lattice, (481, 641)),
    'crowd': (gen_one_threshold_crowd, (1200, 1920)),
    'cluster33': (gen_cluster, (203, 200)),
    'long_hole': (gen_long_hole, (481, 641)),
    'exact_distances': (gen_exact_distances, (203, 200)),
    'half_centroids': (gen_half_centroids, (203, 200)),
}
SCENES = [(64, 64, 1), (67, 130, 2), (203, 200, 3), (481, 641, 4), (1200, 1920, 5)]


_IMAGES = {}


def _image(name):
    if name not in _IMAGES:
        fn, (h, w) = CASES[name]
        _IMAGES[name] = fn(h, w)
        assert _IMAGES[name].shape == (h, w) and _IMAGES[name].dtype == np.uint8
    return _IMAGES[name].copy()


# ---------------------------------------------------------------- the entry point and the comparison
def _run(cpe, gpu, imgs, kp_cap=4096, blob_cap=16384, ws=None):
    """cpe_debug_blob_region on u8 [n,h,w] -> dict of numpy results (ws: the workspace to run in, as the caller left it)"""
    from cpe_amd import api
    imgs = np.ascontiguousarray(imgs)
    n, h, w = imgs.shape
    ws = api.DetectWorkspace(n, h, w, gpu) if ws is None else ws.use(n)
    d = torch.from_numpy(imgs).to(gpu)
    kp = torch.zeros((n, kp_cap, 3), dtype=torch.float32, device=gpu)
    nkp = torch.zeros(n, dtype=torch.int32, device=gpu)
    bl = torch.zeros((n, NTHR, blob_cap, 3), dtype=torch.float64, device=gpu)
    nbl = torch.zeros((n, NTHR), dtype=torch.int32, device=gpu)
    L = cpe.lib.load()
    cpe.lib.check(L.cpe_debug_blob_region(d.data_ptr(), n, h, w, ws.view.data_ptr(), ws.bytes, kp.data_ptr(), kp_cap, nkp.data_ptr(),
                                          bl.data_ptr(), blob_cap, nbl.data_ptr(), torch.cuda.current_stream().cuda_stream),
                  'cpe_debug_blob_region')
    torch.cuda.synchronize()
    nkp_h = nkp.cpu().numpy()
    nbl_h = nbl.cpu().numpy()
    assert (nkp_h <= kp_cap).all() and (nbl_h <= blob_cap).all(), 'raise the test capacities'
    kp_h, bl_h = kp.cpu().numpy(), bl.cpu().numpy()
    return dict(kp=[kp_h[i, :nkp_h[i]] for i in range(n)], blobs=[[bl_h[i, k, :nbl_h[i, k]] for k in range(NTHR)] for i in range(n)],
                nkp=nkp_h, nblobs=nbl_h, state=ws.state(), mc=ws.plane('mask_contour').cpu().numpy(),
                sweep=ws.plane('sweep').cpu().numpy(), clahe=ws.plane('clahe').cpu().numpy())


def _frame(res, i):
    return {k: v[i] for k, v in res.items()}


def _same(a, b, tag):
    """two GPU results of one image: identical"""
    assert np.array_equal(a['nkp'], b['nkp']) and np.array_equal(a['nblobs'], b['nblobs']), tag
    assert np.array_equal(a['kp'].view(np.uint32), b['kp'].view(np.uint32)), tag
    for k in range(NTHR):
        assert np.array_equal(_sorted(a['blobs'][k]), _sorted(b['blobs'][k])), (tag, k)
    assert np.array_equal(a['mc'], b['mc']) and np.array_equal(a['sweep'][[*range(8, 8 + 3 * NTHR)]], b['sweep'][[*range(8, 8 + 3 * NTHR)]]), tag
    sa, sb = a['state'], b['state']
    for key in ('status', 'rect0', 'rect1', 'rect2', 'rect3', 'n_kp', 'n_groups', 'overflow'):
        assert sa[key] == sb[key], (tag, key)


def _sorted(rec):
    rec = np.asarray(rec, np.float64).reshape(-1, 3)
    return rec[np.lexsort((rec[:, 2], rec[:, 1], rec[:, 0]))]


_ORACLE_CACHE = {}


def _oracle(img):
    from oracle import stages as S
    key = (img.shape, img.tobytes())
    if key not in _ORACLE_CACHE:
        kp, stats, blobs = S.simple_blob_detector(img, blobs=True)
        st, mask, rect, nk = S.largest_blob_from_sweep(img)
        holes, outer = [], []
        for k in range(NTHR):
            cs = S.find_contours(img > 50 + 10 * k, 'list', 'none')
            holes.append(sum(1 for _, is_hole in cs if is_hole))
            outer.append(sum(1 for _, is_hole in cs if not is_hole))
        _ORACLE_CACHE[key] = dict(kp=kp, stats=stats, blobs=blobs, status=st, mask=mask, rect=rect, nk=nk, holes=holes, outer=outer)
    return _ORACLE_CACHE[key]


def _check(img, g, tag, allow_group_overflow=False):
    """one frame of a cpe_debug_blob_region result against the oracle, tolerance 0"""
    ref = _oracle(img)
    st = g['state']
    assert np.array_equal(g['clahe'], img), (tag, 'identity table: the sweep image is the input')
    assert list(g['sweep'][8:8 + NTHR]) == ref['holes'], (tag, 'holes', list(g['sweep'][8:8 + NTHR]), ref['holes'])
    assert list(g['sweep'][25:25 + NTHR]) == ref['outer'], (tag, 'outer', list(g['sweep'][25:25 + NTHR]), ref['outer'])
    assert list(g['sweep'][42:42 + NTHR]) == list(ref['stats']), (tag, 'blobs per threshold', list(g['sweep'][42:42 + NTHR]), list(ref['stats']))
    assert list(g['nblobs']) == list(ref['stats']), tag
    for k in range(NTHR):
        a, b = _sorted(g['blobs'][k]), _sorted(ref['blobs'][k])
        assert a.shape == b.shape and np.array_equal(a, b), (tag, 'blobs of threshold', 50 + 10 * k,
                                                             None if a.shape != b.shape else float(np.abs(a - b).max()))
    if allow_group_overflow:
        assert st['overflow'] & OVF_GROUPS, (tag, 'a group longer than GCAP must be reported', st['overflow'])
        return
    assert st['overflow'] == 0, (tag, st['overflow'])
    assert int(g['nkp']) == st['n_kp'] == len(ref['kp']) == ref['nk'], (tag, int(g['nkp']), st['n_kp'], len(ref['kp']))
    assert np.array_equal(g['kp'].view(np.uint32), ref['kp'].view(np.uint32)), (tag, 'key points (group order)')
    assert st['status'] == ref['status'], (tag, st['status'], ref['status'])
    assert np.array_equal(g['mc'], ref['mask']), (tag, 'mask_contour', int((g['mc'] != ref['mask']).sum()))
    if ref['status'] == 0:
        assert (st['rect0'], st['rect1'], st['rect2'], st['rect3']) == ref['rect'], (tag, 'rect')


def _coverage(img):
    """border lengths of the accepted blobs' contours (the median kernel's paths)"""
    from oracle import stages as S
    out = []
    for k in range(NTHR):
        for pts, is_hole in S.find_contours(img > 50 + 10 * k, 'list', 'none'):
            m00, m10, m01 = S.contour_moments(pts)
            if 10 <= m00 < 5000:
                out.append((len(pts), is_hole))
    return out


# ---------------------------------------------------------------- tests
@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(CASES))
def test_blob_stage_case_alone(cpe, orc, gpu, name):
    img = _image(name)
    res = _run(cpe, gpu, img[None])
    _check(img, _frame(res, 0), name)


@pytest.mark.gpu
def test_blob_stage_scenes_at_every_shape(cpe, orc, gpu):
    """64 x 64, 67 x 130, 203 x 200, 481 x 641, 1200 x 1920: widths that are and are not multiples of 16 and 64, heights
    that are not multiples of 8"""
    for h, w, seed in SCENES:
        imgs = np.stack([gen_scene(h, w, seed), gen_scene(h, w, seed + 100)])
        res = _run(cpe, gpu, imgs)
        for i in range(2):
            _check(imgs[i], _frame(res, i), (h, w, seed, i))


@pytest.mark.gpu
@pytest.mark.parametrize('shape', sorted({s for _, s in CASES.values()}))
def test_blob_stage_mixed_batch_equals_alone(cpe, orc, gpu, shape):
    """all cases of one frame size (and a random scene) in one batch, in reversed order as well: identical to each alone"""
    names = [k for k, (_, s) in CASES.items() if s == shape]
    imgs = [_image(k) for k in names] + [gen_scene(shape[0], shape[1], 77)]
    tags = names + ['scene']
    batch = _run(cpe, gpu, np.stack(imgs))
    rev = _run(cpe, gpu, np.stack(imgs[::-1]))
    for i, img in enumerate(imgs):
        alone = _frame(_run(cpe, gpu, img[None]), 0)
        _same(_frame(batch, i), alone, (tags[i], 'batch'))
        _same(_frame(rev, len(imgs) - 1 - i), alone, (tags[i], 'reversed batch'))
        _check(img, alone, tags[i])


@pytest.mark.gpu
@pytest.mark.parametrize('replay', [1, 2, 3])
def test_blob_stage_merge_paths_agree(cpe, orc, gpu, monkeypatch, replay):
    """CPE_MERGE_REPLAY: bit 0 sends every batch of k_blob_merge through the in-order replay, bit 1 ranks every threshold
    by key buckets: the key points must not change"""
    names = ['lattice', 'cluster33', 'long_hole', 'exact_distances', 'half_centroids', 'median_paths', 'equal_unions', 'nested']
    base = {k: _frame(_run(cpe, gpu, _image(k)[None]), 0) for k in names}
    monkeypatch.setenv('CPE_MERGE_REPLAY', str(replay))
    for k in names:
        got = _frame(_run(cpe, gpu, _image(k)[None]), 0)
        _same(got, base[k], (k, replay))
        _check(_image(k), got, (k, replay))


@pytest.mark.gpu
def test_blob_stage_group_capacity_is_reported(cpe, orc, gpu):
    """more than GCAP = 48 centres in one group: OVF_GROUPS in the state, and status 6 from detect_grid_batch -- never a
    silently different key-point list"""
    for per in (3, 4):
        img = gen_cluster(per=per)
        ref = _oracle(img)
        res = _run(cpe, gpu, img[None])
        _check(img, _frame(res, 0), ('cluster', per), allow_group_overflow=True)
        assert ref['nk'] >= 1
    # the same cluster after LAB-L and CLAHE (dark holes stay < 50, the field stays at 255)
    img = gen_cluster(per=4)
    det = cpe.api.detect_grid_batch(torch.from_numpy(img[None]).to(gpu))
    torch.cuda.synchronize()
    assert det['ws'].state()[0]['overflow'] & OVF_GROUPS
    assert int(det['status'][0]) == 6


@pytest.mark.gpu
def test_blob_stage_matches_detect_path(cpe, orc, gpu):
    """the entry applied to the detect path's own CLAHE plane gives the detect path's n_kp, rect and mask_contour"""
    from cpe_amd import synth
    b = synth.render_batch(2, 480, 640, seed=3, with_gt=False)
    frames = torch.cat([b['left'], b['right']])[:3].contiguous()
    det = cpe.api.detect_grid_batch(frames.to(gpu))
    torch.cuda.synchronize()
    cl = det['ws'].plane('clahe').cpu().numpy().copy()
    mc = det['ws'].plane('mask_contour').cpu().numpy().copy()
    sd = det['ws'].state()
    res = _run(cpe, gpu, cl)
    for i in range(3):
        g = _frame(res, i)
        st = g['state']
        assert st['n_kp'] == sd[i]['n_kp'] and int(g['nkp']) == sd[i]['n_kp'], i
        assert all(st[k] == sd[i][k] for k in ('rect0', 'rect1', 'rect2', 'rect3')), i
        assert np.array_equal(g['mc'], mc[i]), i
        _check(cl[i], g, ('rendered', i))


def test_blob_stage_cases_reach_their_paths(orc):
    """CPU: the generators put what they claim in front of the kernels (checked with the oracle's contours)"""
    from oracle import stages as S
    cov = _coverage(_image('median_paths'))
    lens = {n for n, hole in cov if hole}
    assert {MED_FAST - 1, MED_FAST, MED_FAST + 1} <= lens, sorted(x for x in lens if 480 < x < 510)
    assert any(n > SEL_CAP and not hole for n, hole in cov), 'a bright blob with more than SEL_CAP border points'
    assert any(n > MED_FAST for n, hole in _coverage(_image('area_limits')) if hole)
    kp, stats = S.simple_blob_detector(_image('crowd'))
    assert stats.max() > 4096
    kp, stats = S.simple_blob_detector(_image('lattice'))
    assert len(kp) > 1024
    # area limits: pixel count < 5000 but polygon area >= 5000 (rejected by the area test), and pixel count >= 5000
    img = _image('area_limits')
    split = [0, 0, 0]
    for pts, hole in S.find_contours(img > 50, 'list', 'none'):
        if hole:
            a = S.contour_moments(pts)[0]
            split[0] += a >= 5000
            split[1] += 4700 <= a < 5000
    assert split[0] >= 3 and split[1] >= 3, split
    # rings enclosing around 5000 hole pixels: some rejected, the small ones accepted
    kp, stats = S.simple_blob_detector(_image('bright_rings'))
    assert stats.max() >= 1
