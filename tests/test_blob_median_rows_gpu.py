"""The radii of the blob stage (k_blob_median, csrc/region.hip) at every border length at which the kernel takes another
path, through cpe_debug_blob_region with the identity CLAHE table, against the oracle with tolerance 0.

A hole border of up to 128 stored points is handled by a quarter wavefront (16 lanes, 8 points each, four borders at a
time), one of 129 .. 496 points by a whole wavefront with ceil(n / 64) point slots, a longer one by the chain walk, and a
bright component by the distance scratch.  The frames hold dark filled squares, rectangles, diamonds and discs on a bright
ground, with one-pixel grey ramps at their edges, so every shape is a hole of a different size at several thresholds:
a rectangle of a x b pixels has a hole border of 2 (a + b) points, one point less with a corner pixel cut off, and eight
more for every ring of the ramp that has turned dark.  The CPU test checks with the oracle's contours that the lengths
named in LENGTHS are really there."""
import numpy as np
import pytest

from test_blob_stage_gpu import NTHR, _canvas, _check, _frame, _run

MED_Q = 128            # csrc/region.hip: stored borders up to this many points take a quarter wavefront
MED_FAST = 496         # csrc/region.hip: ... up to this many a whole wavefront without the chain walk
CH_PTS = 31            # csrc/region.hip: border points per chunk of the pool
# accepted hole borders that must be present over all frames and thresholds
LENGTHS = (CH_PTS, CH_PTS + 1, CH_PTS + 2, 63, 64, 65, MED_Q - 1, MED_Q, MED_Q + 1, MED_FAST - 1, MED_FAST, MED_FAST + 1)


def _rect(img, y, x, a, b, rings=0, cut=False):
    """dark a x b rectangle at (y, x) with `rings` one-pixel rings around it of 55, 65, ...: ring i is dark from threshold
    50 + 10 i on.  cut: the top-left pixel of the outermost ring (of the rectangle itself without rings) stays bright"""
    for i in range(rings, 0, -1):
        img[y - i:y + a + i, x - i:x + b + i] = 45 + 10 * i
    img[y:y + a, x:x + b] = 0
    if cut:
        img[y - rings, x - rings] = 255


def _radial(img, cy, cx, r, norm, rings=3):
    """dark disc (norm 2) or diamond (norm 1) of radius r with `rings` one-pixel ramps of 55, 65, ... around it"""
    h, w = img.shape
    yy, xx = np.mgrid[0:h, 0:w]
    d = np.hypot(yy - cy, xx - cx) if norm == 2 else (np.abs(yy - cy) + np.abs(xx - cx)).astype(np.float64)
    for i in range(rings, 0, -1):
        img[d <= r + i] = 45 + 10 * i
    img[d <= r] = 0


def frame_short(h, w):
    """borders below 16 and around 32 and 64 points, both parities; squares (tied distances), a diamond and a disc"""
    img = _canvas(h, w)
    _rect(img, 12, 12, 3, 3)                       # 12 points
    _rect(img, 12, 24, 3, 4, cut=True)             # 13
    _rect(img, 12, 40, 6, 10)                      # 32
    _rect(img, 12, 60, 6, 10, cut=True)            # 31
    _rect(img, 12, 80, 7, 10, cut=True)            # 33
    _rect(img, 30, 14, 12, 20, rings=2)            # 64, 72, 80
    _rect(img, 30, 50, 12, 20, cut=True)           # 63
    _rect(img, 30, 80, 13, 20, cut=True)           # 65
    _rect(img, 60, 14, 16, 16, rings=3)            # squares: 64 .. 88
    _rect(img, 60, 50, 15, 15, rings=3, cut=True)
    _rect(img, 60, 90, 30, 30, rings=2)            # 120, 128, 136
    _radial(img, 120, 30, 12, 1)
    _radial(img, 120, 80, 14, 2)
    _radial(img, 120, 130, 9, 2, rings=5)
    for k in range(9):                             # a row of small squares: many quarter-wavefront borders at one threshold
        _rect(img, 150, 12 + 14 * k, 4 + k % 3, 4 + k % 2, rings=1)
    return img


def frame_group_limit(h, w):
    """127, 128 and 129 points (the quarter wavefront's limit) and the slot counts of the whole wavefront (129 .. 496)"""
    img = _canvas(h, w)
    _rect(img, 12, 12, 24, 40)                     # 128
    _rect(img, 12, 60, 24, 40, cut=True)           # 127
    _rect(img, 12, 110, 25, 40, cut=True)          # 129
    _rect(img, 12, 160, 22, 38, rings=4)           # 120, 128, 136, 144, 152
    _rect(img, 50, 14, 30, 60, rings=2)            # 180, 188, 196 (3 .. 4 slots)
    _rect(img, 50, 90, 40, 80, rings=2, cut=True)  # 239 ..: 4 slots
    _rect(img, 50, 190, 44, 100, rings=1)          # 288, 296: 5 slots
    _rect(img, 110, 14, 24, 150, rings=2)          # 348 ..: 6 slots
    _rect(img, 110, 180, 20, 120, rings=1)         # 280, 288
    _radial(img, 165, 40, 20, 2)
    _radial(img, 165, 100, 22, 1)
    _rect(img, 150, 140, 14, 14, rings=3)
    return img


def frame_long(h, w):
    """thin long rectangles around 496 points and beyond beside short borders (one threshold mixes all classes), and a bright
    ring with a dark centre in a dark box (a bright blob: its radius comes from the distance scratch)"""
    img = _canvas(h, w)
    _rect(img, 12, 14, 20, 228)                    # 496
    _rect(img, 38, 14, 20, 228, cut=True)          # 495
    _rect(img, 64, 14, 20, 229, cut=True)          # 497
    _rect(img, 90, 14, 10, 260, rings=1)           # 540, 548: the chain walk
    _rect(img, 106, 14, 18, 200, rings=2)          # 436, 444, 452: 7 slots
    for k in range(12):
        _rect(img, 132, 14 + 18 * k, 5 + k % 4, 6 + k % 3, rings=1, cut=bool(k & 1))
    img[150:190, 240:300] = 0                      # the dark box ...
    img[158:182, 252:288] = 200                    # ... the bright ring ...
    img[164:176, 260:280] = 0                      # ... and its dark centre
    _rect(img, 152, 20, 30, 30, rings=2)           # a square beside them
    return img


FRAMES = (frame_short, frame_group_limit, frame_long)
SHAPES = ((256, 320), (200, 330))                  # 200 rows: not a multiple of 16

_IMGS = {}


def _images(shape):
    if shape not in _IMGS:
        _IMGS[shape] = np.stack([fn(*shape) for fn in FRAMES])
    return _IMGS[shape]


def _accepted(img):
    """per threshold: (border length, is_hole, squared centre distances tie at the middle ranks) of the accepted blobs"""
    from oracle import stages as S
    out = []
    for k in range(NTHR):
        b = img > 50 + 10 * k
        cur = []
        for pts, is_hole in S.find_contours(b, 'list', 'none'):
            m00, m10, m01 = S.contour_moments(pts)
            if not 10 <= m00 < 5000:
                continue
            cx, cy = m10 / m00, m01 / m00
            if b[int(np.rint(cy)), int(np.rint(cx))]:
                continue
            p = np.asarray(pts, np.float64).reshape(-1, 2)
            d = np.sort((cx - p[:, 0]) ** 2 + (cy - p[:, 1]) ** 2)
            n = len(d)
            lo, hi = d[(n - 1) // 2], d[n // 2]
            tied = (d == lo).sum() > 1 and (d == hi).sum() > 1
            cur.append((n, bool(is_hole), bool(tied)))
        out.append(cur)
    return out


_COVERED = set()


def _assert_coverage(shape):
    """the oracle's contours of the frames contain every length the GPU test is about (a missing one fails the test)"""
    if shape in _COVERED:
        return
    per_frame = [_accepted(img) for img in _images(shape)]
    holes = [n for fr in per_frame for thr in fr for n, hole, _ in thr if hole]
    lens = set(holes)
    assert min(lens) < 16, sorted(lens)[:4]
    assert set(LENGTHS) <= lens, sorted(set(LENGTHS) - lens)
    assert any(MED_Q + 1 < n < MED_FAST - 1 for n in lens) and any(n > MED_FAST + 1 for n in lens)
    assert {(n + 63) // 64 for n in lens if MED_Q < n <= MED_FAST} >= {3, 4, 5, 6, 7, 8}, 'every slot count of the whole wavefront'
    assert any(n % 2 for n in holes if n <= MED_Q) and any(n % 2 == 0 for n in holes if n <= MED_Q)
    assert any(tied for fr in per_frame for thr in fr for n, hole, tied in thr if hole and n <= MED_Q), 'both middle ranks on ties'
    # one threshold of one frame mixes quarter-wavefront, whole-wavefront and chain-walk borders
    assert any(min(c) <= MED_Q and any(MED_Q < n <= MED_FAST for n in c) and max(c) > MED_FAST
               for fr in per_frame for thr in fr for c in [[n for n, hole, _ in thr if hole]] if c)
    assert any(not hole for fr in per_frame for thr in fr for n, hole, _ in thr), 'a bright blob (distance scratch)'
    _COVERED.add(shape)


@pytest.mark.parametrize('shape', SHAPES)
def test_median_frames_hold_every_border_class(orc, shape):
    """CPU: the generators put what they claim in front of the kernel"""
    _assert_coverage(shape)


@pytest.mark.gpu
@pytest.mark.parametrize('shape', SHAPES)
def test_median_radii_match_oracle(cpe, orc, gpu, shape):
    """three frames per call: blobs (x, y, r) per threshold and the key points, tolerance 0"""
    _assert_coverage(shape)
    imgs = _images(shape)
    res = _run(cpe, gpu, imgs)
    for i in range(len(imgs)):
        _check(imgs[i], _frame(res, i), (shape, FRAMES[i].__name__))
