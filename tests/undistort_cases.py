"""Cases and second statements for row f-3 in cv2 mode (csrc/undistort.hip: k_undistort_map, k_remap_bilinear4/1) and for
k_remap_cubic on its own.  No GPU, no torch: tests/test_undistort_cases_cpu.py checks that the cases reach what they claim
to reach, tests/test_undistort_limits_gpu.py runs the kernels on them.

  cameras x sizes      every entry of the stripe's inverse matrix non-zero (`general`), maps that leave the source on every
                       side, source coordinates beyond int16 (`wrap`) and beyond int32 / 32 (`saturate`), 0 / 4 / 5 / 8 / 12
                       coefficients; one row per stripe, w > 4096, stripe > h, h on both sides of the 64-row block, the
                       longest running sum and the largest y0
  closed_form          the map in numpy f64 without running sums, stripes included
  remap_bilinear_np    orc_remap_bilinear stated a second time, in int64
  crafted_bilinear     maps that hold every border class of remap_one, the int16 extremes and all 1024 fractions
  crafted_cubic        test_prestep_gpu.camera's f32 map with NaN, inf, -0.0, 1e30 and the edge values in its first entries
  frames               u8 noise, one all-255 and one all-0 frame"""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle  # noqa: E402
import test_prestep_gpu as P  # noqa: E402     (helpers only: no torch at import)

NMAX = 17
FRAME_255, FRAME_0 = 3, 5           # frames(h, w)[3] is all 255, [5] all 0: both are in every call with n >= 8


# ---------------------------------------------------------------- cameras and sizes
def K(h, w, skew=0.0, k3=0.0, k6=0.0, k7=0.0):
    return np.array([0.8 * w + 3, skew, w / 2 + 1.3, k3, 0.81 * w + 3, h / 2 + 0.9, k6, k7, 1.0]).reshape(3, 3)


CAMERAS = dict(                       # name -> (arguments of K, coefficients in OpenCV order)
    none=(dict(), []),
    pincushion4=(dict(skew=0.3), [0.21, 0.05, -0.0011, 0.0009]),
    barrel5=(dict(), [-0.23, 0.09, 0.0013, -0.0008, -0.015]),
    rational8=(dict(skew=0.3), [0.4, -0.1, 0.001, -0.002, 0.05, 0.2, 0.03, 0.01]),
    prism12=(dict(skew=-0.2), [0.1, 0.02, 0.001, -0.002, 0.01, 0.05, 0, 0, 0.01, -0.02, 0.015, 0.005]),
    general=(dict(skew=0.3, k3=0.05, k6=1e-5, k7=-2e-5), [0.21, 0.05, -0.0011, 0.0009, 0.01]),
    wrap=(dict(), [0, 0, 0, 0, 3e4]),               # source coordinates beyond +-32768 px: the int16 of the map wraps
    saturate=(dict(), [0, 0, 0, 0, 1e10]),          # u * 32 beyond +-2^31: sat_int clamps
)

SIZES = [(1, 1), (7, 5), (29, 37), (65, 130), (130, 1000), (33, 4095), (5, 4096), (5, 4097), (3, 5000), (1, 32767), (32767, 1)]


def camera(name, h, w):
    """-> (K 3x3 f64, dist f64[n])"""
    kargs, dist = CAMERAS[name]
    return K(h, w, **kargs), np.array(dist, dtype=np.float64)


def stripe_rows(h, w):
    """rows per stripe of cv2.undistort: 4096 / cols, at least 1, at most rows"""
    return min(max(4096 // max(w, 1), 1), h)


@functools.lru_cache(maxsize=None)
def oracle_map(name, h, w):
    """(map_xy i16 [h,w,2], map_f u16 [h,w]) of oracle.undistort_map; read-only, shared"""
    oracle.build()
    mxy, mf = oracle.undistort_map(*camera(name, h, w), h, w)
    mxy.setflags(write=False); mf.setflags(write=False)
    return mxy, mf


# ---------------------------------------------------------------- the map in closed form
def stripe_inverse(Km, y0):
    """inverse of the new camera matrix of the stripe that starts at row y0 (principal point shifted by y0)"""
    Ar = np.array(Km, dtype=np.float64)
    Ar[1, 2] -= y0
    return np.linalg.inv(Ar)


def closed_form(Km, dist, h, w, stripe=None):
    """source coordinates (u, v) f64 [h,w] of every output pixel: per stripe the inverse matrix applied to (j, row - y0, 1)
    directly (no running sums), then the distortion model as OpenCV documents it, in powers of r^2 (no Horner form).
    `stripe`: rows per stripe, if not cv2.undistort's (to show what the stripes do to a map)"""
    c = np.zeros(12)
    c[:len(dist)] = dist
    k1, k2, p1, p2, k3, k4, k5, k6, s1, s2, s3, s4 = c
    s0 = stripe or stripe_rows(h, w)
    j = np.arange(w, dtype=np.float64)[None, :]
    u = np.empty((h, w)); v = np.empty((h, w))
    for y0 in range(0, h, s0):
        y1 = min(y0 + s0, h)
        ir = stripe_inverse(Km, y0)
        i = np.arange(0, y1 - y0, dtype=np.float64)[:, None]
        X = ir[0, 0] * j + ir[0, 1] * i + ir[0, 2]
        Y = ir[1, 0] * j + ir[1, 1] * i + ir[1, 2]
        W = ir[2, 0] * j + ir[2, 1] * i + ir[2, 2]
        x, y = X / W, Y / W
        r2 = x * x + y * y
        r4, r6 = r2 ** 2, r2 ** 3
        kr = (1 + k1 * r2 + k2 * r4 + k3 * r6) / (1 + k4 * r2 + k5 * r4 + k6 * r6)
        xd = x * kr + 2 * p1 * x * y + p2 * (r2 + 2 * x * x) + s1 * r2 + s2 * r4
        yd = y * kr + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y + s3 * r2 + s4 * r4
        u[y0:y1] = Km[0, 0] * xd + Km[0, 2]
        v[y0:y1] = Km[1, 1] * yd + Km[1, 2]
    return u, v


def to_fixed(u):
    """rint(u * 32), clamped to int32 -> int64"""
    return np.clip(np.rint(u * 32), -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)


def map_fixed(mxy, mf):
    """the map's (u, v) as fixed point int16 * 32 + fraction -> int64"""
    return (mxy[..., 0].astype(np.int64) * 32 + (mf & 31).astype(np.int64),
            mxy[..., 1].astype(np.int64) * 32 + (mf >> 5).astype(np.int64))


def diff21(a, b):
    """a - b modulo 2^21 as a signed number: the int16 wrap of the map's integer part drops out"""
    d = (a - b) & ((1 << 21) - 1)
    return np.where(d >= (1 << 20), d - (1 << 21), d)


# ---------------------------------------------------------------- remap, bilinear: second statement and crafted maps
def remap_bilinear_np(src, mxy, mf):
    """remap(INTER_LINEAR, BORDER_CONSTANT 0) of one u8 frame in int64: weights (32-fx)(32-fy)*32 ..., (sum + 2^14) >> 15"""
    h, w = src.shape
    sx, sy = mxy[..., 0].astype(np.int64), mxy[..., 1].astype(np.int64)
    fx, fy = (mf & 31).astype(np.int64), ((mf >> 5) & 31).astype(np.int64)
    s = src.astype(np.int64)

    def tap(y, x):
        inside = (x >= 0) & (x < w) & (y >= 0) & (y < h)
        return np.where(inside, s[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)], 0)

    tot = (tap(sy, sx) * ((32 - fx) * (32 - fy) * 32) + tap(sy, sx + 1) * (fx * (32 - fy) * 32)
           + tap(sy + 1, sx) * ((32 - fx) * fy * 32) + tap(sy + 1, sx + 1) * (fx * fy * 32))
    return np.clip((tot + (1 << 14)) >> 15, 0, 255).astype(np.uint8)


BILINEAR_SIZES = [(1, 1), (1, 4), (2, 2), (3, 5), (29, 37), (30, 38), (40, 52), (48, 64)]
EXTREMES = [(a, b) for a in (-32768, 0, 32767) for b in (-32768, 0, 32767) if (a, b) != (0, 0)]


def axis_class(s, size):
    """border class of an integer source coordinate along one axis, by which of its two neighbours s, s + 1 are inside:
    0: s < -1 (none), 1: s = -1 (the second), 2: both, 3: s = size - 1 (the first), 4: s >= size (none).
    On an axis of size 1 class 2 does not exist (s = 0 is class 3)."""
    s = np.asarray(s, dtype=np.int64)
    return np.select([s < -1, s == -1, s >= size, s == size - 1], [0, 1, 4, 3], 2)


def reachable_classes(size):
    return [0, 1, 3, 4] if size == 1 else [0, 1, 2, 3, 4]


def border_classes(mxy, h, w):
    """-> (class along x, class along y) of every entry"""
    return axis_class(mxy[..., 0], w), axis_class(mxy[..., 1], h)


def _draw(rng, cls, size):
    return {0: lambda: rng.integers(-3, -1), 1: lambda: -1, 2: lambda: rng.integers(0, size - 1), 3: lambda: size - 1,
            4: lambda: rng.integers(size, size + 3)}[cls]()


@functools.lru_cache(maxsize=None)
def crafted_bilinear(h, w):
    """-> (map_xy i16 [M,h,w,2], map_f u16 [M,h,w]); read-only, shared.  M maps, as many as the size needs to hold, in this order
    of entries: the eight extreme pairs of {-32768, 0, 32767}, then every reachable pair of border classes twice (sx in
    [-3, w + 2], sy in [-3, h + 2]), then uniform draws from those ranges.  Fractions < 1024: all 1024 of them where M*h*w
    allows, random ones otherwise."""
    rng = np.random.default_rng([h, w, 3])
    pairs = [(cx, cy) for cy in reachable_classes(h) for cx in reachable_classes(w)]
    N = h * w
    M = max(1, -(-(len(EXTREMES) + len(pairs)) // N))
    T = M * N
    xy = np.stack([rng.integers(-3, w + 3, T), rng.integers(-3, h + 3, T)], -1)
    xy[:len(EXTREMES)] = EXTREMES
    for k in range(min(2 * len(pairs), T - len(EXTREMES))):
        cx, cy = pairs[k % len(pairs)]
        xy[len(EXTREMES) + k] = (_draw(rng, cx, w), _draw(rng, cy, h))
    f = rng.permutation(T) % 1024 if T >= 1024 else rng.integers(0, 1024, T)
    mxy = np.ascontiguousarray(xy.astype(np.int16).reshape(M, h, w, 2))
    mf = np.ascontiguousarray(f.astype(np.uint16).reshape(M, h, w))
    mxy.setflags(write=False); mf.setflags(write=False)
    return mxy, mf


def identity_bilinear(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.ascontiguousarray(np.stack([xx, yy], -1).astype(np.int16)), np.zeros((h, w), np.uint16)


# ---------------------------------------------------------------- remap, cubic: crafted maps
def cubic_specials(h, w):
    """f32 (x, y) entries that a camera's map does not hold, each with what k_remap_cubic must give for it: 'fill', or the
    (row, column) of the source pixel it returns unchanged, or None (an ordinary inside entry)"""
    f = np.float32
    up, down = np.nextafter(f(w - 1), f(np.inf)), np.nextafter(f(0), f(-1))
    return [((np.nan, 1), 'fill'), ((1, np.nan), 'fill'), ((np.inf, 1), 'fill'), ((1, -np.inf), 'fill'),
            ((-0.0, -0.0), (0, 0)), ((1e30, 1), 'fill'), ((1, -1e30), 'fill'), ((w - 1, h - 1), (h - 1, w - 1)),
            ((up, 1), 'fill'), ((1, down), 'fill'), ((0.5, 0), None), ((-np.inf, 1), 'fill'), ((1, np.inf), 'fill'),
            ((down, 1), 'fill'), ((1, np.nextafter(f(h - 1), f(np.inf))), 'fill'), ((np.nan, np.nan), 'fill'),
            ((-1e30, 1), 'fill'), ((1, 1e30), 'fill'), ((w - 1, 0), (0, w - 1)), ((0, h - 1), (h - 1, 0))]


def crafted_cubic_specials(h, w):
    """the specials that a map of this size holds: all 20 from 100 pixels up, below that the first 11 (the rest would leave a
    5x7 map without an interior entry), and at 3x3 the 9 that fit"""
    return cubic_specials(h, w)[:20 if h * w >= 100 else min(11, h * w)]


@functools.lru_cache(maxsize=None)
def crafted_cubic(h, w):
    """test_prestep_gpu.camera's map f32 [h,w,2] with crafted_cubic_specials in its first entries; read-only, shared"""
    m = np.array(P.oracle_map(h, w))
    sp = crafted_cubic_specials(h, w)
    m.reshape(-1, 2)[:len(sp)] = np.array([s[0] for s in sp], dtype=np.float32)
    m.setflags(write=False)
    return m


def cubic_classes(m):
    """test_prestep_gpu.classes; the integer casts of its NaN and inf entries are masked by `inside`, so their values do not matter"""
    with np.errstate(invalid='ignore'):
        return P.classes(m)


# ---------------------------------------------------------------- frames
@functools.lru_cache(maxsize=None)
def frames(h, w):
    """u8 [NMAX,h,w]: noise (the hardest input for an interpolator's rounding), frame 3 all 255, frame 5 all 0; read-only, shared"""
    a = np.random.default_rng([h, w, 11]).integers(0, 256, (NMAX, h, w), dtype=np.uint8)
    a[FRAME_255] = 255
    a[FRAME_0] = 0
    a.setflags(write=False)
    return a
