"""The cases of tests/undistort_cases.py do what they claim (no GPU: references only).

The oracle (oracle/src/orc_undistort.c, OpenCV's running sums) and the closed form (numpy f64, inverse matrix applied per
pixel) are two statements of one map.  They may differ by the last fixed-point step where u * 32 falls next to a rounding
boundary; how often is a property of the CASES (a camera whose two statements drift apart tests nothing), so it is capped here:
at most 1 unit, in at most 0.2 % of the entries of any case.  Everything else in this file is exact."""
import functools

import numpy as np
import pytest

import oracle
import undistort_cases as U

SHARE_CAP = 0.002
CASES = [(name, h, w) for name in U.CAMERAS for (h, w) in U.SIZES]


@functools.lru_cache(maxsize=None)
def compare(name, h, w):
    """-> (largest difference in fixed-point units, share of unequal u entries, share of unequal v entries)"""
    oracle.build()
    Km, dist = U.camera(name, h, w)
    u, v = U.closed_form(Km, dist, h, w)
    assert np.isfinite(u).all() and np.isfinite(v).all(), 'the oracle defines no value for a NaN: no case may hold one'
    mxy, mf = U.oracle_map(name, h, w)
    assert (mf < 1024).all()
    ou, ov = U.map_fixed(mxy, mf)
    du, dv = U.diff21(ou, U.to_fixed(u)), U.diff21(ov, U.to_fixed(v))
    return max(int(np.abs(du).max()), int(np.abs(dv).max())), float((du != 0).mean()), float((dv != 0).mean())


@pytest.mark.parametrize('name,h,w', CASES)
def test_oracle_map_is_close_to_closed_form(name, h, w):
    worst, su, sv = compare(name, h, w)
    print(f'{name} {h}x{w}: largest difference {worst}, unequal u {100 * su:.4f} %, v {100 * sv:.4f} %')
    assert worst <= 1
    assert max(su, sv) <= SHARE_CAP


def test_largest_share_of_unequal_entries():
    """the figure for the commit message: asserted, and printed with -s"""
    s = {c: max(compare(*c)[1:]) for c in CASES}
    c = max(s, key=s.get)
    print(f'largest share of entries where oracle and closed form differ: {100 * s[c]:.3f} % ({c[0]}, {c[1]}x{c[2]}); {len(s)} cases')
    assert len(s) == 88 and s[c] <= SHARE_CAP


# ---------------------------------------------------------------- reach
def outside(name, h, w):
    """which sides of the source the closed-form map leaves: entries whose bilinear footprint has a neighbour outside"""
    u, v = U.closed_form(*U.camera(name, h, w), h, w)
    return dict(left=(u < 0).any(), right=(u > w - 1).any(), top=(v < 0).any(), bottom=(v > h - 1).any())


def test_general_camera_fills_the_inverse_matrix():
    for (h, w) in U.SIZES:
        ir = U.stripe_inverse(U.camera('general', h, w)[0], 0).ravel()
        assert all(ir[k] != 0 for k in (1, 3, 6, 7)), (h, w)
    for name in U.CAMERAS:
        if name != 'general':
            Km = U.camera(name, 65, 130)[0]
            assert Km[1, 0] == 0 and Km[2, 0] == 0 and Km[2, 1] == 0


def test_general_map_depends_on_the_stripes():
    """with a bottom row other than 0 0 1 the stripes are part of the model: the same camera with one stripe for the whole frame
    has another fixed-point map, at the sizes where a stripe is one row as well"""
    for (h, w) in ((130, 1000), (5, 4097), (3, 5000)):
        Km, dist = U.camera('general', h, w)
        assert U.stripe_rows(h, w) < h
        (u, v), (u1, v1) = U.closed_form(Km, dist, h, w), U.closed_form(Km, dist, h, w, stripe=h)
        n = np.count_nonzero(U.to_fixed(u) != U.to_fixed(u1)) + np.count_nonzero(U.to_fixed(v) != U.to_fixed(v1))
        assert np.array_equal(u[:U.stripe_rows(h, w)], u1[:U.stripe_rows(h, w)]) and n > 0, (h, w)
        print(f'general {h}x{w}: {n} fixed-point values depend on the stripes')


def test_maps_leave_the_source_where_claimed():
    for name in ('pincushion4', 'rational8', 'general'):
        assert all(outside(name, 65, 130).values()), name
    assert not any(outside('barrel5', 130, 1000).values())


def test_wrap_and_saturate_reach_their_casts(orc):
    for (h, w) in ((29, 37), (65, 130), (5, 4096)):
        u, v = U.closed_form(*U.camera('wrap', h, w), h, w)
        assert (np.abs(u) >= 32768).any()
        assert (np.abs(u * 32) < 2.0 ** 31).all() and (np.abs(v * 32) < 2.0 ** 31).all()
    h, w = 29, 37
    u, v = U.closed_form(*U.camera('saturate', h, w), h, w)
    for t in (u, v):
        assert (t * 32 >= 2.0 ** 31).any() and (t * 32 <= -2.0 ** 31).any()
    # a saturated value is 0x7FFFFFFF or 0x80000000: integer part -1 or 0 after the int16 cast, fraction 31 or 0
    mxy, mf = U.oracle_map('saturate', h, w)
    for t, part, frac in ((u, mxy[..., 0], mf & 31), (v, mxy[..., 1], mf >> 5)):
        hi, lo = t * 32 >= 2.0 ** 31, t * 32 <= -2.0 ** 31
        assert (part[hi] == -1).all() and (frac[hi] == 31).all() and (part[lo] == 0).all() and (frac[lo] == 0).all()


def test_sizes_reach_every_stripe_rule():
    s = {(h, w): U.stripe_rows(h, w) for (h, w) in U.SIZES}
    assert s[(7, 5)] == 7 and 4096 // 5 > 7                      # stripe0 > h
    assert s[(33, 4095)] == 1 and s[(5, 4096)] == 1              # one row per stripe, by division
    assert s[(5, 4097)] == 1 and 4096 // 4097 == 0 and s[(3, 5000)] == 1        # the clamp from 0
    assert s[(65, 130)] == 31 and 65 % 31 != 0                   # last stripe partial, h one past a 64-thread block
    assert s[(130, 1000)] == 4 and s[(32767, 1)] == 4096 and s[(1, 32767)] == 1
    assert (29 * 37) % 2 == 1
    assert sorted({len(d) for _, d in U.CAMERAS.values()}) == [0, 4, 5, 8, 12]


# ---------------------------------------------------------------- crafted bilinear maps and the two remap statements
@pytest.mark.parametrize('h,w', U.BILINEAR_SIZES)
def test_crafted_bilinear_maps_hold_every_class(h, w):
    mxy, mf = U.crafted_bilinear(h, w)
    assert mxy.shape[1:] == (h, w, 2) and mf.shape == mxy.shape[:3] and (mf < 1024).all()
    cx, cy = U.border_classes(mxy, h, w)
    seen = set(zip(cx.ravel().tolist(), cy.ravel().tolist()))
    want = {(a, b) for a in U.reachable_classes(w) for b in U.reachable_classes(h)}
    assert want <= seen, sorted(want - seen)
    flat = mxy.reshape(-1, 2)
    assert [tuple(p) for p in flat[:8].tolist()] == U.EXTREMES
    assert flat[8:].min() >= -3 and flat[8:, 0].max() <= w + 2 and flat[8:, 1].max() <= h + 2
    if mf.size >= 1024:
        assert np.array_equal(np.unique(mf), np.arange(1024))
    # the classes are the masks of remap_one: which of the neighbours s, s + 1 lie inside
    for c, s, size in ((cx, mxy[..., 0].astype(np.int64), w), (cy, mxy[..., 1].astype(np.int64), h)):
        in0, in1 = (s >= 0) & (s < size), (s + 1 >= 0) & (s + 1 < size)
        assert np.array_equal(np.isin(c, (2, 3)), in0) and np.array_equal(np.isin(c, (1, 2)), in1)
        assert np.array_equal(c == 0, s < -1) and np.array_equal(c == 4, s >= size)


@pytest.mark.parametrize('h,w', U.BILINEAR_SIZES)
def test_oracle_bilinear_equals_integer_statement(orc, h, w):
    mxy, mf = U.crafted_bilinear(h, w)
    fr = U.frames(h, w)
    for k in range(len(mxy)):
        for f in (0, 1, U.FRAME_255, U.FRAME_0):
            assert np.array_equal(orc.remap_bilinear(fr[f], mxy[k], mf[k]), U.remap_bilinear_np(fr[f], mxy[k], mf[k])), (k, f)
    ixy, izf = U.identity_bilinear(h, w)
    assert np.array_equal(orc.remap_bilinear(fr[0], ixy, izf), fr[0]) and np.array_equal(U.remap_bilinear_np(fr[0], ixy, izf), fr[0])


@pytest.mark.parametrize('name', ['pincushion4', 'general', 'wrap', 'saturate'])
def test_oracle_bilinear_equals_integer_statement_on_camera_maps(orc, name):
    for (h, w) in ((29, 37), (65, 130)):
        mxy, mf = U.oracle_map(name, h, w)
        fr = U.frames(h, w)
        assert np.array_equal(orc.remap_bilinear(fr[0], mxy, mf), U.remap_bilinear_np(fr[0], mxy, mf))


def test_bilinear_weights_sum_to_2_15():
    f = np.arange(1024)
    fx, fy = f & 31, f >> 5
    tot = (32 - fx) * (32 - fy) * 32 + fx * (32 - fy) * 32 + (32 - fx) * fy * 32 + fx * fy * 32
    assert (tot == 1 << 15).all()
    # so a constant frame comes back unchanged wherever all four neighbours are inside, at every fraction
    mxy = np.zeros((32, 32, 2), np.int16)
    assert (U.remap_bilinear_np(np.full((32, 32), 255, np.uint8), mxy, f.astype(np.uint16).reshape(32, 32)) == 255).all()


# ---------------------------------------------------------------- crafted cubic maps
@pytest.mark.parametrize('h,w', [(3, 3), (5, 7), (29, 37)])
def test_crafted_cubic_maps(orc, h, w):
    m = U.crafted_cubic(h, w)
    sp = U.crafted_cubic_specials(h, w)
    flat = m.reshape(-1, 2)
    assert len(sp) == {(3, 3): 9, (5, 7): 11, (29, 37): 20}[(h, w)]
    c = U.cubic_classes(m)
    if (h, w) != (3, 3):
        for k, v in c.items():
            assert v.any(), f'{h}x{w}: no {k} pixel'
    # every entry that is not finite, or beyond the image, is `outside` by the comparisons alone: the oracle (and the kernel)
    # convert it to an integer only behind that test, so nothing undefined is evaluated
    bad = ~np.isfinite(flat).all(1) | (flat[:, 0] < 0) | (flat[:, 1] < 0) | (flat[:, 0] > np.float32(w - 1)) | (flat[:, 1] > np.float32(h - 1))
    assert np.array_equal(bad, c['outside'].ravel())
    assert np.isnan(flat[:len(sp)]).any() and np.isinf(flat[:len(sp)]).any() and np.signbit(flat[4]).all() and (flat[4] == 0).all()
    fr = U.frames(h, w)
    for fill in (0, 201):
        for f in (0, U.FRAME_255):
            out = orc.remap_cubic(fr[f], m, fill).ravel()
            assert (out[bad] == fill).all()
            for k, (xy, want) in enumerate(sp):
                if want == 'fill':
                    assert bad[k] and out[k] == fill, (k, xy)
                elif want is not None:
                    assert not bad[k] and out[k] == fr[f][want], (k, xy)
                else:
                    assert not bad[k]
