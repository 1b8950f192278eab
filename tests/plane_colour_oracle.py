"""Helpers of the planar-target colour tests (test_plane_colour_cpu.py, test_plane_colour_gpu.py): tinted test frames and the
oracle composition of python_grid_detection_plane.detect_grid on a true-colour frame.

The oracle has no colour entry for the planar script, so `detect_grid_plane_bgr` restates orc_detect_grid_plane
(oracle/src/orc_plane.c) step by step from the oracle's exported stages, with the two colour looks of the reference swapped in:
    get_convex_hull(original_img, 5)   (util_plane.py:2590-2689): threshold 127 per channel, BGR2GRAY of the 0/255 image ->
                                       S.get_convex_hull of 255 * (max(B, G, R) > 127)
    indexing_data's gauss7             (util_plane.py:1334-1336): 7x7 blur per channel, then BGR2GRAY -> S.blur7 x 3, S.bgr2gray
Every other step reads S.bgr2gray(bgr).  On grey-replicated frames the composition is S.detect_grid_plane of the grey plane
(checked in test_plane_colour_cpu.py), which pins the restatement to the oracle's own chain."""
import ctypes as C

import numpy as np

from cpe_amd.fit import MAXP as CPE_MAXP        # include/cpe.h

CPE_MAXJ = 16384                                # include/cpe.h


def plane_frames(h, w, n, seed):
    """the planar synthetic frames of tests/test_plane_gpu.py (left views, then right views), u8 [2n,h,w] numpy"""
    import torch
    from cpe_amd import synth
    sc = synth.Scene(h=h, w=w, radius=5000.0, depth=(5340.0, 5400.0), tilt_deg=4.0)
    b = synth.render_batch(n, h, w, seed=seed, scene=sc, with_gt=False)
    return torch.cat([b['left'], b['right']]).numpy()


def tint(g, rng):
    """a colour camera's view of a red laser grid, as tests/test_boundary_gpu.py::test_true_colour_frames makes it: R strong,
    G and B weak, each channel with its own noise, and the saturated spot blooming white on every channel"""
    r = g.astype(np.int32)
    bgr = np.stack([r * 0.18 + rng.integers(0, 6, g.shape), r * 0.35 + rng.integers(0, 6, g.shape), r + rng.integers(-2, 3, g.shape)], 2)
    bgr[g >= 245] = g[g >= 245][:, None]
    return np.clip(bgr, 0, 255).astype(np.uint8)


def red_laser(g, rng):
    """a red-only laser: R carries the grid (up to 255), G and B stay at or below 10; the saturated spot is white"""
    r = g.astype(np.int32)
    bgr = np.stack([rng.integers(0, 6, g.shape) + r // 64, rng.integers(0, 6, g.shape) + r // 64, r + rng.integers(-2, 3, g.shape)], 2)
    bgr[g >= 245] = 255
    return np.clip(bgr, 0, 255).astype(np.uint8)


def any_channel_mask(bgr):
    """cv2.cvtColor(cv2.threshold(img, 127, 255, THRESH_BINARY)[1], BGR2GRAY) as a 0/255 mask: non-zero where any channel > 127"""
    return (255 * (np.asarray(bgr).max(2) > 127)).astype(np.uint8)


def colour_hull(bgr):
    from oracle import stages as S
    return S.get_convex_hull(any_channel_mask(bgr), 127, 5)


def colour_gauss7(bgr):
    from oracle import stages as S
    bgr = np.asarray(bgr)
    return S.bgr2gray(np.stack([S.blur7(np.ascontiguousarray(bgr[..., c])) for c in range(3)], 2))


def detect_grid_plane_bgr(bgr, cap=2 * CPE_MAXP):
    """orc_detect_grid_plane on a colour frame (see the module docstring) -> dict(status, center, xy, id, rect, r0, mask_contour,
    gauss7, n_rows, n_cols).  cap: rows of the scratch table, more than CPE_MAXP so that a frame beyond the capacity is seen"""
    import oracle
    from oracle import stages as S
    lib = S.lib()
    bgr = np.ascontiguousarray(bgr, np.uint8)
    h, w, _ = bgr.shape
    gray = S.bgr2gray(bgr)
    _, binary = oracle.preprocess(gray)
    hm, vm, cent = S.extract_joints(binary)
    st, mc, rect = colour_hull(bgr)
    out = dict(status=st, center=np.zeros(2), xy=np.zeros((0, 2)), id=np.zeros((0, 2), np.int32), rect=rect, r0=0,
               mask_contour=mc, gauss7=None, n_rows=0, n_cols=0)
    if st != 0:
        return out
    x0, y0, rw, rh = rect
    cyl = np.array([(x, y) for x, y in cent if x0 <= x < x0 + rw and y0 <= y < y0 + rh], np.int32).reshape(-1, 2)
    assert len(cyl) <= CPE_MAXJ, 'joint table capacity: not restated here (orc_detect_grid_plane reports status 6)'
    roi_h = np.zeros_like(gray); roi_v = np.zeros_like(gray); r0 = C.c_int(0); spot = (C.c_int * 4)()
    u8 = C.POINTER(C.c_uint8)
    ptr = lambda a: a.ctypes.data_as(u8)
    st = lib.orc_mask_roi_around_center_ex(ptr(hm), ptr(vm), ptr(mc), ptr(gray), h, w, ptr(roi_h), ptr(roi_v), C.byref(r0), spot, 1)
    out.update(status=st, r0=r0.value)
    if st != 0:
        return out
    exp_h = np.zeros_like(gray); exp_v = np.zeros_like(gray)
    lib.orc_expand_line_roi_ex(ptr(roi_h), ptr(mc), h, w, 201, 8, 700, ptr(exp_h), None)
    lib.orc_expand_line_roi_ex(ptr(roi_v), ptr(mc), h, w, 201, 8, 700, ptr(exp_v), None)
    cw, ch = min(rw, w - x0), min(rh, h - y0)
    _, lab_h = S.connected_components(exp_h[y0:y0 + ch, x0:x0 + cw])
    _, lab_v = S.connected_components(exp_v[y0:y0 + ch, x0:x0 + cw])
    rows = S.group_points(cyl, lab_h, x0, y0)
    cols = S.group_points(cyl, lab_v, x0, y0)
    S.fit_lines_plane(rows, cols)
    S.intersections_plane(rows, cols, rect)
    S.clean_plane(rows, cols)
    g7 = colour_gauss7(bgr)
    center = np.zeros(2); xy = np.zeros((cap, 2)); ids = np.zeros((cap, 2), np.int32)
    n = lib.orc_index_points_plane(C.byref(rows), C.byref(cols), ptr(g7), h, w, r0.value, center.ctypes.data_as(C.POINTER(C.c_double)),
                                   xy.ctypes.data_as(C.POINTER(C.c_double)), ids.ctypes.data_as(C.POINTER(C.c_int)), cap)
    out.update(gauss7=g7, n_rows=rows.nlines, n_cols=cols.nlines)
    assert n <= CPE_MAXP, 'grid point capacity: not restated here'
    if n < 0:
        st = -n
    else:
        out.update(center=center, xy=xy[:n].copy(), id=ids[:n].copy())
    out['status'] = st
    return out


def blur7_written(h, w, rect, r0):
    """bool [h,w]: the pixels the 7x7 blur of the detect call writes for a frame with status 0 -- the 64 x 32 tiles that are not
    skipped because they lie farther than the largest indexing window (+1) from the region rectangle (csrc/masks.hip k_blur7_bgr)"""
    half = int(r0 / 5.0)
    half = 3 if half < 3 else (half + 5 if half > 10 else half)
    m = max(half, int(r0 / 4.5)) + 1
    x0, y0, rw, rh = rect
    out = np.zeros((h, w), bool)
    for gy0 in range(0, h, 32):
        for gx0 in range(0, w, 64):
            if gx0 > x0 + rw + m or gx0 + 64 < x0 - m or gy0 > y0 + rh + m or gy0 + 32 < y0 - m:
                continue
            out[gy0:gy0 + 32, gx0:gx0 + 64] = True
    return out
