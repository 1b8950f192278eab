"""The bucket scatter of the blob sweep (k_bk_pass, csrc/region.hip) through cpe_debug_blob_region with the identity CLAHE
table: the pixels of the working rectangle sorted by grey-level bucket, and everything downstream of it (blobs and key
points against the oracle, tolerance 0).

A thread of the kernel owns four consecutive frame indices (one dword of the image) in each of its rounds, a workgroup 8192
of them; the bright forest's first nodes link runs of one bucket inside aligned chunks of 64 indices.  The frames put the
rectangle's edges, runs and the workgroup boundary where those units break: an odd left edge inside a 64-index chunk, runs
across a 64-index boundary and across the frame's row end (rectangle = frame), an 8192-index boundary inside a rectangle
row, a pixel count that is no multiple of 8192 (and, at 203 x 330, none of 4: every second frame starts unaligned), every
bucket 1 .. 17 in use, a frame that is all rectangle and one with no rectangle at all."""
import numpy as np
import pytest
import torch

from test_blob_stage_gpu import NTHR, _check

SHAPES = ((250, 320), (200, 336), (203, 330))
BK_CHUNK = 8192        # csrc/region.hip: frame indices per workgroup of k_bk_pass
SW_BS, SW_BO = 76, 94  # csrc/region.hip: bucket sizes / first entries in the sweep record (CPE_PLANE_SWEEP)
CPE_ST_NO_REGION = 1
assert sum(1 for _, w in SHAPES if w % 64) >= 2


def _level(img):
    """csrc/cpe_dev.h sweep_level: 0: v <= 50, b: 50 + 10 (b - 1) < v <= 50 + 10 b, 17: v > 210"""
    v = img.astype(np.int32)
    return np.where(v <= 50, 0, np.minimum((v - 41) // 10, 17))


def _pattern(h, w, seed):
    """blocks of 23 x 9 pixels of the 17 buckets' grey levels with dark 5 x 5 holes, and a band of per-pixel random levels"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = (55 + 10 * ((xx // 23 + 3 * (yy // 9)) % 17)).astype(np.uint8)
    img[(yy % 27 >= 11) & (yy % 27 < 16) & (xx % 46 >= 30) & (xx % 46 < 35)] = 20
    band = slice(h // 2, h // 2 + 12)
    img[band] = rng.integers(40, 256, size=img[band].shape, dtype=np.uint8)
    return img


def frame_window(h, w):
    """the pattern inside x 37 .. w - 22, y 21 .. h - 30 (odd left edge, inside a 64-index chunk), dark outside"""
    img = np.zeros((h, w), np.uint8)
    img[21:h - 29, 37:w - 21] = _pattern(h, w, 1)[21:h - 29, 37:w - 21]
    return img


def frame_full(h, w):
    """every pixel above the lowest threshold; rows end and begin in one bucket (a run across the row end)"""
    img = np.maximum(_pattern(h, w, 2), 51)                   # (the holes are dark from threshold 60 on)
    img[:, :6] = 215
    img[:, w - 6:] = 215
    return img


def frame_empty(h, w):
    return np.random.default_rng(3).integers(0, 51, size=(h, w), dtype=np.uint8)


FRAMES = (frame_window, frame_full, frame_empty)
_IMGS = {}


def _images(shape):
    if shape not in _IMGS:
        _IMGS[shape] = np.stack([fn(*shape) for fn in FRAMES])
    return _IMGS[shape]


def _bbox(img):
    ys, xs = np.nonzero(img > 50)
    return (int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())) if len(ys) else None


_COVERED = set()


def _assert_coverage(shape):
    """CPU: the frames hold the cases the module names (a missing one fails the test)"""
    if shape in _COVERED:
        return
    from oracle import stages as S
    h, w = shape
    win, full, empty = _images(shape)
    assert (h * w) % BK_CHUNK != 0
    x0, y0, x1, y1 = _bbox(win)
    lv = _level(win)
    assert x0 % 2 == 1 and x0 > 0
    assert any((y * w + x0) % 64 not in (0, 63) for y in range(y0, y1 + 1)), 'left edge inside a 64-index chunk'
    idx = np.arange(h * w).reshape(h, w)
    same = (lv[:, 1:] == lv[:, :-1]) & (lv[:, 1:] > 0)
    assert (same & (idx[:, 1:] % 64 == 0)).any(), 'a run of one bucket across a 64-index boundary'
    inner = (idx % BK_CHUNK == 0) & (lv > 0)
    inner[:, :x0 + 1] = False
    assert inner[y0:y1 + 1].any(), 'a workgroup boundary inside a row of the rectangle'
    assert set(np.unique(lv)) >= set(range(1, NTHR + 1)), 'every bucket in use'
    assert _bbox(full) == (0, 0, w - 1, h - 1) and (full > 50).all()
    lf = _level(full)
    wrap = [y for y in range(1, h) if lf[y, 0] == lf[y - 1, w - 1] and (y * w) % 64 != 0]
    # (at a width that is a multiple of 64 every row starts a chunk: the other two widths hold this case)
    assert wrap or w % 64 == 0, "a run across the rectangle's left edge (the row end of a frame that is all rectangle)"
    assert _bbox(empty) is None and S.largest_blob_from_sweep(empty)[0] == CPE_ST_NO_REGION
    _COVERED.add(shape)


@pytest.mark.parametrize('shape', SHAPES)
def test_bucket_frames_hold_their_cases(orc, shape):
    _assert_coverage(shape)


@pytest.mark.gpu
@pytest.mark.parametrize('shape', SHAPES)
def test_bucket_lists_and_blobs(cpe, orc, gpu, shape):
    from cpe_amd import api
    _assert_coverage(shape)
    imgs = _images(shape)
    n, h, w = imgs.shape
    kp_cap, blob_cap = 4096, 16384
    ws = api.DetectWorkspace(n, h, w, gpu)
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
    nkp_h, nbl_h = nkp.cpu().numpy(), nbl.cpu().numpy()
    assert (nkp_h <= kp_cap).all() and (nbl_h <= blob_cap).all()
    kp_h, bl_h = kp.cpu().numpy(), bl.cpu().numpy()
    state, sweep = ws.state(), ws.plane('sweep').cpu().numpy()
    mc, clahe = ws.plane('mask_contour').cpu().numpy(), ws.plane('clahe').cpu().numpy()
    off, per = api.workspace_row(n, h, w, 'bucket_pixels')       # not overlaid: the lists survive the call
    assert per == h * w * 4
    lists = ws.view[off:off + n * per].view(torch.int32).reshape(n, h * w).cpu().numpy()
    for i in range(n):
        tag = (shape, FRAMES[i].__name__)
        lv = _level(imgs[i]).reshape(-1)
        if FRAMES[i] is frame_empty:
            assert state[i]['status'] == CPE_ST_NO_REGION and nkp_h[i] == 0, tag
            assert not sweep[i][SW_BS + 1:SW_BS + NTHR + 1].any(), tag
        else:
            sizes = np.bincount(lv, minlength=NTHR + 1)
            assert list(sweep[i][SW_BS + 1:SW_BS + NTHR + 1]) == list(sizes[1:]), (tag, 'bucket sizes')
            assert list(sweep[i][SW_BO + 1:SW_BO + NTHR + 1]) == list(np.cumsum(sizes[1:]) - sizes[1:]), (tag, 'bucket offsets')
            for b in range(1, NTHR + 1):
                o = int(sweep[i][SW_BO + b])
                got = np.sort(lists[i, o:o + sizes[b]])
                assert np.array_equal(got, np.flatnonzero(lv == b)), (tag, 'entries of bucket', b)
        g = dict(kp=kp_h[i, :nkp_h[i]], blobs=[bl_h[i, k, :nbl_h[i, k]] for k in range(NTHR)], nkp=nkp_h[i], nblobs=nbl_h[i],
                 state=state[i], mc=mc[i], sweep=sweep[i], clahe=clahe[i])
        _check(imgs[i], g, tag)
