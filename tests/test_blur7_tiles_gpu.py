"""The 7 x 7 blur of the masks stage (k_blur_fused<3>, csrc/masks.hip) through cpe_debug_masks against oracle.stages.blur7,
tolerance 0, on frames whose rows are and are not 4-byte aligned and with region rectangles at every frame edge and corner
and at the tile boundaries (tiles of 64 x 32 pixels).

The kernel blurs the tiles within half + 1 pixels of the region rectangle (half follows from r0, the radius of the saturated
spot) and leaves the others untouched; tiles whose window lies inside the frame on 4-byte aligned rows are loaded as dwords,
the others byte by byte with the reflected border.  The grey plane is seeded random bytes with one saturated disc (the masks
stage needs a spot to go on to the blur); one frame is all 255."""
import numpy as np
import pytest
import torch

import masks_cases as M

SHAPES = ((480, 640), (483, 650), (600, 801))
CPE_ST_NO_REGION = 1


def _rects(h, w):
    """(x, y, w, h): at the four corners, along the four edges, at tile boundaries +- 1, on tile boundaries, the frame"""
    return [(0, 0, 40, 30), (w - 40, 0, 40, 30), (0, h - 30, 40, 30), (w - 40, h - 30, 40, 30),
            (200, 0, 50, 20), (200, h - 20, 50, 20), (0, 200, 20, 50), (w - 20, 200, 20, 50),
            (63, 31, 66, 34), (65, 33, 62, 30), (127, 95, 130, 66), (128, 64, 64, 32), (0, 0, w, h)]


_CASES = {}


def _cases(shape):
    """one frame per rectangle, one all-255 frame and one frame without a region"""
    if shape in _CASES:
        return _CASES[shape]
    h, w = shape
    rng = np.random.default_rng(h * 1000 + w)
    out = []
    rects = _rects(h, w)
    for k, rect in enumerate(rects):
        g = rng.integers(0, 256, size=(h, w), dtype=np.uint8)
        M.disc(g, 300 + 20 * (k % 5), 240 + 10 * (k % 7), 12 + k % 4)
        out.append(M.case(np.zeros((h, w), np.uint8), gray=g, rect=rect))
    out.append(M.case(np.zeros((h, w), np.uint8), gray=np.full((h, w), 255, np.uint8), rect=(100, 100, 200, 150)))
    g = rng.integers(0, 256, size=(h, w), dtype=np.uint8)
    M.disc(g, 320, 240, 12)
    out.append(M.case(np.zeros((h, w), np.uint8), gray=g, rect=(0, 0, w, h), status=CPE_ST_NO_REGION))
    _CASES[shape] = out
    return out


def _grown(h, w, rect, r0):
    """the rectangle grown by half + 1 (half as k_blur_fused derives it from r0), clipped to the frame: slices (rows, cols)"""
    half = int(r0 / 5.0)
    half = 3 if half < 3 else (half + 5 if half > 10 else half)
    m = max(half, int(r0 / 4.5)) + 1
    x, y, rw, rh = rect
    return slice(max(y - m, 0), min(y + rh + m, h)), slice(max(x - m, 0), min(x + rw + m, w))


_COVERED = {}


def _assert_coverage(shape):
    """CPU, oracle alone: every frame but the last reaches the blur (status 0), and the rectangles are where they claim"""
    if shape in _COVERED:
        return _COVERED[shape]
    from oracle import stages as S
    h, w = shape
    cases = _cases(shape)
    refs = []
    for c in cases[:-1]:
        st, _, _, r0, _ = S.mask_roi_around_center(np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8), c['mc'], c['gray'], False)
        assert st == 0, ('the masks stage must reach the blur', c['rect'], st)
        refs.append((r0, S.blur7(c['gray'])))
    assert cases[-1]['status'] == CPE_ST_NO_REGION
    assert (cases[-2]['gray'] == 255).all()
    rs = [c['rect'] for c in cases]
    assert any(x == 0 and y == 0 for x, y, _, _ in rs) and any(x + rw == w and y + rh == h for x, y, rw, rh in rs)
    assert any(x + rw == w and y == 0 for x, y, rw, rh in rs) and any(x == 0 and y + rh == h for x, y, rw, rh in rs)
    assert any(x % 64 == 63 and y % 32 == 31 for x, y, _, _ in rs) and any(x % 64 == 1 and y % 32 == 1 for x, y, _, _ in rs)
    assert any(x % 64 == 0 and y % 32 == 0 and (x + rw) % 64 == 0 and (y + rh) % 32 == 0 and x > 0 for x, y, rw, rh in rs)
    assert (0, 0, w, h) in rs
    _COVERED[shape] = refs
    return refs


@pytest.mark.parametrize('shape', SHAPES)
def test_blur7_cases_reach_the_blur(orc, shape):
    _assert_coverage(shape)


@pytest.mark.gpu
@pytest.mark.parametrize('shape', SHAPES)
def test_blur7_equals_oracle_around_rect(cpe, orc, gpu, shape):
    h, w = shape
    refs = _assert_coverage(shape)
    cases = _cases(shape)
    st = lambda k: torch.from_numpy(np.stack([c[k] for c in cases])).to(gpu)
    rect = torch.tensor([c['rect'] for c in cases], dtype=torch.int32)
    status = torch.tensor([c['status'] for c in cases], dtype=torch.int32)
    ws = cpe.api.debug_masks(st('binary'), st('gray'), st('mc'), rect, status)
    torch.cuda.synchronize()
    blur = ws.plane('blur7').cpu().numpy()
    state = ws.state()
    assert state[-1]['status'] == CPE_ST_NO_REGION
    for i, c in enumerate(cases[:-1]):
        r0_ref, b7 = refs[i]
        assert state[i]['status'] == 0 and state[i]['r0'] == r0_ref, (i, c['rect'], state[i]['status'], state[i]['r0'], r0_ref)
        rows, cols = _grown(h, w, c['rect'], state[i]['r0'])
        bad = blur[i][rows, cols] != b7[rows, cols]
        assert not bad.any(), (shape, c['rect'], int(bad.sum()), np.argwhere(bad)[:4].tolist())
