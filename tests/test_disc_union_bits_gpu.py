"""The disc union of the region stage drawn straight into its one-bit plane (region.hip: k_disc_keypoints, k_disc_bands), through
cpe_debug_blob_region with an identity CLAHE table, against the oracle with tolerance 0.

mask_contour, rect, status and the key-point count are compared with oracle.stages.largest_blob_from_sweep.  mask_contour is the
filled hull of the union's largest component only, so the union itself is compared as well: the plane the stage leaves in the
workspace (row `bits`, one plane per frame) is decoded with the tiled layout tests/test_bitplane_layout_cpu.py restates and
set against cv2.circle (oracle.stages.circle_fill) of the oracle's key points.  Widths that are not a multiple of 16 keep the
byte image; one such case runs beside the others.

Every image is a few dots (a bright square with a dark core: one key point at its centre) placed so that the disc
  - is cut by one of the four frame borders, or by two in a corner;
  - has rows on both sides of a border between two 64-row bands;
  - overlaps a disc of the next band;
  - ends in the last, partial 64-pixel word of the row (w = 80) or in the last whole one (w = 320);
  - lies in the last band of a frame whose height is not a multiple of 8;
and one frame of every batch holds no group at all (status 1)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bitplane_util import decode_plane, plane_words, workspace_row  # noqa: E402

BAND = 64              # csrc/region.hip: DB_R


def dot(img, y, x, half=3, core=1):
    """a bright square with a dark core, clipped to the frame: one persistent blob -> one key point at (x, y)"""
    h, w = img.shape
    img[max(y - half, 0):min(y + half + 1, h), max(x - half, 0):min(x + half + 1, w)] = 210
    img[max(y - core, 0):min(y + core + 1, h), max(x - core, 0):min(x + core + 1, w)] = 30
    return img


def _img(h, w, dots):
    img = np.zeros((h, w), np.uint8)
    for y, x in dots:
        dot(img, y, x)
    return img


# name -> (h, w, dots (y, x), what the discs must do: a list of (property, index of the dot))
CASES = {
    'top_80':      (64, 80, [(4, 40)], [('top', 0)]),
    'bottom_80':   (64, 80, [(59, 30)], [('bottom', 0)]),
    'left_80':     (64, 80, [(30, 4)], [('left', 0)]),
    'right_80':    (64, 80, [(30, 75)], [('right', 0), ('last_word', 0)]),
    'corner_80':   (64, 80, [(4, 75), (59, 4)], [('top', 0), ('right', 0), ('bottom', 1), ('left', 1)]),
    'partial_80':  (64, 80, [(30, 66)], [('last_word', 0), ('spans_words', 0)]),
    'h70_80':      (70, 80, [(65, 40), (30, 70)], [('straddle', 0), ('bottom', 0), ('last_word', 1)]),
    'straddle':    (130, 320, [(63, 100)], [('straddle', 0)]),
    'two_bands':   (130, 320, [(58, 200), (69, 202)], [('overlap', 0), ('bands_differ', 0)]),
    'last_band':   (130, 320, [(125, 60)], [('straddle', 0), ('bottom', 0)]),
    'right_320':   (130, 320, [(90, 315)], [('right', 0), ('last_word', 0)]),
    'many':        (250, 320, [(y, x) for y in range(4, 250, 30) for x in range(4, 320, 26)],
                    [('top', 0), ('left', 0), ('bottom', 116), ('right', 116), ('straddle', 26)]),
    'word_edges':  (250, 320, [(40, 64), (128, 128), (192, 191), (127, 256), (245, 315)],
                    [('spans_words', 0), ('straddle', 1), ('straddle', 2), ('straddle', 3), ('bottom', 4), ('right', 4)]),
    'bytes_83':    (70, 83, [(65, 40), (30, 78), (4, 4)], [('bottom', 0), ('right', 1), ('top', 2), ('left', 2)]),     # w % 16 != 0: the byte image
}
EMPTY = {(64, 80): np.zeros((64, 80), np.uint8), (70, 80): np.full((70, 80), 40, np.uint8), (130, 320): np.zeros((130, 320), np.uint8),
         (250, 320): np.full((250, 320), 45, np.uint8), (70, 83): np.zeros((70, 83), np.uint8)}


def case_image(name):
    h, w, dots, _ = CASES[name]
    return _img(h, w, dots)


def disc_params(kp):
    """(cx, cy, er) of a key point (x, y, size) f32, as k_discs / k_disc_keypoints compute them"""
    radius = np.float32(kp[2]) / np.float32(2)
    return int(kp[0]), int(kp[1]), int(float(radius) + 4)


_ORACLE = {}


def oracle_of(img):
    """-> dict(kp, status, mask, rect, nk, union): the union is cv2.circle of every key point"""
    from oracle import stages as S
    key = (img.shape, img.tobytes())
    if key not in _ORACLE:
        kp, _ = S.simple_blob_detector(img)
        st, mask, rect, nk = S.largest_blob_from_sweep(img)
        union = np.zeros_like(img)
        for k in kp:
            cx, cy, er = disc_params(k)
            S.circle_fill(union, cx, cy, er, 255)
        _ORACLE[key] = dict(kp=kp, status=st, mask=mask, rect=rect, nk=nk, union=union)
    return _ORACLE[key]


def _run(cpe, gpu, imgs):
    from cpe_amd import api
    imgs = np.ascontiguousarray(imgs)
    n, h, w = imgs.shape
    ws = api.DetectWorkspace(n, h, w, gpu)
    d = torch.from_numpy(imgs).to(gpu)
    cap = 1024
    kp = torch.zeros((n, cap, 3), dtype=torch.float32, device=gpu)
    nkp = torch.zeros(n, dtype=torch.int32, device=gpu)
    bl = torch.zeros((n, 17, 64, 3), dtype=torch.float64, device=gpu)
    nbl = torch.zeros((n, 17), dtype=torch.int32, device=gpu)
    L = cpe.lib.load()
    cpe.lib.check(L.cpe_debug_blob_region(d.data_ptr(), n, h, w, ws.view.data_ptr(), ws.bytes, kp.data_ptr(), cap, nkp.data_ptr(),
                                          bl.data_ptr(), 64, nbl.data_ptr(), torch.cuda.current_stream().cuda_stream),
                  'cpe_debug_blob_region')
    torch.cuda.synchronize()
    off, _ = workspace_row(L, n, h, w, 'bits')
    pw = plane_words(h, w)
    planes = ws.view[off:off + n * pw * 8].cpu().numpy().view('<u8').reshape(n, pw)     # plane f of the run: frame f's disc union
    return dict(state=ws.state(), mc=ws.plane('mask_contour').cpu().numpy(), nkp=nkp.cpu().numpy(), planes=planes)


def _check(img, res, i, tag):
    ref = oracle_of(img)
    st = res['state'][i]
    h, w = img.shape
    assert st['overflow'] == 0, tag
    assert st['n_kp'] == int(res['nkp'][i]) == ref['nk'] == len(ref['kp']), (tag, st['n_kp'], ref['nk'])
    union, clean = decode_plane(res['planes'][i], h, w)
    assert clean, (tag, 'bits at columns >= w, rows >= h or in the zero tile columns')
    assert np.array_equal(union, ref['union'] != 0), (tag, 'disc union', int((union != (ref['union'] != 0)).sum()))
    assert st['status'] == ref['status'], (tag, st['status'], ref['status'])
    assert np.array_equal(res['mc'][i], ref['mask']), (tag, 'mask_contour', int((res['mc'][i] != ref['mask']).sum()))
    if ref['status'] == 0:
        assert (st['rect0'], st['rect1'], st['rect2'], st['rect3']) == ref['rect'], (tag, 'rect')


SHAPES = sorted({(h, w) for h, w, _, _ in CASES.values()})


@pytest.mark.gpu
@pytest.mark.parametrize('shape', SHAPES)
def test_disc_union_plane_and_region_match_oracle(cpe, orc, gpu, shape):
    """all cases of one frame size and a frame without any group in one batch, the empty frame in the middle"""
    names = [k for k, v in CASES.items() if (v[0], v[1]) == shape]
    imgs = [case_image(k) for k in names]
    imgs.insert(len(imgs) // 2, EMPTY[shape]); names.insert(len(names) // 2, 'empty')
    res = _run(cpe, gpu, np.stack(imgs))
    for i, img in enumerate(imgs):
        _check(img, res, i, (shape, names[i]))
    k = names.index('empty')
    assert res['state'][k]['status'] == 1 and res['state'][k]['n_kp'] == 0 and not res['mc'][k].any() and not res['planes'][k].any()
    assert sum(s['status'] == 0 for s in res['state']) == len(imgs) - 1


def test_disc_union_cases_do_what_they_claim(orc):
    """CPU, the oracle alone: every dot gives one key point at its centre, and the discs touch what the case names"""
    for name, (h, w, dots, props) in CASES.items():
        ref = oracle_of(case_image(name))
        discs = {(cy, cx): er for cx, cy, er in (disc_params(k) for k in ref['kp'])}
        assert sorted(discs) == sorted(dots), (name, sorted(discs), sorted(dots))
        assert ref['status'] == 0, name
        for what, idx in props:
            cy, cx = dots[idx]
            er = discs[(cy, cx)]
            ok = {'top': cy - er < 0, 'bottom': cy + er >= h, 'left': cx - er < 0, 'right': cx + er >= w,
                  'last_word': (min(cx + er, w - 1) >> 6) == ((w - 1) >> 6),
                  'spans_words': (max(cx - er, 0) >> 6) != (min(cx + er, w - 1) >> 6),
                  'straddle': max(cy - er, 0) // BAND != min(cy + er, h - 1) // BAND}
            if what in ok:
                assert ok[what], (name, what, idx, (cy, cx, er))
            elif what == 'bands_differ':
                (ya, xa), (yb, xb) = dots[idx], dots[idx + 1]
                assert ya // BAND != yb // BAND, name
            elif what == 'overlap':
                (ya, xa), (yb, xb) = dots[idx], dots[idx + 1]
                one = np.zeros((h, w), np.uint8); two = np.zeros((h, w), np.uint8)
                from oracle import stages as S
                S.circle_fill(one, xa, ya, discs[(ya, xa)], 255); S.circle_fill(two, xb, yb, discs[(yb, xb)], 255)
                assert (one & two).any() and (one & ~two).any() and (two & ~one).any(), name
            else:
                raise KeyError(what)
    for shape, img in EMPTY.items():
        ref = oracle_of(img)
        assert ref['status'] == 1 and ref['nk'] == 0, shape
    assert any(h % 8 for h, _, _, _ in CASES.values()) and {80, 320} <= {w for _, w, _, _ in CASES.values()}
