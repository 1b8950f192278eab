"""k_open20_joints and k_roi_base (csrc/masks.hip) at the edges of their decomposition, through cpe_debug_masks, tolerance 0.

The kernels march 16-pixel lanes down bands of rows inside strips of 960 columns (tests/bitrow_cases.py states the
decomposition and makes the inputs; tests/test_bitrow_generators_cpu.py shows that each input reaches its edge).  Per frame:
  - hmask / vmask against stages.extract_joints and the scipy restatement of the 20-tap openings;
  - roi_h / roi_v against stages.mask_roi_around_center and a scipy 3x3 opening of mask & spot & mask_contour;
  - exp_h / exp_v against stages.expand_line_roi (the seed base & mask_contour and what the expansion adds);
  - the one-bit planes themselves, decoded from the workspace: the joints mask, hmask and vmask where rows are a multiple
    of 16 pixels, and the base of both fragment masks against close3x3(roi); zero in the guard tile columns, at columns
    >= w and at rows >= h."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bitrow_cases as B  # noqa: E402
import masks_cases as M  # noqa: E402
import workspace_poison as P  # noqa: E402
from bitplane_util import decode_plane, plane_words  # noqa: E402
from masks_cases import scipy_open20, scipy_open3, spot_mask  # noqa: E402

PLANES = ('hmask', 'vmask', 'roi_h', 'roi_v', 'exp_h', 'exp_v')
BITS = ('jbits', 'hbits', 'vbits', 'base_h', 'base_v')


def _run(cpe, gpu, cases, ws=None):
    """cpe_debug_masks on cases of one frame size -> per-frame dicts: the byte planes, the state, and the one-bit planes as
    (bool [h, w], clean)"""
    st = lambda k: torch.from_numpy(np.stack([c[k] for c in cases])).to(gpu)
    rect = torch.tensor([c['rect'] for c in cases], dtype=torch.int32)
    status = torch.tensor([c['status'] for c in cases], dtype=torch.int32)
    ws = cpe.api.debug_masks(st('binary'), st('gray'), st('mc'), rect, status, ws=ws)
    torch.cuda.synchronize()
    n = len(cases)
    h, w = cases[0]['binary'].shape
    planes = {k: ws.plane(k).cpu().numpy() for k in PLANES}
    state = ws.state()
    pw = plane_words(h, w)

    def words(row, count):
        off, _ = cpe.api.workspace_row(n, h, w, row)
        return ws.view[off:off + count * pw * 8].cpu().numpy().view('<u8').reshape(count, pw)
    jb, lm, bb = words('joint_bits', n), words('joints_mask', 2 * n) if w % 16 == 0 else None, words('bits', 2 * n)
    out = []
    for i in range(n):
        d = {k: planes[k][i] for k in PLANES}
        d['state'] = state[i]
        d['jbits'] = decode_plane(jb[i], h, w)
        d['hbits'] = decode_plane(lm[i], h, w) if lm is not None else None
        d['vbits'] = decode_plane(lm[n + i], h, w) if lm is not None else None
        d['base_h'], d['base_v'] = decode_plane(bb[i], h, w), decode_plane(bb[n + i], h, w)
        out.append(d)
    return out


def _same(a, b, tag):
    for k in PLANES:
        assert np.array_equal(a[k], b[k]), (tag, k)
    for k in BITS:
        if a[k] is not None:
            assert a[k][1] and b[k][1] and np.array_equal(a[k][0], b[k][0]), (tag, k)
    for k in ('status', 'r0', 'n_joints', 'n_joints_all', 'n_seg0', 'n_seg1', 'overflow'):
        assert a['state'][k] == b['state'][k], (tag, k)


_REF = {}


def _oracle(key, c):
    if key not in _REF:
        _REF[key] = M.oracle(c)
    return _REF[key]


def _check(c, g, ref, tag, expansion=True):
    """one frame against the oracle; c: the case as the kernels must read it (mask_contour zero outside rect)"""
    from oracle import stages as S
    st = g['state']
    for k, horizontal in (('hmask', True), ('vmask', False)):
        assert np.array_equal(g[k], ref[k]), (tag, k, int((g[k] != ref[k]).sum()))
        assert np.array_equal(g[k], scipy_open20(c['binary'], horizontal)), (tag, k, 'scipy')
    bits, clean = g['jbits']
    assert clean, (tag, 'jbits: bits outside the image')
    assert np.array_equal(bits, (ref['hmask'] & ref['vmask']) != 0), (tag, 'jbits')
    for k, m in (('hbits', 'hmask'), ('vbits', 'vmask')):
        if g[k] is not None:
            assert g[k][1], (tag, k, 'bits outside the image')
            assert np.array_equal(g[k][0], ref[m] != 0), (tag, k)
    assert st['overflow'] == 0 and st['status'] == ref['status'], (tag, 'status', st['status'], ref['status'], st['overflow'])
    if ref['status'] == 1:              # no region: zeros everywhere
        for k in ('roi_h', 'roi_v', 'exp_h', 'exp_v'):
            assert not g[k].any(), (tag, k)
        for k in ('base_h', 'base_v'):
            assert g[k][1] and not g[k][0].any(), (tag, k)
        return
    if ref['status'] != 0:
        return
    cm = spot_mask(c, ref['spot'], False)
    for key, m in (('h', ref['hmask']), ('v', ref['vmask'])):
        roi = g['roi_' + key]
        assert np.array_equal(roi, ref['roi_' + key]), (tag, 'roi_' + key, int((roi != ref['roi_' + key]).sum()))
        assert np.array_equal(roi, scipy_open3(m & cm & c['mc'])), (tag, 'roi_' + key, 'scipy')
        bits, clean = g['base_' + key]
        assert clean, (tag, 'base_' + key, 'bits outside the image')
        want = S.close_rect(ref['roi_' + key], 3, 3) != 0
        assert np.array_equal(bits, want), (tag, 'base_' + key, int((bits != want).sum()))
        if expansion:
            assert np.array_equal(g['exp_' + key], ref['exp_' + key]), (tag, 'exp_' + key, int((g['exp_' + key] != ref['exp_' + key]).sum()))


def _one(cpe, gpu, key, c):
    g = _run(cpe, gpu, [c, dict(c, status=1)])
    _check(c, g[0], _oracle(key, c), key)
    _check(dict(c, status=1), g[1], M.oracle(dict(c, status=1)), (key, 'no region'))
    return g[0]


@pytest.mark.gpu
def test_horizontal_runs_and_gaps_at_lane_word_and_strip_edges(cpe, orc, gpu):
    _one(cpe, gpu, 'runs_h', B.get('runs_h', B.gen_runs_h))


@pytest.mark.gpu
@pytest.mark.parametrize('h', B.HEIGHTS)
def test_vertical_runs_and_gaps_at_band_edges(cpe, orc, gpu, h):
    """heights one below, at and one above a band of either kernel, and the lowest frame the entry takes (64 rows: a frame
    lower than the 20-row window is refused before it reaches the kernels)"""
    _one(cpe, gpu, ('runs_v', h), B.get(('runs_v', h), B.gen_runs_v, h))
    _one(cpe, gpu, ('height', h), B.get(('height', h), B.gen_height, h))


@pytest.mark.gpu
@pytest.mark.parametrize('w', B.WIDTHS)
def test_blobs_at_every_width(cpe, orc, gpu, w):
    g = _one(cpe, gpu, ('width', w), B.get(('width', w), B.gen_width, w))
    assert g['hmask'].any() and g['vmask'].any() and g['jbits'][0].any()
    assert (g['hbits'] is not None) == (w % 16 == 0)


@pytest.mark.gpu
@pytest.mark.parametrize('holes', [False, True])
def test_single_pixels_at_cell_corners(cpe, orc, gpu, holes):
    _one(cpe, gpu, ('specks', holes), B.get(('specks', holes), B.gen_specks, holes))


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(B.RECTS))
def test_rectangles(cpe, orc, gpu, name):
    for full in (False, True):
        _one(cpe, gpu, ('rect', name, full), B.get(('rect', name, full), B.gen_rect, name, full))


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['mid_word', 'from_strip_edge', 'band_by_margin'])
def test_mask_contour_outside_the_rectangle_does_not_leak(cpe, orc, gpu, name):
    """the planes of the two kernels are those of the clean case (the expansion, which takes mask_contour as it comes, is
    not compared)"""
    noisy, clean = B.with_mc_outside(B.get(('rect', name, True), B.gen_rect, name, True))
    g = _run(cpe, gpu, [noisy])[0]
    _check(clean, g, _oracle(('rect', name, True), clean), ('mc outside', name), expansion=False)


@pytest.mark.gpu
def test_batch_with_a_frame_without_region_equals_alone(cpe, orc, gpu):
    names = ('mid_word', 'frame', 'strip_by_margin', 'one_wide', 'bottom_border')
    cases = [B.get(('rect', k, False), B.gen_rect, k, False) for k in names]
    cases.insert(2, dict(cases[0], status=1))
    cases.append(B.get(('specks', True), B.gen_specks, True))
    batch = _run(cpe, gpu, cases)
    rev = _run(cpe, gpu, cases[::-1])
    for i, c in enumerate(cases):
        alone = _run(cpe, gpu, [c])[0]
        _same(batch[i], alone, (i, 'batch'))
        _same(rev[len(cases) - 1 - i], alone, (i, 'reversed batch'))
    _check(cases[2], batch[2], M.oracle(cases[2]), 'no region in the batch')


@pytest.mark.gpu
@pytest.mark.parametrize('h,w', [(195, B.WIDE), (83, 576), (90, 801)])
def test_planes_after_a_poisoned_workspace(cpe, orc, gpu, h, w):
    """every byte of the workspace 0xFF before the call: the one-bit planes, their guard tile columns and the rows >= h of
    the last tile row (195, 83 and 90 are no multiples of 8) come out as on a fresh workspace"""
    b, mc = B.gen_blobs(h, w, seed=5)
    c = B.bcase(b, mc, spot=B.spot_for(h, w))
    cases = [c, dict(c, status=1), B.bcase(np.full((h, w), 255, np.uint8), spot=B.spot_for(h, w))]
    ws = P.workspace(len(cases), h, w, gpu)
    P.fill(ws, 0xFF)
    got = _run(cpe, gpu, cases, ws=ws)
    for i, ci in enumerate(cases):
        _check(ci, got[i], M.oracle(ci), ('poisoned', i))
    assert got[2]['hbits'] is None or (got[2]['hbits'][0].all() and got[2]['vbits'][0].all())
    fresh = _run(cpe, gpu, cases)
    for i in range(len(cases)):
        _same(got[i], fresh[i], ('poisoned', i))
