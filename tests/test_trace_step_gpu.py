"""The step loop of the border followers (csrc/cpe_dev.h BitWin, trace_border, StatVisitor; csrc/region.hip StoreVisitor,
k_blob_trace) through cpe_debug_blob_region, as tests/test_blob_stage_gpu.py drives it: an identity table, so the image is what
SimpleBlobDetector sweeps, and every frame is compared with oracle/stages.simple_blob_detector and largest_blob_from_sweep with
tolerance 0 -- blobs (x, y, r) of all 17 thresholds as f64, key points as f32 bits, the hole and outer-border counts against
find_contours, status, rect, mask_contour and overflow 0.  The images are tests/trace_step_cases.py (one idea each: chunk
limits of the stored border points, pixels passed twice, the edges of the tracer's bit window, lanes in lockstep, coordinates
up to 4095); tests/test_trace_step_cases_cpu.py holds them to their claims.  A border of one point occurs (a lone bright pixel)
but encloses no area, so it is followed and never accepted: its length is checked among the contours, not among the blobs."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trace_step_cases as T  # noqa: E402
import workspace_poison as WP  # noqa: E402
from test_blob_stage_gpu import _check, _coverage, _frame, _oracle, _run, _same  # noqa: E402

SMALL = [n for n in T.CASES if not n.startswith('far_')]
KP_CAP, BLOB_CAP = 4096, 16384


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(T.CASES))
def test_trace_step_case_alone(cpe, orc, gpu, name):
    img = T.get(name)
    if name in ('hole_lengths', 'ring_lengths'):      # every chunk limit occurs among the accepted blobs, by the oracle's contours
        lens = {n for n, is_hole in _coverage(img) if bool(is_hole) == (name == 'hole_lengths')}
        assert set(T.LENGTHS[1:]) <= lens, sorted(set(T.LENGTHS[1:]) - lens)
    if name == 'ring_lengths':                        # and the border of one point among the contours (area 0: never accepted)
        from oracle import stages as S
        assert any(len(p) == 1 and not is_hole for p, is_hole in S.find_contours(img > 50, 'list', 'none'))
    res = _run(cpe, gpu, img[None], KP_CAP, BLOB_CAP)
    _check(img, _frame(res, 0), name)


@pytest.mark.gpu
def test_pool_runs_out_without_a_flag(cpe, orc, gpu):
    """more hole borders at one threshold than its chunk pool serves (every 6-pixel hole reserves two chunks, and the oracle
    counts more than MAXCH_SMALL / 2 of them): the borders that find the pool empty are followed again for their distances
    -- same blobs, and overflow stays 0 (as _check asserts)"""
    img = T.get('pool_runs_out')
    assert 2 * _oracle(img)['holes'][1] > T.MAXCH_SMALL and img.size // 256 < T.MAXCH_SMALL
    g = _frame(_run(cpe, gpu, img[None], KP_CAP, BLOB_CAP), 0)
    _check(img, g, 'pool_runs_out')
    assert g['state']['overflow'] == 0


@pytest.mark.gpu
@pytest.mark.parametrize('value', [0xFF, 0x00])
def test_trace_step_stale_workspace(cpe, orc, gpu, value):
    """the same images in a workspace filled with 0xFF / 0x00 before the call: identical results"""
    for shape in sorted({T.get(n).shape for n in SMALL}):
        names = [n for n in SMALL if T.get(n).shape == shape]
        imgs = np.stack([T.get(n) for n in names])
        clean = _run(cpe, gpu, imgs, KP_CAP, BLOB_CAP)
        ws = WP.workspace(len(names), shape[0], shape[1], gpu)
        WP.fill(ws, value)
        stale = _run(cpe, gpu, imgs, KP_CAP, BLOB_CAP, ws=ws)
        for i, n in enumerate(names):
            _same(_frame(stale, i), _frame(clean, i), (n, value))
            _check(imgs[i], _frame(stale, i), (n, value))


@pytest.mark.gpu
def test_trace_step_mixed_batch_equals_alone(cpe, orc, gpu):
    """every case of one frame size in one batch (a case that has its size to itself: beside its own copy turned by 180
    degrees), and in reversed order: each frame identical to its run alone"""
    for shape in sorted({T.get(n).shape for n in T.CASES}):
        names = [n for n in T.CASES if T.get(n).shape == shape]
        imgs = [T.get(n) for n in names]
        if len(names) == 1:
            names, imgs = names + [names[0] + ' turned'], imgs + [np.ascontiguousarray(imgs[0][::-1, ::-1])]
        batch = _run(cpe, gpu, np.stack(imgs), KP_CAP, BLOB_CAP)
        rev = _run(cpe, gpu, np.stack(imgs[::-1]), KP_CAP, BLOB_CAP)
        for i, n in enumerate(names):
            alone = _frame(_run(cpe, gpu, imgs[i][None], KP_CAP, BLOB_CAP), 0)
            _same(_frame(batch, i), alone, (n, 'batch'))
            _same(_frame(rev, len(names) - 1 - i), alone, (n, 'reversed batch'))
