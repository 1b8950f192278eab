"""k_seg_trace (csrc/masks.hip) with bit windows for the SEG_LPW lanes that trace only, through api.debug_masks against the
masks oracle as tests/test_masks_stage_gpu.py runs it (tolerance 0: masks, fragment counts, gang / glen as f32 bits, expanded
masks, overflow).  The generators are those of tests/masks_cases.py, whose vertex counts tests/test_masks_generators_cpu.py
checks; the first test here asserts from the oracle's own fragment table that each limit occurs:
  - fragments of 4, 5, 200 and 201 CHAIN_APPROX_SIMPLE vertices, the MINV / MAXVS limits of <5,200>, in one frame;
  - more fragments in a frame than one turn of the grid takes: 2 210 in a frame alone (512 workgroups of SEG_LPW = 4 lanes;
    more than MAXSEG, so OVF_SEGS is the expected flag), and 546 in every frame of a batch of 128 (128 workgroups a frame);
  - fragments that cross the edges of the tracer's window (a multiple of 8 rows and 32 columns): staircases that fall a row
    every 4 columns over 200 columns, combs 440 columns long;
  - the planar instantiation <8,700> once, at 7, 8, 700 and 701 vertices."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import masks_cases as M  # noqa: E402
from test_masks_stage_gpu import _check, _run, _same  # noqa: E402

SEG_LPW = 4          # csrc/masks.hip


def gen_limits(counts, w, bars=True):
    """one comb per vertex count of `counts` (masks_cases.COMBS), 20 rows apart, and with `bars` a plain 26 x 4 bar
    (4 vertices) and one with a cut corner (5)"""
    h = 20 * (len(counts) + 1) + 60
    b = np.zeros((h, w), np.uint8)
    if bars:
        M.bar(b, 8, 10, 26, 4)
        M.bar(b, 60, 10, 26, 4, ('tl',))
    for i, c in enumerate(counts):
        teeth, ch, step = M.COMBS[c]
        M.comb(b, 8, 30 + 20 * i, teeth, ch, step)
    return M.case(b, spot=(w - 24, h - 20, 12))


def gen_fragment_field(h=300, w=420):
    """546 fragments of 5 vertices, 7 rows and 30 columns apart"""
    b = np.zeros((h, w), np.uint8)
    n = 0
    for y in range(2, h - 6, 7):
        for x in range(2, w - 28, 30):
            M.bar(b, x, y, 26, 4, ('tl',))
            n += 1
    assert n == 42 * 13
    return M.case(b, spot=(w - 16, h - 16, 12))


def _vertex_counts(ref_roi):
    return sorted(v for v, _, _ in M.fragment_table(ref_roi))


@pytest.mark.gpu
def test_seg_trace_vertex_limits(cpe, orc, gpu):
    c = gen_limits((200, 201), 520)
    ref = M.oracle(c)
    assert _vertex_counts(ref['roi_h']) == [4, 5, 200, 201]
    assert ref['seg_h'][1] == 2                      # 5 and 200 are fragments, 4 and 201 are not
    g = _run(cpe, gpu, [c])[0]
    _check(c, g, ref, 'limits 4 5 200 201')


@pytest.mark.gpu
def test_seg_trace_planar_vertex_limits(cpe, orc, gpu):
    c = gen_limits((7, 8, 700, 701), 1500, bars=False)
    ref = M.oracle(c, 'plane')
    assert _vertex_counts(ref['roi_h']) == [7, 8, 700, 701]
    assert ref['seg_h'][1] == 2
    g = _run(cpe, gpu, [c], 'plane')[0]
    _check(c, g, ref, 'limits 7 8 700 701', 'plane')


@pytest.mark.gpu
def test_seg_trace_second_turn_alone_and_in_a_batch(cpe, orc, gpu):
    c = M.get('many_fragments')
    ref = M.oracle(c)
    assert ref['seg_h'][0] > 512 * SEG_LPW           # a frame alone gets 512 workgroups
    _check(c, _run(cpe, gpu, [c])[0], ref, 'many_fragments', ovf=M.OVF_SEGS)
    c = gen_fragment_field()
    ref = M.oracle(c)
    n = 128                                          # 16384 / 128 = 128 workgroups a frame
    assert M.MAXSEG >= ref['seg_h'][1] > 128 * SEG_LPW and ref['seg_h'][1] >= 520
    g = _run(cpe, gpu, [c] * n)
    for i in (0, 1, 63, 127):
        _check(c, g[i], ref, ('fragment field', i))
    for i in range(1, n):
        for k in ('n_seg0', 'n_seg1', 'gang0', 'glen0', 'overflow', 'status'):
            assert g[i]['state'][k] == g[0]['state'][k], (i, k)
        assert np.array_equal(g[i]['exp_h'], g[0]['exp_h']), i


@pytest.mark.gpu
def test_seg_trace_fragments_across_window_edges(cpe, orc, gpu):
    from oracle import stages as S
    for name in ('stairs_200', 'counts_200', 'fan_odd'):
        c = M.get(name)
        ref = M.oracle(c)
        spans = [np.ptp(p, axis=0) for p, _ in S.find_contours(ref['roi_h'] > 0, 'external', 'simple')]
        assert max(s[0] for s in spans) > 64, name   # wider than a window
        alone = _run(cpe, gpu, [c])[0]
        _check(c, alone, ref, name)
        pair = _run(cpe, gpu, [c, c])
        _same(pair[1], alone, (name, 'second frame'))
    c = M.get('stairs_200')
    spans = [np.ptp(p, axis=0) for p, _ in S.find_contours(M.oracle(c)['roi_h'] > 0, 'external', 'simple')]
    assert max(s[1] for s in spans) > 16             # and taller
