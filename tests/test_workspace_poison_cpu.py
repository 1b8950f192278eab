"""The ground the workspace-poisoning tests stand on (tests/test_workspace_poison_gpu.py), without a GPU:
  - the rows of a layout, each padded to the 256-byte boundary that follows it, cover the whole block, and two rows share
    bytes only as different sides of one overlay -- so filling row after row reaches every byte the library is given;
  - every frame of every detect case ends, in the oracle, in the status the GPU test counts on (a condition on the inputs
    alone: an edit to a generator cannot silently drop a status from the coverage)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import workspace_poison as P  # noqa: E402

SHAPES = [(1, 64, 64), (3, 480, 640), (5, 480, 640), (3, 483, 650), (5, 483, 650), (4, 600, 800), (3, 1200, 1920), (2, 65, 801)]


@pytest.mark.parametrize('shape', SHAPES)
def test_padded_rows_cover_the_block(cpe, shape):
    n = shape[0]
    rows = P.rows(*shape)
    total = P.total_bytes(*shape)
    assert total % 256 == 0
    spans = sorted(P.row_span(r, n, padded=True) for r in rows)
    assert spans[0][0] == 0
    reach = 0
    for a, b in spans:
        assert a <= reach, ('a gap no row covers', reach, a)
        reach = max(reach, b)
    assert reach == total
    # the padding itself is at most 255 bytes per row: what fill_row leaves out of a row's slot the row's readers cannot
    # tell from the slot of the next row, and the whole-block patterns (A, B, F) reach it
    assert all(P.row_span(r, n, True)[1] - P.row_span(r, n)[1] < 256 for r in rows)


@pytest.mark.parametrize('shape', SHAPES)
def test_rows_overlap_only_across_the_sides_of_one_overlay(cpe, shape):
    n = shape[0]
    spans = sorted((*P.row_span(r, n, padded=True), r) for r in P.rows(*shape))
    for i, (a0, a1, a) in enumerate(spans):
        for b0, b1, b in spans[i + 1:]:
            if b0 >= a1:
                break
            assert a['overlay'] != 0 and a['overlay'] == b['overlay'] and a['side'] != b['side'], (a['name'], b['name'])


def test_row_names_do_not_depend_on_the_layout(cpe):
    assert len({tuple(r['name'] for r in P.rows(*s)) for s in SHAPES}) == 1
    names = P.row_names(480, 640)
    assert len(set(names)) == len(names) and {'best', 'state', 'discs', 'grayin', 'base_h', 'joints_mask'} <= set(names)


@pytest.mark.parametrize('case', P.DETECT_CASES)
def test_case_frames_reach_their_status(orc, case):
    c = P.detect_case(case)
    assert P.oracle_status(case) == c['status']
    assert 3 <= len(c['status']) <= 5 and P.ST_OK in c['status'] and any(s != P.ST_OK for s in c['status'])


def test_cases_cover_the_early_endings_and_both_label_paths(orc):
    seen = {s for case in P.DETECT_CASES for s in P.detect_case(case)['status']}
    assert {P.ST_OK, P.ST_NO_REGION, P.ST_NO_SPOT, P.ST_NO_LINES} <= seen
    widths = {P.detect_case(case)['frames'].shape[2] % 16 == 0 for case in P.DETECT_CASES}
    assert widths == {True, False}                       # word-level and byte-level passes
    assert any(P.detect_case(case)['frames'].ndim == 4 for case in P.DETECT_CASES)
    assert not P.detect_case('grey480')['frames'][1].any()     # the all-zero frame
    assert np.array_equal(P.detect_case('grey480')['frames'][0], P._stereo(480, 640, 0)[0])
