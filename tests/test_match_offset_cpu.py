"""The Python reference of the index-shift search (tests/match_offset_cases.py) on its own, without a GPU: it recovers every
applied shift, sets the flags the header lists, and lets (0,0) win its ties.  The GPU test compares the kernel with this
reference at tolerance 0, so what is asserted here is what the kernel is held to."""
import numpy as np
import pytest

import match_offset_cases as M

CASES = M.cases()


def test_winner_key_prefers_the_unshifted_and_then_the_smaller_shift():
    cands = M.candidates(2, 2)
    def win(hot):
        s = np.zeros(len(cands), np.int32)
        for c in hot:
            s[cands.index(c)] = 9
        return cands[M.pick_winner(cands, s)]
    assert win([]) == (0, 0)                                     # all equal
    assert win([(1, 0), (-1, 0), (0, 0), (0, 1)]) == (0, 0)       # (0,0) wins every tie it is part of
    assert win([(1, 0), (-1, 0)]) == (-1, 0)                      # then dc ascending
    assert win([(1, 0), (0, 1), (0, -1)]) == (0, -1)              # the smaller |dc| first, then dr ascending
    assert win([(2, 0), (1, 1), (-1, -1)]) == (-1, -1)            # |dc|+|dr| equal, |dc| 1 < 2
    assert win([(2, 2), (1, 0)]) == (1, 0)
    s = np.zeros(len(cands), np.int32)
    s[cands.index((2, -1))] = 3
    assert cands[M.pick_winner(cands, s)] == (2, -1)              # a larger score beats any tie-break
    assert cands[0] == (-2, -2) and cands[1] == (-2, -1) and cands[5] == (-1, -2)    # dc outer, dr inner, ascending


@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_reference_recovers_shift_and_sets_flags(orc, case):
    ref = M.references()[case['name']]
    p = case['params']
    ncand = (2 * p['win_c'] + 1) * (2 * p['win_r'] + 1)
    assert ref['scores'].shape == (ncand,) and ref['score'][0] == ref['scores'].max()
    assert ref['score'][1] == (np.sort(ref['scores'])[-2] if ncand > 1 else 0)
    assert ref['score'][2] == ref['scores'][M.candidates(p['win_c'], p['win_r']).index((0, 0))]
    assert ref['score'][3] >= ref['score'][0]                     # inliers are kept pairs
    print(case['name'], 'offset', ref['offset'], 'score', ref['score'], 'flags', ref['flags'])
    if case['expect_offset'] is not None:
        assert tuple(ref['offset']) == tuple(case['expect_offset'])
    ef = case['expect_flags']
    if ef == 'edge':
        assert ref['flags'] & M.EDGE
    elif ef == 'weak':
        assert ref['flags'] & M.WEAK and tuple(ref['offset']) == (0, 0) and ref['score'][0] < p['min_score']
    elif ef is not None:
        assert ref['flags'] == ef
    n1 = min(max(case['cnt1'], 0), M.MAXP)
    assert np.array_equal(ref['id1_out'], case['t1'][:n1, 2:4].astype(np.int32) + ref['offset'])
    if ref['flags'] & (M.WEAK | M.OVERFLOW):
        assert tuple(ref['offset']) == (0, 0) and not ref['flags'] & M.SHIFTED
    if ref['flags'] & M.OVERFLOW:
        assert not ref['scores'].any()


def test_true_shift_stands_clear_of_the_runner_up(orc):
    """the evidence of DESIGN 3.7 as an assertion: on the ground-truth tables the winner has at least 1.5 times the
    runner-up's inliers"""
    for c in CASES:
        if c['name'].startswith('gt') and c['expect_offset'] is not None:
            s = M.references()[c['name']]['score']
            assert s[0] >= 1.5 * s[1], (c['name'], s)
