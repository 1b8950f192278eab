"""The cases and the numpy reference of tests/fused_tri_cases.py, checked without a GPU: the export's declaration, truth on exact
inputs, the ceiling of the derived tolerances, the margin of every decision from its gate, the order / duplicate / taken rules
on hand-made tables, and the measured noisy bounds."""
import math
import os
import re

import numpy as np
import pytest

import fused_tri_cases as FC
import plane_fit_cases as PC
import table_tri_cases as TC


def _all_references():
    for name in FC.frame_cases():
        for nb in (0, 1):
            yield f'{name} need_both {nb}', FC.frame_reference(name, nb)
    for name in FC.call_cases():
        for i, r in enumerate(FC.call_reference(name)):
            yield f'{name} frame {i}', r


def test_export_is_declared(cpe):
    hdr = open(os.path.join(os.path.dirname(cpe.lib.__file__), '..', 'include', 'cpe.h')).read()
    assert 'cpe_fused_triangulate_batch' in cpe.lib.declared_symbols()
    assert int(re.search(r'#define CPE_VERSION (\d+)', hdr).group(1)) >= 122
    res, args = cpe.lib._SIGS['cpe_fused_triangulate_batch']
    assert len(args) == 24 and 'CPE_FUSED_FLAG_TRUNCATED' in hdr
    assert [f[0] for f in cpe.lib.CpeFusedTriParams._fields_] == ['swap', 'need_both', 'min_sin', 'sigma_px', 'sigma_mm', 'max_res', 'max_px']
    assert hasattr(cpe.fit, 'fused_triangulate_batch') and hasattr(cpe.fit, 'fit_single_cylinder_fused_batch')
    assert 'res' in cpe.pipeline.FUSED_FIT_OUTPUTS


@pytest.mark.parametrize('swap', [0, 1])
def test_reference_returns_truth_on_exact_inputs(swap):
    """true planes and exact pixels: the true points within the reference's own tolerance, paired or not"""
    idx, X = TC.cylinder_hits()
    uv1, uv2 = PC.project_pair(X, 0.0, None)
    t = TC.rig_table(-12, 12)
    if swap:
        t = TC.transposed(t)
    k = np.arange(len(idx))
    s1, s2 = k[k % 3 != 1], k[k % 3 != 2]
    r = FC.reference((dict(xy=uv1[s1], id=idx[s1]), dict(xy=uv2[s2], id=idx[s2])), t, swap=swap)
    assert r['m'] == len(idx) and r['counts'].tolist() == [len(idx), len(s1) + len(s2) - len(idx), len(idx) - len(s2), len(idx) - len(s1), 0, 0]
    truth = np.where((r['src'][:, 1] >= 0)[:, None], X[s1][np.maximum(r['src'][:, 1], 0)], X[s2][np.maximum(r['src'][:, 2], 0)])
    err = np.linalg.norm(r['X'] - truth, axis=1)
    # exact inputs are exact to the rounding of the pixels: |X| eps / (pixel angle) -- a few 1e-10 mm; the tolerance plus 1e-9
    print(f'swap {swap}: worst point error {err.max():.2e} mm, worst tolerance {r["tol_X"].max():.2e}, stats {r["stats"]}')
    assert (err <= r['tol_X'] + 1e-9).all() and r['stats'][1] <= 1e-6 and r['stats'][3] <= 1e-9
    assert (r['src'][:, 0] >> 2 == 3).all()


def test_tolerances_and_margins():
    worst_t, worst_m = 0.0, math.inf
    for what, r in _all_references():
        if r['m']:
            assert r['tol_X'].max() <= 1e-6, f'{what}: tol_X {r["tol_X"].max():.3e}'
            worst_t = max(worst_t, r['tol_X'].max())
        assert r['margin'] > 1e-6, f'{what}: a decision within {r["margin"]:.3e} of its gate'
        worst_m = min(worst_m, r['margin'])
    print(f'largest tol_X {worst_t:.3e} mm, smallest margin {worst_m:.3e}')
    for name in ('index off by one, max_res', 'index off by one, max_px', 'max_px', 'max_res'):
        for r in FC.call_reference(name):
            assert r['margin'] > 1e-3, f'{name}: margin {r["margin"]:.3e}'


def test_cases_cover_what_they_claim():
    c = FC.frame_cases()
    r = FC.frame_reference('counts 2048 / 3000')
    assert r['m'] == FC.MAXP and r['counts'][1] > 1900 and min(r['counts'][2:6]) > 0 and r['flags'] == FC.FLAG_TRUNCATED
    r = FC.frame_reference('thirds')
    assert min(r['counts'][1:4]) > 100 and r['counts'][4] > 0
    assert FC.frame_reference('index span overflow')['flags'] == FC.FLAG_OVERFLOW
    assert FC.frame_reference('both empty')['m'] == 0 and FC.frame_reference('both empty')['flags'] == 0
    r = FC.frame_reference('indices outside the table')
    assert r['counts'][1] > 0 and r['counts'][2] == r['counts'][3] == 0 and r['counts'][4] > 0 and (r['src'][:, 0] == 3).all()
    r = FC.call_reference('every line refused')[0]
    assert r['counts'][1] > 0 and r['counts'][2] == r['counts'][3] == 0 and (r['src'][:, 0] == 3).all() and not r['stats'][2:].any()
    r = FC.call_reference('truncation')[0]
    assert r['m'] == FC.MAXP and r['counts'].tolist() == [FC.MAXP, 0, FC.MAXP, 0, 0, 100] and r['flags'] == FC.FLAG_TRUNCATED
    for name, n_ref in (('index off by one, max_res', 1), ('max_px', 1), ('max_res', 1)):
        free = FC.reference(FC.call_cases()[name]['frames'][0], FC.call_cases()[name]['table'])
        got = FC.call_reference(name)[0]
        assert got['counts'][4] >= free['counts'][4] + n_ref and got['m'] > 0, f'{name}: the gate refuses nothing'
    nb = FC.call_reference('need_both')[1]
    assert nb['counts'][4] > FC.frame_reference('thirds')['counts'][4]
    assert set(c) >= {'duplicates', 'nan pixels'}
    assert FC.frame_reference('nan pixels')['counts'][4] >= 8


def _hand(ids1, ids2):
    """tables of exact pixels of the cylinder's points with these (col,row) indices; a repeated index gets a moved pixel"""
    idx, X = TC.cylinder_hits()
    uv1, uv2 = PC.project_pair(X, 0.0, None)
    look = {(int(a), int(b)): k for k, (a, b) in enumerate(idx)}
    def tab(ids, uv):
        xy = np.array([uv[look[i]] for i in ids]) + 0.125 * np.arange(len(ids))[:, None]
        return dict(xy=xy, id=np.array(ids, np.int32).reshape(-1, 2))
    return tab(ids1, uv1), tab(ids2, uv2)


def test_order_duplicates_and_taken_on_hand_made_tables():
    a, b, c, d, e, g = (0, 0), (1, 0), (2, 1), (-1, 3), (0, 5), (3, -2)
    t = TC.rig_table(-12, 12)
    # table 1: a b a c d; table 2: c e a a g.  Pairs: a -> slot 2 of table 2 (the first a), b alone, a again -> slot 2 again, c -> 0,
    # d alone; then the untaken of table 2 in its order: e (1), the second a (3), g (4)
    r = FC.reference(_hand([a, b, a, c, d], [c, e, a, a, g]), t)
    assert r['src'][:, 1:].tolist() == [[0, 2], [1, -1], [2, 2], [3, 0], [4, -1], [-1, 1], [-1, 3], [-1, 4]]
    assert (r['src'][:, 0] & 3).tolist() == [3, 1, 3, 3, 1, 2, 2, 2]
    assert r['idx'].tolist() == [list(x) for x in (a, b, a, c, d, e, a, g)]
    assert r['counts'].tolist() == [8, 3, 2, 3, 0, 0]
    # an empty table on either side: the other one, one ray each
    r = FC.reference(_hand([a, b, a, c, d], []), t)
    assert r['src'][:, 1:].tolist() == [[k, -1] for k in range(5)] and (r['src'][:, 0] & 3 == 1).all()
    r = FC.reference(_hand([], [c, e, a, a, g]), t)
    assert r['src'][:, 1:].tolist() == [[-1, k] for k in range(5)] and (r['src'][:, 0] & 3 == 2).all()
    # a one-ray point is the one-camera reference's, to the bit
    K2, T21 = TC.camera(2)
    t2 = _hand([], [c, e, a, a, g])[1]
    one = TC.ref_table_triangulate(t2['xy'], t2['id'], 5, K2, T21, t['P'], t['status'], t['lo'], t['hi'])
    assert np.array_equal(r['X'], one['X']) and np.array_equal(r['res'][:, 2:], one['res']) and not r['res'][:, :2].any()


@pytest.mark.parametrize('kind', ['rig', 'noisy'])
def test_noisy_fused_beats_the_two_ray_point(kind):
    """seeds 0..4: the fused mean error at the defaults is below that of the two-ray point on the same pixels, and inside the
    stored bound"""
    for seed in FC.NOISY_SEEDS:
        case = FC.noisy_case(seed, kind)
        e = FC.mean_errors(case)
        print(f'{kind} seed {seed}: fused {e["fused"]:.4f} mm, two-ray {e["two_ray"]:.4f} mm, stats {case["ref"]["stats"]}')
        assert case['ref']['m'] == case['n_points'] and case['ref']['counts'][1] == case['n_points']
        assert e['fused'] < e['two_ray']
        assert e['fused'] <= FC.NOISY_FUSED_BOUNDS[kind]['mean_mm']
        assert 0.5 * FC.NOISY_FUSED_BOUNDS[kind]['mean_mm'] >= e['fused'] - 1e-4, 'the stored bound is not twice the worst seed'


@pytest.mark.parametrize('kind', ['rig', 'noisy'])
def test_noisy_frame_with_thirds_missing_returns_every_point(kind):
    for seed in FC.NOISY_SEEDS:
        case = FC.noisy_case(seed, kind, True)
        r, e = case['ref'], FC.mean_errors(case)
        print(f'{kind} seed {seed}: counts {r["counts"]}, pairs {e["fused"]:.4f}, left {e["left"]:.4f}, right {e["right"]:.4f} mm')
        assert r['m'] == case['n_points'] and r['counts'][4] == 0 and min(r['counts'][1:4]) > 100
        assert len({tuple(i) for i in r['idx'].tolist()}) == case['n_points']
        assert e['fused'] <= FC.NOISY_FUSED_BOUNDS[kind]['mean_mm']
        assert e['left'] <= TC.NOISY_TRI_BOUNDS[1]['mean_mm'] and e['right'] <= TC.NOISY_TRI_BOUNDS[2]['mean_mm']
