"""The cases and the two references of curvature_cases.py against each other, without a GPU: the generators are what they
claim (ties where claimed, no gate value near a bound), the ordered reference agrees with the LAPACK one within the tolerance
formula the GPU test uses, and the reference alone meets what the GPU test asks of the kernels on the grid + plane case."""
import numpy as np
import pytest

import curvature_cases as cc


def _tied(P, k=20):
    s = np.sort(cc.neighbours(P, k)[1], 1)[:, :k + 1]
    return int((s[:, 1:] == s[:, :-1]).any(1).sum())


def test_grid_ties_before_the_noise_and_none_after():
    assert _tied(cc.grid_points(0, noise=0.0, rotate=False)[0]) > 300      # the tie rule is exercised (the GPU test runs this frame)
    assert _tied(cc.named_points('grid')) == 0
    for s in range(3):
        assert _tied(cc.cylinder_points(s)) == 0


def test_duplicates_rank_by_index():
    nbr = cc.neighbours(cc.named_points('dup'), 20)[0]
    for p in (3, 7, 100, 200):
        assert nbr[p, :4].tolist() == [3, 7, 100, 200]


def test_pack_poisons_every_slot_past_the_count():
    X, cnt = cc.pack(cc.mixed_batch())
    assert cnt.tolist() == [0, 5, 240, cc.MAXP + 7]
    for i, c in enumerate(cnt):
        assert np.isfinite(X[i, :cc.used(c)]).all() and np.isnan(X[i, cc.used(c):]).all()


@pytest.mark.parametrize('mode', [cc.REFERENCE, cc.INTERCEPT])
@pytest.mark.parametrize('name', ['cyl0', 'grid', 'dup', 'wall', 'count6', 'count21', 'count65', 'count257'])
def test_ordered_reference_agrees_with_lapack_within_the_tolerance(name, mode):
    for k in cc.KS[mode]:
        o, l = cc.reference(name, k, mode, 'ordered'), cc.reference(name, k, mode, 'lapack')
        fair = l['cond'] < cc.COND_MAX
        assert fair.mean() > 0.9 and (k < 20 or fair.sum() >= len(fair) - 4)
        eL, eK = cc.value_errors(o, l)
        assert (eL[fair] <= cc.tol(l['cond'][fair])).all() and (eK[fair] <= cc.tol(l['cond'][fair])).all(), (name, mode, k)
        assert np.abs((o['normal'] ** 2).sum(1) - 1).max() < 64 * cc.EPS


def test_plane_frame_has_exactly_zero_curvature_and_no_gated_point():
    P = cc.named_points('plane')
    for mode in (cc.REFERENCE, cc.INTERCEPT):
        o = cc.ordered(P, 20, mode)
        assert np.abs(o['L']).max() == 0.0
        c = cc.consensus(P, o)
        assert c['n_gated'] == 0 and c['status'] == 5 and not c['axis'].any()


@pytest.mark.parametrize('mode', [cc.REFERENCE, cc.INTERCEPT])
def test_no_gate_value_near_a_bound(mode):
    for name in cc.CONSENSUS_NAMES:
        assert cc.clear_of_bounds(cc.reference(name, 20, mode, 'ordered'), cc.GATE_DEFAULT), name
    assert cc.clear_of_bounds(cc.reference('wall', 20, mode, 'ordered'), cc.GATE_BAND)
    assert cc.clear_of_bounds(cc.reference('wall', 20, mode, 'ordered'), (0.25, 30.0, 60.0))


def test_reference_alone_gates_the_cylinder_and_not_the_plane():
    P, is_cyl, org, d = cc.grid_plus_plane(0)
    c = cc.consensus(P, cc.reference('wall', 20, cc.INTERCEPT, 'ordered'), cc.GATE_BAND)
    assert c['n_gated'] == 425 and np.array_equal(c['gate'], is_cyl)
    assert cc.angle_deg(c['axis'][3:6], d) < 1.0
    assert abs(c['axis'][6] - cc.R) < 0.05 * cc.R            # the small-neighbourhood bias is about -1 to -3 %


def test_intercept_mode_gives_curvatures_in_mm_and_the_reference_mode_does_not():
    P = cc.named_points('cyl0')
    r1 = cc.consensus(P, cc.reference('cyl0', 20, cc.INTERCEPT, 'ordered'))
    assert r1['n_gated'] == len(P) and abs(r1['axis'][6] - cc.R) < 0.05 * cc.R
    r0 = cc.gate_values(cc.reference('cyl0', 20, cc.REFERENCE, 'ordered')['L'])[2]
    assert np.median(r0) > 1.1 * cc.R                       # estCurvatures.m as it stands: 53-57 mm for a 45 mm cylinder
