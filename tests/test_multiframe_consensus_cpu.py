"""The consensus over frames (cpe_multi_frame_consensus_batch) on the CPU: its pair schedule, why it exists -- the plain LM form is
pulled away by frames with a wrong cylinder -- and its numpy reference on the scenes of multiframe_consensus_cases.

Measured with ref_consensus, per-frame fits by oracle.fit_cylinder(mode=1), make_scene(24, seed, 0.1, npts=200), seeds 0-9
(`pytest -s` prints the table):
    0 of 24 displaced   plain LM 0.0024-0.0086 deg, 0.008-0.034 mm off Ttrue; consensus the same pose, all 24 frames inliers
    3 of 24 displaced   plain LM 0.67-7.07 deg, 4.4-33.8 mm;   consensus at most 0.0081 deg, 0.0355 mm, exactly the 3 rejected
    8 of 24 displaced   plain LM 0.64-10.12 deg, 4.5-33.7 mm;  consensus at most 0.0096 deg, 0.0433 mm, exactly the 8 rejected
Every run converged in one round.  The worst of the twenty with displaced frames, 0.009595 deg and 0.043275 mm
(multiframe_consensus_cases.MEASURED_WORST), doubled, are NOISY_CONSENSUS_BOUNDS."""
import numpy as np
import pytest

import multiframe_cases as mc
import multiframe_consensus_cases as cc
import multiframe_lm_cases as lc


def test_symbols_are_declared(cpe):
    names = cpe.lib.declared_symbols()
    assert 'cpe_multi_frame_consensus_batch' in names and 'cpe_multi_frame_consensus_workspace_bytes' in names
    res, args = cpe.lib._SIGS['cpe_multi_frame_consensus_batch']
    assert len(args) == 26
    assert [n for n, _ in cpe.lib.CpeConsensusParams._fields_] == ['tau', 'max_hyp', 'max_rounds', 'min_inliers']
    assert cpe.lib.CONSENSUS_MAX_HYP == cc.MAX_HYP
    assert hasattr(cpe.multiframe, 'fit_multi_frame_consensus_gpu')


@pytest.mark.parametrize('u', [2, 3, 4, 5, 45, 64, 65, 1024])
def test_pairs(u):
    every = {(a, b) for a in range(u) for b in range(a + 1, u)}
    for max_hyp in sorted({1, 2, u - 1, u, u + 1, 130, 2048, 4096} - {0}):
        R, H, dense = cc.plan(u, max_hyp)
        ps = cc.pairs(u, max_hyp)
        assert len(ps) == H and 1 <= H <= max_hyp
        assert all(0 <= a < u and 0 <= b < u and a != b for a, b, _ in ps)
        live = [(min(a, b), max(a, b)) for a, b, first in ps if first]
        assert len(set(live)) == len(live), 'a pair that is not void occurs once'
        if (u // 2) * u <= max_hyp:
            assert dense and set(live) == every, 'every unordered pair is covered where max_hyp allows'
        if not dense:
            assert H == min(R * u, max_hyp) and all(first for _, _, first in ps)
            # spread: with at least u hypotheses every frame starts one
            assert max_hyp < u or {a for a, _, _ in ps} == set(range(u))
    assert cc.plan(45, 2048)[1] == 990


def _scene(orc, seed, n_bad):
    P, cnt, angles, Ttrue, bad = cc.displaced_scene(24, seed, n_bad, noise=0.1, npts=200)
    TAGV = np.stack([mc.get_TAGVcyl(*a).ravel() for a in angles])
    return P, cnt, TAGV, cc.per_frame_fits(orc, P, cnt), Ttrue, bad


@pytest.mark.parametrize('n_bad', [3, 8])
def test_plain_lm_is_pulled_away(orc, n_bad):
    """why the feature exists: the all-frame initial pose + LM over every frame"""
    for seed in range(4):
        P, cnt, TAGV, raw, Ttrue, bad = _scene(orc, seed, n_bad)
        got = lc.fit(lc.Problem(P, cnt, TAGV), raw)
        rot, tr = cc.pose_errors(got['T'], Ttrue)
        print(f'{n_bad} of 24 displaced, seed {seed}: plain LM {rot:.3f} deg {tr:.2f} mm off Ttrue')
        assert rot > 0.5


@pytest.mark.parametrize('n_bad', [0, 3, 8])
def test_reference_rejects_the_displaced_frames(orc, n_bad):
    worst = [0.0, 0.0]
    for seed in range(10 if n_bad else 4):
        P, cnt, TAGV, raw, Ttrue, bad = _scene(orc, seed, n_bad)
        r = cc.ref_consensus(P, cnt, TAGV, raw)
        assert r['status'] == cc.ST_OK
        rot, tr = cc.pose_errors(r['T'], Ttrue)
        worst = [max(worst[0], rot), max(worst[1], tr)]
        print(f'{n_bad} of 24 displaced, seed {seed}: consensus {rot:.4f} deg {tr:.4f} mm off Ttrue, rejected '
              f'{np.flatnonzero(r["inlier"] == 0).tolist()}, rounds {r["info"][3]}, margin {r["inlier_margin"]:.3g}, gap {r["key_gap"]:.3g}')
        assert np.flatnonzero(r['inlier'] == 0).tolist() == bad and r['n_inliers'] == 24 - n_bad
        assert r['flags'] == cc.CONVERGED
        assert rot <= cc.NOISY_CONSENSUS_BOUNDS['rot_deg'] and tr <= cc.NOISY_CONSENSUS_BOUNDS['tr_mm']
    print(f'{n_bad} of 24 displaced: worst {worst[0]:.4f} deg {worst[1]:.4f} mm')
    if n_bad:
        assert worst[0] <= cc.MEASURED_WORST['rot_deg'] and worst[1] <= cc.MEASURED_WORST['tr_mm'], 'the measured figures have moved'


@pytest.mark.parametrize('name', sorted(cc.CASES))
def test_cases_are_decided_with_a_margin(orc, name):
    s = cc.build(name, orc)
    r = s['ref']
    print(f'{name}: status {r["status"]} info {r["info"]} flags {r["flags"]} inliers {r["n_inliers"]} margin {r["inlier_margin"]:.3g} '
          f'gap {r["key_gap"]:.3g}')
    assert r['inlier_margin'] > 1e-3 and r['key_gap'] > 1e-6
    if s['expect'] == 'few':
        assert r['status'] == cc.ST_FEW
    else:
        assert r['status'] == cc.ST_OK
        assert np.flatnonzero(r['inlier'] == 0).tolist() == s['out']


def test_the_two_round_case_needs_two_rounds(orc):
    s = cc.build('two_rounds', orc)
    r0 = cc.ref_consensus(s['P'], s['cnt'], s['TAGV'], s['raw'], s['keep'], **dict(s['cons'], max_rounds=0))
    r = s['ref']
    late = sorted(set(r['fitted']) - set(r0['fitted']))
    assert r['info'][3] == 2 and r['flags'] == cc.CONVERGED and len(late) == 1 and late[0] not in s['bad']
    f, tau = late[0], s['cons']['tau']
    print(f'frame {f}: rms / tau {np.sqrt(r0["frame_terms"][f]) / tau:.4f} at x0, {np.sqrt(r["frame_terms"][f]) / tau:.4f} at x')
    assert 1.0 < np.sqrt(r0['frame_terms'][f]) / tau < 1.25 and np.sqrt(r['frame_terms'][f]) < tau
