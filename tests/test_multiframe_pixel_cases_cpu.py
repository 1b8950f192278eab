"""The numpy reference of cpe_multi_frame_fit_pixels_batch (tests/multiframe_pixel_cases.py) checked against itself: the Jacobian of
rule 6 against central differences, the margins of every decision, the members at every accepted pose, the restated loop against
scipy, the level of J'J, the accuracy tables of the module docstring and what sel_cos = min_cos does.  No GPU."""
import os
import re

import numpy as np
import pytest

import multiframe_lm_cases as LM
import multiframe_pixel_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(M.cases()) + ['full tables']


def _fitted():
    return [(n, g, r) for n in NAMES for g, r in enumerate(M.reference(n)) if r['status'] == M.ST_OK]


def test_the_header_declares_the_call_and_the_kernel_uses_the_cases_waves():
    hdr = open(os.path.join(ROOT, 'include', 'cpe.h')).read()
    assert int(re.search(r'#define CPE_VERSION (\d+)', hdr).group(1)) >= 130 and '130: cpe_multi_frame_fit_pixels_batch' in hdr
    src = open(os.path.join(ROOT, 'cylinder-pose-estimation_amd', 'csrc', 'fit.hip')).read()
    assert int(re.search(r'#define CPE_MFPX_WAVES (\d+)', src).group(1)) == M.WAVES


def test_the_cases_hold_the_shapes_the_kernel_can_go_wrong_at():
    kept = {len(r['kept']) for n in NAMES for r in M.reference(n)}
    assert {0, 1, 2, 3, M.WAVES + 1, 2 * M.WAVES + 1} <= kept
    per_cam = {c for n in NAMES for r in M.reference(n) for p in r['grp'].probs for c in p.n}
    assert {0, 5, 63, 64, 65, 130, M.MAXP} <= per_cam
    assert M.reference('gate 4 px')[0]['counts'][3] == 3
    assert M.reference('refused lines')[0]['counts'][2] > 300
    st = [r['status'] for r in M.reference('three groups')]
    assert st == [0, 0, M.ST_FEW_POINTS, M.ST_FEW_POINTS] and [len(r['kept']) for r in M.reference('three groups')] == [2, 4, 0, 1]
    assert [r['status'] for r in M.reference('NaN start in one group')] == [M.ST_FEW_POINTS, 0]


def test_jacobian_against_central_differences():
    r = M.reference('2 WAVES + 1 frames')[0]
    grp, S, x = r['grp'], r['S'], M.cases()['2 WAVES + 1 frames']['x0'][0]
    T = LM.vec2T(x)
    _, J = grp.jacobian(x, S)
    worst = 0.0
    for k in range(6):
        def moved(h):
            d = np.zeros(6); d[k] = h
            Tn = np.eye(4)
            Tn[:3, :3] = LM.rot_exp(d[:3]) @ T[:3, :3]
            Tn[:3, 3] = T[:3, 3] + d[3:]
            return np.concatenate([e['r'].reshape(-1) for e in grp.evaluate([M.frame_cyl(Tn, A) for A in grp.A], S)])
        h = 1e-6 if k < 3 else 1e-4
        num = (moved(h) - moved(-h)) / (2 * h)
        worst = max(worst, float(np.abs(num - J[:, k]).max() / np.abs(J[:, k]).max()))
    print(f'rule 6 against central differences: {worst:.2e} of the largest entry of a column')
    assert worst < 1e-6


@pytest.mark.parametrize('name', NAMES)
def test_every_decision_has_a_margin(name):
    for g, r in enumerate(M.reference(name)):
        if r['S'] is not None:
            m = min(r['margins'].values())
            assert m > 1e-6, f'{name} group {g}: margin {m:.2e} in {r["margins"]}'


def test_no_member_fails_at_an_accepted_pose():
    for name, g, r in _fitted():
        for x in r['path']:
            assert all(e['ok'].all() for e in r['grp'].evaluate(r['grp'].cyls(x), r['S'])), f'{name} group {g}'
        if name != 'sel_cos = min_cos':
            assert r['nan_trials'] == 0, f'{name} group {g}: {r["nan_trials"]} NaN trials with sel_cos 0.35'


def test_restated_loop_against_scipy():
    wp = wf = 0.0
    for name, g, r in _fitted():
        o = r['opt']
        assert o['feasible']
        dp, df = M.pose_difference(r['T'], o['T']), r['fvals'][1] / o['f'] - 1
        wp, wf = max(wp, dp), max(wf, abs(df))
    print(f'restated loop against scipy over {len(_fitted())} groups: pose {wp:.3e}, f / f_ls - 1 {wf:.3e}')
    assert wp <= M.PIXMF_POSE_BOUND and wf <= M.PIXMF_F_BOUND
    assert 2 * wp > 0.5 * M.PIXMF_POSE_BOUND and 2 * wf > 0.5 * M.PIXMF_F_BOUND, 'the recorded bounds are not twice the worst any more'


def test_level_of_the_normal_matrix():
    worst = 0.0
    for name, g, r in _fitted():
        N64 = np.zeros((6, 6)); N64[np.triu_indices(6)] = r['N']
        _, Jl = r['grp'].jacobian(r['x'], r['S'], dtype=np.longdouble)
        Nl = Jl.T @ Jl
        d = np.sqrt(np.diag(Nl).astype(np.float64))
        worst = max(worst, max(abs(float(N64[a, b] - Nl[a, b])) / (d[a] * d[b]) for a in range(6) for b in range(a, 6)))
    print(f'J\'J in float64 against long double: {worst:.3e} of sqrt(N_aa N_bb)')
    assert 16 * worst <= M.PIXMF_N_BOUND <= 64 * worst


@pytest.mark.parametrize('which', ['all', 'third'])
def test_accuracy_tables(which):
    worst = np.zeros(2)
    for F, seed in M.ACCURACY_RUNS:
        run = M.accuracy_run(F, seed, which)
        r = run['ref']
        assert r['status'] == M.ST_OK and r['nan_trials'] == 0
        assert 0.34 < r['stats'][2] < 0.37                                     # 0.25 sqrt 2 px
        pf, pt = M.per_frame_errors(F, seed, which), M.point_fit_errors(F, seed, which)
        print(f'{which} F = {F} seed {seed}: all frames {run["err"][0]:.4f} deg {run["err"][1]:.4f} mm; per frame {pf[0]:.4f} {pf[1]:.4f}; '
              f'points {pt[0]:.4f} {pt[1]:.4f}; iterations {r["iters"][0]}, {r["stats"][2]:.4f} px')
        assert run['err'][0] < pf[0] / 5 and run['err'][1] < pf[1] / 4
        worst = np.maximum(worst, run['err'])
    assert (worst <= M.ACCURACY_BOUNDS).all()
    if which == 'third':                                                        # the worst of the ten runs is one of these
        assert (2 * worst > 0.9 * np.array(M.ACCURACY_BOUNDS)).all(), 'the recorded bounds are not twice the worst any more'


def test_membership_at_the_evaluation_gate_stalls():
    for seed, (iters, nans, rms) in M.STALL.items():
        r = M.accuracy_run(8, seed, 'all', 0.1)['ref']
        good = M.accuracy_run(8, seed, 'all')['ref']
        print(f'seed {seed}: sel_cos 0.1: {r["iters"][0]} iterations, {r["nan_trials"]} NaN trials, {r["stats"][2]:.4f} px; sel_cos 0.35: '
              f'{good["iters"][0]} iterations, {good["stats"][2]:.4f} px')
        assert r['iters'][0] > 5 * good['iters'][0] and r['nan_trials'] > 20 and abs(r['stats'][2] - rms) < 5e-3   # recorded: iters, nans
        assert r['stats'][2] > 0.40 and good['stats'][2] < 0.36 and good['nan_trials'] == 0
