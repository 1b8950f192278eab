"""The numpy reference of cpe_multi_frame_fit_pixels_angles_batch (tests/multiframe_joint_cases.py) checked against itself: the
Jacobian of rule 5, angle columns included, against central differences; the margins of every decision; the block solve of one trial
against a dense solve; the restated loop against scipy on all 6 + 2 F unknowns; stiff weights against the fixed-angle reference; the
level of the blocks in float64; and the acceptance comparisons on perturbed and on exact scenes.  No GPU."""
import os
import re

import numpy as np
import pytest

import multiframe_joint_cases as J
import multiframe_lm_cases as LM
import multiframe_pixel_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(J.cases())


def _fitted():
    return [(n, g, r) for n in NAMES for g, r in enumerate(J.reference(n)) if r['status'] == J.ST_OK]


def _recorded(measured, bound, what):
    """a recorded bound holds, and is still what is measured (within a factor 2 either way would hide nothing: 0.5 .. 1)"""
    assert measured <= bound, f'{what}: measured {measured:.3e} above the recorded {bound:.3e}'
    assert measured > 0.5 * bound, f'{what}: the recorded {bound:.3e} is not what is measured any more ({measured:.3e})'


def test_the_header_declares_the_call_and_the_kernel_uses_the_cases_constants():
    hdr = open(os.path.join(ROOT, 'include', 'cpe.h')).read()
    assert int(re.search(r'#define CPE_VERSION (\d+)', hdr).group(1)) >= 131 and '131: cpe_multi_frame_fit_pixels_angles_batch' in hdr
    assert re.search(r'^CPE_API int32_t cpe_multi_frame_fit_pixels_angles_batch\(', hdr, flags=re.M)
    assert int(re.search(r'#define CPE_MFJOINT_MAXF (\d+)', hdr).group(1)) == J.MAXF
    src = open(os.path.join(ROOT, 'cylinder-pose-estimation_amd', 'csrc', 'fit.hip')).read()
    assert int(re.search(r'constexpr int MFJ_WAVES = (\d+);', src).group(1)) == J.WAVES


def test_the_cases_hold_the_shapes_the_kernel_can_go_wrong_at():
    kept = {len(r['kept']) for n in NAMES for r in J.reference(n)}
    assert {0, 1, 2, 3, J.WAVES, J.WAVES + 1, 2 * J.WAVES + 1} <= kept
    per_cam = {c for n in NAMES for r in J.reference(n) for p in r['grp'].probs for c in p.n}
    assert {0, 5, 63, 64, 65, 130} <= per_cam
    r = J.reference('2 WAVES + 1 frames, one without a member')[0]
    assert r['status'] == J.ST_OK and sum(len(s) == 0 for s in r['S']) == 1
    empty = [i for i, s in enumerate(r['S']) if len(s) == 0][0]
    assert r['angles'][empty].tobytes() == r['grp'].q0[empty].tobytes() and (r['angles'] != r['grp'].q0).any(1).sum() == len(r['S']) - 1
    assert J.reference('gate 4 px')[0]['counts'][3] == 3
    st = [r['status'] for r in J.reference('three groups')]
    assert st == [0, 0, J.ST_FEW_POINTS, J.ST_FEW_POINTS] and [len(r['kept']) for r in J.reference('three groups')] == [2, 4, 0, 1]
    assert [r['status'] for r in J.reference('NaN start in one group')] == [J.ST_FEW_POINTS, 0]
    pole = J.reference('a tilt start at the pole')
    assert [r['status'] for r in pole] == [J.ST_FEW_POINTS, 0] and len(pole[0]['S'][1]) == 0 and len(pole[0]['S'][0]) > 0


def test_jacobian_against_central_differences():
    name = '2 WAVES + 1 frames, one without a member'
    r = J.reference(name)[0]
    grp, S, x = r['grp'], r['S'], J.cases()[name]['x0'][0]
    q = grp.q0 + 1e-3 * np.random.default_rng(1).standard_normal(grp.q0.shape)
    rows = grp.jacobians(x, q, S)
    Jx, Jq = np.concatenate([j[1] for j in rows]), [j[2] for j in rows]
    pixels = lambda xx, qq: grp.residual_vector(xx, qq, S)[:len(Jx)]
    worst = 0.0
    for k in range(6):
        d = np.zeros(6); h = 1e-6 if k < 3 else 1e-4
        d[k] = h
        num = (pixels(J.step_pose(x, d), q) - pixels(J.step_pose(x, -d), q)) / (2 * h)
        worst = max(worst, float(np.abs(num - Jx[:, k]).max() / np.abs(Jx[:, k]).max()))
    row = 0
    for i, jq in enumerate(Jq):
        for k in range(2):
            if not len(jq):
                continue
            d = np.zeros_like(q); d[i, k] = 1e-6
            num = (pixels(x, q + d) - pixels(x, q - d)) / 2e-6
            assert not num[:row].any() and not num[row + len(jq):].any(), 'the angles of a frame move another frame\'s residuals'
            worst = max(worst, float(np.abs(num[row:row + len(jq)] - jq[:, k]).max() / np.abs(jq[:, k]).max()))
        row += len(jq)
    print(f'rule 5 against central differences: {worst:.2e} of the largest entry of a column')
    assert worst < 1e-6


@pytest.mark.parametrize('name', NAMES + ['capacity'])
def test_every_decision_has_a_margin(name):
    for g, r in enumerate(J.reference(name)):
        if r['S'] is not None:
            m = min(r['margins'].values())
            assert m > 1e-6, f'{name} group {g}: margin {m:.2e} in {r["margins"]}'


def test_the_block_solve_is_the_dense_solve():
    worst = 0.0
    for name, g, r in _fitted():
        B = r['grp'].blocks(J.cases()[name]['x0'][g], r['grp'].q0, r['S'])
        for lam in (1e-3, 1.0):
            dx, dq = J.block_solve(*B, lam)
            ex, eq = J.dense_solve(*B, lam)
            worst = max(worst, float(np.abs(dx - ex).max() / np.abs(ex).max()), float(np.abs(dq - eq).max() / max(np.abs(eq).max(), 1e-300)))
    print(f'block solve against the dense (6 + 2 F) solve: {worst:.2e} relative')
    assert worst < 1e-9                                    # both are backward stable; the dense system's condition is about 1e6


def test_restated_loop_against_scipy():
    wp = wa = wf = 0.0
    for name, g, r in _fitted():
        o = r['opt']
        assert o['feasible'] and r['nan_trials'] == 0, f'{name} group {g}'
        wp = max(wp, M.pose_difference(r['T'], o['T']))
        wa = max(wa, float(np.abs(r['angles'] - o['q']).max()))
        wf = max(wf, abs(r['fvals'][1] / o['f'] - 1))
    print(f'restated loop against scipy over {len(_fitted())} groups: pose {wp:.3e}, angles {wa:.3e}, F / F_ls - 1 {wf:.3e}')
    _recorded(wp, J.JOINT_POSE_BOUND, 'pose')
    _recorded(wa, J.JOINT_ANGLE_BOUND, 'angles')
    _recorded(wf, J.JOINT_F_BOUND, 'F')


def test_stiff_weights_give_the_fixed_angle_optimum():
    worst = 0.0
    for name in ('two frames', 'three frames, tails', 'WAVES + 1 frames', 'gate 4 px'):
        case = J.cases()[name]
        kw = dict(swap=case['swap'], min_cos=case['min_cos'], sel_cos=case['sel_cos'], gate_px=case['gate_px'])
        fixed = M.ref_group(case['fr1'], case['fr2'], case['TAGV'], case['x0'][0], case['table'], **kw)
        stiff = J.ref_group(case['fr1'], case['fr2'], case['angles'], case['x0'][0], case['table'], 1e9, 1e9, **kw)
        assert fixed['status'] == stiff['status'] == J.ST_OK and all(np.array_equal(a, b) for a, b in zip(fixed['S'], stiff['S']))
        assert np.abs(stiff['angles'] - case['angles']).max() < 1e-12
        worst = max(worst, M.pose_difference(fixed['T'], stiff['T']))
    print(f'both weights 1e9 against the fixed-angle reference: pose {worst:.3e}')
    _recorded(2 * worst, J.JOINT_FIXED_BOUND, 'stiff weights')


def test_level_of_the_blocks():
    worst = 0.0
    for name, g, r in _fitted():
        U, gx, V, W, gq = r['grp'].blocks(r['x'], r['angles'], r['S'])
        Ul, _, Vl, Wl, _ = r['grp'].blocks(r['x'], r['angles'], r['S'], dtype=np.longdouble)
        Nl = Ul.copy()
        for v, w in zip(Vl, Wl):
            det = v[0, 0] * v[1, 1] - v[0, 1] * v[0, 1]
            Nl = Nl - w @ (np.array([[v[1, 1], -v[0, 1]], [-v[0, 1], v[0, 0]]], np.longdouble) / det) @ w.T
        N = J.reduced(U, V, W)
        dn = np.sqrt(np.diag(Nl).astype(np.float64))
        worst = max(worst, float((np.abs((N - Nl).astype(np.float64)) / (dn[:, None] * dn[None, :])).max()))
        for v, w, vl, wl in zip(V, W, Vl, Wl):
            dv = np.sqrt(np.diag(vl).astype(np.float64))
            worst = max(worst, float((np.abs((v - vl).astype(np.float64)) / (dv[:, None] * dv[None, :])).max()),
                        float((np.abs((w - wl).astype(np.float64)) / (dn[:, None] * dv[None, :])).max()))
    print(f'N, V and W in float64 against long double: {worst:.3e} of the square root of the two diagonal entries')
    assert 16 * worst <= J.JOINT_N_BOUND <= 64 * worst


def test_acceptance_on_perturbed_scenes():
    for F, seed in J.ACCURACY_RUNS:
        run = J.accuracy_run(F, seed)
        assert run['fixed']['status'] == run['joint']['status'] == J.ST_OK and run['joint']['nan_trials'] == 0
        ef, ej = run['err_fixed'], run['err_joint']
        Tt = M.TTRUE
        pf, pj = (np.degrees(LM.rotation_between(Tt[:3, :3], r['T'].reshape(4, 4)[:3, :3])) for r in (run['fixed'], run['joint']))
        tf, tj = (float(np.linalg.norm(Tt[:3, 3] - r['T'].reshape(4, 4)[:3, 3])) for r in (run['fixed'], run['joint']))
        print(f'F = {F:2d} seed {seed}: fixed {run["px_fixed"]:.3f} px {ef[0]:.4f} deg {ef[1]:.4f} mm angles {run["angle_rms_fixed"]:.5f} rad '
              f'T {pf:.3f} deg {tf:.3f} mm; joint {run["px_joint"]:.3f} px {ej[0]:.4f} deg {ej[1]:.4f} mm angles {run["angle_rms_joint"]:.5f} rad '
              f'T {pj:.3f} deg {tj:.3f} mm; iterations {run["joint"]["iters"][0]}')
        assert ej[0] < ef[0] and ej[1] < ef[1], f'F = {F} seed {seed}: the joint fit\'s frame axes are not nearer'
        assert run['px_joint'] < 0.40
        assert run['angle_rms_joint'] < run['angle_rms_fixed']


def test_exact_angles_cost_a_stated_multiple():
    worst = np.zeros(2)
    for F, seed in J.ACCURACY_RUNS:
        run = J.accuracy_run(F, seed, exact=True)
        assert run['fixed']['status'] == run['joint']['status'] == J.ST_OK
        ratio = np.array(run['err_joint']) / np.array(run['err_fixed'])
        print(f'exact angles, F = {F:2d} seed {seed}: fixed {run["err_fixed"][0]:.4f} deg {run["err_fixed"][1]:.4f} mm; joint {run["err_joint"][0]:.4f} deg '
              f'{run["err_joint"][1]:.4f} mm; ratio {ratio[0]:.2f} {ratio[1]:.2f}; {run["px_joint"]:.3f} px')
        worst = np.maximum(worst, ratio)
    assert (worst <= J.EXACT_MULTIPLE).all(), f'{worst} above the stated {J.EXACT_MULTIPLE}'
    assert (2 * worst > 0.9 * np.array(J.EXACT_MULTIPLE)).all(), 'the recorded multiple is not twice the worst any more'
