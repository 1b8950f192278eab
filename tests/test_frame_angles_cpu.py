"""The numpy restatement of the frame-angle solver (tests/frame_angles_cases.py) against the oracle's chain, central
differences and scipy, and the finding that shapes the interface: a two-angle LM started at (0, 0) ends in a second minimum
for some frames, the closed-form start does not.  Run with -s for the measured figures.

Measured on the 360 frame fits (make_scene(12, seed, noise), seeds 0-9, noise 0 / 0.05 / 0.3, counts 5 ... 2048), the start made
from a direction 0.02 rad off the true axis, chain derivatives in closed form:
    start up to 0.0203 rad from the truth; <= 4 iterations, <= 16 evaluations
    to scipy's optimum: angles 1.6e-8 rad, f relative excess 2.8e-11 (the frames with noise)
    to the truth: 7.2e-12 rad without noise, 7.2e-4 rad at 0.05 mm, 4.3e-3 rad at 0.3 mm
    closed-form columns against the oracle's chain: 0.5 ulp of 1 (direction), 0.75 ulp of its scale (column 4)
    from (0, 0): 30 of 360 end 0.35-0.46 rad from the truth; from the closed-form start: 0 of 360"""
import math
import os
import re

import numpy as np
import pytest

import frame_angles_cases as fc
import multiframe_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ('cpe_agv_chain_batch', 'cpe_frame_angles_lm_batch')


@pytest.fixture(scope='module')
def angle_pairs():
    """1000 pairs: pan over (-1.5, 1.5), tilt over (-1.2, 1.2), with 0, +-tiny and |tilt| near 1 among them"""
    rng = np.random.default_rng(7)
    q = np.stack([rng.uniform(-1.5, 1.5, 1000), rng.uniform(-1.2, 1.2, 1000)], 1)
    q[:8] = [[0, 0], [1e-300, -1e-300], [-1e-9, 1e-9], [0.3, 1.0], [-0.3, -1.0], [1.5, 1.2], [-1.5, -1.2], [0, 1e-17]]
    return q


@pytest.fixture(scope='module')
def fits():
    """the 360 frame fits, each with the restatement's result from its closed-form start and scipy's optimum from the truth"""
    out = fc.frame_fits()
    for s in out:
        s['lm'] = fc.lm(s['prob'], s['start'])
        s['ls'] = fc.scipy_optimum(s['prob'], s['truth'])
    return out


def test_header_and_loader_declare_the_exports(cpe):
    hdr = open(os.path.join(ROOT, 'include', 'cpe.h')).read()
    for name in EXPORTS:
        assert re.search(r'CPE_API\s+int32_t\s+' + name + r'\s*\(', hdr), f'{name} is not declared in include/cpe.h'
        assert name in cpe.lib._SIGS, f'{name} is not listed in cpe_amd/lib.py'
        assert name in cpe.lib.declared_symbols()
    assert 'BUILD-DEFINED' in hdr[hdr.index('cpe_agv_chain_batch('):]
    assert int(re.search(r'#define CPE_VERSION (\d+)', hdr).group(1)) >= 114
    assert callable(cpe.multiframe.agv_chain_batch) and callable(cpe.multiframe.estimate_frame_angles_gpu)


def test_closed_form_columns_equal_the_oracle_chain(orc, angle_pairs):
    """4 ulp of the entry's scale: 1 for the direction column, for column 4 the lengths it is made of, 574.2 + 143.1 |tan(tilt)|"""
    a, p = fc.chain_columns(angle_pairs[:, 0], angle_pairs[:, 1])
    worst_a = worst_p = 0.0
    for i, (pan, tilt) in enumerate(angle_pairs):
        A = orc.get_TAGVcyl(float(pan), float(tilt)).reshape(4, 4)
        assert np.array_equal(A[3], [0, 0, 0, 1])
        ea = np.abs(a[i] - A[:3, 1]).max() / np.spacing(1.0)
        ep = np.abs(p[i] - A[:3, 3]).max() / np.spacing(fc.LINKS + 143.1 * abs(math.tan(tilt)))
        worst_a, worst_p = max(worst_a, ea), max(worst_p, ep)
    print(f'closed-form columns against oracle.get_TAGVcyl: direction {worst_a:.2f} ulp of 1, column 4 {worst_p:.2f} ulp of its scale')
    assert worst_a <= 4 and worst_p <= 4


def test_closed_form_derivatives_match_central_differences(angle_pairs):
    """h = 1e-5: truncation h^2/6 |f'''|, with |f'''| <= 1 for the direction and <= 431 + 143.1 (2 sec^4 + 4 sec^2 tan^2) <= 4.6e4
    for column 4 at |tilt| <= 1.2, is 1.7e-11 and 7.7e-7; rounding eps scale / h is 1e-11 and 1e-8.  Bounds 1e-9 and 1e-5."""
    h = 1e-5
    pan, tilt = angle_pairs[:, 0], angle_pairs[:, 1]
    da_pan, da_tilt, dp_pan, dp_tilt = fc.chain_derivatives(pan, tilt)
    num = lambda k, dpan, dtilt: (fc.chain_columns(pan + dpan, tilt + dtilt)[k] - fc.chain_columns(pan - dpan, tilt - dtilt)[k]) / (2 * h)
    errs = dict(da_pan=np.abs(da_pan - num(0, h, 0)).max(), da_tilt=np.abs(da_tilt - num(0, 0, h)).max(),
                dp_pan=np.abs(dp_pan - num(1, h, 0)).max(), dp_tilt=np.abs(dp_tilt - num(1, 0, h)).max())
    print('closed-form derivatives against central differences:', {k: f'{v:.3g}' for k, v in errs.items()})
    assert errs['da_pan'] <= 1e-9 and errs['da_tilt'] <= 1e-9
    assert errs['dp_pan'] <= 1e-5 and errs['dp_tilt'] <= 1e-5


def test_residual_jacobian_matches_central_differences():
    """the chained Jacobian of the residuals, on three frames of one scene.  h = 1e-6: third derivatives of a residual are of
    the order of the lever arm (574 mm) / sqrt(n), so truncation and rounding (1e-16 * 45 / 1e-6) stay below 1e-6 (1 + max|J|)"""
    P, cnt, angles, Ttrue = mc.make_scene(3, 5, 0.05)
    h = 1e-6
    for i in range(3):
        prob = fc.FrameProblem(P[i, :cnt[i]], Ttrue)
        q = angles[i] + [0.01, -0.02]
        _, J = prob.residuals_jacobian(q)
        for k in range(2):
            dq = np.zeros(2); dq[k] = h
            num = (prob.residuals(q + dq) - prob.residuals(q - dq)) / (2 * h)
            err = np.abs(J[:, k] - num).max()
            print(f'frame {i} column {k}: max|J| {np.abs(J[:, k]).max():.4g} error {err:.3g}')
            assert err <= 1e-6 * (1 + np.abs(J).max())


def test_start_formula_inverts_the_chain_axis(angle_pairs):
    """the start made from the chain's own axis (either sign) is the angle pair, for any pose: 1e-12 covers asin / atan2 of
    entries a few ulp off at |tilt| <= 1.2 (d asin = eps / cos(tilt) <= 3 eps)"""
    _, _, _, Ttrue = mc.make_scene(1, 0, 0.0)
    worst = 0.0
    for i, (pan, tilt) in enumerate(angle_pairs):
        A = mc.get_TAGVcyl(pan, tilt)
        assert np.abs(A[:3, 1] - fc.chain_columns(pan, tilt)[0]).max() <= 4 * np.spacing(1.0)
        for T in (np.eye(4), Ttrue):
            d = (T @ A)[:3, 1] * (1.0 if i % 2 else -1.0) * (1 + i % 3)
            worst = max(worst, fc.angle_distance(fc.start_from_direction(T, d), (pan, tilt)))
    print(f'start formula against the angles the axis was made from: {worst:.3g} rad')
    assert worst <= 1e-12


def test_restatement_against_scipy(fits):
    start_off = max(fc.angle_distance(s['start'], s['truth']) for s in fits)
    dq = max(fc.angle_distance(s['lm'][0], s['ls'][0]) for s in fits)
    df = max(s['lm'][1] / s['ls'][1] - 1 for s in fits if s['noise'] > 0)
    iters, evals = max(s['lm'][2] for s in fits), max(s['lm'][3] for s in fits)
    print(f'{len(fits)} frame fits: start up to {start_off:.3g} rad off; to scipy: angles {dq:.3g} rad, f relative excess {df:.3g}; '
          f'iterations <= {iters}, evaluations <= {evals}')
    for noise in fc.FIT_NOISES:
        print(f'  noise {noise}: to the truth {max(fc.angle_distance(s["lm"][0], s["truth"]) for s in fits if s["noise"] == noise):.3g} rad')
    assert len(fits) == 360
    for s in fits:
        assert fc.angle_distance(s['lm'][0], s['ls'][0]) <= 1e-5
        if s['noise'] == 0:                     # both are rounding residue there: tol_f 1e-3, as the multi-frame LM test
            assert s['lm'][1] <= 1e-8
        else:
            assert s['lm'][1] <= s['ls'][1] * (1 + 1e-6)


def test_noise_free_fits_reach_the_truth(fits):
    clean = [s for s in fits if s['noise'] == 0]
    assert len(clean) == 120
    worst = max(fc.angle_distance(s['lm'][0], s['truth']) for s in clean)
    print(f'noise-free: {worst:.3g} rad from the true angles')
    assert worst <= 1e-5


def test_zero_start_ends_in_a_second_minimum(fits):
    """a documented fact, not a requirement on the solver: why a missing start must never mean (0, 0)"""
    far = lambda q, s: fc.angle_distance(q, s['truth']) > 0.1
    zero = [(fc.lm(s['prob'], [0.0, 0.0])[0], s) for s in fits]
    lost = [fc.angle_distance(q, s['truth']) for q, s in zero if far(q, s)]
    closed = sum(far(s['lm'][0], s) for s in fits)
    print(f'start (0, 0): {len(lost)} of {len(fits)} frame fits end {min(lost, default=0):.2f}-{max(lost, default=0):.2f} rad from the truth; '
          f'closed-form start: {closed} of {len(fits)}')
    assert len(lost) > 0
    assert closed == 0


def test_gpu_scenes_meet_the_condition_on_their_input(orc):
    """every frame of every scene of test_frame_angles_gpu.py has a per-frame fit within AXIS_OFF of its true axis, and each seed
    is the first that does (frame_angles_cases.GPU_SEEDS)"""
    def worst(F, seed, noise):
        P, cnt, angles, Ttrue = mc.make_scene(F, seed, noise)
        w = 0.0
        for i in sorted(range(F), key=lambda i: cnt[i]):
            r = orc.fit_cylinder(P[i, :cnt[i]], mc.RADIUS)
            assert r['status'] == 0
            w = max(w, fc.axis_off(Ttrue, angles[i], r['cyl'][3:6]))
            if w > fc.AXIS_OFF:
                break
        return w
    for (F, noise), seed in fc.GPU_SEEDS.items():
        w = worst(F, seed, noise)
        print(f'F = {F} noise {noise} seed {seed}: fitted axes within {w:.3g} rad of the true ones')
        assert w <= fc.AXIS_OFF
        if seed and F < 65:                                  # (the 65-frame seeds were found by this search, 177 and 188 scenes long)
            assert all(worst(F, s, noise) > fc.AXIS_OFF for s in range(seed))


def test_five_points_do_not_pin_the_axis_down(orc):
    """a documented limit of the closed-form start: the per-frame fit of a 5-point frame can end far from the true axis (four
    unknowns, five points), the start made from it is then far off and the solver ends in another minimum; the nominal angle as
    the start reaches the truth"""
    c = fc.FAR_FIT
    P, cnt, angles, Ttrue = mc.make_scene(c['F'], c['seed'], c['noise'])
    i = c['frame']
    assert cnt[i] == 5
    r = orc.fit_cylinder(P[i, :5], mc.RADIUS)
    off = fc.axis_off(Ttrue, angles[i], r['cyl'][3:6])
    prob = fc.FrameProblem(P[i, :5], Ttrue)
    start = fc.start_from_direction(Ttrue, r['cyl'][3:6])
    q, f, _, _ = fc.lm(prob, start)
    nominal = np.deg2rad(np.round(np.rad2deg(angles[i])))
    qn, fn, _, _ = fc.lm(prob, nominal)
    far = [fc.axis_off(T, a[k], orc.fit_cylinder(Pk[k, :5], mc.RADIUS)['cyl'][3:6])
           for seed in range(20) for noise in (0.0, 0.05) for Pk, ck, a, T in [mc.make_scene(12, seed, noise)] for k in (0, 6)]
    print(f'5-point frame: fitted axis {off:.3g} rad from the true one (per-frame f = {r["fvals"][1]:.3g}), start {fc.angle_distance(start, angles[i]):.3g} '
          f'rad off -> result {fc.angle_distance(q, angles[i]):.3g} rad off (f = {f:.3g}); from the nominal angle {fc.angle_distance(qn, angles[i]):.3g} rad; '
          f'{sum(v > fc.AXIS_OFF for v in far)} of {len(far)} 5-point frames are fitted more than {fc.AXIS_OFF} rad off, the worst {max(far):.3g}')
    assert off > 1.0
    assert fc.angle_distance(q, angles[i]) > 0.1
    assert fc.angle_distance(qn, angles[i]) <= 1e-5
