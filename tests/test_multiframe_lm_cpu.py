"""Why the multi-frame fit has an LM form, on the CPU: on synthetic scenes the reference-faithful path (the initial pose of
fitCylinderWPts3sAngs.m:40-69 with the linear-indexing quirk, then fminsearch -- orc.multi_fit) does not reach the true pose,
the all-frame initial pose + LM (multiframe_lm_cases, the numpy restatement of cpe_multi_frame_fit_lm_batch) does.

The bounds: f <= f(Ttrue), because Ttrue is a feasible pose and the minimiser must not end above it; f <= f_ls (1 + 1e-6) with
f_ls scipy's least_squares(method='lm', xtol = ftol = 1e-14) from Ttrue, the figure the per-frame LM test uses; on the
noise-free scene f <= tol_f 1e-3 = 1e-8, which is what the stop rule resolves.  `pytest -s` prints the table of DESIGN 3.7."""
import numpy as np
import pytest

import multiframe_cases as mc
import multiframe_lm_cases as lc

SEEDS = range(10)


def per_frame_fits(orc, P, cnt):
    raw = np.zeros((len(cnt), 2, 6))
    for i in range(len(cnt)):
        r = orc.fit_cylinder(P[i, :cnt[i]], mc.RADIUS)
        raw[i, 0], raw[i, 1] = r['cyl0'], r['cyl']
    return raw


def solve(orc, P, cnt, angles, Ttrue):
    TAGV = np.stack([orc.get_TAGVcyl(*a) for a in angles])
    raw = per_frame_fits(orc, P, cnt)
    prob = lc.Problem(P, cnt, TAGV)
    got = lc.fit(prob, raw)
    assert got is not None
    _, f_ls = lc.scipy_optimum(prob, Ttrue)
    return dict(TAGV=TAGV, raw=raw, prob=prob, got=got, f_ls=f_ls, f_true=prob.f(lc.T2vec(Ttrue)))


@pytest.mark.parametrize('seed', SEEDS)
def test_faithful_path_misses_and_lm_finds_the_pose(orc, seed):
    P, cnt, angles, Ttrue = mc.make_scene(12, seed, 0.05, npts=200)
    s = solve(orc, P, cnt, angles, Ttrue)
    nm = orc.multi_fit(P, cnt, s['TAGV'], s['raw'], mc.RADIUS)
    nm_deg, lm_deg = lc.rotation_error_deg(nm['T'], Ttrue), lc.rotation_error_deg(s['got']['T'], Ttrue)
    f = s['got']['fvals'][1]
    print(f'seed {seed}: faithful x0 f0 {nm["fvals"][0]:.3g} -> Nelder-Mead f {nm["fvals"][1]:.3g}, {nm_deg:.1f} deg off, {nm["iters"]} iterations '
          f'{nm["evals"]} evaluations | all-frame x0 f0 {s["got"]["fvals"][0]:.3g} -> LM f {f!r}, f_ls {s["f_ls"]!r}, f(Ttrue) {s["f_true"]!r}, '
          f'{lm_deg:.4f} deg and {np.linalg.norm(s["got"]["T"][:3, 3] - Ttrue[:3, 3]):.3f} mm off, {s["got"]["iters"]} iterations '
          f'{s["got"]["evals"]} evaluations')
    assert nm_deg > 10.0
    assert f <= s['f_true']
    assert f <= s['f_ls'] * (1 + 1e-6)


@pytest.mark.parametrize('name', sorted(mc.CASES))
def test_lm_on_the_gpu_scenes(orc, name):
    s = solve(orc, *mc.case_scene(name))
    f = s['got']['fvals'][1]
    print(f'{name}: f0 {s["got"]["fvals"][0]:.3g} f {f!r} f_ls {s["f_ls"]!r} f(Ttrue) {s["f_true"]!r} iterations {s["got"]["iters"]} '
          f'evaluations {s["got"]["evals"]}')
    if mc.CASES[name]['noise'] == 0:
        assert f <= 1e-8
    else:
        assert f <= s['f_true']
        assert f <= s['f_ls'] * (1 + 1e-6)


def test_jacobian_of_the_restatement():
    """the analytic Jacobian against central differences of the residuals along the LM's own perturbation"""
    P, cnt, angles, Ttrue = mc.case_scene('F3')
    prob = lc.Problem(P, cnt, np.stack([mc.get_TAGVcyl(*a) for a in angles]))
    x = lc.T2vec(Ttrue) + np.array([0.01, -0.02, 0.015, 0.5, -0.3, 0.8])
    T = lc.vec2T(x)
    _, J = prob.residuals_jacobian(x)
    h = 1e-6
    for k in range(6):
        d = np.zeros(6); d[k] = h
        moved = []
        for sgn in (1, -1):
            Tn = np.eye(4)
            Tn[:3, :3] = lc.rot_exp(sgn * d[:3]) @ T[:3, :3]
            Tn[:3, 3] = T[:3, 3] + sgn * d[3:]
            moved.append(prob.residuals(lc.T2vec(Tn)))
        num = (moved[0] - moved[1]) / (2 * h)
        assert np.abs(num - J[:, k]).max() <= 1e-6 * max(1.0, np.abs(J[:, k]).max())


def test_header_and_sigs_declare_the_lm_entry_point(cpe):
    assert 'cpe_multi_frame_fit_lm_batch' in cpe.lib.declared_symbols()
    res, args = cpe.lib._SIGS['cpe_multi_frame_fit_lm_batch']
    assert len(args) == len(cpe.lib._SIGS['cpe_multi_frame_fit_batch'][1]) + 1
