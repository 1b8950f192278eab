"""The reference and the cases of tests/proj_model_cases.py, without a GPU: the reference recovers truth, its tolerances and
margins are what the GPU comparison needs, the noisy bounds are what the module records, and the shifted frames are trimmed
exactly."""
import numpy as np
import pytest

import plane_fit_cases as PC
import proj_model_cases as M


def test_noise_free_tables_give_the_true_model():
    for frames in ([dict(X=f['Xtrue'], idx=f['idx']) for f in PC.multi_pose(0)[:3]], M._plain(M.cylinder_frames(0, 4, 0.0))):
        X, I, cnt = PC.pack(frames)
        ref = M.ref_projector_model(X, I, cnt, -12, 12)
        assert ref['status'] == M.ST_OK and ref['f'] <= 1e-18
        assert np.abs(ref['x'] - M.true_model()).max() <= 1e-9
        # the closed-form start is exact on such tables already
        s = M.start(M._lines(ref['R'], ref['keep'], 1e-4))
        e = M.model_errors(s)
        assert e['normal_deg'] <= 1e-9 and e['offset_mm'] <= 1e-9
    # the cylinder frames hold no negative column, and the model has their planes
    assert min(int(f['idx'][:, 0].min()) for f in M.cylinder_frames(0)) == 0


@pytest.mark.parametrize('name', list(M.cases()))
def test_case_reference(name):
    ref = M.reference(name)
    case = M.cases()[name]
    assert (ref['status'] == M.ST_FEW_POINTS) == (name in M.FEW)
    if name in M.FEW:
        assert not ref['x'].any()
        return
    assert ref['margin'] > 1e-6, f'{name}: a residual within {ref["margin"]:.2e} of tau'
    if name in M.GAUGE:
        assert ref['cond'] > 1e12
        return
    assert ref['tol'] <= 1e-6, f'{name}: tolerance {ref["tol"]:.2e}'
    step, _ = M.gn_step(ref['R'], ref['keep'], ref['x'])
    assert np.abs(step).max() <= 1e-12
    for k in range(2):
        assert abs(np.linalg.norm(ref['x'][3 + 6 * k:6 + 6 * k]) - 1) <= 4 * M.EPS
    assert ref['kept'].sum() == ref['frame_counts'][:, [0, 2]].sum() == ref['count'].sum() == ref['mask'].sum()
    if 'x0' in case:
        assert np.abs(ref['x'] - M.reference('boards 3')['x']).max() <= ref['tol']        # another start, the same optimum


def test_noisy_bounds_are_twice_the_measured_values():
    for kind in ('boards', 'cyl'):
        worst = dict(normal_deg=0.0, offset_mm=0.0)
        for seed in M.NOISY_SEEDS:
            e = M.model_errors(M.noisy_reference(kind, seed)['x'])
            worst = {k: max(worst[k], e[k]) for k in worst}
        print(kind, worst)
        for k, w in worst.items():
            assert 0.45 * M.NOISY_BOUNDS[kind][k] <= w <= 0.55 * M.NOISY_BOUNDS[kind][k], f'{kind} {k}: measured {w:.4f}, recorded {M.NOISY_BOUNDS[kind][k] / 2:.4f}'


def test_shifted_frames_are_trimmed_exactly():
    ref, clean = M.reference('shifted'), M.reference('cylinder 12')
    fc = ref['frame_counts']
    assert ref['rounds'] == 2
    for f in range(len(fc)):
        n = len(M.cylinder_frames(0)[f]['X'])
        assert fc[f].tolist() == ([0, n, n, 0] if f in M.SHIFTED else [n, 0, n, 0])
    # what is left is the clean fit without the two frames' column residuals: as close to truth as the clean fit
    e, ec = M.model_errors(ref['x']), M.model_errors(clean['x'])
    assert e['normal_deg'] <= M.NOISY_BOUNDS['cyl']['normal_deg'] and e['offset_mm'] <= M.NOISY_BOUNDS['cyl']['offset_mm']
    assert ec['normal_deg'] <= M.NOISY_BOUNDS['cyl']['normal_deg']
    # and without the band the two frames ruin it
    assert M.model_errors(M.reference('shifted 0 rounds')['x'])['normal_deg'] > 1.0
    # a clean table loses nothing to the band
    assert not M.reference('trimmed clean')['frame_counts'][:, [1, 3]].any()
