"""cpe_fit_plane_batch and cpe_index_planes_batch (csrc/fit.hip k_fit_plane, k_index_planes, k_planes_centre) against the numpy
reference of tests/plane_fit_cases.py at the tolerances derived there; masks, counts, flags and statuses exactly."""
import ctypes as C

import numpy as np
import pytest
import torch

import plane_fit_cases as PC

pytestmark = pytest.mark.gpu

FIT_KEYS = ('P', 'T', 'grid', 'stats', 'n_inliers', 'inlier_mask', 'plane_flags', 'status')


def _fit(cpe, gpu, frames, tau, max_rounds=4, poison=None):
    X, I, cnt = (torch.from_numpy(a).to(gpu) for a in PC.pack(frames, poison))
    out = cpe.fit.fit_plane_batch(X, I, cnt, tau=tau, max_rounds=max_rounds)
    torch.cuda.synchronize()
    return {k: out[k].cpu().numpy() for k in FIT_KEYS}


def _frame(out, i):
    return dict(P=out['P'][i], T=out['T'][i], grid=out['grid'][i], stats=out['stats'][i], n_inliers=out['n_inliers'][i],
                mask=out['inlier_mask'][i], flags=out['plane_flags'][i], status=out['status'][i])


@pytest.mark.parametrize('tau', [0.0, PC.TAU], ids=['fitplane', 'trimmed'])
def test_fit_plane_batches_of_1_3_65(cpe, gpu, tau):
    seen = set()
    for names, frames in PC.batches(tau):
        a = _fit(cpe, gpu, frames, tau, poison=41)          # NaN, infinities and garbage indices past every count
        b = _fit(cpe, gpu, frames, tau)                     # zeros there
        for k in FIT_KEYS:
            assert a[k].tobytes() == b[k].tobytes(), f'{k} depends on slots past the count'
        for i, name in enumerate(names):
            ref = PC.fit_reference(tau, name)
            g = _frame(a, i)
            if ref['status'] == 0:
                print(f'{name}: normal {PC.angle(g["P"][:3], ref["P"][:3]):.2e} / {ref["tol_angle"]:.2e}  P4 {abs(g["P"][3] - ref["P"][3]):.2e} / '
                      f'{ref["tol_off"]:.2e}  grid {np.abs(g["grid"] - ref["grid"]).max():.2e} / {ref["tol_grid"]:.2e}')
            PC.compare_fit(g, ref, f'{name} (frame {i} of {len(names)})')
            seen.add(name)
    assert seen == set(PC.fit_cases(tau))


def test_trimming_stops_after_max_rounds(cpe, gpu):
    fr, tau = PC.slow_trim_case()
    for mr, refits in ((0, 0), (2, 2), (4, 4), (8, 5)):
        ref = PC.ref_fit_plane(fr['X'], fr['idx'], len(fr['X']), tau, mr)
        assert ref['stats'][6] == refits
        PC.compare_fit(_frame(_fit(cpe, gpu, [fr], tau, mr, poison=3), 0), ref, f'max_rounds {mr}')


def _raw_fit(cpe, gpu, X, I, cnt, prm):
    n = len(cnt)
    o = dict(P=torch.full((n, 4), 7.0, dtype=torch.float64, device=gpu), T=torch.full((n, 16), 7.0, dtype=torch.float64, device=gpu),
             grid=torch.full((n, 9), 7.0, dtype=torch.float64, device=gpu), stats=torch.full((n, 8), 7.0, dtype=torch.float64, device=gpu),
             ninl=torch.full((n,), 7, dtype=torch.int32, device=gpu), mask=torch.full((n, PC.MAXP), 7, dtype=torch.uint8, device=gpu),
             flags=torch.full((n,), 7, dtype=torch.int32, device=gpu), st=torch.full((n,), 7, dtype=torch.int32, device=gpu))
    rc = cpe.lib.load().cpe_fit_plane_batch(X.data_ptr(), I.data_ptr(), cnt.data_ptr(), n, None if prm is None else C.addressof(prm),
                                            *(o[k].data_ptr() for k in ('P', 'T', 'grid', 'stats', 'ninl', 'mask', 'flags', 'st')),
                                            torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, o


def test_null_params_are_the_defaults_and_every_output_is_written(cpe, gpu):
    """outputs pre-filled with 7: a failed frame is zeroed, the mask is written to the end of the table"""
    fr, _ = PC.slow_trim_case()
    frames = [fr, PC.fit_cases(0.0)['collinear'], PC.fit_cases(0.0)['count 0']]
    X, I, cnt = (torch.from_numpy(a).to(gpu) for a in PC.pack(frames, poison=5))
    rc, o = _raw_fit(cpe, gpu, X, I, cnt, None)
    assert rc == 0
    want = _fit(cpe, gpu, frames, 0.0, 4, poison=5)
    for k, w in (('P', 'P'), ('T', 'T'), ('grid', 'grid'), ('stats', 'stats'), ('ninl', 'n_inliers'), ('mask', 'inlier_mask'),
                 ('flags', 'plane_flags'), ('st', 'status')):
        assert o[k].cpu().numpy().tobytes() == want[w].tobytes(), k
    assert want['status'].tolist() == [0, 5, 5] and not want['inlier_mask'][1:].any() and not want['P'][1:].any()
    for bad in (cpe.lib.CpePlaneFitParams(0.5, -1, 0), cpe.lib.CpePlaneFitParams(0.5, 65, 0), cpe.lib.CpePlaneFitParams(float('nan'), 4, 0)):
        rc, _ = _raw_fit(cpe, gpu, X, I, cnt, bad)
        assert rc == -1
    with pytest.raises(cpe.lib.CpeError):
        cpe.fit.fit_plane_batch(X, I, cnt, tau=1.0, max_rounds=65)
    z = torch.zeros(0, dtype=torch.int32, device=gpu)
    assert cpe.fit.fit_plane_batch(X[:0], I[:0], z)['P'].shape == (0, 4)


def test_fit_single_plane_equals_selector_plus_fit(cpe, gpu, orc):
    K1, K2, T21 = PC.rig()[:3]
    boards = [PC.board(10.0, -20.0, 340.0), PC.board(-22.0, 5.0, 390.0), PC.board(0.0, 0.0, 365.0)]
    pairs = [PC.stereo_tables(n, P4, seed=50 + i) for i, (n, P4) in enumerate(boards)]
    pairs.append((pairs[0][0][:0], pairs[0][1]))                                     # an empty left table
    g1 = cpe.fit.GridTables.from_lists([p[0] for p in pairs], gpu)
    g2 = cpe.fit.GridTables.from_lists([p[1] for p in pairs], gpu)
    for kw in (dict(), dict(tau=0.6, max_rounds=3, selector=cpe.fit.SEL_THRESHOLD, th=0.5)):
        out = cpe.fit.fit_single_plane_batch(g1, g2, K1, K2, T21, **kw)
        sel = cpe.fit.select_triangulate_batch(g1, g2, K1, K2, T21, kw.get('selector', cpe.fit.SEL_CHOOSE_IDX), 3, kw.get('th', 0.3))
        fit = cpe.fit.fit_plane_batch(sel['pts3'], sel['idx'], sel['m'], tau=kw.get('tau', 0.0), max_rounds=kw.get('max_rounds', 4))
        torch.cuda.synchronize()
        for k in ('p1', 'p2', 'idx', 'pts3', 'err', 'm', 'mean_err', 'flags'):
            assert torch.equal(out[k], sel[k]), k
        for k in FIT_KEYS:
            assert out[k].cpu().numpy().tobytes() == fit[k].cpu().numpy().tobytes(), k
        assert out['status'].tolist() == [0, 0, 0, 5] and out['m'][3] == 0
        X, I, m = (sel[k].cpu().numpy() for k in ('pts3', 'idx', 'm'))
        got = {k: fit[k].cpu().numpy() for k in FIT_KEYS}
        for i, (n, P4) in enumerate(boards):
            ref = PC.ref_fit_plane(X[i], I[i], m[i], kw.get('tau', 0.0), kw.get('max_rounds', 4))
            assert ref['margin'] > 1e-6 and ref['n_inliers'] > 300
            PC.compare_fit(_frame(got, i), ref, f'board {i}')
            assert np.degrees(PC.angle(ref['P'][:3], n)) <= PC.NOISY_BOUNDS['normal_deg']


# ------------------------------------------------------------------------------------------------------ laser planes
def _index(cpe, gpu, case, poison=None, **kw):
    X, I, cnt, use, ok = PC.index_case_arrays(case, poison)
    t = lambda a: None if a is None else torch.from_numpy(a).to(gpu)
    out = cpe.fit.index_planes_batch(t(X), t(I), t(cnt), case['lo'], case['hi'], use=t(use), frame_ok=t(ok), **kw)
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


@pytest.mark.parametrize('name', list(PC.index_cases()))
def test_index_planes_against_reference(cpe, gpu, name):
    case = PC.index_cases()[name]
    ref = PC.index_reference(name)
    a, b = _index(cpe, gpu, case, poison=13), _index(cpe, gpu, case)
    for k in ('P', 'stats', 'count', 'frames', 'status', 'centre', 'centre_status'):
        assert a[k].tobytes() == b[k].tobytes(), f'{k} depends on slots past the count'
    ok = ref['status'] == 0
    if ok.any():
        ang = max(PC.angle(a['P'][k, j, :3], ref['P'][k, j, :3]) for k in range(2) for j in range(ok.shape[1]) if ok[k, j])
        print(f'{name}: worst normal {ang:.2e} / {ref["tol_angle"][ok].min():.2e}  centre {np.abs(a["centre"] - ref["centre"]).max():.2e} / '
              f'{ref["tol_centre"]:.2e}')
    PC.compare_index_planes(a, ref, name)


def test_index_planes_refuses_a_bad_range(cpe, gpu):
    case = PC.index_cases()['2 frames']
    X, I, cnt = (torch.from_numpy(a).to(gpu) for a in PC.pack(case['frames']))
    with pytest.raises(ValueError):
        cpe.fit.index_planes_batch(X, I, cnt, -128, 128)              # L = 257
    with pytest.raises(ValueError):
        cpe.fit.index_planes_batch(X, I, cnt, 3, 2)
    L = cpe.lib.load()
    o = [torch.zeros(2 * 257 * 4, dtype=torch.float64, device=gpu) for _ in range(2)] + \
        [torch.zeros(2 * 257, dtype=torch.int32, device=gpu) for _ in range(3)] + \
        [torch.zeros(4, dtype=torch.float64, device=gpu), torch.zeros(1, dtype=torch.int32, device=gpu)]
    s = torch.cuda.current_stream().cuda_stream
    call = lambda lo, hi, spread: L.cpe_index_planes_batch(X.data_ptr(), I.data_ptr(), cnt.data_ptr(), 2, None, None, lo, hi, spread,
                                                           *(t.data_ptr() for t in o), s)
    assert call(-128, 128, 1e-4) == -1 and call(1, 0, 1e-4) == -1 and call(-2 ** 31, 2 ** 31 - 1, 1e-4) == -1
    assert call(0, 0, -1.0) == -1 and call(-128, 127, 1e-4) == 0
    torch.cuda.synchronize()


def test_min_spread_refuses_flat_lines(cpe, gpu):
    """lambda_mid / lambda_max of the 12-frame lines is 0.39 and more: a threshold of 0.5 and of 0.3 split them as the reference says"""
    case = PC.index_cases()['12 frames']
    X, I, cnt, _, _ = PC.index_case_arrays(case)
    for ms in (0.3, 0.5, 0.0):
        ref = PC.ref_index_planes(X, I, cnt, -12, 12, min_spread=ms)
        assert ref['spread_margin'] > 1e-6
        PC.compare_index_planes(_index(cpe, gpu, case, min_spread=ms), ref, f'min_spread {ms}')
    assert 0 < (PC.ref_index_planes(X, I, cnt, -12, 12, min_spread=0.5)['status'] == 0).sum() < 42


def test_twelve_noisy_frames_against_truth(cpe, gpu):
    """per-frame planes with the trimming on, the table over their inliers, the projector's centre: within the bounds measured on the
    reference (tests/plane_fit_cases.py)"""
    fr = PC.multi_pose(1)
    X, I, cnt = (torch.from_numpy(a).to(gpu) for a in PC.pack(fr))
    fit = cpe.fit.fit_plane_batch(X, I, cnt, tau=1.0)
    tab = cpe.fit.index_planes_batch(X, I, cnt, -12, 12, use=fit['inlier_mask'], frame_ok=(fit['status'] == 0).to(torch.int32))
    torch.cuda.synchronize()
    assert fit['status'].tolist() == [0] * 12 and (fit['n_inliers'] == 425).all() and int(tab['centre_status']) == 0
    st = tab['status'].cpu().numpy()
    assert (st == 0).sum() == 42
    e = PC.noisy_errors(fit['P'].cpu().numpy(), tab['P'].cpu().numpy(), st, tab['centre'].cpu().numpy(), fr, -12)
    print(e)
    for k, b in PC.NOISY_BOUNDS.items():
        assert e[k] <= b, (k, e[k], b)
