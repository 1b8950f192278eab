"""The cases and the numpy reference of tests/table_tri_cases.py, checked without a GPU: truth on exact inputs, the ceiling of
the derived tolerances, the margin of every decision from its gate, the measured noisy bounds, and fit.LaserTable."""
import numpy as np
import pytest

import plane_fit_cases as PC
import table_tri_cases as TC


def _all_references():
    c = TC.frame_cases()
    for name in c:
        for nb in (0, 1):
            yield f'{name} need_both {nb}', TC.frame_reference(name, nb)
    for name in TC.call_cases():
        for i, r in enumerate(TC.call_reference(name)):
            yield f'{name} frame {i}', r


@pytest.mark.parametrize('cam', [1, 2])
@pytest.mark.parametrize('swap', [0, 1])
def test_reference_returns_truth_on_exact_inputs(cam, swap):
    """true planes (all through the projector's centre) and exact pixels: the true points to 1e-9 mm, for either camera and
    either assignment of the families"""
    idx, X = TC.cylinder_hits()
    uv = PC.project_pair(X, 0.0, None)[cam - 1]
    t = TC.rig_table(-12, 12)
    if swap:
        t = TC.transposed(t)
    K, Tc = TC.camera(cam)
    r = TC.ref_table_triangulate(uv, idx, len(uv), K, Tc, t['P'], t['status'], t['lo'], t['hi'], swap=swap)
    assert r['m'] == len(X) >= 400 and r['counts'].tolist() == [len(X), len(X), 0, 0]
    assert np.array_equal(r['src'][:, 1], np.arange(len(X))) and (r['src'][:, 0] == 3).all() and np.array_equal(r['idx'], idx)
    err = np.linalg.norm(r['X'] - X, axis=1).max()
    print(f'camera {cam} swap {swap}: worst point error {err:.2e} mm, worst |res| {r["stats"][1]:.2e}')
    assert err <= 1e-9 and r['stats'][1] <= 1e-9
    # one plane alone gives the same point: the cut of the ray with it
    for bad in ((), tuple(range(-12, 13))):
        one = TC.with_status(t, bad0=bad if bad else tuple(range(-12, 13)), bad1=bad)
        r1 = TC.ref_table_triangulate(uv, idx, len(uv), K, Tc, one['P'], one['status'], one['lo'], one['hi'], swap=swap)
        if bad:
            assert r1['m'] == 0 and r1['counts'].tolist() == [0, 0, len(X), 0] and not r1['stats'].any()
        else:
            assert r1['m'] == len(X) and r1['counts'][1] == 0 and np.linalg.norm(r1['X'] - X, axis=1).max() <= 1e-9
            assert (r1['src'][:, 0] == (1 if swap else 2)).all()         # family 0 is refused: the component that addresses family 1


def test_wrong_family_assignment_is_not_truth():
    """the swap matters: the families exchanged without saying so puts the points millimetres off"""
    idx, X = TC.cylinder_hits()
    uv = PC.project_pair(X, 0.0, None)[0]
    t = TC.rig_table(-12, 12)
    r = TC.ref_table_triangulate(uv, idx, len(uv), PC.rig()[0], None, t['P'], t['status'], t['lo'], t['hi'], swap=1)
    assert r['stats'][1] > 1.0


def test_true_table_of_a_scene_is_the_rig_s():
    from cpe_amd import synth
    t = TC.true_table(synth.Scene(1200, 1920))
    N = t['hi']
    assert t['lo'] == -N and t['P'].shape == (2, 2 * N + 1, 4) and not t['status'].any()
    assert np.allclose(t['P'], TC.rig_table(-N, N)['P'], rtol=0, atol=1e-12)
    small = TC.true_table(synth.Scene(480, 640))
    assert small['hi'] == max(synth.Scene(480, 640).half_lines, synth.Scene(480, 640).half_lines_v)
    Op = -synth.make_rig(synth.Scene(480, 640))[3][:3, :3].T @ synth.make_rig(synth.Scene(480, 640))[3][:3, 3]
    assert np.abs(small['P'][..., :3] @ Op + small['P'][..., 3]).max() <= 1e-12


def test_tolerances_stay_under_their_ceiling():
    worst = 0.0
    for what, r in _all_references():
        if r['m']:
            worst = max(worst, r['tol_X'].max(), r['tol_res'].max())
            assert r['tol_X'].max() <= 1e-8 and r['tol_res'].max() <= 1e-8, what
    print(f'largest derived tolerance {worst:.3e}')
    assert worst > 0


def test_no_decision_lies_at_its_gate():
    seen = 0
    for what, r in _all_references():
        assert r['margin'] > 1e-6, (what, r['margin'])
        seen += 1
    assert seen >= 40
    for seed in TC.NOISY_SEEDS:
        for cam in (1, 2):
            assert TC.noisy_case(seed, cam)['ref']['margin'] > 1e-6


def test_cases_cover_what_they_claim():
    c = TC.frame_cases()
    ref = lambda name, nb=0: TC.frame_reference(name, nb)
    assert [ref(f'count {k}')['counts'][[0, 2, 3]].sum() for k in (1, 63, 64, 65, 127, 128, 129)] == [1, 63, 64, 65, 127, 128, 129]
    assert ref('count -1')['m'] == 0 and ref('count 0')['m'] == 0
    assert ref('count 2048')['counts'].sum() - ref('count 2048')['counts'][1] == 2048 and ref('count 2048')['counts'][2] > 0
    assert np.array_equal(ref('count 3000')['counts'], ref('count 2048')['counts'])
    r = ref('refused across rounds')
    assert r['m'] == 190 and r['counts'].tolist() == [190, 190, 10, 0]
    assert r['src'][61:64, 1].tolist() == [61, 67, 68] and r['src'][120:123, 1].tolist() == [125, 131, 132]
    assert ref('all refused')['counts'].tolist() == [0, 0, 150, 0] and ref('none refused')['counts'].tolist() == [200, 200, 0, 0]
    r0, r1 = ref('one component out of range'), ref('one component out of range', 1)
    assert r0['m'] == 150 and set(r0['src'][:, 0].tolist()) == {1, 2, 3} and r1['m'] == 50 and (r1['src'][:, 0] == 3).all()
    assert ref('nan pixels')['counts'][2] >= 4 and 5 not in ref('nan pixels')['src'][:, 1]
    # refused lines: one family, the other, both
    r = ref('count 129')
    ids, bits = r['idx'], r['src'][:, 0]
    assert (bits[(ids[:, 0] == 3) & (ids[:, 1] != 7) & (ids[:, 1] != -4)] == 2).all() and (bits[(ids[:, 1] == -4) & (ids[:, 0] != 3) & (ids[:, 0] != 7)] == 1).all()
    assert not ((ids[:, 0] == 7) & (ids[:, 1] == 7)).any()
    cr = TC.call_reference
    assert cr('every line refused')[0]['counts'][2] == len(TC.cylinder_frame()[0])
    assert 0 < cr('L 1')[0]['m'] < 60 and (cr('L 1')[0]['src'][:, 0] != 3).sum() == cr('L 1')[0]['m'] - 1
    assert cr('L 256')[1]['counts'].tolist() == [2048, 2048, 0, 0]
    assert cr('plane contains the ray, alone')[0]['counts'].tolist() == [0, 0, 1, 0]
    assert cr('plane contains the ray, beside a good one')[0]['counts'].tolist() == [1, 1, 0, 0]
    assert cr('plane contains the ray, default min_sin')[0]['counts'].tolist() == [1, 1, 0, 0]
    assert cr('plane behind the camera')[0]['counts'].tolist() == [0, 0, 0, 1]
    free, gated = cr('index off by one, no gate')[0], cr('index off by one, max_res')[0]
    n1 = int((TC.cylinder_frame()[0][:, 0] == 1).sum())
    assert free['counts'][3] == 0 and free['stats'][1] > 0.5 and gated['counts'][3] == n1 and gated['stats'][1] <= 0.5
    assert not (gated['idx'][:, 0] == 1).any()
    nt = cr('noisy table')[0]
    assert nt['counts'][1] == nt['m'] >= 400 and cr('noisy table both')[0]['m'] == nt['m'] and nt['stats'][0] > 0.01     # (its 8 refused lines are columns the cylinder does not reach)


def test_noisy_bounds_are_twice_the_worst_seed(orc):
    """the figures in the docstring of tests/table_tri_cases.py: measured here again, NOISY_TRI_BOUNDS must be twice the worst seed"""
    for cam in (1, 2):
        worst = dict(mean_mm=0.0, worst_mm=0.0, axis_deg=0.0, axis_mm=0.0)
        for seed in TC.NOISY_SEEDS:
            case = TC.noisy_case(seed, cam)
            r = case['ref']
            assert r['m'] >= 400 and (case['table']['status'] == 0).sum() == 42
            fit = orc.fit_cylinder(r['X'], TC.RADIUS, mode=1)          # (the build's LM: the simplex stalls on two of the seeds)
            assert fit['status'] == 0
            e = TC.noisy_errors(r['X'], case['Xtrue'], fit['cyl'])
            print(f'camera {cam} seed {seed}: ' + '  '.join(f'{k} {v:.4f}' for k, v in e.items()) + f'  rms res {r["stats"][0]:.4f}  objective {fit["fvals"][1]:.2f}')
            worst = {k: max(worst[k], e[k]) for k in worst}
        print(f'camera {cam} worst: ' + '  '.join(f'{k} {v:.4f}' for k, v in worst.items()))
        for k, v in worst.items():
            b = TC.NOISY_TRI_BOUNDS[cam][k]
            assert abs(b - 2 * v) <= 2 * 5e-5 + 1e-12, f'camera {cam} {k}: bound {b} is not twice the measured {v:.4f} (rounded to 4 places)'


def test_laser_table_round_trip_and_swap(cpe, tmp_path):
    import torch
    t = TC.with_status(TC.rig_table(-5, 7), (2,), (-1, 0))
    out = dict(P=torch.from_numpy(t['P']), status=torch.from_numpy(t['status']), lo=-5, hi=7,
               centre=torch.tensor([45.0, -18.0, 0.0, 0.02], dtype=torch.float64), centre_status=torch.zeros(1, dtype=torch.int32))
    for fam in ('col', 'row'):
        tab = cpe.fit.LaserTable.from_index_planes(out, -5, 7, fam)
        path = tmp_path / f'table_{fam}.npz'
        tab.save(str(path))
        back = cpe.fit.LaserTable.load(str(path), 'cpu')
        assert (back.lo, back.hi, back.family0) == (-5, 7, fam)
        for k in ('P', 'status', 'centre', 'centre_status'):
            a, b = getattr(tab, k), getattr(back, k)
            assert a.dtype == b.dtype and a.numpy().tobytes() == b.numpy().tobytes(), k
        # GridTables.id is (col, row): no swap when family 0 holds the columns; the planar detector's (row, col) the other way
        assert back.swap_for() == (0 if fam == 'col' else 1) and back.swap_for('row_col') == (1 if fam == 'col' else 0)
    assert cpe.fit.LaserTable.from_index_planes(out).family0 == 'col'
    with pytest.raises(ValueError):
        cpe.fit.LaserTable.from_index_planes(out, -5, 7, 'diagonal')
    with pytest.raises(ValueError):
        cpe.fit.LaserTable.from_index_planes(out, -5, 8, 'col')         # 14 indices for 13 lines
    with pytest.raises(ValueError):
        cpe.fit.LaserTable(torch.zeros(2, 257, 4, dtype=torch.float64), torch.zeros(2, 257, dtype=torch.int32), -128, 128,
                           torch.zeros(4, dtype=torch.float64), torch.zeros(1, dtype=torch.int32))
