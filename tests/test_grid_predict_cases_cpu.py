"""The cases and the numpy references of tests/grid_predict_cases.py, checked without a GPU: the exports' declarations, truth at
the true pose, the ceiling of the derived tolerances, the margin of every decision from its gate, the hand-made assignment
tables, and the refinement chain on the three scenarios: no kept point ever carries a wrong index, and the axis ends inside the
measured bounds."""
import math
import os
import re

import numpy as np
import pytest

import grid_predict_cases as G
import plane_fit_cases as PC
import table_tri_cases as TC


def test_exports_are_declared(cpe):
    hdr = open(os.path.join(os.path.dirname(cpe.lib.__file__), '..', 'include', 'cpe.h')).read()
    names = cpe.lib.declared_symbols()
    assert 'cpe_grid_predict_batch' in names and 'cpe_grid_assign_batch' in names
    assert int(re.search(r'#define CPE_VERSION (\d+)', hdr).group(1)) >= 124 and '124: cpe_grid_predict_batch, cpe_grid_assign_batch' in hdr
    assert len(cpe.lib._SIGS['cpe_grid_predict_batch'][1]) == 19 and len(cpe.lib._SIGS['cpe_grid_assign_batch'][1]) == 22
    assert [n for n, _ in cpe.lib.CpeGridPredictParams._fields_] == ['win_lo', 'win_hi', 'min_cos', 'img_w', 'img_h']
    assert [n for n, _ in cpe.lib.CpeGridAssignParams._fields_] == ['tau_px', 'ratio', 'swap', 'reserved']
    assert f'#define CPE_PRED_MAXN {G.PRED_MAXN}' in hdr and float(re.search(r'#define CPE_PRED_MIN_W2 (\S+)', hdr).group(1)) == G.MIN_W2
    for k, name in enumerate(('OK', 'NO_FRAME', 'NO_PLANE', 'PARALLEL', 'MISS', 'GRAZING')):
        assert f'#define CPE_PRED_{name} {k}' in hdr and getattr(cpe.fit, 'PRED_' + name) == k
    assert cpe.fit.PRED_MAXN == G.PRED_MAXN
    for fn in ('grid_predict_batch', 'grid_assign_batch', 'fit_single_cylinder_refined_batch'):
        assert hasattr(cpe.fit, fn)


def test_the_listing_of_renumbered_frames(cpe, tmp_path):
    """run_experiment's refine['frames']: the frames where a point of either image was re-numbered, with the round they took"""
    from cpe_amd import experiment
    import torch
    names = ['-10', '00', '10', '20']
    got = experiment.refine_listing(names, torch.tensor([2, 0, 1, 2], dtype=torch.int32), torch.tensor([[42, 40], [0, 0], [0, 175], [0, 0]], dtype=torch.int32))
    assert got == [dict(index=0, name='-10', round=2, left=42, right=40), dict(index=2, name='10', round=1, left=0, right=175)]
    assert experiment.refine_listing(names, np.zeros(4, np.int32), np.zeros((4, 2), np.int32)) == []
    t = cpe.fit.LaserTable(torch.zeros(2, 3, 4, dtype=torch.float64), torch.zeros(2, 3, dtype=torch.int32), -1, 1, torch.zeros(4, dtype=torch.float64),
                           torch.full((1,), 5, dtype=torch.int32))
    assert t.centre_ok is None and t.has_centre() is False and t.centre_ok is False and t.to('cpu').centre_ok is False
    good = cpe.fit.LaserTable(t.P, t.status, -1, 1, t.centre, torch.zeros(1, dtype=torch.int32))
    assert good.has_centre() is True
    for tab, ok in ((t, False), (good, True)):                 # a saved table knows it without asking the device
        tab.save(str(tmp_path / 'table.npz'))
        assert cpe.fit.LaserTable.load(str(tmp_path / 'table.npz')).centre_ok is ok


def test_true_pose_predicts_the_true_grid():
    """at the true pose every OK node of the rig table is the projector ray's cut with the cylinder (cylinder_hits, computed
    another way) and its noise-free projection, within the reference's own tolerance plus the truth's roundings (1e-9)"""
    idx, X = TC.cylinder_hits(cols=range(G.LO, G.HI + 1), rows=range(G.LO, G.HI + 1))
    uv = PC.project_pair(X, 0.0, None)
    r = G.predict_reference('one frame')[0]
    j = (idx[:, 0] - G.LO) * r['Nv'] + (idx[:, 1] - G.LO)
    ok = r['state'] == G.OK
    assert ok.sum() > 700 and ok[j].sum() == ok.sum(), 'an OK node is not among the rays that hit'
    assert set(np.unique(r['state'][j])) <= {G.OK, G.GRAZING} and (r['state'][np.setdiff1d(np.arange(len(ok)), j)] == G.MISS).all()
    hit = ok[j]
    eX = np.abs(r['X'][j][hit] - X[hit]).max(1)
    assert (eX <= r['tol_X'][j][hit] + 1e-9).all(), f'X off the truth by {eX.max():.3e}'
    for c in (0, 1):
        seen = ((r['vis'][j] >> c) & 1).astype(bool)
        assert seen.sum() > 650
        ep = np.abs(r['px'][c][j][seen] - uv[c][seen]).max(1)
        print(f'camera {c + 1}: {seen.sum()} visible nodes, px off the truth by {ep.max():.2e}, X by {eX.max():.2e}')
        assert (ep <= r['tol_px'][c][j][seen] + 1e-9).all()


def test_tolerances_and_margins_of_the_predictions():
    worst_x = worst_p = 0.0
    worst_m = math.inf
    states = np.zeros(6, np.int64)
    for name in G.predict_cases():
        for f, r in enumerate(G.predict_reference(name)):
            assert r['tol_X'].max() <= G.TOL_X_BOUND and r['tol_px'].max() <= G.TOL_PX_BOUND, f'{name} frame {f}'
            assert r['margin'] > 1e-6, f'{name} frame {f}: a decision {r["margin"]:.2e} from its gate ({r["margins"]})'
            worst_x, worst_p, worst_m = max(worst_x, r['tol_X'].max()), max(worst_p, r['tol_px'].max()), min(worst_m, r['margin'])
            states += np.bincount(r['state'], minlength=6)
    print(f'worst tol_X {worst_x:.2e} mm, tol_px {worst_p:.2e} px, smallest margin {worst_m:.2e}; states {states.tolist()}')
    assert states.all() or states[G.PARALLEL] == 0          # (PARALLEL has its own test below)
    assert all(states[k] > 0 for k in (G.OK, G.NO_FRAME, G.NO_PLANE, G.MISS, G.GRAZING))


def test_parallel_planes_and_the_states_in_order():
    """two families holding the same plane: |w|^2 = 0 -> PARALLEL; NO_PLANE comes before it, NO_FRAME before everything"""
    K1, K2, T21 = PC.rig()[:3]
    t = TC.rig_table(-2, 2)
    P = t['P'].copy()
    P[1, 1] = P[0, 3]                                        # node (1, -1): the same plane twice
    st = t['status'].copy()
    st[0, 0] = 5
    r = G.ref_grid_predict(G.POSES['true'], True, G.RADIUS, K1, K2, T21, P, st, -2, 2, PC.rig()[5])
    assert r['state'][3 * 5 + 1] == G.PARALLEL and (r['state'][:5] == G.NO_PLANE).all()
    # (the other three nodes of that line cut two column planes: a line through the projector that passes the cylinder by)
    assert (r['state'][[1 * 5 + 1, 2 * 5 + 1, 4 * 5 + 1]] == G.MISS).all() and r['counts'][0] == 25 - 5 - 1 - 3
    r = G.ref_grid_predict(G.POSES['true'] * 0, True, G.RADIUS, K1, K2, T21, P, st, -2, 2, PC.rig()[5])
    assert (r['state'] == G.NO_FRAME).all() and not r['X'].any() and not r['counts'].any()


def test_margins_of_the_assignments():
    px, vis = G.main_pixels()
    worst = math.inf
    seen = np.zeros(8, np.int64)
    calls = [(f'{c["names"][i]}', c, i) for c in G.main_group_calls(list(G.main_frames()), px, vis) for i in range(len(c['frames']))]
    calls += [(f'{name} [{i}]', c, i) for name, c in G.special_calls().items() for i in range(len(c['frames']))]
    for what, call, i in calls:
        r = G.assign_reference(dict(call, frames=call['frames'][i:i + 1], px=call['px'][i:i + 1], vis=call['vis'][i:i + 1]))[0]
        assert r['margin'] > 1e-6, f'{what}: a decision {r["margin"]:.2e} from its gate'
        assert r['tol_dist'].max(initial=0) <= 1e-14
        worst = min(worst, r['margin'])
        seen += r['counts']
    print(f'smallest margin {worst:.2e}; counts over all images {seen.tolist()}')
    assert all(seen[:7] > 0), 'a refusal class has no case'


def test_hand_made_tables():
    """mirrored pixels at equal distances: the lowest slot keeps the node; swap exchanges the id components; a single visible
    node has no second-nearest, so only tau_px refuses; no visible node refuses everything"""
    c = G.special_calls()
    r = G.assign_reference(c['mirrored ties'])[0]
    assert r['src'].tolist() == [0, 5, 7, 10, 12] and r['counts'].tolist() == [5, 3, 2, 0, 3, 0, 5, 0]
    assert r['id'].tolist() == [[0, 5], [-2, 6], [-1, 5], [2, 3], [-2, 3]] and r['dist'][0] == math.sqrt(0.3125) and r['dist'][1] == 0.125
    assert r['node_slot'][12] == 0 and r['node_slot'][3] == 5 and (r['node_slot'] >= 0).sum() == 5
    s = G.assign_reference(c['mirrored ties, swap'])[0]
    assert np.array_equal(s['id'], r['id'][:, ::-1]) and np.array_equal(s['src'], r['src'])
    one, short = G.assign_reference(c['single visible node'])
    assert one['src'].tolist() == [0] and one['counts'].tolist() == [1, 1, 0, 0, 9, 0, 3, 0] and short['m'] == 1
    assert G.assign_reference(c['no visible node'])[0]['counts'].tolist() == [0, 0, 0, 13, 0, 0, 0, 0]
    big, clamped, _ = G.assign_reference(c['count 2048'])
    assert big['counts'][[0, 3, 4, 5, 6]].sum() == G.MAXP and np.array_equal(big['src'], clamped['src'])


@pytest.mark.parametrize('table', ['rig', 'noisy'])
@pytest.mark.parametrize('name', G.SCENARIOS)
def test_refinement_never_keeps_a_wrong_index(name, table):
    """the three scenarios, seeds 0..4, through the reference chain: no kept point carries a wrong index in any round, and the
    axis after the last round is inside REFINE_BOUNDS"""
    b = G.REFINE_BOUNDS[name]
    for seed in TC.NOISY_SEEDS:
        t = TC.rig_table(G.LO, G.HI) if table == 'rig' else TC.noisy_table(seed)
        s = G.scenario(name, seed)
        r = G.refine_chain(s['gp1'], s['gp2'], t)
        assert r['first']['status'] == 0 and len(r['rounds']) == 2
        for k, rd in enumerate(r['rounds']):
            for a, true in ((rd['a1'], s['true1']), (rd['a2'], s['true2'])):
                assert np.array_equal(a['id'], true[a['src']]), f'{name} seed {seed} round {k + 1}: a kept point carries a wrong index'
            assert rd['status'] == 0
        last = r['rounds'][-1]
        deg, mm = TC.axis_errors(r['cyl'])
        print(f'{name} {table} seed {seed}: first {r["first"]["pairs"]} pairs, axis {TC.axis_errors(r["first"]["cyl"])}; rounds kept '
              f'{[(rd["a1"]["m"], rd["a2"]["m"]) for rd in r["rounds"]]}, re-numbered {[(int(rd["a1"]["counts"][2]), int(rd["a2"]["counts"][2])) for rd in r["rounds"]]}; '
              f'axis {deg:.4f} deg {mm:.4f} mm')
        assert deg <= b['axis_deg'] and mm <= b['axis_mm']
        if name != 'third_missing':
            assert min(last['a1']['m'], last['a2']['m']) >= 410
        else:
            assert last['a1']['m'] + last['a1']['counts'][4] == len(s['gp1']) and last['a1']['m'] >= len(s['gp1']) - 3
