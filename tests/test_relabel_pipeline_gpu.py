"""The re-labelling inside the planar chain: FramePipeline(target='plane', relabel={}) against its layers called by hand and
against the oracle chain (oracle planar detect -> ref_grid_relabel -> oracle.choose_idx -> oracle.triangulate -> ref_fit_plane);
experiment.run_plane_experiment(relabel={}) against the true laser planes; and that nothing changes without the option.

The boards are the rendered ones of tests/relabel_cases.py (640 x 480, 8 frames); TABLE_BOUNDS are those of
tests/test_relabel_cases_cpu.py, twice what the numpy chain measures on the same boards."""
import json
import warnings

import numpy as np
import pytest
import torch

import index_shift_cases as SC
import plane_fit_cases as PC
import proj_model_cases as M
import relabel_cases as RC

pytestmark = pytest.mark.gpu

H, W, F = RC.H, RC.W, 8
TABLE_BOUNDS = RC.TABLE_BOUNDS
TAU = 1.0           # mm: with the lines re-labelled the pairs are the same grid points, so the band is the noise's, not 12 mm


def _hand(cpe, gpu, b, n, relabel):
    """detect, grid_relabel_batch on both images' tables, fit_single_plane_batch without the option"""
    det = cpe.api.detect_grid_batch(torch.cat([b['left'][:n], b['right'][:n]]).to(gpu), target='plane')
    tabs = cpe.fit.GridTables(det['xy'], det['id'], det['n'])
    rl = cpe.fit.grid_relabel_batch(tabs, det['center'], **relabel)
    t = rl['tables']
    g1, g2 = cpe.fit.GridTables(t.xy[:n], t.id[:n], t.cnt[:n]), cpe.fit.GridTables(t.xy[n:], t.id[n:], t.cnt[n:])
    return det, rl, cpe.fit.fit_single_plane_batch(g1, g2, b['K1'], b['K2'], b['T21'], tau=TAU)


def test_pipeline_equals_its_layers_and_the_oracle_chain(cpe, orc, gpu):
    from cpe_amd import pipeline
    n = 3
    b = RC.boards(30.0, 7, F)
    pipe = pipeline.FramePipeline(H, W, b['K1'], b['K2'], b['T21'], 0.0, chunk=n, device=gpu, target='plane', plane=dict(tau=TAU), relabel={})
    rec, det, out = pipe.run_chunk(b['left'][:n].to(gpu), b['right'][:n].to(gpu))
    det_h, rl, hand = _hand(cpe, gpu, b, n, {})
    torch.cuda.synchronize()
    for k in ('P', 'T', 'grid', 'stats', 'n_inliers', 'inlier_mask', 'plane_flags', 'status', 'm', 'pts3', 'idx', 'mean_err'):
        assert out[k].cpu().numpy().tobytes() == hand[k].cpu().numpy().tobytes(), k
    assert torch.equal(out['relabel_counts'], torch.stack([rl['counts'][:n], rl['counts'][n:]], 1))
    assert torch.equal(out['relabel_flags'], torch.stack([rl['flags'][:n], rl['flags'][n:]], 1)) and not out['relabel_flags'].any()
    # the interleaved layout (run_raw's) reads the same centres
    pairs = torch.stack([b['left'][:n], b['right'][:n]], 1).contiguous().to(gpu)
    rec2, _, out2 = pipe.run_chunk(pairs[:, 0], pairs[:, 1])
    torch.cuda.synchronize()
    assert torch.equal(rec.view(torch.int64), rec2.view(torch.int64)) and torch.equal(out['relabel_counts'], out2['relabel_counts'])
    # the oracle chain
    got = {k: out[k].cpu().numpy() for k in ('P', 'T', 'grid', 'stats', 'n_inliers', 'inlier_mask', 'plane_flags', 'status', 'm', 'pts3', 'idx')}
    counts = out['relabel_counts'].cpu().numpy()
    for i, f in enumerate(RC.oracle_frames(30.0, 7, F)[:n]):
        assert np.array_equal(counts[i], f['ref']['counts']), f'frame {i}: line counts\n{counts[i]}\n{f["ref"]["counts"]}'
        for k in range(2):                                           # the kernel's tables are the reference's
            j, m_ = i + k * n, int(f['ref']['cnt'][k])
            assert int(rl['tables'].cnt[j]) == m_
            assert np.array_equal(rl['tables'].id[j, :m_].cpu().numpy(), f['ref']['id'][k, :m_])
            assert np.array_equal(rl['tables'].xy[j, :m_].cpu().numpy(), f['ref']['xy'][k, :m_])
        (xy1, id1), (xy2, id2) = f['tables']
        c1, c2, idx, _ = orc.choose_idx(np.concatenate([xy1, id1], 1), np.concatenate([xy2, id2], 1), b['K1'], b['K2'], b['T21'])
        X, err = orc.triangulate(c1, c2, b['K1'], b['K2'], b['T21'])
        m = int(got['m'][i])
        assert m == len(X) and m >= 60
        assert np.array_equal(got['idx'][i, :m], idx) and np.array_equal(got['pts3'][i, :m], X)
        ref = PC.ref_fit_plane(X, idx, m, TAU, 4)
        r = X @ b['plane_n'][i] - b['plane_d'][i]
        print(f'frame {i}: m {m} inliers {ref["n_inliers"]} rms {ref["stats"][0]:.3f} mm, off the true board at most {np.abs(r).max():.3f} mm, '
              f'relabel margin {f["ref"]["margin"]:.2e}, fit margin {ref["margin"]:.2e}')
        assert ref['status'] == 0 and ref['margin'] > 1e-6 and ref['spread_margin'] > 1e-6
        PC.compare_fit(dict(P=got['P'][i], T=got['T'][i], grid=got['grid'][i], stats=got['stats'][i], n_inliers=got['n_inliers'][i],
                            mask=got['inlier_mask'][i], flags=got['plane_flags'][i], status=got['status'][i]), ref, f'frame {i}')
        # the per-frame condition of tests/test_relabel_cases_cpu.py, on chooseIdx's pairs (frame 0: 70 of 77; frames 1, 2: all)
        assert (np.abs(r) < 1.0).mean() >= 0.80
    _, _, st, st_l, st_r = pipeline.unpack_counters(rec[:, 15])
    assert st.tolist() == [0] * n and st_l.tolist() == [0] * n and st_r.tolist() == [0] * n


def test_without_relabel_nothing_changes(cpe, gpu):
    from cpe_amd import pipeline
    b = RC.boards(30.0, 7, F)
    left, right = b['left'][:2].to(gpu), b['right'][:2].to(gpu)
    args = (H, W, b['K1'], b['K2'], b['T21'], 0.0)
    plain = pipeline.FramePipeline(*args, chunk=2, device=gpu, target='plane', plane=dict(tau=12.0))
    named = pipeline.FramePipeline(*args, chunk=2, device=gpu, target='plane', plane=dict(tau=12.0), relabel=None)
    r1, det, o1 = plain.run_chunk(left, right)
    r2, _, o2 = named.run_chunk(left, right)
    g1 = cpe.fit.GridTables(det['xy'][:2], det['id'][:2], det['n'][:2]); g2 = cpe.fit.GridTables(det['xy'][2:], det['id'][2:], det['n'][2:])
    hand = cpe.fit.fit_single_plane_batch(g1, g2, b['K1'], b['K2'], b['T21'], tau=12.0)
    torch.cuda.synchronize()
    assert torch.equal(r1.view(torch.int64), r2.view(torch.int64)) and set(o1) == set(o2) == set(hand) and 'relabel_counts' not in o1
    for k in hand:
        if isinstance(hand[k], torch.Tensor) and k != '_ws':
            assert o1[k].cpu().numpy().tobytes() == hand[k].cpu().numpy().tobytes(), k
    with_rl = pipeline.FramePipeline(*args, chunk=2, device=gpu, target='plane', plane=dict(tau=12.0), relabel={}).run_chunk(left, right)[2]
    assert set(with_rl) == set(o1) | {'relabel_counts', 'relabel_flags'} and not torch.equal(with_rl['idx'], o1['idx'])


def test_refusals(cpe, gpu):
    from cpe_amd import pipeline
    b = RC.boards(30.0, 7, F)
    args = (H, W, b['K1'], b['K2'], b['T21'], 45.0)
    for kw in (dict(relabel={}), dict(target='cylinder', relabel={}), dict(target='cylinder', relabel=dict(min_pts=4))):
        with pytest.raises(ValueError, match='relabel'):
            pipeline.FramePipeline(*args, device=gpu, **kw)
    z = lambda *s, dt=torch.float64: torch.zeros(s, dtype=dt, device=gpu)
    g = cpe.fit.GridTables(z(1, RC.MAXP, 2), z(1, RC.MAXP, 2, dt=torch.int32), z(1, dt=torch.int32))
    with pytest.raises(ValueError, match='center'):
        cpe.fit.fit_single_plane_batch(g, g, b['K1'], b['K2'], b['T21'], relabel={})
    with pytest.raises(TypeError):
        cpe.fit.fit_single_plane_batch(g, g, b['K1'], b['K2'], b['T21'], relabel=dict(th=1), center1=z(1, 2), center2=z(1, 2))


def _folder(tmp_path, b):
    from PIL import Image
    for i in range(F):
        Image.fromarray(b['left'][i].numpy()).save(tmp_path / f'b{i}L.png')
        Image.fromarray(b['right'][i].numpy()).save(tmp_path / f'b{i}R.png')
    lens = lambda K: dict(IntrinsicMatrix=np.asarray(K, dtype=np.float64).tolist(), RadialDistortion=[0.0, 0.0], TangentialDistortion=[0.0, 0.0])
    (tmp_path / 'cam.json').write_text(json.dumps(dict(LeftCamera=lens(b['K1']), RightCamera=lens(b['K2']))))
    return str(tmp_path), str(tmp_path / 'cam.json'), b['K1'], b['K2'], b['T21']


def test_run_plane_experiment_builds_the_true_table(cpe, gpu, tmp_path):
    """8 boards of 30 deg, seed 7: with relabel={} the table is `consistent` and within TABLE_BOUNDS of the scene's true planes;
    without it the same folder gives the warning and a table centimetres off.  The result has the plain keys plus `relabel`"""
    from cpe_amd import experiment
    b = RC.boards(30.0, 7, F)
    args = _folder(tmp_path, b)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter('always')
        res = experiment.run_plane_experiment(*args, tau=TAU, device=gpu, chunk=3, relabel={})
    assert not [w for w in seen if 'laser planes' in str(w.message)]     # no warning about the table with the option
    with pytest.warns(UserWarning):
        plain = experiment.run_plane_experiment(*args, tau=TAU, device=gpu, chunk=3)
    again = experiment.run_plane_experiment(*args, tau=TAU, device=gpu, chunk=8, relabel=dict(min_pts=3, merge_frac=0.65))
    torch.cuda.synchronize()
    assert set(res) == set(plain) | {'relabel'} and set(res['relabel']) == {'counts', 'flags'}
    assert set(plain) == {'names', 'records', 'P', 'T', 'grid', 'stats', 'pts3', 'idx', 'cnt', 'n_inliers', 'inlier_mask', 'plane_flags',
                          'skipped', 'table', 'consistent', 'laser_table'}
    assert tuple(res['relabel']['counts'].shape) == (F, 2, 2, 4) and tuple(res['relabel']['flags'].shape) == (F, 2)
    assert not res['relabel']['flags'].any() and (res['relabel']['counts'][..., 3] >= 7).all()
    for k in ('records', 'pts3', 'idx', 'cnt', 'inlier_mask'):
        assert res[k].cpu().numpy().tobytes() == again[k].cpu().numpy().tobytes(), k
    assert plain['consistent'] is False and res['consistent'] is True and res['skipped'] == []
    tab = res['table']
    fig = RC.table_figures(tab['P'].cpu().numpy(), tab['status'].cpu().numpy(), tab['centre'].cpu().numpy(), tab['lo'], b['scene'])
    fig['centre_rms_mm'] = float(tab['centre'][3])
    print('relabel:', fig, 'inliers', res['n_inliers'].tolist(), 'of', res['cnt'].tolist())
    for k, bound in TABLE_BOUNDS.items():
        assert fig[k] <= bound, f'{k}: {fig[k]:.4f} > {bound:.4f}'
    assert res['laser_table'].family0 == 'row' and (res['laser_table'].lo, res['laser_table'].hi) == (tab['lo'], tab['hi'])
    ptab = plain['table']
    pfig = RC.table_figures(ptab['P'].cpu().numpy(), ptab['status'].cpu().numpy(), ptab['centre'].cpu().numpy(), ptab['lo'], b['scene'])
    print('plain:', pfig)
    assert pfig['worst_deg'] > 20 * TABLE_BOUNDS['worst_deg']


def test_leftover_frames_and_the_index_shift_chain(cpe, gpu, tmp_path):
    """8 boards of 20 deg, seed 4, where the re-labelling leaves frames a line off (tests/test_relabel_cases_cpu.py: the free
    table is 2.6 deg / 17 mm off), with projector=dict(tau=1, renumber={}) added.  Asserted: what the numpy chain gives on the
    same points -- ref_index_shift against the call's own first table gives the call's shifts, scores and flags (the first
    fits themselves end in different fixed points of the trimming loop, tests/test_index_shift_pipeline_gpu.py, and are not
    compared).  Whether the leftover frames are repaired is printed, not asserted.

    Measured: one frame of the eight (frame 3) is left with its two images a line apart, so its 24 stereo points are not grid
    points at all (median 38 mm off the true board; all other frames 0.09-0.32 mm).  The projector model trims all 24 + 24 of
    its residuals (projector_shifted == [3]) and fits the other seven: rms 0.049 mm, `consistent` True, its table 0.080 deg /
    0.39 mm off the true planes, where the free table of the same run is not consistent (centre rms 3.7 mm).  The index-shift
    search does NOT repair the frame: it scores 0 at every candidate and is flagged WEAK, because a shift of the indices
    cannot move points that were triangulated from two different grid points.  So the chain excludes such a frame; it does
    not bring it back (Limits)."""
    from cpe_amd import experiment
    b = RC.boards(20.0, 4, F)
    args = _folder(tmp_path, b)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        res = experiment.run_plane_experiment(*args, tau=TAU, device=gpu, relabel={}, projector=dict(tau=TAU, renumber={}))
        base = experiment.run_plane_experiment(*args, tau=TAU, device=gpu, relabel={})
    torch.cuda.synchronize()
    assert set(res) == set(base) | {'projector', 'projector_shifted', 'projector_renumbered'}
    for k in ('records', 'pts3', 'idx', 'cnt', 'inlier_mask'):
        assert res[k].cpu().numpy().tobytes() == base[k].cpu().numpy().tobytes(), k
    assert torch.equal(res['relabel']['counts'], base['relabel']['counts'])
    pm = res['projector']
    assert pm is not None and set(pm) == {'fit', 'model', 'laser_table', 'first', 'shift'}
    X, I, cnt, use = (res[k].cpu().numpy() for k in ('pts3', 'idx', 'cnt', 'inlier_mask'))
    # every frame's points against the true board, and the true offset of its rows / columns: which frames are a line off
    off = [float(np.median(np.abs(X[i, :cnt[i]] @ b['plane_n'][i] - b['plane_d'][i]))) for i in range(F)]
    lo, hi = pm['fit']['lo'], pm['fit']['hi']
    table = cpe.fit.ProjectorModel.from_fit(pm['first'], 'row').table(lo, hi)
    sh = {k: v.cpu().numpy() for k, v in pm['shift'].items()}
    ref = SC.ref_index_shift(X, I, cnt, table.P.cpu().numpy(), table.status.cpu().numpy(), lo, hi, use=use, tau=TAU)
    print(f'median |distance to the true board| per frame {np.round(off, 3).tolist()} mm; first fit info {pm["first"]["info"].tolist()} '
          f'trimmed {pm["first"]["frame_counts"][:, [1, 3]].T.tolist()}\nshift {sh["shift"].T.tolist()} flags {sh["flags"].T.tolist()} '
          f'score {sh["score"][..., :2].tolist()}\nrenumbered {res["projector_renumbered"]} shifted {res["projector_shifted"]} '
          f'model status {pm["model"].status} rms {pm["model"].rms:.3f} consistent {res["consistent"]} (free table: {base["consistent"]}, '
          f'centre rms {float(base["table"]["centre"][3]):.3f} mm); margin {ref["margin"]:.2e}')
    assert ref['margin'] > 1e-6
    for k in ('shift', 'score', 'scores', 'flags'):
        assert np.array_equal(sh[k], ref[k]), f'{k}\n{sh[k]}\n{ref[k]}'
    if pm['model'].status == 0:
        fig = M.table_errors(pm['laser_table'].P.cpu().numpy(), pm['laser_table'].lo, _true_rows_first(b['scene']))
        print(f'model table against the true planes: {fig[0]:.4f} deg, {fig[1]:.4f} mm')


def _true_rows_first(scene):
    """table_tri_cases.true_table with family 0 = row, as the planar detector's ids"""
    import table_tri_cases as TC
    t = TC.true_table(scene)
    return dict(t, P=t['P'][::-1].copy(), status=t['status'][::-1].copy())
