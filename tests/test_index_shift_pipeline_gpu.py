"""fit.fit_projector_model_renumbered and experiment.run_experiment(projector=dict(renumber=...)): the fit, the table, the
index-shift search and the refit as one enqueued chain, against the references of tests/proj_model_cases.py and
tests/index_shift_cases.py, against the layers called by hand, against the oracle chain, and against the scene's true planes.

TABLE_BOUND is the one of tests/test_proj_model_pipeline_gpu.py: twice what the oracle chain measures on the same batch."""
import functools
import json

import numpy as np
import pytest
import torch

import index_shift_cases as SC
import plane_fit_cases as PC
import proj_model_cases as M
import table_tri_cases as TC

pytestmark = pytest.mark.gpu

H, W, SEED, F = 480, 640, 3, 8
TAU = 1.0
TABLE_BOUND = dict(normal_deg=2 * 0.0741, offset_mm=2 * 0.1196)
STEMS = [f'0{i}' for i in range(F)]
FIT_KEYS = ('model', 'info', 'moments', 'count', 'frames', 'inlier_mask', 'frame_counts')


def _dev(gpu, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in arrays]


def test_renumbered_fit_brings_the_shifted_frames_back(cpe, gpu):
    X, I, cnt = PC.pack(M.shifted_frames(0))
    dX, dI, dc = _dev(gpu, X, I, cnt)
    out = cpe.fit.fit_projector_model_renumbered(dX, dI, dc, -12, 12, tau=TAU)
    plain = cpe.fit.fit_projector_model(dX, dI, dc, -12, 12, tau=TAU)
    torch.cuda.synchronize()
    assert set(out) == {'first', 'table', 'shift', 'fit', 'lo', 'hi'} and (out['lo'], out['hi']) == (-16, 16)
    for k in FIT_KEYS:
        assert out['first'][k].cpu().numpy().tobytes() == plain[k].cpu().numpy().tobytes(), k
    assert (out['table'].lo, out['table'].hi, out['table'].family0) == (-16, 16, 'col')
    ref = SC.reference('shifted model table 0')
    for k in ('shift', 'score', 'scores', 'flags'):
        assert np.array_equal(out['shift'][k].cpu().numpy(), ref[k]), k
    assert np.array_equal(out['shift']['idx'].cpu().numpy(), ref['idx'])
    # (rms is compared where the kernel and the reference read the same table, tests/test_index_shift_gpu.py: here the table is
    # the kernels' own model's, which is the reference's to its tolerance only)
    fc, info = out['fit']['frame_counts'].cpu().numpy(), out['fit']['info'].cpu().numpy()
    assert not fc[:, [1, 3]].any() and (fc[:, [0, 2]] == 225).all()
    assert info[0] == 0 and info[1] == 0 and info[4:6].tolist() == [2700, 2700]
    clean = M.reference('cylinder 12')
    x = out['fit']['model'].cpu().numpy()[:15]
    d = np.abs(x - clean['x']).max()
    print(f'refit against the clean reference: {d:.3e} (tol {clean["tol"] + 1e-8:.3e}), LM iterations {info[2]}')
    assert d <= clean['tol'] + 1e-8
    # the same with the families called (row, col)
    rows = cpe.fit.fit_projector_model_renumbered(dX, dI, dc, -12, 12, tau=TAU, family0='row')
    assert rows['table'].family0 == 'row' and torch.equal(rows['shift']['shift'], out['shift']['shift'])
    assert torch.equal(rows['fit']['model'], out['fit']['model'])


def test_clean_frames_are_left_alone(cpe, gpu):
    X, I, cnt = PC.pack(M.cases()['cylinder 12']['frames'])
    dX, dI, dc = _dev(gpu, X, I, cnt)
    out = cpe.fit.fit_projector_model_renumbered(dX, dI, dc, -12, 12, tau=TAU, win=(2, 5), shift_tau=0.5, shift_min_score=100)
    torch.cuda.synchronize()
    assert (out['lo'], out['hi']) == (-17, 17) and tuple(out['shift']['scores'].shape) == (12, 16)
    assert not out['shift']['shift'].any() and not out['shift']['flags'].any() and torch.equal(out['shift']['idx'], dI)
    assert out['fit']['info'][4:6].tolist() == [2700, 2700]


def test_refusals(cpe, gpu):
    X, I, cnt = PC.pack(M.cases()['boards 3']['frames'])
    dX, dI, dc = _dev(gpu, X, I, cnt)
    with pytest.raises(ValueError):
        cpe.fit.fit_projector_model_renumbered(dX, dI, dc, -12, 12)                    # tau defaults to 0: no trimming
    with pytest.raises(ValueError):
        cpe.fit.fit_projector_model_renumbered(dX, dI, dc, -12, 12, tau=-1.0)
    with pytest.raises(ValueError):
        cpe.fit.fit_projector_model_renumbered(dX, dI, dc, -124, 124, tau=TAU)         # 249 + 8 lines
    cpe.fit.fit_projector_model_renumbered(dX, dI, dc, -124, 123, tau=TAU)             # 256 lines
    with pytest.raises(ValueError):
        cpe.fit.fit_projector_model_renumbered(dX, dI, dc, -12, 12, tau=TAU, win=(9, 0))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------ rendered frames
@functools.lru_cache(maxsize=None)
def _scene():
    from cpe_amd import synth
    return synth.render_batch(F, H, W, seed=SEED)


def _folder(tmp_path, b):
    from PIL import Image
    L, R = b['left'].numpy(), b['right'].numpy()
    for i, st in enumerate(STEMS):
        Image.fromarray(L[i]).save(tmp_path / f'{st}L.png')
        Image.fromarray(R[i]).save(tmp_path / f'{st}R.png')
    lens = lambda K: dict(IntrinsicMatrix=np.asarray(K, dtype=np.float64).tolist(), RadialDistortion=[0.0, 0.0], TangentialDistortion=[0.0, 0.0])
    (tmp_path / 'cam.json').write_text(json.dumps(dict(LeftCamera=lens(b['K1']), RightCamera=lens(b['K2']))))
    return str(tmp_path), str(tmp_path / 'cam.json'), b['K1'], b['K2'], b['T21'], b['radius']


def _by_hand(cpe, gpu, args):
    """the layers under run_experiment(match_offset={}): read, pre-step, FramePipeline.run_raw -> the fits with the points' indices"""
    from cpe_amd import experiment, iotool, pipeline
    cam_l, cam_r = iotool.load_camera_data(args[1])
    raw = [torch.from_numpy(np.stack([experiment.read_raw_image(f'{args[0]}/{s}{side}.png') for s in STEMS])).to(gpu) for side in 'LR']
    pre = iotool.StereoPrestep(cam_l, cam_r, H, W, gpu)
    fits = pipeline.alloc_fits(F, gpu)
    fits['idx'] = torch.zeros((F, cpe.fit.MAXP, 2), dtype=torch.int32, device=gpu)
    pipeline.FramePipeline(H, W, *args[2:], chunk=F, device=gpu, match={}).run_raw(raw[0], raw[1], pre, fits)
    torch.cuda.synchronize()
    return fits


def test_run_experiment_renumber_on_consistent_frames(cpe, gpu, tmp_path):
    """the frames of the batch agree after match_offset: nothing is re-numbered, three keys are added, nothing else changes"""
    from cpe_amd import experiment
    args = _folder(tmp_path, _scene())
    res = experiment.run_experiment(*args, device=gpu, chunk=3, multi_frame=False, match_offset={}, projector=dict(tau=TAU, renumber={}))
    plain = experiment.run_experiment(*args, device=gpu, chunk=3, multi_frame=False, match_offset={})
    single = experiment.run_experiment(*args, device=gpu, chunk=3, multi_frame=False, match_offset={}, projector=dict(tau=TAU))
    torch.cuda.synchronize()
    assert set(res) == set(plain) | {'projector', 'projector_shifted', 'projector_renumbered'}
    assert set(single) == set(plain) | {'projector', 'projector_shifted'} and set(single['projector']) == {'fit', 'model', 'laser_table'}
    for k in plain:
        if isinstance(plain[k], torch.Tensor):
            assert res[k].cpu().numpy().tobytes() == plain[k].cpu().numpy().tobytes(), k
    assert res['projector_renumbered'] == [] and res['projector_shifted'] == [] and res['skipped'] == []
    pm = res['projector']
    assert set(pm) == {'fit', 'model', 'laser_table', 'first', 'shift'}
    for k in FIT_KEYS:
        assert pm['first'][k].cpu().numpy().tobytes() == single['projector']['fit'][k].cpu().numpy().tobytes(), k
    assert not pm['shift']['shift'].any() and pm['model'].status == 0
    lo, hi = single['projector']['fit']['lo'], single['projector']['fit']['hi']
    assert (pm['fit']['lo'], pm['fit']['hi']) == (lo - 4, hi + 4)
    # nothing moved, so the refit has the first fit's residuals and, started at its optimum, its model
    assert pm['fit']['info'][4:6].tolist() == pm['first']['info'][4:6].tolist()
    assert (pm['fit']['model'][:15] - pm['first']['model'][:15]).abs().max().item() <= 1e-8
    with pytest.raises(ValueError):
        experiment.run_experiment(*args, device=gpu, chunk=3, multi_frame=False, match_offset={}, projector=dict(renumber={}))
    with pytest.raises(TypeError):
        experiment.run_experiment(*args, device=gpu, chunk=3, multi_frame=False, match_offset={}, projector=dict(tau=TAU, renumber=dict(th=1)))


def test_two_frames_numbered_off_are_recovered(cpe, orc, gpu, tmp_path):
    """frame 2 numbered one row up and frame 5 two columns down, in both images alike, on the device: the chain gives (0, -1) and
    (+2, 0), its table is the true one within TABLE_BOUND, and the oracle chain's points give the same shifts and scores.

    The first fit here is a hard one: the 8 frames hold 33 to 44 points on 3 or 4 columns, 10 mm apart at the cylinder, and the
    frame two columns off pulls the untrimmed column planes of round 0 far off (that model's b_0 is useless).  The trimming
    loop then runs on a non-convex problem, and the kernels' LM and the reference's scipy + Gauss-Newton end in different fixed
    points of it.  Measured, first band -> kept column + row residuals of 296 + 296:
        kernels    1, 1.5, 2, 2.5, 3 mm -> 135 + 258 after 2 refits (20 to 22 column residuals of most frames trimmed);
                   4 mm -> 263 + 258 (exactly the 33 + 38 residuals of the two frames trimmed); 0.5 mm -> CPE_ST_FEW_POINTS
        reference  1 mm -> 139 + 258; 2 mm -> 263 + 258 after 4 refits; 3, 4 mm -> 214 + 258
    Against the kernels' first table the search finds both shifts at every band from 1 to 4 mm.  Below 4 mm it is a near thing
    for the columns: frame 5 scores 22 of its 33 points at d = +2 against 11 elsewhere, exactly the lead of 2 that the rule asks
    for, and the column family of the frames 1 to 3 leads 16 : 10 or 17 : 11 at d = 0, is flagged WEAK and stays at 0, which
    is right; the row shift of frame 2 scores 38 : 0.  The refit then keeps 296 + 296 with no trimming round.  Against the reference's first table the column shift is found at
    2 mm only (at 1 mm it ties 11 : 11).  So what the chain repairs is what the first fit's trimming leaves standing, and the
    first fits are not compared here: the search is, on one table -- the oracle chain's points with ref_index_shift against
    the table the call itself made.  Its margin there is asserted."""
    b = _scene()
    fits = _by_hand(cpe, gpu, _folder(tmp_path, b))
    idx = fits['idx'].clone()
    idx[2, :, 1] += 1
    idx[5, :, 0] -= 2
    m = fits['m'].cpu().numpy()
    seen = np.concatenate([idx[i, :m[i]].cpu().numpy() for i in range(F)])
    lo, hi = int(seen.min()), int(seen.max())
    ok = torch.ones(F, dtype=torch.int32, device=gpu)
    out = cpe.fit.fit_projector_model_renumbered(fits['pts3'], idx, fits['m'], lo, hi, frame_ok=ok, tau=TAU)
    torch.cuda.synchronize()
    want = np.zeros((F, 2), np.int32)
    want[2, 1], want[5, 0] = -1, 2
    sh = {k: v.cpu().numpy() for k, v in out['shift'].items()}
    print(f'range {lo}..{hi}; first fit info {out["first"]["info"].tolist()}, trimmed per frame '
          f'{out["first"]["frame_counts"][:, [1, 3]].T.tolist()}; refit info {out["fit"]["info"].tolist()}')
    print(f'shift {sh["shift"].T.tolist()} flags {sh["flags"].T.tolist()}\nscore {sh["score"].tolist()}\nscores {sh["scores"].tolist()}')
    assert np.array_equal(sh['shift'], want), sh['shift'].tolist()
    assert (sh['flags'][want != 0] == cpe.fit.SHIFT_SHIFTED).all() and not (sh['flags'][want == 0] & cpe.fit.SHIFT_SHIFTED).any()
    for i in range(F):                                                   # the numbering of the run is back
        assert torch.equal(out['shift']['idx'][i, :m[i]], fits['idx'][i, :m[i]]) and not out['shift']['idx'][i, m[i]:].any()
    fc1, fc2 = out['first']['frame_counts'].cpu().numpy(), out['fit']['frame_counts'].cpu().numpy()
    assert fc1[2, 3] > 0 and fc1[5, 1] > 0 and not fc2[:, [1, 3]].any()
    assert int(out['fit']['info'][0]) == 0
    n = max(abs(out['lo']), abs(out['hi']))
    tab = cpe.fit.ProjectorModel.from_fit(out['fit']).table(-n, n)
    deg, mm = M.table_errors(tab.P.cpu().numpy(), -n, TC.true_table(b['scene']))
    print(f'refit on {out["lo"]}..{out["hi"]}: {deg:.4f} deg, {mm:.4f} mm off the true planes; scores {sh["score"][[2, 5]].tolist()}')
    assert deg <= TABLE_BOUND['normal_deg'] and mm <= TABLE_BOUND['offset_mm']
    # the oracle chain's points with the same re-numbering, and ref_index_shift against the call's own table
    ch = M.oracle_chain(orc, b, match=True, tau=TAU)
    frames = [dict(X=f['X'], idx=f['idx'].copy()) for f in ch['frames']]
    frames[2]['idx'][:, 1] += 1
    frames[5]['idx'][:, 0] -= 2
    X, I, cnt = PC.pack(frames)
    assert np.array_equal(cnt, m) and all(np.array_equal(I[i, :m[i]], idx[i, :m[i]].cpu().numpy()) for i in range(F))
    t = out['table']
    assert (t.lo, t.hi) == (lo - 4, hi + 4) == (out['lo'], out['hi'])
    ref = SC.ref_index_shift(X, I, cnt, t.P.cpu().numpy(), t.status.cpu().numpy(), t.lo, t.hi, tau=TAU)
    print(f'margin of the search on the oracle chain\'s points {ref["margin"]:.3e}')
    assert ref['margin'] > 1e-6
    for k in ('shift', 'score', 'scores', 'flags'):
        assert np.array_equal(sh[k], ref[k]), f'{k}\n{sh[k]}\n{ref[k]}'
    # and the refit is the model of the frames as the run numbered them
    x = out['fit']['model'].cpu().numpy()[:15]
    assert np.abs(x - ch['x']).max() <= ch['tol'] + 1e-8, f'refit {np.abs(x - ch["x"]).max():.3e} off the unshifted chain\'s model'


def test_run_plane_experiment_renumber(cpe, gpu, tmp_path):
    """rendered boards (whose numbering is the open item of DESIGN.md section 3.7): the option runs and adds only its three keys"""
    import warnings
    from PIL import Image
    from cpe_amd import experiment, synth
    b = synth.render_batch(4, H, W, seed=2, scene=synth.Scene(h=H, w=W, target='plane', tilt_deg=4.0), with_gt=False)
    for i in range(4):
        Image.fromarray(b['left'][i].numpy()).save(tmp_path / f'b{i}L.png')
        Image.fromarray(b['right'][i].numpy()).save(tmp_path / f'b{i}R.png')
    lens = lambda K: dict(IntrinsicMatrix=np.asarray(K, dtype=np.float64).tolist(), RadialDistortion=[0.0, 0.0], TangentialDistortion=[0.0, 0.0])
    (tmp_path / 'cam.json').write_text(json.dumps(dict(LeftCamera=lens(b['K1']), RightCamera=lens(b['K2']))))
    args = (str(tmp_path), str(tmp_path / 'cam.json'), b['K1'], b['K2'], b['T21'])
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        plain = experiment.run_plane_experiment(*args, device=gpu)
        res = experiment.run_plane_experiment(*args, device=gpu, projector=dict(tau=TAU, renumber=dict(win=(2, 2), min_score=4)))
    assert set(res) == set(plain) | {'projector', 'projector_shifted', 'projector_renumbered'}
    for k in ('records', 'P', 'T', 'pts3', 'idx', 'cnt', 'inlier_mask'):
        assert res[k].cpu().numpy().tobytes() == plain[k].cpu().numpy().tobytes(), k
    pm = res['projector']
    assert pm is not None and set(pm) == {'fit', 'model', 'laser_table', 'first', 'shift'} and pm['model'].family0 == 'row'
    assert isinstance(res['projector_renumbered'], list) and tuple(pm['shift']['scores'].shape) == (4, 10)
    print(f'boards: model status {pm["model"].status}, renumbered {res["projector_renumbered"]}, shifted {res["projector_shifted"]}')
