"""cpe_match_offset_batch (csrc/fit.hip k_match_prepare / k_match_score / k_match_pick) against the Python reference of
tests/match_offset_cases.py at tolerance 0; the fit with the search off and on unshifted tables against the fit without it;
and the frame the feature is for: frame 1 of synth.render_batch(8, 480, 640, seed=3), whose left table the detector numbers
one column too high."""
import functools
import json

import numpy as np
import pytest
import torch

import match_offset_cases as M
from test_ground_truth import BOUNDS

pytestmark = pytest.mark.gpu


def _tables(cpe, gpu, group, poison=True):
    xy1, id1, c1, xy2, id2, c2 = (torch.from_numpy(a).to(gpu) for a in M.pack(group, poison))
    return cpe.fit.GridTables(xy1, id1, c1), cpe.fit.GridTables(xy2, id2, c2)


def _groups():
    """cases that can share a call: the same rig and the same parameters"""
    g = {}
    for c in M.cases():
        g.setdefault((c['size'], tuple(sorted(c['params'].items()))), []).append(c)
    return list(g.values())


@pytest.mark.parametrize('poison', [True, False], ids=['poison_padding', 'zero_padding'])
def test_kernel_equals_reference_exactly(cpe, gpu, poison):
    refs = M.references()
    seen = 0
    for group in _groups():
        if not poison:
            group = group[::-1]
        K1, K2, T21 = M.case_rig(group[0])
        g1, g2 = _tables(cpe, gpu, group, poison)
        out = cpe.fit.match_offset_batch(g1, g2, K1, K2, T21, M.R, **group[0]['params'])
        torch.cuda.synchronize()
        off, sc, scs, fl, ido = (out[k].cpu().numpy() for k in ('offset', 'score', 'scores', 'flags', 'id1'))
        assert np.array_equal(out['tables'].id.cpu().numpy(), ido) and out['tables'].xy is g1.xy and out['tables'].cnt is g1.cnt
        for i, c in enumerate(group):
            ref = refs[c['name']]
            print(c['name'], 'gpu offset', off[i], 'score', sc[i], 'flags', fl[i], '| ref', ref['offset'], ref['score'], ref['flags'])
            assert np.array_equal(scs[i], ref['scores']), c['name']
            assert np.array_equal(off[i], ref['offset']) and np.array_equal(sc[i], ref['score']) and fl[i] == ref['flags'], c['name']
            n1 = len(ref['id1_out'])
            assert np.array_equal(ido[i, :n1], ref['id1_out']), c['name']
            assert not ido[i, n1:].any(), c['name']                # slots past the count are not written
            seen += 1
    assert seen == len(M.cases())


def test_scores_are_optional_and_defaults_are_the_header_s(cpe, gpu):
    group = [c for c in M.cases() if c['name'] in ('gt640_shift1_0', 'garbage10')]
    K1, K2, T21 = M.case_rig(group[0])
    g1, g2 = _tables(cpe, gpu, group)
    a = cpe.fit.match_offset_batch(g1, g2, K1, K2, T21, M.R)                       # defaults of fit.py
    b = cpe.fit.match_offset_batch(g1, g2, K1, K2, T21, M.R, want_scores=False)
    # NULL params: the defaults of the library
    L = cpe.lib.load()
    n = 2
    ws_bytes = L.cpe_match_offset_workspace_bytes(n, 4, 4)
    assert ws_bytes == n * 4 * (8 + 2 * 81 + 128 * 128) and L.cpe_match_offset_workspace_bytes(n, 9, 0) == 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=gpu)
    K = [torch.as_tensor(np.asarray(k, np.float64).ravel()).to(gpu) for k in (K1, K2, T21)]
    off = torch.zeros((n, 2), dtype=torch.int32, device=gpu); sc = torch.zeros((n, 4), dtype=torch.int32, device=gpu)
    fl = torch.zeros(n, dtype=torch.int32, device=gpu); ido = torch.zeros((n, M.MAXP, 2), dtype=torch.int32, device=gpu)
    args = [g1.xy.data_ptr(), g1.id.data_ptr(), g1.cnt.data_ptr(), g2.xy.data_ptr(), g2.id.data_ptr(), g2.cnt.data_ptr(), n,
            K[0].data_ptr(), K[1].data_ptr(), K[2].data_ptr(), M.R, None, ws.data_ptr(), ws_bytes, off.data_ptr(), sc.data_ptr(), None,
            fl.data_ptr(), ido.data_ptr(), torch.cuda.current_stream().cuda_stream]
    cpe.lib.check(L.cpe_match_offset_batch(*args), 'cpe_match_offset_batch')
    torch.cuda.synchronize()
    assert b['scores'] is None
    for x in (b, dict(offset=off, score=sc, flags=fl, id1=ido)):
        for k in ('offset', 'score', 'flags', 'id1'):
            assert torch.equal(a[k], x[k]), k
    assert a['offset'].cpu().tolist() == [[1, 0], [0, 0]] and a['flags'].cpu().tolist()[0] == M.SHIFTED and a['flags'].cpu().tolist()[1] & M.WEAK
    # refusals: a small workspace, a window past CPE_MATCH_MAX_WIN, id1_out = id1
    short = list(args); short[13] = ws_bytes - 1
    assert L.cpe_match_offset_batch(*short) == -3
    alias = list(args); alias[18] = g1.id.data_ptr()
    assert L.cpe_match_offset_batch(*alias) == -1
    prm = cpe.lib.CpeMatchParams(9, 4, 0.3, 0.5, 8, 8)
    import ctypes
    bad = list(args); bad[11] = ctypes.addressof(prm)
    assert L.cpe_match_offset_batch(*bad) == -1
    with pytest.raises(ValueError):
        cpe.fit.match_offset_batch(g1, g2, K1, K2, T21, M.R, win_c=9)


FIT_KEYS = ('p1', 'p2', 'idx', 'pts3', 'err', 'm', 'mean_err', 'flags', 'cyl_raw', 'cyl', 'T', 'fvals', 'iters', 'status')


def test_no_change_when_off_or_unshifted(cpe, gpu):
    """match=None is today's call (selector, then fit) plus three zero tensors; with the search on and tables that need no
    shift every existing output is the same"""
    fit = cpe.fit
    names = ('gt640_shift0_0', 'lattice63', 'window0', 'span127', 'duplicates', 'empty_left', 'kept4', 'garbage10')
    group = []
    for c in M.cases():
        if c['name'] in names:
            # the tables of the shifted cases without their shift: the right indices moved back
            t2 = c['t2'].copy()
            if c['expect_offset'] is not None and len(t2):
                t2[:, 2:4] -= np.array(c['expect_offset'])
            group.append(dict(c, t2=t2))
    assert len(group) == len(names)
    K1, K2, T21 = M.case_rig(group[0])
    g1, g2 = _tables(cpe, gpu, group)
    sel = fit.select_triangulate_batch(g1, g2, K1, K2, T21, fit.SEL_CHOOSE_IDX, 3, 0.3)
    today = dict(sel)
    today.update(fit.fit_cylinder_batch(sel['pts3'], sel['m'], M.R))
    off = fit.fit_single_cylinder_batch(g1, g2, K1, K2, T21, M.R)
    on = fit.fit_single_cylinder_batch(g1, g2, K1, K2, T21, M.R, match={})
    torch.cuda.synchronize()
    assert (today['status'] == 0).sum() >= 5
    for k in FIT_KEYS:
        assert torch.equal(today[k], off[k]), k
        assert torch.equal(today[k], on[k]), k
    for k, shape in (('offset', (len(group), 2)), ('match_score', (len(group), 4)), ('match_flags', (len(group),))):
        assert off[k].dtype == torch.int32 and tuple(off[k].shape) == shape and not off[k].any()
        assert on[k].dtype == torch.int32 and tuple(on[k].shape) == shape
    assert not on['offset'].any() and not (on['match_flags'] & M.SHIFTED).any()
    assert on['match_score'][:, 0].cpu().tolist()[0] >= 8


def _axis_error(cyl, org0, dir0):
    o, d = np.asarray(cyl[:3]), np.asarray(cyl[3:])
    d = d / np.linalg.norm(d)
    ang = np.degrees(np.arccos(min(1.0, abs(float(d @ dir0)))))
    off = (o - org0) - ((o - org0) @ dir0) * dir0
    return ang, float(np.linalg.norm(off))


@functools.lru_cache(maxsize=None)
def _rendered():
    from cpe_amd import synth
    return synth.render_batch(8, 480, 640, seed=3)


def test_end_to_end_frame_with_a_shifted_left_table(cpe, gpu):
    from cpe_amd import pipeline
    b = _rendered()
    left, right = b['left'].to(gpu), b['right'].to(gpu)
    bound = BOUNDS[(480, 640)]
    recs = {}
    for key, match in (('off', None), ('on', {})):
        pipe = pipeline.FramePipeline(480, 640, b['K1'], b['K2'], b['T21'], b['radius'], chunk=8, device=gpu, match=match)
        rec, det, out = pipe.run_chunk(left, right)
        torch.cuda.synchronize()
        recs[key] = (rec.cpu().numpy(), {k: out[k].cpu().numpy() for k in ('offset', 'match_score', 'match_flags', 'status', 'm')})
    rec0, out0 = recs['off']
    rec1, out1 = recs['on']
    ang0, off0 = _axis_error(rec0[1, 6:12], b['axis_org'][1], b['axis_dir'][1])
    ang1, off1 = _axis_error(rec1[1, 6:12], b['axis_org'][1], b['axis_dir'][1])
    print('frame 1 without the search: status', out0['status'][1], 'm', out0['m'][1], 'axis', ang0, 'deg', off0, 'mm')
    print('frame 1 with the search   : status', out1['status'][1], 'm', out1['m'][1], 'axis', ang1, 'deg', off1, 'mm', 'offset', out1['offset'][1],
          'score', out1['match_score'][1], 'flags', out1['match_flags'][1])
    # what the feature is for: a status-0 fit that is silently wrong
    assert out0['status'][1] == 0 and off0 > bound['origin']
    assert not out0['offset'].any() and not out0['match_score'].any() and not out0['match_flags'].any()
    assert out1['offset'][1].tolist() == [-1, 0] and out1['match_flags'][1] == M.SHIFTED
    assert out1['status'][1] == 0 and ang1 <= bound['angle'] and off1 <= bound['origin']
    others = [i for i in range(8) if i != 1]
    assert not out1['offset'][others].any() and not (out1['match_flags'][others] & M.SHIFTED).any()
    assert np.array_equal(rec0[others].view(np.uint64), rec1[others].view(np.uint64))

    # the pipeline hands the new per-frame outputs out beside the fit outputs
    fits = pipeline.alloc_fits(8, gpu)
    assert fits['offset'].shape == (8, 2) and fits['match_score'].shape == (8, 4) and fits['match_flags'].shape == (8,)
    assert pipeline.REC == 16


def test_run_experiment_uses_shifted_frames_and_skips_weak_ones(cpe, gpu, tmp_path):
    """frames 0-3 of the rendered batch (frame 1 needs the shift) and a black pair (no tables: WEAK) as a folder"""
    from PIL import Image
    from cpe_amd import experiment
    b = _rendered()
    stems = ['-10', '-21', '00', '1-2']
    L, Rr = b['left'].numpy(), b['right'].numpy()
    for i, st in enumerate(stems):
        Image.fromarray(L[i]).save(tmp_path / f'{st}L.png')
        Image.fromarray(Rr[i]).save(tmp_path / f'{st}R.png')
    for side in 'LR':
        Image.fromarray(np.zeros((480, 640), np.uint8)).save(tmp_path / f'3-3{side}.png')
    lens = lambda K: dict(IntrinsicMatrix=np.asarray(K, dtype=np.float64).tolist(), RadialDistortion=[0.0, 0.0], TangentialDistortion=[0.0, 0.0])
    (tmp_path / 'cam.json').write_text(json.dumps(dict(LeftCamera=lens(b['K1']), RightCamera=lens(b['K2']))))
    args = (str(tmp_path), str(tmp_path / 'cam.json'), b['K1'], b['K2'], b['T21'], b['radius'])
    plain = experiment.run_experiment(*args, chunk=4, multi_frame='lm')
    res = experiment.run_experiment(*args, chunk=4, multi_frame='lm', match_offset={})
    assert set(res) == set(plain) | {'offset', 'match_score', 'match_flags'}
    names = res['names']
    shifted, black = names.index('-21'), names.index('3-3')
    fl = res['match_flags'].cpu().tolist()
    assert res['offset'].cpu().tolist()[shifted] == [-1, 0] and fl[shifted] == M.SHIFTED
    assert fl[black] & M.WEAK
    assert [s['index'] for s in res['skipped']] == [black] and res['skipped'][0]['match'] == fl[black]
    assert all('match' not in s for s in plain['skipped']) and [s['index'] for s in plain['skipped']] == [black]
    others = [i for i in range(len(names)) if i != shifted]
    assert np.array_equal(res['records'].cpu().numpy()[others].view(np.uint64), plain['records'].cpu().numpy()[others].view(np.uint64))
    assert res['T_cam_agv'] is not None and res['T_cam_agv'] != plain['T_cam_agv']      # the corrected frame is used
