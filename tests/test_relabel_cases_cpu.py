"""The reference and the cases of tests/relabel_cases.py, checked without a GPU: the declaration, that the rule recovers the true
indices behind every label pattern, the margins that let the GPU test compare integers exactly, and the rule on the oracle's
detections of rendered boards.

Measured with ref_grid_relabel (defaults: min_pts 3, merge_frac 0.65) on the oracle's planar detections of
synth.render_batch(4, 480, 640, seed, Scene(target='plane', tilt_deg)), tilts 4, 20, 30 deg x seeds 2, 4, 7 = 36 frames; a pair
is two points of equal ids in the two images, triangulated with oracle.triangulate:

    on the detector's ids   0-43 of 67-97 pairs per frame lie within 1 mm of the true board (worst share 43 / 93)
    re-labelled             30 of 36 frames have every pair within 1 mm (70-84 pairs, rms 0.12-0.59 mm); the other six keep
                            60 / 70, 65 / 70, 70 / 82 (85.4 %, the worst), 72 / 84, 77 / 81 and 83 / 84

and the free table of ref_index_planes over 8 boards (pairs with a reprojection error < 1 px, a band of 1 mm per frame)
against table_tri_cases.true_table(scene), relabel_cases.TABLE_MEASURED (TABLE_BOUNDS are twice these: one seed's spread is not known
better):

    tilt 30, seed 7   19 lines, worst plane 0.1683 deg, median 0.0347 deg; the planes meet within 0.2503 mm rms at a centre
                      1.1313 mm from the true one (on the detector's ids: 58.3 deg, 83 mm)
    tilt 20, seed 4   2.583 deg, 16.79 mm, 3.98 mm rms: some frames stay a line off (asserted below as it is, not bounded:
                      what such frames are left to is the index-shift chain, tests/test_relabel_pipeline_gpu.py)"""
import re

import numpy as np
import pytest

import relabel_cases as RC

TABLE_MEASURED, TABLE_BOUNDS = RC.TABLE_MEASURED, RC.TABLE_BOUNDS


def test_symbol_is_declared(cpe):
    import os
    assert 'cpe_grid_relabel_batch' in cpe.lib.declared_symbols()
    res, args = cpe.lib._SIGS['cpe_grid_relabel_batch']
    assert len(args) == 16
    hdr = open(os.path.join(os.path.dirname(cpe.lib.SO_PATH), '..', 'include', 'cpe.h')).read()
    assert int(re.search(r'#define CPE_VERSION (\d+)', hdr).group(1)) >= 123 and '123: cpe_grid_relabel_batch' in hdr
    assert [n for n, _ in cpe.lib.CpeRelabelParams._fields_] == ['swap', 'min_pts', 'merge_frac', 'dir']
    for name, val in (('FLAG_NO_CENTRE', RC.NO_CENTRE), ('FLAG_OVERFLOW', RC.OVERFLOW), ('FLAG_FEW_LINES', RC.FEW_LINES),
                      ('LINE_KEPT', RC.KEPT), ('LINE_UNSUPPORTED', RC.UNSUPPORTED), ('LINE_PHANTOM', RC.PHANTOM), ('MAX_INC', RC.MAX_INC)):
        assert int(re.search(rf'#define CPE_RELABEL_{name} (\d+)', hdr).group(1)) == val
    assert (cpe.fit.RELABEL_NO_CENTRE, cpe.fit.RELABEL_OVERFLOW, cpe.fit.RELABEL_FEW_LINES) == (RC.NO_CENTRE, RC.OVERFLOW, RC.FEW_LINES)
    assert (cpe.fit.LINE_KEPT, cpe.fit.LINE_UNSUPPORTED, cpe.fit.LINE_PHANTOM) == (RC.KEPT, RC.UNSUPPORTED, RC.PHANTOM)


@pytest.mark.parametrize('name', list(RC.cases()))
def test_margin_tolerance_and_truth(name):
    case, r = RC.cases()[name], RC.reference(name)
    assert r['margin'] > 1e-6, f'{name}: a decision lies within {r["margin"]:.2e} of its threshold'
    assert r['tol'].max() <= 1e-6
    if case['true'] is not None:
        RC.check_true(case, r)


def test_cases_cover_what_they_name():
    R = RC.reference
    full = 13 * 9
    for name in ('identity', 'reflection', 'permutation', 'offset'):
        assert R(name)['cnt'].tolist() == [full] * 4 and not R(name)['flags'].any()
        assert np.array_equal(R(name)['id'], R('identity')['id']) and np.array_equal(R(name)['src'], R('identity')['src'])
    assert R('int32 ends')['label'][0, 0, 0] == RC.I32_MIN and R('int32 ends')['label'][0, 1, 8] == RC.I32_MAX
    m = R('measured pattern')
    assert m['counts'][:, 0].tolist() == [[14, 14, 2, 12]] * 3 and m['counts'][:, 1].tolist() == [[8, 8, 1, 7]] * 3
    assert m['cnt'].tolist() == [12 * 7 - 3] * 3
    assert (m['state'][:, 0, 5] == RC.PHANTOM).all() and (m['state'][:, 0, 7] == RC.PHANTOM).all()     # the labels -1 and +1
    assert (m['state'][:, 1, 7] == RC.PHANTOM).all() and (m['points'][:, 1, 7] == 3).all()             # label 4: the fragment
    one, two = R('one line removed'), R('two lines removed')
    assert sorted(set(one['id'][0, :one['cnt'][0], 0].tolist())) == [-6, -5, -4, -3, -2, -1, 0, 1, 3, 4, 5, 6]
    assert sorted(set(two['id'][0, :two['cnt'][0], 0].tolist())) == [-6, -5, -4, -3, -2, -1, 0, 1, 4, 5, 6]
    assert sorted(set(two['id'][2, :two['cnt'][2], 1].tolist())) == [-4, -3, -2, -1, 0, 1, 4]
    s = R('single line')
    assert s['flags'].tolist() == [RC.FEW_LINES << 1] * 2 + [RC.FEW_LINES] and not s['cnt'].any() and s['counts'][0, 0].tolist() == [1, 1, 0, 1]
    assert s['index'][0, 0, 0] == 0 and s['state'][0, 0, 0] == RC.KEPT and (s['state'][0, 1, :9] == RC.UNSUPPORTED).all()
    assert (R('single point per line')['flags'] == RC.FEW_LINES * 3).all()
    assert R('two rows min_pts 2')['cnt'].tolist() == [18, 18] and R('min_pts 5')['cnt'].tolist() == [65] * 3
    d = R('dir -1')
    assert np.array_equal(d['id'][:3, :, 0], -R('identity')['id'][:3, :, 0]) and np.array_equal(d['id'][:3, :, 1], R('identity')['id'][:3, :, 1])
    assert np.array_equal(R('swap 1 transposed')['id'][..., ::-1], R('identity')['id'][:3])
    assert R('nan inf pixels')['cnt'].tolist() == [114, 114, 117]
    assert R('nan centre')['flags'].tolist() == [0, RC.NO_CENTRE, RC.NO_CENTRE] and R('nan centre')['cnt'].tolist() == [full, 0, 0]
    for k, n in (('1 lines', 1), ('2 lines', 2), ('3 lines', 3), ('64 lines', 64), ('65 lines', 65), ('256 lines', 256)):
        assert R(k)['counts'][0, 0].tolist() == [n, n, 0, n]
    assert R('256 lines')['cnt'].tolist() == [RC.MAXP] and R('span 255')['cnt'].tolist() == [RC.MAXP]
    assert R('span 256')['flags'].tolist() == [RC.OVERFLOW, 0] and R('span 256')['cnt'].tolist() == [0, full]
    assert R('span 256 component 1')['flags'].tolist() == [RC.OVERFLOW]
    assert R('counts')['cnt'].tolist() == [0, 0, 0, 0, 63, 64, 65, 2048, 2048]
    assert len(RC.cases()['65 images']['tables']) == 65 and len(RC.cases()['permutation']['tables']) == 4


@pytest.fixture(scope='module')
def rendered(orc):
    """per rendered frame: (good, pairs) on the detector's ids and re-labelled"""
    out = {}
    for tilt, seed in RC.RENDERED:
        b = RC.boards(tilt, seed)
        for i, f in enumerate(RC.oracle_frames(tilt, seed)):
            r_det = RC.off_board(b, i, *[(d['xy'], d['id']) for d in f['det']])[0]
            r_new = RC.off_board(b, i, *f['tables'])[0]
            good = r_new[np.abs(r_new) < 1]
            out[tilt, seed, i] = dict(det=(int((np.abs(r_det) < 1).sum()), len(r_det)), new=(len(good), len(r_new)),
                                      rms=float(np.sqrt((good * good).mean())))
            print(tilt, seed, i, out[tilt, seed, i])
    return out


def test_rendered_boards_pair_on_the_true_lines(rendered):
    """at least 30 of the 36 frames have every joined pair within 1 mm of the true board, none keeps fewer than 80 %; on the
    detector's own ids no frame has more than 60 % (module docstring: 30 frames, worst 85.4 %; worst 43 of 93)"""
    assert len(rendered) == 36
    full = [k for k, v in rendered.items() if v['new'][0] == v['new'][1]]
    worst = min(v['new'][0] / v['new'][1] for v in rendered.values())
    worst_det = max(v['det'][0] / v['det'][1] for v in rendered.values())
    print(f'{len(full)} frames complete, worst share {worst:.3f}; on the detector\'s ids at most {worst_det:.3f}')
    assert all(v['new'][1] >= 60 for v in rendered.values())
    assert len(full) >= 30 and worst >= 0.80
    assert worst_det <= 0.60
    assert sorted(v['new'] for v in rendered.values() if v['new'][0] != v['new'][1]) == [(60, 70), (65, 70), (70, 82), (72, 84), (77, 81), (83, 84)]
    assert all(0.1 < v['rms'] < 0.6 for v in rendered.values())


def test_free_table_of_eight_boards(orc):
    """(30 deg, seed 7): within TABLE_BOUNDS of the true table; on the detector's ids tens of degrees and centimetres off.
    (20 deg, seed 4): frames stay a row off and the table shows it -- recorded, not bounded"""
    t = RC.board_table(30.0, 7)
    f = dict(t['figures'], centre_rms_mm=float(t['table']['centre'][3]))
    print('30 deg, seed 7:', f, t['frames'])
    assert t['table']['centre_status'] == 0 and (t['lo'], t['hi']) == (-5, 6) and f['lines'] == 19
    for k, bound in TABLE_BOUNDS.items():
        assert f[k] <= bound, f'{k}: {f[k]:.4f} > {bound:.4f}'
    raw = RC.board_table(30.0, 7, relabelled=False)
    print('on the detector\'s ids:', raw['figures'])
    assert raw['figures']['worst_deg'] > 20 and raw['figures']['centre_mm'] > 20
    off = RC.board_table(20.0, 4)
    g = dict(off['figures'], centre_rms_mm=float(off['table']['centre'][3]))
    print('20 deg, seed 4:', g, off['frames'])
    assert g['worst_deg'] > TABLE_BOUNDS['worst_deg'] and g['centre_rms_mm'] > 1.0        # not `consistent`: the leftover frames show
