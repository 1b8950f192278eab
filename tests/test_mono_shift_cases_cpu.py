"""The references of tests/mono_shift_cases.py on the CPU: the vote cases keep their margins, and the repair chain -- votes, the
candidates' fits, the rms rule, one re-numbering round, with the references and the oracle's LM alone -- finds every frame-wide
shift, keeps no point under a wrong index, rejects the epipolar alias and ends inside MONO_REPAIR_BOUNDS."""
import math
import os
import re

import numpy as np
import pytest

import mono_shift_cases as MC
import table_tri_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_call():
    hdr = open(os.path.join(ROOT, 'include', 'cpe.h')).read()
    assert int(re.search(r'#define CPE_VERSION (\d+)', hdr).group(1)) >= 127 and '127: cpe_mono_shift_batch' in hdr
    assert 'CPE_API int32_t cpe_mono_shift_batch(' in hdr and 'it lies on the plane of whatever index it carries. */' not in hdr


@pytest.mark.parametrize('name', list(MC.cases()))
def test_case_margins_and_shape(name):
    """no decision of a case lies within 1e-6 of its gate; the outputs are consistent with themselves"""
    case, p = MC.cases()[name], MC.params(MC.cases()[name])
    ncand = (2 * p['win'][0] + 1) * (2 * p['win'][1] + 1)
    for f, r in enumerate(MC.reference(name)):
        assert r['margin'] > 1e-6, f'{name}, frame {f}: margin {r["margin"]:.3e}'
        assert r['scores'].shape == (ncand,) and r['cand'].shape == (p['top_k'], 2)
        top = sorted(r['scores'], reverse=True)
        assert r['score'][0] == top[0] == r['cand_score'][0] and r['score'][1] == (top[1] if ncand > 1 else 0)
        assert r['score'][2] == r['scores'][p['win'][0] * (2 * p['win'][1] + 1) + p['win'][1]]
        assert (r['cand_score'][min(ncand, p['top_k']):] == -1).all() and not r['cand'][min(ncand, p['top_k']):].any()
        assert (np.diff(r['cand_score'][:min(ncand, p['top_k'])]) <= 0).all()


def test_cases_cover_what_they_claim():
    ref = lambda name: MC.reference(name)
    assert [tuple(r['cand'][0]) for r in ref('edge winner')][:3] == [(4, 0), (1, -4), (-2, 2)]
    assert [int(r['flags']) & MC.EDGE for r in ref('edge winner')] == [MC.EDGE, MC.EDGE, 0, 0]
    tie = ref('alias ties at tau 0.5')[0]
    assert tie['cand_score'][0] == tie['cand_score'][1] == 283 and int(tie['flags']) & MC.WEAK and tuple(tie['cand'][0]) == (2, -1)
    lose = ref('alias loses at tau 0.1')[0]
    assert lose['cand_score'][0] == 283 and lose['cand_score'][1] < 283 and tuple(lose['cand'][1]) == (-3, 1)
    nat = ref('natural')[0]
    assert int(nat['flags']) == 0 and nat['score'].tolist() == [424, 0, 424, 424] and nat['rms'][0] < 0.05
    assert int(ref('empty frame, min_score 0')[0]['flags']) == 0 and int(ref('empty frame, min_score 8')[0]['flags']) == MC.WEAK
    assert ref('wild indices')[0]['score'][3] == 424 and ref('nan pixels')[0]['score'][3] == 420
    assert ref('count 2048')[0]['score'][3] == 2048 and tuple(ref('count 2048')[0]['cand'][0]) == (0, 1)
    assert len(MC.cases()['65 frames']['frames']) == 65 and len(MC.cases()['one frame']['frames']) == 1


def test_the_residuals_separate_right_from_wrong_pairs():
    """at the true indices every point's max |res| stays below tau = 0.1 mm (measured: 0.089 mm), and no other shift of the window
    keeps all points below 0.39 mm (measured: the rms of (res0, res1) is at least 0.43 mm there): what makes the vote exact"""
    for cam in (1, 2):
        for which in ('rig', 'noisy'):
            for seed in range(5):
                idx, _, uv1, uv2 = TC.cylinder_frame(0.25, seed)
                K, Tc = TC.camera(cam)
                t = MC.chain_table(which, seed)
                r = MC.ref_mono_shift(uv1 if cam == 1 else uv2, idx, len(idx), K, Tc, t['P'], t['status'], t['lo'], t['hi'], tau=0.1)
                assert r['score'][0] == r['score'][2] == 424 and r['rms'][0] < 0.05
                wide = MC.ref_mono_shift(uv1 if cam == 1 else uv2, idx, len(idx), K, Tc, t['P'], t['status'], t['lo'], t['hi'], tau=0.39)
                others = np.delete(wide['scores'], 40)
                assert others.max() < 424, 'a wrong pair of indices keeps every point below 0.39 mm'


@pytest.mark.parametrize('name', MC.SCENARIOS + ('frame_shift_w8',))
def test_chain(name):
    """the chain on both cameras, both tables (frame_shift_w8: the table that covers the window) and the seeds 0..4"""
    tables = ('rig',) if name == 'frame_shift_w8' else ('rig', 'noisy')
    for which in tables:
        kept, deg, mm, ratios = [], [], [], []
        for cam in (1, 2):
            for seed in range(5):
                s = MC.scenario(name, seed, cam)
                r = MC.chain_reference(name, seed, cam, which)
                e = MC.chain_errors(r, s['true'])
                what = f'{name}, {which} table, camera {cam}, seed {seed}'
                assert r['vote']['margin'] > 1e-6, f'{what}: vote margin {r["vote"]["margin"]:.3e}'
                assert r['shift'] == s['shift'], f'{what}: shift {r["shift"]}, true {s["shift"]}'
                assert r['trusted'] == MC.TRUSTED[name] and bool(r['flags'] & MC.WEAK) != r['trusted'], f'{what}: flags {r["flags"]}'
                assert r.get('rms_gate', math.inf) > 0.1, f'{what}: the rms rule decides within {r["rms_gate"]:.3f} of its gate'
                assert r['round_taken'] == 1 and e['wrong'] == 0, f'{what}: {e["wrong"]} kept points carry a wrong index'
                b = MC.MONO_REPAIR_BOUNDS[name]
                assert e['axis_deg'] <= b['axis_deg'] and e['axis_mm'] <= b['axis_mm'], f'{what}: {e}'
                kept.append(e['kept']); deg.append(e['axis_deg']); mm.append(e['axis_mm'])
                if math.isfinite(r['ratio']):
                    ratios.append(r['ratio'])
        got = dict(kept=min(kept), axis_deg=round(max(deg), 4), axis_mm=round(max(mm), 4), ratio=round(min(ratios), 3) if ratios else None)
        print(f'{name}, {which}: {got}')
        assert got == MC.MEASURED[name, which], f'{name}, {which}: measured {got}, recorded {MC.MEASURED[name, which]}'
        if name == 'frame_shift_w8':
            assert len(ratios) == 10 and min(ratios) > 1.5, 'the alias is eligible for every seed and camera and loses by the rms rule'


def test_alias_in_the_window_is_eligible_and_rejected():
    """frame_shift_w8: the alias has the second most votes, at least half the winner's, and a fit rms 2.5 times the true shift's"""
    for cam, alias in ((1, (-7, 3)), (2, (5, 4))):
        r = MC.chain_reference('frame_shift_w8', 0, cam, 'rig')
        assert tuple(r['vote']['cand'][1]) == alias and r['eligible'][:2].all() and r['cand_rms'][1] > 2.4 * r['cand_rms'][0]
        assert r['shift'] == (-2, 1) and r['flags'] == MC.SHIFTED
