"""The calls whose output bits tests/golden/lm_parent_bits.npz pins: the iterates of the two Levenberg-Marquardt kernels that
no oracle restates bit for bit, cpe_multi_frame_fit_lm_batch and cpe_frame_angles_lm_batch.  tools/record_lm_bits.py runs
collect() at the commit BEFORE a change to those kernels and stores the bits; test_lm_recorded_bits_gpu.py runs it again and
compares.  Every input is regenerated from the seeds of multiframe_cases / frame_angles_cases, so the file holds outputs only.

    multi-frame LM   scenes F2, F3, F17, F33: alone, max_iter 1 and 2, from the far start of
                     test_far_start_ends_within_the_caps, as the four-group table of test_groups_equal_single_calls with and
                     without its frame_ok mask, and the status cases of test_statuses
    frame angles     the eight scenes of frame_angles_cases.GPU_SEEDS: the closed-form start, the nominal start of
                     test_given_start, max_iter 1 from zero, the pole and far starts of
                     test_iteration_cap_and_far_start_end_within_the_caps (F = 13 and 65), the poses of test_several_poses
"""
import math

import numpy as np

import frame_angles_cases as fc
import multiframe_cases as mc

R = mc.RADIUS
MF_NAMES = sorted(mc.CASES)                                                     # F17 F2 F3 F33, the order of the table
MF_KEYS = ('x0', 'x', 'T', 'fvals', 'iters', 'n_used', 'status', 'frame_terms')
FA_KEYS = ('angles0', 'angles', 'fvals', 'iters', 'TAGV', 'Tcyl', 'status')
FA_SCENES = [(F, noise) for F in fc.GPU_FRAMES for noise in fc.GPU_NOISES]
GROUP_START = [22, 55, 0, 17, 17, 19, 22, 18, 55]                               # test_groups_equal_single_calls
MASKED_OUT = [0, 5, 16, 20, 30, 54]
FAR_STARTS = [[1.2, 1.5], [-3.0, -1.56], [0.0, math.pi / 2], [1e6, 0.0]]        # the third lies beyond the tilt limit


def as_bits(a):
    """an output array as the integers the comparison is made on: f64 -> its uint64 bits, i32 as it is"""
    a = np.ascontiguousarray(a)
    if a.dtype == np.float64:
        return a.view(np.uint64)
    assert a.dtype == np.int32, a.dtype
    return a


def collect(dev):
    """-> {call/output: bits}, and per kernel the list of (call, iters [.,2], start evaluations, max_iter or None) the recorder
    checks its coverage conditions on"""
    import torch
    from cpe_amd import fit, multiframe
    out, runs = {}, {'mf': [], 'fa': []}
    host = lambda res, keys: {k: res[k].cpu().numpy() for k in keys}

    def put(call, res):
        for k, v in res.items():
            out[f'{call}/{k}'] = as_bits(v)

    # ------------------------------------------------------------------------------------------------- multi-frame LM
    scenes = {}
    for name in MF_NAMES:
        P, cnt, angles, _ = mc.case_scene(name)
        TAGV = np.stack([mc.get_TAGVcyl(*a).ravel() for a in angles])
        Pd, cd = torch.from_numpy(P).to(dev), torch.from_numpy(cnt).to(dev)
        per = fit.fit_cylinder_batch(Pd, cd, R)
        assert not per['status'].any()
        scenes[name] = dict(Pd=Pd, cd=cd, rawd=per['cyl_raw'].contiguous(), TAGVd=torch.from_numpy(TAGV).to(dev))

    def mf(call, s, **kw):
        res = host(multiframe.fit_multi_frame_gpu(s['Pd'], s['cd'], s['rawd'], s['TAGVd'], R, method='lm', **kw), MF_KEYS)
        put('mf/' + call, res)
        runs['mf'].append((call, res['iters'], 1 if kw.get('x0') is not None else 2, kw.get('max_iter')))
        return res

    single = {}
    for name in MF_NAMES:
        s = scenes[name]
        single[name] = mf(f'{name}/alone', s)
        mf(f'{name}/max_iter1', s, max_iter=1)
        mf(f'{name}/max_iter2', s, max_iter=2)
        quirk = multiframe.fit_multi_frame_gpu(s['Pd'], s['cd'], s['rawd'], s['TAGVd'], R, max_fun_evals=10)
        assert int(quirk['status'][0]) == 0
        mf(f'{name}/far', s, x0=quirk['x0'])
    table = {k: torch.cat([scenes[n][k] for n in MF_NAMES]).contiguous() for k in ('Pd', 'cd', 'rawd', 'TAGVd')}
    ok = np.ones(55, np.int32)
    ok[MASKED_OUT] = 0
    mf('table/all_frames', table, group_start=GROUP_START)
    mf('table/frame_ok', table, group_start=GROUP_START, frame_ok=torch.from_numpy(ok).to(dev))
    s = scenes['F3']
    for i, gs in enumerate(([3, 0], [-1, 3], [0, 4])):
        mf(f'status/range{i}', s, group_start=gs)
    one = torch.tensor([0, 1, 0], dtype=torch.int32, device=dev)
    mf('status/one_kept', s, frame_ok=one)
    mf('status/one_kept_x0', s, frame_ok=one, x0=[[0.0] * 6])
    raw = s['rawd'].clone()
    raw[[0, 2]] = 0
    blind = dict(s, rawd=raw.clone())
    mf('status/one_usable', blind)
    raw[0, 1, 3] = float('nan')
    mf('status/nan_row', dict(s, rawd=raw))
    mf('status/one_usable_x0', blind, x0=torch.from_numpy(single['F3']['x0'].copy()).to(dev))

    # --------------------------------------------------------------------------------------------------- frame angles
    def fa(call, s, **kw):
        args = dict(pts3=s['Pd'], cnt=s['cd'], cyl_raw=s['rawd'], T=s['Td'], radius=R)
        args.update(kw)
        res = host(multiframe.estimate_frame_angles_gpu(**args), FA_KEYS)
        put('fa/' + call, res)
        runs['fa'].append((call, res['iters'], 1, kw.get('max_iter')))
        return res

    for F, noise in FA_SCENES:
        P, cnt, angles, Ttrue = fc.gpu_scene(F, noise)
        Pd, cd = torch.from_numpy(P).to(dev), torch.from_numpy(cnt).to(dev)
        per = fit.fit_cylinder_batch(Pd, cd, R)
        assert not per['status'].any()
        s = dict(Pd=Pd, cd=cd, rawd=per['cyl_raw'].contiguous(), Td=torch.from_numpy(Ttrue.reshape(1, 16)).to(dev))
        tag = f'F{F}_noise{noise}'
        fa(f'{tag}/default', s)
        fa(f'{tag}/nominal', s, a0=torch.from_numpy(np.deg2rad(np.round(np.rad2deg(angles)))).to(dev))
        fa(f'{tag}/max_iter1', s, a0=torch.zeros((F, 2), dtype=torch.float64, device=dev), max_iter=1)
        if F >= 13:
            fa(f'{tag}/far', s, a0=torch.tensor((FAR_STARTS * 17)[:F], dtype=torch.float64, device=dev))
        if (F, noise) == (13, 0.05):                                            # test_several_poses
            T1, T2 = Ttrue.copy(), Ttrue.copy()
            T1[:3, 3] += [1.0, -2.0, 3.0]
            c, sn = math.cos(0.01), math.sin(0.01)
            T2[:3, :3] = np.array([[c, -sn, 0], [sn, c, 0], [0, 0, 1.0]]) @ T2[:3, :3]
            idx = np.array([i % 3 for i in range(F)], np.int32)
            idx[:3] = [2, 2, 0]
            fa(f'{tag}/poses', s, T=torch.from_numpy(np.stack([Ttrue.ravel(), T1.ravel(), T2.ravel()])).to(dev),
               pose_index=torch.from_numpy(idx).to(dev))
    return out, runs
