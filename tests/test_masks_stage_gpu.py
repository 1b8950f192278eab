"""The masks stage on its own (cpe_debug_masks, include/cpe.h) against the oracle, with tolerance 0.

The entry runs joints_mask_stage, spot_stage and masks_stage of the library, then the 7x7 blur, on a ridge mask, a grey frame,
a mask_contour, a rectangle and a region status of the test's choosing (tests/masks_cases.py: one idea per generator; the
CPU file tests/test_masks_generators_cpu.py checks that each reaches its edge).  Per frame:
  - hmask / vmask against stages.extract_joints and a scipy restatement of the 20-tap openings;
  - the joints inside rect (values and order) and n_joints_all;
  - status, r0 and spot against stages.mask_roi_around_center, and blur19 > 240 on every pixel;
  - roi_h / roi_v, and a scipy 3x3 opening of mask & spot & mask_contour;
  - exp_h / exp_v against stages.expand_line_roi(roi, mask_contour, 91 + r0) (201 and 8 .. 700 for the planar target),
    n_seg against its count of valid fragments and gang / glen as f32 bits;
  - the 7x7 blur where the detect path writes it;
  - overflow: 0, or exactly the bit a case is built to hit (the planes of the capped step are then not compared).
Each case runs alone, inside a mixed batch and in reversed order: the three runs are bit-identical."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import masks_cases as M  # noqa: E402
import plane_colour_oracle as PC  # noqa: E402
from masks_cases import scipy_open20, scipy_open3, spot_mask  # noqa: E402

PLANES = ('hmask', 'vmask', 'roi_h', 'roi_v', 'exp_h', 'exp_v', 'blur19', 'blur7')
STATE = ('status', 'r0', 'spot0', 'spot1', 'spot2', 'spot3', 'n_joints', 'n_joints_all', 'n_seg0', 'n_seg1', 'gang0', 'gang1',
         'glen0', 'glen1', 'overflow')


def _run(cpe, gpu, cases, target='cylinder', ws=None):
    """cpe_debug_masks on a list of cases of one frame size -> list of per-frame dicts of numpy results (ws: the workspace to run
    in, as the caller left it)"""
    st = lambda k: torch.from_numpy(np.stack([c[k] for c in cases])).to(gpu)
    rect = torch.tensor([c['rect'] for c in cases], dtype=torch.int32)
    status = torch.tensor([c['status'] for c in cases], dtype=torch.int32)
    ws = cpe.api.debug_masks(st('binary'), st('gray'), st('mc'), rect, status, ws=ws, target=target)
    torch.cuda.synchronize()
    planes = {k: ws.plane(k).cpu().numpy() for k in PLANES}
    joints = ws.plane('joints').cpu().numpy()
    state = ws.state()
    raw = ws.plane('state').cpu().numpy()        # gang / glen as bits
    out = []
    for i in range(len(cases)):
        d = {k: planes[k][i] for k in PLANES}
        d['state'] = state[i]
        names = cpe.api._STATE_FIELDS
        d['bits'] = {k: int(np.uint32(raw[i, names.index(k)])) for k in ('gang0', 'gang1', 'glen0', 'glen1')}
        d['joints'] = joints[i, :min(state[i]['n_joints'], M.MAXJ)].copy()
        out.append(d)
    return out


def _same(a, b, tag):
    for k in PLANES[:-1]:
        assert np.array_equal(a[k], b[k]), (tag, k)
    sa = a['state']
    if sa['status'] == 0:        # the 7x7 blur is written for frames with status 0 only, around rect
        wr = PC.blur7_written(*a['blur7'].shape, (sa['rect0'], sa['rect1'], sa['rect2'], sa['rect3']), sa['r0'])
        assert np.array_equal(a['blur7'][wr], b['blur7'][wr]), (tag, 'blur7')
    for k in STATE:
        assert a['state'][k] == b['state'][k], (tag, k, a['state'][k], b['state'][k])
    if not sa['overflow'] & M.OVF_JOINTS:     # past CPE_MAXJ, which joints are kept is not defined (the frame ends in overflow)
        assert np.array_equal(a['joints'], b['joints']), tag


_REF = {}


def _oracle(name, c, target):
    key = (name, target)
    if key not in _REF:
        _REF[key] = M.oracle(c, target)
    return _REF[key]


def _check(c, g, ref, tag, target='cylinder', ovf=0):
    """one frame of a cpe_debug_masks result against the oracle, tolerance 0"""
    st = g['state']
    assert np.array_equal(g['hmask'], ref['hmask']) and np.array_equal(g['vmask'], ref['vmask']), (tag, 'h / v masks')
    assert np.array_equal(g['hmask'], scipy_open20(c['binary'], True)) and np.array_equal(g['vmask'], scipy_open20(c['binary'], False)), tag
    assert np.array_equal(g['blur19'] > 240, ref['spot_plane']), (tag, 'blur19 > 240', int(((g['blur19'] > 240) != ref['spot_plane']).sum()))
    assert st['overflow'] == ovf, (tag, 'overflow', st['overflow'], ovf)
    assert st['status'] == ref['status'], (tag, 'status', st['status'], ref['status'])
    assert st['r0'] == ref['r0'] and (st['spot0'], st['spot1'], st['spot2'], st['spot3']) == ref['spot'], (tag, 'spot')
    if ref['status'] != 0:
        if ref['status'] == 1:              # no region: nothing of the rectangle is looked at
            for k in ('roi_h', 'roi_v', 'exp_h', 'exp_v'):
                assert not g[k].any(), (tag, k)
        assert st['n_joints'] == 0 and st['n_seg0'] == 0 and st['n_seg1'] == 0, tag
        return
    assert st['n_joints_all'] == len(ref['joints_all']), (tag, 'n_joints_all', st['n_joints_all'], len(ref['joints_all']))
    if ovf & M.OVF_JOINTS:
        assert len(ref['joints']) > M.MAXJ and st['n_joints'] == M.MAXJ, tag
    else:
        assert st['n_joints'] == len(ref['joints']) and np.array_equal(g['joints'], ref['joints']), (tag, 'joints (values, order)')
    cm = spot_mask(c, ref['spot'], target == 'plane')
    for k, m in (('roi_h', ref['hmask']), ('roi_v', ref['vmask'])):
        assert np.array_equal(g[k], ref[k]), (tag, k, int((g[k] != ref[k]).sum()))
        assert np.array_equal(g[k], scipy_open3(m & cm & c['mc'])), (tag, k, 'scipy')
    for which, key in ((0, 'h'), (1, 'v')):
        nc, nv, gang, glen = ref['seg_' + key]
        assert st[f'n_seg{which}'] == nv, (tag, key, 'valid fragments', st[f'n_seg{which}'], nv)
        if nv > M.MAXSEG:
            assert ovf & M.OVF_SEGS, tag
            continue                                   # median and expansion of the first MAXSEG fragments only
        assert (g['bits'][f'gang{which}'], g['bits'][f'glen{which}']) == (gang, glen), (tag, key, 'gang / glen bits')
        if ovf & M.OVF_KERNEL:
            continue                                   # the kernel does not fit: no expansion
        assert np.array_equal(g['exp_' + key], ref['exp_' + key]), (tag, 'exp_' + key, int((g['exp_' + key] != ref['exp_' + key]).sum()))
    h, w = c['gray'].shape
    wr = PC.blur7_written(h, w, c['rect'], ref['r0'])
    assert np.array_equal(g['blur7'][wr], ref['blur7'][wr]), (tag, 'blur7')


def _targets(name):
    return M.CASES[name][1] if name in M.CASES else M.BIG[name][1]


def _ovf(name):
    return M.CASES[name][2] if name in M.CASES else M.BIG[name][2]


CASE_TARGETS = [(n, t) for n in sorted(M.CASES) for t in M.CASES[n][1]]


@pytest.mark.gpu
@pytest.mark.parametrize('name,target', CASE_TARGETS)
def test_masks_stage_case_alone(cpe, orc, gpu, name, target):
    c = M.get(name)
    g = _run(cpe, gpu, [c], target)[0]
    _check(c, g, _oracle(name, c, target), (name, target), target, _ovf(name))


MIX_SHAPE = (600, 800)


@pytest.mark.gpu
@pytest.mark.parametrize('target', ['cylinder', 'plane'])
def test_masks_stage_mixed_batch_equals_alone(cpe, orc, gpu, target):
    """every case that fits, padded to one frame size (zeros right and below), in one batch and in reversed order, plus a
    no-region copy of the first: each frame identical to its run alone, and equal to the oracle"""
    H, W = MIX_SHAPE
    names = [n for n in sorted(M.CASES) if target in M.CASES[n][1] and M.get(n)['binary'].shape[0] <= H and
             M.get(n)['binary'].shape[1] <= W]
    cases = [M.pad(M.get(n), H, W) for n in names]
    cases.append(dict(cases[0], status=1))
    tags = names + ['no region']
    batch = _run(cpe, gpu, cases, target)
    rev = _run(cpe, gpu, cases[::-1], target)
    for i, c in enumerate(cases):
        alone = _run(cpe, gpu, [c], target)[0]
        _same(batch[i], alone, (tags[i], 'batch'))
        _same(rev[len(cases) - 1 - i], alone, (tags[i], 'reversed batch'))
        _check(c, alone, M.oracle(c, target), (tags[i], 'padded'), target, _ovf(tags[i]) if i < len(names) else 0)
    assert len(cases) >= (20 if target == 'cylinder' else 10)


@pytest.mark.gpu
def test_masks_stage_at_every_width(cpe, orc, gpu):
    """64 .. 4096 columns: k_open20_joints<64> up to 2880, <32> from 2881; the joints and masks at every word edge"""
    for w in M.WIDTHS:
        c = M.gen_widths(96, w)
        g = _run(cpe, gpu, [c, dict(c, status=1)])
        ref = M.oracle(c)
        _check(c, g[0], ref, ('width', w))
        _check(dict(c, status=1), g[1], M.oracle(dict(c, status=1)), ('width', w, 'no region'))
        assert ref['status'] == 0 and len(ref['joints']) > 0


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(M.BIG))
def test_masks_stage_big_frames(cpe, orc, gpu, name):
    c = M.get(name)
    for target in _targets(name):
        g = _run(cpe, gpu, [c], target)[0]
        _check(c, g, M.oracle(c, target), (name, target), target, _ovf(name))


@pytest.mark.gpu
@pytest.mark.parametrize('h,w', [(480, 640), (1200, 1920), (2160, 3840)])
def test_masks_stage_matches_detect_path(cpe, orc, gpu, h, w):
    """the entry fed the detect path's own binary, grey frame, mask_contour, rect and region status reproduces that call's
    masks-stage planes and state on rendered frames"""
    from cpe_amd import synth
    b = synth.render_batch(1, h, w, seed=7, with_gt=False)
    frames = torch.cat([b['left'], b['right']]).contiguous().to(gpu)
    det = cpe.api.detect_grid_batch(frames)
    torch.cuda.synchronize()
    ws = det['ws']
    pl = {k: ws.plane(k).clone() for k in ('binary', 'mask_contour')}
    sd = ws.state()
    want = {k: ws.plane(k).cpu().numpy() for k in PLANES}
    joints = ws.plane('joints').cpu().numpy()
    rect = torch.tensor([[s['rect0'], s['rect1'], s['rect2'], s['rect3']] for s in sd], dtype=torch.int32)
    status = torch.tensor([1 if s['status'] == 1 else 0 for s in sd], dtype=torch.int32)
    ws2 = cpe.api.debug_masks(pl['binary'], frames, pl['mask_contour'], rect, status)
    torch.cuda.synchronize()
    got = {k: ws2.plane(k).cpu().numpy() for k in PLANES}
    g_joints = ws2.plane('joints').cpu().numpy()
    s2 = ws2.state()
    n_ok = 0
    for i in range(frames.shape[0]):
        assert sd[i]['overflow'] == 0
        mstat = sd[i]['status'] if sd[i]['status'] in (1, 2) else 0      # 3, 4: the lines stage's verdicts
        assert s2[i]['status'] == mstat, i
        for k in STATE[1:]:
            if k in ('n_joints_all',) and mstat != 0:
                continue
            assert s2[i][k] == sd[i][k], (i, k, s2[i][k], sd[i][k])
        for k in ('hmask', 'vmask', 'roi_h', 'roi_v', 'exp_h', 'exp_v'):
            assert np.array_equal(got[k][i], want[k][i]), (i, k)
        assert np.array_equal(got['blur19'][i] > 240, want['blur19'][i] > 240), i
        nj = sd[i]['n_joints']
        assert np.array_equal(g_joints[i, :nj], joints[i, :nj]), i
        if mstat == 0:
            wr = PC.blur7_written(h, w, (sd[i]['rect0'], sd[i]['rect1'], sd[i]['rect2'], sd[i]['rect3']), sd[i]['r0'])
            assert np.array_equal(got['blur7'][i][wr], want['blur7'][i][wr]), i
            n_ok += 1
    assert n_ok >= 1
