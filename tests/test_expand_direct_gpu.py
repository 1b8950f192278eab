"""The fragment expansion writing straight into the expanded masks (k_roi_base seeds exp = base & mask_contour, k_seg_expand
adds its pixels on bit rows), through cpe_debug_masks against the oracle with tolerance 0 on roi_*, exp_*, n_seg*, the gang /
glen bits and the overflow word.  The inputs are tests/expand_cases.py (tests/test_expand_cases_cpu.py checks that each
reaches its edge): a mask_contour that is not the rectangle, end points at word and frame edges, hundreds of fragments with
overlapping supports, frames that must leave nothing behind in a reused workspace, and both stream modes."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import expand_cases as E  # noqa: E402
import masks_cases as M  # noqa: E402
import test_masks_stage_gpu as T  # noqa: E402  (its _run / _check / _same: one frame against the oracle, two runs against each other)

_REF = {}


def _oracle(key, c, target):
    if (key, target) not in _REF:
        _REF[(key, target)] = M.oracle(c, target)
    return _REF[(key, target)]


@pytest.mark.gpu
@pytest.mark.parametrize('target', ['cylinder', 'plane'])
@pytest.mark.parametrize('notch', [False, True])
def test_mask_contour_is_not_the_rectangle(cpe, orc, gpu, notch, target):
    """a 12-gon (and the 12-gon with two-pixel notches of zeros) as mask_contour: its edge runs through fragments, through
    pixels the closing adds (base outside mask_contour) and through expansion supports"""
    c = E.gen_polygon(notch)
    g = T._run(cpe, gpu, [c], target)[0]
    T._check(c, g, _oracle(('polygon', notch), c, target), ('polygon', notch, target), target)
    assert not g['exp_h'][c['mc'] == 0].any() and not g['exp_v'][c['mc'] == 0].any()
    assert (g['exp_h'] > g['roi_h']).any() and (g['exp_v'] > g['roi_v']).any()


# 640: rows on 16-byte boundaries (the word-level labelling reads base's one-bit plane, its bytes are not written); 648: the
# byte-level labelling, 8 pixels per load / store in k_roi_base; 650 and 801: byte by byte
@pytest.mark.gpu
@pytest.mark.parametrize('w', [640, 648, 650, 801])
@pytest.mark.parametrize('r0,target', [(21, 'cylinder'), (22, 'cylinder'), (21, 'plane')])
def test_end_points_at_word_and_frame_edges(cpe, orc, gpu, w, r0, target):
    """end points at columns 0, 1, 31, 32, 62, 63 (mod 64), within 7 px of every frame edge and in two corners; kernels 112 and
    113 (even and odd ks / 2) and the planar target's 201"""
    c = E.gen_edges(w, r0)
    g = T._run(cpe, gpu, [c], target)[0]
    ref = _oracle(('edges', w, r0), c, target)
    T._check(c, g, ref, ('edges', w, r0, target), target)
    assert g['state']['r0'] == r0
    assert (g['exp_h'] > g['roi_h']).any() and (g['exp_v'] > g['roi_v']).any()


@pytest.mark.gpu
def test_many_fragments_with_overlapping_supports(cpe, orc, gpu):
    """more than 500 valid fragments per mask, below MAXSEG: every workgroup of the expansion takes several fragments, and
    neighbouring end points 2 - 3 px apart make several workgroups store the same bytes"""
    c = E.gen_many()
    g = T._run(cpe, gpu, [c])[0]
    ref = _oracle('many', c, 'cylinder')
    T._check(c, g, ref, 'many')
    assert 500 <= g['state']['n_seg0'] < M.MAXSEG and 500 <= g['state']['n_seg1'] < M.MAXSEG


def _run_in(cpe, gpu, ws, cases, target='cylinder'):
    """T._run inside a workspace that is kept between calls -> (per-frame results, the workspace)"""
    st = lambda k: torch.from_numpy(np.stack([c[k] for c in cases])).to(gpu)
    rect = torch.tensor([c['rect'] for c in cases], dtype=torch.int32)
    status = torch.tensor([c['status'] for c in cases], dtype=torch.int32)
    ws = cpe.api.debug_masks(st('binary'), st('gray'), st('mc'), rect, status, ws=ws, target=target)
    torch.cuda.synchronize()
    planes = {k: ws.plane(k).cpu().numpy() for k in T.PLANES}
    joints = ws.plane('joints').cpu().numpy()
    state = ws.state()
    out = []
    for i in range(len(cases)):
        d = {k: planes[k][i] for k in T.PLANES}
        d['state'] = state[i]
        d['joints'] = joints[i, :min(state[i]['n_joints'], M.MAXJ)].copy()
        out.append(d)
    return out, ws


@pytest.mark.gpu
@pytest.mark.parametrize('target', ['cylinder', 'plane'])
def test_nothing_stale_in_a_reused_workspace(cpe, orc, gpu, target):
    """[busy frame, frame without a region, frame whose rect is a 40-row strip far from the busy content] in every rotation in
    one workspace, so that every slot held a busy frame before: the planes of the frame without a region are zero, and every
    frame equals its run alone (exp is written in full by k_roi_base: nothing else clears it)"""
    busy, strip = E.gen_busy(), E.gen_strip()
    cases = [busy, dict(busy, status=1), strip]
    alone = [T._run(cpe, gpu, [c], target)[0] for c in cases]
    T._check(busy, alone[0], M.oracle(busy, target), ('busy', target), target)
    T._check(strip, alone[2], M.oracle(strip, target), ('strip', target), target)
    ws = None
    for rot in range(4):
        order = [(i + rot) % 3 for i in range(3)]
        got, ws2 = _run_in(cpe, gpu, ws, [cases[i] for i in order], target)
        assert ws is None or ws2 is ws
        ws = ws2
        for slot, i in enumerate(order):
            T._same(got[slot], alone[i], (target, 'rotation', rot, 'frame', i))
            if i == 1:
                for k in ('roi_h', 'roi_v', 'exp_h', 'exp_v'):
                    assert not got[slot][k].any(), (rot, k)
            if i == 2:
                y = strip['rect'][1]
                assert not got[slot]['exp_h'][:y].any() and not got[slot]['exp_v'][:y].any()


def _with_serial(on, fn):
    old = os.environ.get('CPE_SERIAL')
    try:
        if on:
            os.environ['CPE_SERIAL'] = '1'
        else:
            os.environ.pop('CPE_SERIAL', None)
        return fn()
    finally:
        if old is None:
            os.environ.pop('CPE_SERIAL', None)
        else:
            os.environ['CPE_SERIAL'] = old


@pytest.mark.gpu
def test_stream_modes_agree(cpe, orc, gpu):
    """one mixed batch of the cases above with CPE_SERIAL=1 and without, and rendered frames through the detect path (whose
    vertical direction runs on the helper stream unless CPE_SERIAL is set): identical planes and state"""
    H, W = E.STALE_SHAPE
    busy = E.gen_busy()
    cases = [busy, E.gen_strip(), dict(busy, status=1), M.pad(E.gen_polygon(False), H, W)]
    a = _with_serial(True, lambda: T._run(cpe, gpu, cases))
    b = _with_serial(False, lambda: T._run(cpe, gpu, cases))
    for i in range(len(cases)):
        T._same(a[i], b[i], ('debug_masks', i))
    from cpe_amd import synth
    r = synth.render_batch(2, 480, 640, seed=11, with_gt=False)
    frames = torch.cat([r['left'], r['right']]).contiguous().to(gpu)

    def detect():
        det = cpe.api.detect_grid_batch(frames)
        torch.cuda.synchronize()
        ws = det['ws']
        return {k: ws.plane(k).cpu().numpy() for k in ('roi_h', 'roi_v', 'exp_h', 'exp_v')}, ws.state()

    (pa, sa), (pb, sb) = _with_serial(True, detect), _with_serial(False, detect)
    for k in pa:
        assert np.array_equal(pa[k], pb[k]), k
    n_exp = 0
    for i in range(frames.shape[0]):
        for k in ('status', 'r0', 'n_seg0', 'n_seg1', 'gang0', 'gang1', 'glen0', 'glen1', 'overflow'):
            assert sa[i][k] == sb[i][k], (i, k)
        n_exp += bool((pa['exp_h'][i] > pa['roi_h'][i]).any())
    assert n_exp >= 1
