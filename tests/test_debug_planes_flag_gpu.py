"""detect_grid_batch(debug_planes=False) (CPE_DETECT_SKIP_DEBUG_PLANES, include/cpe.h) against the default call on the same
frames, with tolerance 0: the point tables, the state records and every public plane that stays defined are identical.

Shapes of test_detect_small_frames_stage_by_stage: 480 x 640 (width a multiple of 64) and 600 x 800 (a multiple of 16, the
last 64-pixel word of a row is partial) take the word-level path, where hmask / vmask / roi_h / roi_v are not written and
plane() refuses them; 602 x 801 and 483 x 650 take the byte path, which needs the bytes and ignores the flag.

What "defined" means for the planes that a call only writes in part: blur7 inside the region rectangle of a good frame (the
blur skips tiles away from it), joints up to n_joints, labels (union-find links of exp_h, whose interior pointers depend on
the order the unions happened in) as the root every pixel of exp_h resolves to."""
import numpy as np
import pytest
import torch

FULL = ('binary', 'mask_contour', 'exp_h', 'exp_v', 'clahe', 'blur19', 'sweep')
DEBUG = ('hmask', 'vmask', 'roi_h', 'roi_v')
TABLES = ('xy', 'id', 'n', 'center', 'status')


def _frames(h, w, seed):
    from cpe_amd import synth
    b = synth.render_batch(2, h, w, seed=seed, with_gt=False)
    return torch.cat([b['left'], b['right']])[:3].contiguous()


def _roots(lab, mask):
    """root of every pixel of mask in a plane of union-find links (-1 elsewhere)"""
    flat = lab.reshape(-1).astype(np.int64)
    idx = np.flatnonzero(mask.reshape(-1))
    cur = flat[idx]
    for _ in range(64):
        nxt = flat[cur]
        if np.array_equal(nxt, cur):
            break
        cur = nxt
    else:
        raise AssertionError('label links do not resolve')
    out = np.full(flat.shape, -1, np.int64)
    out[idx] = cur
    return out


def _snapshot(cpe, gpu, frames, debug_planes):
    det = cpe.api.detect_grid_batch(frames.to(gpu), debug_planes=debug_planes)
    torch.cuda.synchronize()
    ws = det['ws']
    snap = {k: det[k].cpu().numpy() for k in TABLES}
    snap['state'] = ws.state()
    for k in FULL + ('blur7', 'joints', 'labels'):
        snap[k] = ws.plane(k).cpu().numpy()
    return snap, ws


def _compare(a, b, tag):
    for k in TABLES + FULL:
        assert np.array_equal(a[k], b[k]), (tag, k)
    assert a['state'] == b['state'], (tag, [(k, s[k], t[k]) for s, t in zip(a['state'], b['state']) for k in s if s[k] != t[k]])
    for f, st in enumerate(a['state']):
        assert np.array_equal(a['joints'][f, :st['n_joints']], b['joints'][f, :st['n_joints']]), (tag, f, 'joints')
        if st['status'] != 0:
            continue
        x, y, rw, rh = st['rect0'], st['rect1'], st['rect2'], st['rect3']
        assert np.array_equal(a['blur7'][f, y:y + rh, x:x + rw], b['blur7'][f, y:y + rh, x:x + rw]), (tag, f, 'blur7')
        m = a['exp_h'][f] != 0
        assert m.any() and np.array_equal(_roots(a['labels'][f], m), _roots(b['labels'][f], m)), (tag, f, 'labels')


@pytest.mark.gpu
@pytest.mark.parametrize('h,w,seed,serial', [(480, 640, 0, False), (600, 800, 4, False), (602, 801, 6, False), (483, 650, 8, False),
                                             (600, 800, 4, True)])
def test_skipping_the_debug_planes_changes_nothing_else(cpe, gpu, monkeypatch, h, w, seed, serial):
    if serial:
        monkeypatch.setenv('CPE_SERIAL', '1')       # looked at on every call: every kernel on the caller's stream
    frames = _frames(h, w, seed)
    full, ws_full = _snapshot(cpe, gpu, frames, True)
    dbg = {k: ws_full.plane(k).cpu().numpy() for k in DEBUG}
    lean, ws_lean = _snapshot(cpe, gpu, frames, False)
    tag = (h, w, 'serial' if serial else 'overlapped')
    _compare(full, lean, tag)
    assert int((full['status'] == 0).sum()) >= 1, (tag, full['status'])
    assert all(dbg[k].any() for k in DEBUG), tag
    if w % 16 == 0:
        for k in DEBUG:
            with pytest.raises(RuntimeError, match='debug_planes=False'):
                ws_lean.plane(k)
        assert ws_lean.plane('exp_h') is not None
        # the workspace serves a default call again: the planes are back
        again = cpe.api.detect_grid_batch(frames.to(gpu), ws_lean)
        torch.cuda.synchronize()
        for k in DEBUG:
            assert np.array_equal(again['ws'].plane(k).cpu().numpy(), dbg[k]), (tag, k, 'after a default call on the same workspace')
    else:
        for k in DEBUG:
            assert np.array_equal(ws_lean.plane(k).cpu().numpy(), dbg[k]), (tag, k, 'byte path: the flag is ignored')
