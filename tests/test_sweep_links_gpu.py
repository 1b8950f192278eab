"""The links of the blob sweep's two forests (csrc/region.hip) through cpe_debug_blob_region, against the oracle at tolerance 0.

The bright forest keeps a merge history per node, "absorbed by X at step j", written where the link is made: by the winning
compare-and-swap of a union (uf_unite_hist, csrc/cpe_dev.h), and by k_bk_pass for the members of a run of one bucket that it
links to the run's first pixel.  k_enclosed_all follows that history to credit every hole to the bright component that
encloses it at each threshold.  The pass over the pixels that join (sw_new_body) stores a parent only where that shortens a
path: not for a pixel already one hop from its root, not for a run member whose first pixel shares its 64-byte line.

The images (tests/sweep_links_cases.py) put holes behind every kind of link, merges at chosen steps beside a blob that a
wrongly timed history would prune, and the deep paths the store rule has to keep short.  Compared with
oracle/stages.simple_blob_detector, largest_blob_from_sweep and find_contours: blobs per threshold, the accepted blobs, the
hole and outer counters of CPE_PLANE_SWEEP, the key points as bits, mask_contour, rect and status.  The CPU test at the end
shows from the oracle alone that every image reaches the situation it is built for."""
import numpy as np
import pytest
import torch

import sweep_links_cases as G

NTHR = G.NTHR
SW_HOLES, SW_OUTER, SW_BLOBS = 8, 25, 42      # CPE_PLANE_SWEEP: per-threshold counters of a frame's sweep record

_CASES = {}


def _cases(shape):
    if shape not in _CASES:
        _CASES[shape] = G.cases(*shape)
        for img, _ in _CASES[shape].values():
            assert img.shape == shape and img.dtype == np.uint8
            img.setflags(write=False)
    return _CASES[shape]


def _run(cpe, gpu, imgs, ws=None, kp_cap=256, blob_cap=256):
    """cpe_debug_blob_region on u8 [n, h, w] -> one dict of numpy results per frame"""
    from cpe_amd import api
    imgs = np.array(imgs, dtype=np.uint8, order='C')      # a copy: the cases themselves are read-only
    n, h, w = imgs.shape
    ws = api.DetectWorkspace(n, h, w, gpu) if ws is None else ws.use(n)
    d = torch.from_numpy(imgs).to(gpu)
    kp = torch.zeros((n, kp_cap, 3), dtype=torch.float32, device=gpu)
    nkp = torch.zeros(n, dtype=torch.int32, device=gpu)
    bl = torch.zeros((n, NTHR, blob_cap, 3), dtype=torch.float64, device=gpu)
    nbl = torch.zeros((n, NTHR), dtype=torch.int32, device=gpu)
    L = cpe.lib.load()
    cpe.lib.check(L.cpe_debug_blob_region(d.data_ptr(), n, h, w, ws.view.data_ptr(), ws.bytes, kp.data_ptr(), kp_cap, nkp.data_ptr(),
                                          bl.data_ptr(), blob_cap, nbl.data_ptr(), torch.cuda.current_stream().cuda_stream),
                  'cpe_debug_blob_region')
    torch.cuda.synchronize()
    nkp_h, nbl_h = nkp.cpu().numpy(), nbl.cpu().numpy()
    assert (nkp_h <= kp_cap).all() and (nbl_h <= blob_cap).all(), 'raise the test capacities'
    kp_h, bl_h = kp.cpu().numpy(), bl.cpu().numpy()
    state, mc = ws.state(), ws.plane('mask_contour').cpu().numpy()
    sweep, clahe = ws.plane('sweep').cpu().numpy(), ws.plane('clahe').cpu().numpy()
    return [dict(kp=kp_h[i, :nkp_h[i]].copy(), blobs=[_sorted(bl_h[i, k, :nbl_h[i, k]]) for k in range(NTHR)], nblobs=nbl_h[i].copy(),
                 state=dict(state[i]), mc=mc[i].copy(), counters=sweep[i][SW_HOLES:SW_HOLES + 3 * NTHR].copy(), clahe=clahe[i].copy())
            for i in range(n)]


def _sorted(rec):
    rec = np.asarray(rec, np.float64).reshape(-1, 3)
    return rec[np.lexsort((rec[:, 2], rec[:, 1], rec[:, 0]))]


_ORACLE = {}


def _oracle(img):
    """what the oracle says of one image, computed once"""
    from oracle import stages as S
    key = (img.shape, img.tobytes())
    if key not in _ORACLE:
        kp, stats, blobs = S.simple_blob_detector(img, blobs=True)
        status, mask, rect, nk = S.largest_blob_from_sweep(img)
        contours = [S.find_contours(img > 50 + 10 * k, 'list', 'none') for k in range(NTHR)]
        _ORACLE[key] = dict(kp=kp, stats=[int(v) for v in stats], blobs=[_sorted(b) for b in blobs], status=status, mask=mask, rect=rect,
                            nk=nk, contours=contours, holes=[sum(1 for _, hole in c if hole) for c in contours],
                            outer=[sum(1 for _, hole in c if not hole) for c in contours])
    return _ORACLE[key]


def _check(img, g, tag):
    """one frame's GPU result against the oracle, tolerance 0"""
    ref = _oracle(img)
    st = g['state']
    c = g['counters']
    assert np.array_equal(g['clahe'], img), (tag, 'identity table: the sweep image is the input')
    assert list(c[:NTHR]) == ref['holes'], (tag, 'holes per threshold', list(c[:NTHR]), ref['holes'])
    assert list(c[NTHR:2 * NTHR]) == ref['outer'], (tag, 'outer components per threshold', list(c[NTHR:2 * NTHR]), ref['outer'])
    assert list(c[2 * NTHR:]) == ref['stats'], (tag, 'blobs per threshold', list(c[2 * NTHR:]), ref['stats'])
    assert list(g['nblobs']) == ref['stats'], tag
    for k in range(NTHR):
        a, b = g['blobs'][k], ref['blobs'][k]
        assert a.shape == b.shape and np.array_equal(a, b), (tag, 'accepted blobs of threshold', 50 + 10 * k, a, b)
    assert st['overflow'] == 0, (tag, st['overflow'])
    assert len(g['kp']) == st['n_kp'] == len(ref['kp']) == ref['nk'], (tag, len(g['kp']), st['n_kp'], len(ref['kp']), ref['nk'])
    assert np.array_equal(g['kp'].view(np.uint32), ref['kp'].view(np.uint32)), (tag, 'key points, as bits')
    assert st['status'] == ref['status'], (tag, st['status'], ref['status'])
    assert np.array_equal(g['mc'], ref['mask']), (tag, 'mask_contour', int((g['mc'] != ref['mask']).sum()))
    if ref['status'] == 0:
        assert (st['rect0'], st['rect1'], st['rect2'], st['rect3']) == ref['rect'], (tag, 'rect')


def _same(a, b, tag):
    """two GPU results of one image, bit for bit"""
    assert np.array_equal(a['kp'].view(np.uint32), b['kp'].view(np.uint32)), (tag, 'key points')
    assert np.array_equal(a['nblobs'], b['nblobs']) and np.array_equal(a['counters'], b['counters']), (tag, 'counters')
    for k in range(NTHR):
        assert np.array_equal(a['blobs'][k].view(np.uint64), b['blobs'][k].view(np.uint64)), (tag, 'blobs of threshold', 50 + 10 * k)
    assert np.array_equal(a['mc'], b['mc']), (tag, 'mask_contour')
    for key in ('status', 'rect0', 'rect1', 'rect2', 'rect3', 'n_kp', 'n_groups', 'overflow'):
        assert a['state'][key] == b['state'][key], (tag, key)


_ALONE = {}


def _alone(cpe, gpu, shape, name):
    """the image in a batch of one, in a workspace of its own: computed once, shared by the tests"""
    if (shape, name) not in _ALONE:
        _ALONE[shape, name] = _run(cpe, gpu, _cases(shape)[name][0][None])[0]
    return _ALONE[shape, name]


FAMILIES = ('member', 'overcount', 'two_absorptions', 'stacks', 'long_runs')


@pytest.mark.gpu
@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('shape', G.SHAPES)
def test_sweep_links_case_alone(cpe, orc, gpu, shape, family):
    names = [k for k in _cases(shape) if k.startswith(family)]
    assert names
    for name in names:
        _check(_cases(shape)[name][0], _alone(cpe, gpu, shape, name), (shape, name))


@pytest.mark.gpu
@pytest.mark.parametrize('shape', G.SHAPES)
def test_sweep_links_overcount_keeps_the_ring(cpe, orc, gpu, shape):
    """above the merge the ring is accepted from its outer border and from its hole; from the merge on only from its hole"""
    for name, (img, facts) in _cases(shape).items():
        if not name.startswith('overcount'):
            continue
        g = _alone(cpe, gpu, shape, name)
        cy, cx = facts['ring_centre']
        for k in range(NTHR):
            near = sum(1 for x, y, _ in g['blobs'][k] if abs(x - cx) < 1.5 and abs(y - cy) < 1.5)
            assert near == (2 if k > facts['merge_slot'] else 1), (shape, name, 'threshold', 50 + 10 * k, near)


@pytest.mark.gpu
@pytest.mark.parametrize('shape', G.SHAPES)
def test_sweep_links_mixed_batch_equals_alone(cpe, orc, gpu, shape):
    """every image inside a mixed batch, and inside the reversed batch: the bits of the image alone"""
    cs = _cases(shape)
    names = list(cs)
    batch = _run(cpe, gpu, np.stack([cs[k][0] for k in names]))
    rev = _run(cpe, gpu, np.stack([cs[k][0] for k in names[::-1]]))
    for i, name in enumerate(names):
        alone = _alone(cpe, gpu, shape, name)
        _same(batch[i], alone, (shape, name, 'batch'))
        _same(rev[len(names) - 1 - i], alone, (shape, name, 'reversed batch'))
        _check(cs[name][0], batch[i], (shape, name, 'batch'))


@pytest.mark.gpu
@pytest.mark.parametrize('shape', G.SHAPES)
def test_sweep_links_second_run_in_one_workspace(cpe, orc, gpu, shape):
    """a workspace that held another image's forests, histories and lists gives the bits of a fresh one"""
    from cpe_amd import api
    cs = _cases(shape)
    names = list(cs)
    ws = api.DetectWorkspace(1, shape[0], shape[1], gpu)
    _run(cpe, gpu, cs[names[-1]][0][None], ws=ws)
    for i, name in enumerate(names):            # each image follows the one before it in the list (the first: the last)
        got = _run(cpe, gpu, cs[name][0][None], ws=ws)[0]
        _same(got, _alone(cpe, gpu, shape, name), (shape, name, 'after', names[i - 1]))
        _check(cs[name][0], got, (shape, name, 'after', names[i - 1]))


# ---------------------------------------------------------------- CPU: the images reach their situations
def _hole_starts(img, k):
    """the pixel west of every hole's first pixel at threshold slot k (cv2.findContours starts a hole border there)"""
    return {(int(p[0][0]), int(p[0][1])) for p, hole in _oracle(img)['contours'][k] if hole}


def _runs_of_one_bucket(img, y, x):
    """(first x, length) of the run of one bucket that holds pixel (x, y)"""
    lv = G.level(img)[y]
    a = b = x
    while a > 0 and lv[a - 1] == lv[x]:
        a -= 1
    while b + 1 < len(lv) and lv[b + 1] == lv[x]:
        b += 1
    return a, b - a + 1


@pytest.mark.parametrize('shape', G.SHAPES)
def test_sweep_links_images_reach_their_cases(orc, shape):
    h, w = shape
    cs = _cases(shape)
    assert G.SHAPES[0][1] % 16 == 0 and G.SHAPES[1][1] % 16 != 0, 'both plane builders: in the CLAHE pass, in a pass of their own'
    for name, (img, facts) in cs.items():
        ys, xs = np.nonzero(img > 50)
        rect = (int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max()))
        touches = rect[0] == 0 or rect[1] == 0 or rect[2] == w - 1 or rect[3] == h - 1
        assert touches == (name == 'member_frame_edge'), (name, rect)
        lv = G.level(img)
        if name.startswith('member'):
            for run in facts['runs']:
                x, y = run['west']
                # a hole begins east of the run's last pixel at every threshold at which the run and the field are bright
                for k in range(min(run['bucket'], 10)):
                    assert (x, y) in _hole_starts(img, k), (name, run, k)
                assert lv[y, x] == run['bucket'] == lv[y, x - 1] and (y * w + x) % 64 != 0 and x - 1 >= rect[0], (name, run, 'a member')
                a, n = _runs_of_one_bucket(img, y, x)
                assert (a, n) == (run['x0'], G.RUN_LEN), (name, run)
                cuts = [i for i in range(y * w + a, y * w + a + n) if i % 64 == 0]
                if facts['kind'] == 'inside':
                    assert not cuts and a > rect[0]
                elif facts['kind'] == 'cross64':
                    assert len(cuts) == 1 and y * w + a < cuts[0] < y * w + x, (name, cuts)     # the member's first pixel is the chunk's
                else:
                    assert a == rect[0], (name, 'the run starts at the left edge of the rectangle')
        elif name.startswith('overcount'):
            ref = _oracle(img)
            cy, cx = facts['ring_centre']
            ms = facts['merge_slot']
            assert max(facts['panes']) < 5000 <= sum(facts['panes'])
            near = [sum(1 for x, y, _ in ref['blobs'][k] if abs(x - cx) < 1.5 and abs(y - cy) < 1.5) for k in range(NTHR)]
            assert near == [1] * (ms + 1) + [2] * (NTHR - 1 - ms), (name, near)     # accepted on both sides; its outer border above
            assert ref['outer'] == [1] * (ms + 1) + [2] * (NTHR - 1 - ms), (name, ref['outer'])
            assert ref['holes'] == [5] * NTHR, (name, ref['holes'])
            # the ring's component is the raster-first one: the frame's root is absorbed by the ring's, with the panes' totals
            first = np.flatnonzero(lv.reshape(-1) == 17)[0]
            assert (first // w, first % w) == (G.MARGIN, G.MARGIN) and lv[G.MARGIN + 2, G.MARGIN + 2] == 0
        elif name == 'two_absorptions':
            ref = _oracle(img)
            k = facts['step_slot']
            assert ref['outer'][k + 1] == 3 and ref['outer'][k] == 1 and ref['outer'][k - 1] == 1, (name, ref['outer'])
            assert ref['holes'] == [3] * NTHR
            joiners = np.argwhere(lv == k + 1)
            assert len(joiners) == 16 and len(set(joiners[:, 1])) == 1, 'two connectors of one bucket'
            for j in (k + 1, k, k - 1):
                assert _hole_starts(img, j) == set(facts['wests']), (name, j)
            assert len({lv[y, x] for x, y in facts['wests']}) == 1 and lv[facts['wests'][0][1], facts['wests'][0][0]] == 17
        elif name.startswith('stacks'):
            k = facts['slot']
            grow = 2 if facts['dark'] else 0        # a hole's border runs through the bright pixels around it
            boxes = sorted((int(p[:, 1].max() - p[:, 1].min()) + 1 - grow, int(p[:, 0].max() - p[:, 0].min()) + 1 - grow)
                           for p, hole in _oracle(img)['contours'][k] if hole == facts['dark'])
            wide = 21 if facts['dark'] else 20      # a staircase: one column per row (and one more, two pixels per row)
            assert boxes == sorted([(n, 1) for n in G.STACK_HEIGHTS] + [(G.STAIR_HEIGHT, wide)] * 2), (name, boxes)
            assert min(facts['heights']) >= 8 and max(facts['heights']) == 40
            core = k if facts['dark'] else k + 1    # bucket of the stacks; the side pixels join one step later
            for y, x in np.argwhere(lv == core):
                assert lv[y, x - 1] in (core, core + (1 if facts['dark'] else -1)) and lv[y, x + 1] in (core, core + (1 if facts['dark'] else -1))
        elif name.startswith('long_runs'):
            k = facts['slot']
            ref = _oracle(img)
            for y, x in facts['rows']:
                a, n = _runs_of_one_bucket(img, y, x)
                assert (a, n) == (x, G.LONG_RUN) and n > 16 and lv[y, x] == (k if facts['dark'] else k + 1), (name, y, a, n)
            spans = sorted(int(p[:, 0].max() - p[:, 0].min()) + 1 for p, hole in ref['contours'][k] if hole == facts['dark'])
            before = ref['holes' if facts['dark'] else 'outer'][k - 1 if facts['dark'] else k + 1]
            assert before == 4, (name, before)
            if facts['dark']:       # 4-connected: the run that touches corners only stays a hole of its own
                assert spans == [22, 22, G.LONG_RUN + 2, facts['span'] + 2], (name, spans)
            else:                   # 8-connected: both runs bridge their pair
                assert spans == [facts['span']] * 2, (name, spans)
        else:
            raise AssertionError(name)
