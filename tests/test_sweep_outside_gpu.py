"""Dark components that reach the border of the working rectangle, through cpe_debug_blob_region, against the oracle at
tolerance 0.

A dark component is a hole at a threshold exactly if none of its pixels lies on the rectangle's border.  The dark forest of the
sweep (csrc/region.hip) says so with a link: "outside" is a terminal parent, -1, smaller than every pixel index, so the atomic
minimum that links the larger root under the smaller also makes a component that is united with outside an outside tree, and
every later union with it inherits that (uf_find_out / uf_find_c_out / uf_unite_out, csrc/cpe_dev.h).  k_sw_outside links the
border components of the first labelling, a joining pixel on the border has outside among its partners (sw_unite_body), the
walk over the joining pixels ends at a root or at -1 (sw_new_body), and an absorbed hole hands its total over only to a root
(sw_old_body).  No walk may index with -1.

The images (tests/sweep_outside_cases.py): one border pixel opens a hole, on each side and in each corner, at the first, a
middle and the last step; border components of the first labelling beside holes that stay; a hand-over of a total followed by
the way out; a pre-linked run along the top row; diagonal contact only; a hole absorbed into outside in the step in which it
absorbs another; frames without a bright or without a dark pixel.  Compared as in tests/test_sweep_links_gpu.py, whose
helpers this module uses: holes, outer components and blobs per threshold, the accepted blobs, key points as bits,
mask_contour, rect, status, overflow 0.  The CPU test shows from the oracle alone that every image reaches its situation.

At the end, the row-wise first labelling (k_ccl_init, csrc/ccl.hip) on rectangles narrower than one 64-pixel chunk and
4 x 64 + 1 wide, through cpe_debug_dark_labels: both paths against each other and against numpy's runs."""
import numpy as np
import pytest

import sweep_outside_cases as G
import test_sweep_links_gpu as T
import test_dark_labels_gpu as D

NTHR = G.NTHR
BATCH = 16

_CASES = {}


def _cases(shape):
    if shape not in _CASES:
        _CASES[shape] = G.cases(*shape)
        for img, _ in _CASES[shape].values():
            assert img.shape == shape and img.dtype == np.uint8
            img.setflags(write=False)
    return _CASES[shape]


_ALONE = {}


def _alone(cpe, gpu, shape, name):
    """the image in a batch of one, in a workspace of its own: computed once, shared by the tests"""
    if (shape, name) not in _ALONE:
        _ALONE[shape, name] = T._run(cpe, gpu, _cases(shape)[name][0][None])[0]
    return _ALONE[shape, name]


FAMILIES = ('open_all', 'open_top', 'open_bottom', 'open_left', 'open_right', 'open_tl', 'open_tr', 'open_bl', 'open_br',
            'first_labelling', 'handover', 'run_on_border', 'diagonal', 'absorbed_into_outside', 'degenerate')


def test_sweep_outside_families_cover_the_cases():
    for shape in G.SHAPES:
        for name in _cases(shape):
            assert sum(name.startswith(f) for f in FAMILIES) == 1, name


@pytest.mark.gpu
@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('shape', G.SHAPES)
def test_sweep_outside_case_alone(cpe, orc, gpu, shape, family):
    names = [k for k in _cases(shape) if k.startswith(family)]
    assert names
    for name in names:
        img, facts = _cases(shape)[name]
        g = _alone(cpe, gpu, shape, name)
        T._check(img, g, (shape, name))
        if facts['holes'] is not None:          # and the count the image was built for, slot by slot
            assert list(g['counters'][:NTHR]) == facts['holes'], (shape, name, list(g['counters'][:NTHR]))


@pytest.mark.gpu
@pytest.mark.parametrize('shape', G.SHAPES)
def test_sweep_outside_mixed_batch_equals_alone(cpe, orc, gpu, shape):
    """every image inside mixed batches of 16, and inside the reversed batches: the bits of the image alone"""
    cs = _cases(shape)
    for order in (list(cs), list(cs)[::-1]):
        for a in range(0, len(order), BATCH):
            names = order[a:a + BATCH]
            batch = T._run(cpe, gpu, np.stack([cs[k][0] for k in names]))
            for i, name in enumerate(names):
                T._same(batch[i], _alone(cpe, gpu, shape, name), (shape, name, 'batch from', order[a]))
                T._check(cs[name][0], batch[i], (shape, name, 'batch from', order[a]))


@pytest.mark.gpu
@pytest.mark.parametrize('shape', G.SHAPES)
def test_sweep_outside_second_call_in_one_workspace(cpe, orc, gpu, shape):
    """a second call, with other images, in the same workspace equals a fresh one: no -1 of an earlier call leaks.  Batches of
    16 follow each other, so every frame slot holds another image's forest from the call before"""
    from cpe_amd import api
    cs = _cases(shape)
    names = list(cs)
    ws = api.DetectWorkspace(BATCH, shape[0], shape[1], gpu)
    T._run(cpe, gpu, np.stack([cs[k][0] for k in names[-BATCH:]]), ws=ws)
    for a in range(0, len(names), BATCH):
        part = names[a:a + BATCH]
        got = T._run(cpe, gpu, np.stack([cs[k][0] for k in part]), ws=ws)
        for i, name in enumerate(part):
            T._same(got[i], _alone(cpe, gpu, shape, name), (shape, name, 'second call'))
            T._check(cs[name][0], got[i], (shape, name, 'second call'))


# ---------------------------------------------------------------- CPU: the images reach their situations
@pytest.mark.parametrize('shape', G.SHAPES)
def test_sweep_outside_images_reach_their_cases(orc, shape):
    h, w = shape
    assert G.SHAPES[0][1] % 16 == 0 and G.SHAPES[1][1] % 16 != 0, 'both plane builders, both first labellings'
    for name, (img, facts) in _cases(shape).items():
        ref = T._oracle(img)
        lv = G.level(img)
        if name.startswith('degenerate'):
            assert ref['holes'] == [0] * NTHR, (name, ref['holes'])
            assert (img > 50).any() == (facts['kind'] in ('none_dark', 'white')) and (img <= 50).any() == (facts['kind'] in ('none_bright', 'black'))
            continue
        ys, xs = np.nonzero(img > 50)
        rect = (int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max()))
        m = facts['margin']
        assert rect == (m, m, w - m - 1, h - m - 1), (name, rect)
        assert name.endswith('_frame') == (m == 0), name
        # the hole count of the named slot falls by the named number at the named step
        assert ref['holes'] == facts['holes'], (name, ref['holes'], facts['holes'])
        k = facts['slot']
        if 0 < k < NTHR:
            assert ref['holes'][k - 1] - ref['holes'][k] == facts['drop'] > 0, (name, ref['holes'])
        else:
            assert len(set(ref['holes'])) == 1, (name, ref['holes'])
        on_border = np.zeros((h, w), bool)
        on_border[[rect[1], rect[3]], rect[0]:rect[2] + 1] = True
        on_border[rect[1]:rect[3] + 1, [rect[0], rect[2]]] = True
        if name.startswith('open'):
            # the openers are the only border pixels below bucket 17, and the holes count 16 or 9 pixels each until they go
            # (bucket 17: the openers are pixels of the field, nothing opens)
            assert {(int(y), int(x)) for y, x in np.argwhere(on_border & (lv < 17))} == (set(facts['openers']) if k < 17 else set()), name
            assert all(lv[y, x] == facts['slot'] for y, x in facts['openers'])
            places = G.SIDES + G.CORNERS if name.startswith('open_all') else (name.split('_')[1],)
            assert facts['drop'] == len(places)
            assert sorted(_hole_pixel_counts(img)) == sorted(9 if p in G.CORNERS else 16 for p in places), name
        elif name.startswith('first_labelling'):
            assert (on_border & (lv == 0)).sum() > 40 and not (on_border & (lv > 0) & (lv < 17)).any(), name
            for side in (on_border[rect[1]], on_border[rect[3]]):
                assert side.any()
        elif name.startswith('handover'):
            j = facts['merge_slot']
            assert ref['holes'][j - 1] == 2 and ref['holes'][j] == 1 and ref['holes'][j + 1] == 1 and ref['holes'][j + 2] == 0
            assert int((lv == j).sum()) == 3 and sorted(_hole_pixel_counts(img)) == sorted(facts['parts'][:2]), name
            if 'big' in name:
                assert max(facts['parts']) < 5000 <= sum(facts['parts'])
            assert int((on_border & (lv == j + 2)).sum()) == 1 and not (on_border & (lv < j + 2)).any(), name
            dark0 = np.flatnonzero((lv == 0)[m:h - m, m:w - m].reshape(-1))
            assert (lv == 0)[m:h - m, m:w - m].reshape(-1)[dark0[0]:dark0[0] + 5].all(), 'the 5 x 5 hole is raster-first'
        elif name.startswith('run_on_border'):
            y, x, n = facts['run']
            assert (y, x) == (rect[1], rect[0]) and (lv[y, x:x + n] == facts['slot']).all() and lv[y, x + n] == 17
            assert any(i % 64 == 0 for i in range(y * w + x + 1, y * w + x + n)), 'a multiple of 64 in frame indices inside the run'
            assert n > 64, 'and one in columns counted from the rectangle'
        elif name.startswith('diagonal'):
            assert (on_border & (lv == 0)).any() and (on_border & (lv == 8)).any()
        elif name.startswith('absorbed_into_outside'):
            j = facts['slot']
            assert int((lv == j).sum()) == 4 and not (on_border & (lv == j)).any() and (on_border & (lv == 0)).any(), name
        else:
            raise AssertionError(name)


def _hole_pixel_counts(img):
    """pixel counts of the dark 4-connected components of bucket 0 away from the frame's dark surround (plain flood fill)"""
    dark = G.level(img) == 0
    h, w = dark.shape
    seen = np.zeros_like(dark)
    out = []
    for y0, x0 in np.argwhere(dark):
        if seen[y0, x0]:
            continue
        stack, n, edge = [(int(y0), int(x0))], 0, False
        seen[y0, x0] = True
        while stack:
            y, x = stack.pop()
            n += 1
            edge = edge or y in (0, h - 1) or x in (0, w - 1)
            for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
                if 0 <= yy < h and 0 <= xx < w and dark[yy, xx] and not seen[yy, xx]:
                    seen[yy, xx] = True
                    stack.append((yy, xx))
        if not edge:
            out.append(n)
    return out


# ---------------------------------------------------------------- the row-wise first labelling on narrow and odd rectangles
def _numpy_runs(frame, rect):
    """label plane of the row-wise first labelling as the sweep needs it, before the merge, reduced to what both paths must
    agree with after it: (dark mask in the rectangle, first pixel of every pixel's run of one bucket outside the set, in
    64-pixel chunks from the rectangle's left edge)"""
    h, w = frame.shape
    x0, y0, x1, y1 = rect
    lv = G.level(frame)
    pre = np.full((h, w), -1, np.int64)
    for y in range(y0, y1 + 1):
        for x in range(x0, x1 + 1):
            if lv[y, x] == 0:
                continue
            cont = x > x0 and ((x - x0) & 63) != 0 and lv[y, x - 1] == lv[y, x]
            pre[y, x] = pre[y, x - 1] if cont else y * w + x
    return lv == 0, pre


@pytest.mark.gpu
@pytest.mark.parametrize('h,w,rw', [(64, 288, 37), (64, 288, 4 * 64 + 1), (72, 281, 4 * 64 + 1), (72, 281, 1)])
def test_dark_labels_narrow_and_odd_rectangles(cpe, gpu, h, w, rw):
    """rectangles narrower than one chunk and one pixel wider than four chunks, rows 16-byte aligned (288) and not (281): path 0
    against path 1 bit for bit, and both against numpy: the pre-linked runs outside the set, the set's components as
    scipy-free flood fills would give them (every dark pixel carries a root of its own 4-connected component)"""
    rng = np.random.default_rng(h * 1000 + w + rw)
    n = 3
    frames = D._frames(rng, n, h, w)
    frames[1, :, ::3] = np.where(frames[1, :, ::3] > D.THR, 95, frames[1, :, ::3])      # long runs of one bucket across chunks
    frames[1, 5:9] = 95
    rects = [[3 + 7 * i, 2 + i, 3 + 7 * i + rw - 1, h - 3 - i] for i in range(n)]
    assert all(0 <= r[0] <= r[2] < w and 0 <= r[1] <= r[3] < h for r in rects)
    want = D._run(cpe, gpu, frames, rects, 0)
    got = D._run(cpe, gpu, frames, rects, 1)
    for i in range(n):
        tag = (h, w, rw, i)
        x0, y0, x1, y1 = rects[i]
        for k in (0, 1):
            assert np.array_equal(got[k][i], want[k][i]), (tag, k, int((got[k][i] != want[k][i]).sum()))
        assert got[3][i] == want[3][i], tag
        kq = int(want[3][i])
        roots = np.sort(got[2][i, :kq])
        assert np.array_equal(roots, np.sort(want[2][i, :kq])), tag
        dark, pre = _numpy_runs(frames[i], rects[i])
        win = np.zeros((h, w), bool)
        win[y0:y1 + 1, x0:x1 + 1] = True
        lab = got[0][i].astype(np.int64)
        assert np.array_equal(lab[win & ~dark], pre[win & ~dark]), (tag, 'pre-linked runs outside the set')
        ind = win & dark
        assert np.array_equal(np.unique(lab[ind]), roots), tag
        assert int(got[1][i].reshape(-1)[roots].sum()) == int(ind.sum()), tag
        # 4-neighbours inside the set share a label; a label's pixels are dark pixels of the rectangle
        assert (lab[:, 1:][ind[:, 1:] & ind[:, :-1]] == lab[:, :-1][ind[:, 1:] & ind[:, :-1]]).all(), tag
        assert (lab[1:][ind[1:] & ind[:-1]] == lab[:-1][ind[1:] & ind[:-1]]).all(), tag
        assert ind.reshape(-1)[roots].all(), tag
