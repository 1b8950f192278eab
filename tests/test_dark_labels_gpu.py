"""The first labelling of the blob sweep's dark forest (cpe_debug_dark_labels, include/cpe.h): the passes the region stage
runs (path 1, ccl_dark_first: the set read as the complement of the one-bit plane of img > thr, word-level finish) against the
general pass ccl_label (path 0, byte-level passes), bit for bit: labels inside and outside the set (the sweep's pre-linked runs), per-root pixel
counts, the root list (as a set) and its length.  Path 1 reads the first of a stack of 17 planes per frame, as the region
stage keeps them, and every case has several frames.

Sizes: 1920x1200 (the product's frames), 656 wide (a multiple of 16 but not of 64: a partial last word column), 801 wide
(rows not 16-byte aligned: both paths are the byte-level passes).  Rectangles start and end off the 64-pixel word grid
and off the 8-row strips."""
import numpy as np
import pytest
import torch

THR = 50
MAXROOTS = 262144      # include/cpe.h CPE_MAXROOTS_DEBUG


def _frames(rng, n, h, w):
    """grey levels around the threshold in large smooth patches (a few big dark components, long runs across words), with
    specks and noise (many one-pixel components, runs of one bucket outside the set) and dark rows / columns"""
    out = np.empty((n, h, w), np.uint8)
    for i in range(n):
        cy, cx = max(h // 32, 2), max(w // 32, 2)
        coarse = rng.integers(0, 120, size=(cy, cx)).astype(np.float32)
        big = np.kron(coarse, np.ones((h // cy + 1, w // cx + 1), np.float32))[:h, :w]
        img = big + rng.normal(0, 6 + 4 * i, size=(h, w))
        img[rng.random((h, w)) < 0.02] = 255
        img[rng.random((h, w)) < 0.02] = 0
        img[:, rng.integers(0, w, 3)] = 10
        img[rng.integers(0, h, 3), :] = 30
        out[i] = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    return out


def _run(cpe, gpu, frames, rects, path, ws=None):
    from cpe_amd import api
    n, h, w = frames.shape
    g = torch.from_numpy(frames).to(gpu)
    rect = torch.tensor(rects, dtype=torch.int32, device=gpu)
    ws = api.DetectWorkspace(n, h, w, gpu) if ws is None else ws.use(n)
    lab = torch.empty((n, h, w), dtype=torch.int32, device=gpu)
    cnt = torch.empty((n, h, w), dtype=torch.int32, device=gpu)
    roots = torch.empty((n, MAXROOTS), dtype=torch.int32, device=gpu)
    n_roots = torch.empty(n, dtype=torch.int32, device=gpu)
    L = cpe.lib.load()
    cpe.lib.check(L.cpe_debug_dark_labels(g.data_ptr(), n, h, w, THR, rect.data_ptr(), path, ws.view.data_ptr(), ws.bytes,
                                          lab.data_ptr(), cnt.data_ptr(), roots.data_ptr(), n_roots.data_ptr(),
                                          torch.cuda.current_stream().cuda_stream), 'cpe_debug_dark_labels')
    torch.cuda.synchronize()
    return lab.cpu().numpy(), cnt.cpu().numpy(), roots.cpu().numpy(), n_roots.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize('h,w,n', [(1200, 1920, 2), (300, 656, 3), (602, 801, 2)])
def test_dark_labels_match_byte_passes(cpe, gpu, h, w, n):
    rng = np.random.default_rng(h * 7 + w)
    frames = _frames(rng, n, h, w)
    rects = [[0, 0, w - 1, h - 1]] + [[int(rng.integers(1, 70)), int(rng.integers(1, 20)), int(w - rng.integers(1, 70)),
                                       int(h - rng.integers(1, 20))] for _ in range(n - 1)]
    want = _run(cpe, gpu, frames, rects, 0)
    got = _run(cpe, gpu, frames, rects, 1)
    for i in range(n):
        x0, y0, x1, y1 = rects[i]
        tag = (h, w, i)
        assert np.array_equal(got[0][i], want[0][i]), (tag, int((got[0][i] != want[0][i]).sum()))
        assert np.array_equal(got[1][i], want[1][i]), (tag, int((got[1][i] != want[1][i]).sum()))
        assert got[3][i] == want[3][i], tag
        k = int(want[3][i])
        assert 0 < k <= got[2].shape[1], tag
        r = np.sort(got[2][i, :k])
        assert np.array_equal(r, np.sort(want[2][i, :k])), tag
        # and what the labelling means: every pixel of the set in the rectangle carries its root, the roots are the set's
        # components, their counts add up to the set
        win = np.zeros((h, w), bool)
        win[y0:y1 + 1, x0:x1 + 1] = True
        dark = win & (frames[i] <= THR)
        lab = got[0][i]
        assert np.array_equal(np.unique(lab[dark]), r), tag
        assert (lab.reshape(-1)[r] == r).all(), tag
        assert int(got[1][i].reshape(-1)[r].sum()) == int(dark.sum()), tag
