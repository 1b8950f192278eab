"""LAB-L + CLAHE and the blob detector's 17 threshold planes (cpe_debug_clahe_planes, include/cpe.h): the passes the region
stage runs (fused 1: where rows start on 16-byte boundaries the apply pass writes the planes, the bucket sizes and the box
itself) against the byte-level apply followed by the planes' own pass (fused 0), bit for bit; and both against what the
CLAHE image they wrote says: planes[t] = cl > 50 + 10 t in the 64 x 8 tile layout, zero tile columns and zero rows below
the frame, bucket sizes, box of the pixels > 50.

Sizes: 1920x1200 (the product's frames), 1920x1203 (a partial last tile row; CLAHE pads the frame to 1924 columns),
656 wide (a multiple of 16 but not of 64), 640x480 (the smoke test's frames), 801 wide (rows not 16-byte aligned: both
paths are the byte-level ones).  Frames are bright up to their borders, so the box touches the frame's edges."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from clahe_cases import expected as _expected  # noqa: E402  (planes, bucket sizes and box as a CLAHE image defines them)

NTHR = 17


def _frames(rng, n, h, w):
    out = np.empty((n, h, w), np.uint8)
    for i in range(n):
        cy, cx = max(h // 40, 2), max(w // 40, 2)
        coarse = rng.integers(0, 256, size=(cy, cx)).astype(np.float32)
        img = np.kron(coarse, np.ones((h // cy + 1, w // cx + 1), np.float32))[:h, :w] + rng.normal(0, 12 + 8 * i, size=(h, w))
        img[rng.random((h, w)) < 0.01] = 255
        if i == 1:   # dark frame edges: the box lies inside
            img[:5], img[-7:], img[:, :9], img[:, -3:] = 0, 0, 0, 0
        out[i] = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    return out


def _run(cpe, gpu, frames, fused):
    from cpe_amd import api
    n, h, w = frames.shape
    th8, tc = (h + 7) // 8, (w + 63) // 64 + 2
    g = torch.from_numpy(frames).to(gpu)
    ws = api.DetectWorkspace(n, h, w, gpu)
    cl = torch.empty((n, h, w), dtype=torch.uint8, device=gpu)
    planes = torch.empty((n, NTHR, th8, tc, 8), dtype=torch.int64, device=gpu)
    buckets = torch.empty((n, NTHR + 1), dtype=torch.int32, device=gpu)
    box = torch.empty((n, 4), dtype=torch.int32, device=gpu)
    L = cpe.lib.load()
    cpe.lib.check(L.cpe_debug_clahe_planes(g.data_ptr(), n, h, w, fused, ws.view.data_ptr(), ws.bytes, cl.data_ptr(),
                                           planes.data_ptr(), buckets.data_ptr(), box.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream), 'cpe_debug_clahe_planes')
    torch.cuda.synchronize()
    return cl.cpu().numpy(), planes.cpu().numpy().view(np.uint64), buckets.cpu().numpy(), box.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize('h,w,n', [(1200, 1920, 2), (1203, 1920, 2), (480, 656, 3), (480, 640, 2), (602, 801, 2)])
def test_clahe_planes_match_byte_passes(cpe, gpu, h, w, n):
    rng = np.random.default_rng(h * 11 + w)
    frames = _frames(rng, n, h, w)
    cl0, pl0, bk0, box0 = _run(cpe, gpu, frames, 0)
    cl1, pl1, bk1, box1 = _run(cpe, gpu, frames, 1)
    assert np.array_equal(cl1, cl0), 'CLAHE image differs from the byte-level apply'
    want_pl, want_bk, want_box = _expected(cl0)
    assert np.array_equal(pl0, want_pl), 'planes of the separate pass differ from cl > threshold'
    assert np.array_equal(pl1, want_pl), 'planes of the apply pass differ from cl > threshold'
    assert np.array_equal(bk0[:, 1:], want_bk[:, 1:]) and np.array_equal(bk1[:, 1:], want_bk[:, 1:]), 'bucket sizes'
    assert np.array_equal(box0, want_box) and np.array_equal(box1, want_box), 'box of the pixels > 50'
