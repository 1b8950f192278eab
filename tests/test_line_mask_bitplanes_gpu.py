"""hmask and vmask as one-bit planes (masks.hip: k_open20_joints, line_masks_as_bits).  Where rows are a multiple of 16 pixels
the two masks are handed to k_roi_base as tiled one-bit planes kept in the workspace row `joints_mask`: n frames of hmask,
then n frames of vmask.  After a default call the planes must hold exactly the public byte planes: bit = byte != 0 for
every pixel, zero at columns >= w (the last word of an 800-pixel row is partial), at rows >= h (490 is not a multiple of 8)
and in the zero tile columns."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bitplane_util import decode_plane, plane_words, workspace_row  # noqa: E402


def test_decode_plane_inverts_the_tiled_layout():
    """CPU: decode_plane against the packing tests/test_bitplane_layout_cpu.py checks the header with"""
    rng = np.random.default_rng(5)
    for h, w in ((480, 640), (490, 800), (67, 80)):
        mask = rng.random((h, w)) < 0.4
        mask[:, -1] = True; mask[-1, :] = True
        th, ww = (h + 7) // 8, (w + 63) // 64
        pad = np.zeros((8 * th, 64 * (ww + 2)), np.uint8)
        pad[:h, 64:64 + w] = mask
        words = np.packbits(pad.reshape(8 * th, ww + 2, 64), axis=-1, bitorder='little').view('<u8')[..., 0]
        words = words.reshape(th, 8, ww + 2).transpose(0, 2, 1).reshape(-1)
        assert words.size == plane_words(h, w)
        got, clean = decode_plane(words, h, w)
        assert clean and np.array_equal(got, mask)
        words = words.copy(); words[7] = 1                      # a bit in the zero tile column
        assert not decode_plane(words, h, w)[1]


@pytest.mark.gpu
@pytest.mark.parametrize('h,w,seed', [(480, 640, 0), (600, 800, 4), (490, 800, 12)])
def test_line_mask_planes_equal_the_byte_planes(cpe, gpu, h, w, seed):
    from cpe_amd import synth
    b = synth.render_batch(2, h, w, seed=seed, with_gt=False)
    frames = torch.cat([b['left'], b['right']])[:3].contiguous()
    n = frames.shape[0]
    det = cpe.api.detect_grid_batch(frames.to(gpu))
    torch.cuda.synchronize()
    ws = det['ws']
    L = cpe.lib.load()
    off, per = workspace_row(L, n, h, w, 'joints_mask')
    pw = plane_words(h, w)
    assert per == h * w and 2 * pw * 8 <= per
    words = ws.view[off:off + 2 * n * pw * 8].cpu().numpy().view('<u8').reshape(2, n, pw)
    hm, vm = ws.plane('hmask').cpu().numpy(), ws.plane('vmask').cpu().numpy()
    assert hm.any() and vm.any()
    assert hm[:, :, 64 * ((w - 1) // 64):].any() and hm[:, 8 * ((h - 1) // 8):].any(), 'the last word and the last tile row hold pixels'
    for f in range(n):
        for k, name, ref in ((0, 'hmask', hm), (1, 'vmask', vm)):
            got, clean = decode_plane(words[k, f], h, w)
            assert clean, (name, f, 'bits outside the image')
            assert np.array_equal(got, ref[f] != 0), (name, f, int((got != (ref[f] != 0)).sum()))
