"""Helpers of the tests that read one-bit planes out of the detect workspace: the tiled layout of csrc/cpe_dev.h restated in
numpy (as tests/test_bitplane_layout_cpu.py restates it) and the lookup of a row of the workspace table."""
import numpy as np


def plane_words(h, w):
    """u64 words of one plane (bit_plane_words)"""
    return ((h + 7) // 8) * ((w + 63) // 64 + 2) * 8


def decode_plane(words, h, w):
    """u64 words of one tiled plane (cpe_dev.h) -> (bool [h, w], True if every bit outside the image is zero)"""
    th, ww = (h + 7) // 8, (w + 63) // 64
    assert words.size == th * (ww + 2) * 8
    rows = words.reshape(th, ww + 2, 8).transpose(0, 2, 1).reshape(8 * th, ww + 2)
    bits = np.unpackbits(np.ascontiguousarray(rows).view(np.uint8).reshape(8 * th, (ww + 2) * 8), axis=1, bitorder='little')
    inside = bits[:h, 64:64 + w].astype(bool)
    outside = bits.copy()
    outside[:h, 64:64 + w] = 0
    return inside, not outside.any()


def workspace_row(L, n, h, w, name):
    """(offset, bytes per frame) of a row of the workspace table (cpe_amd.api.workspace_row; L: the loaded library, unused)"""
    from cpe_amd import api
    return api.workspace_row(n, h, w, name)
