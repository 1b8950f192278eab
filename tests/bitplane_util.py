"""Helpers of the tests that read one-bit planes out of the detect workspace: the tiled layout of csrc/cpe_dev.h restated in
numpy (as tests/test_bitplane_layout_cpu.py restates it) and the lookup of a row of the workspace table."""
import ctypes as C

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
    """(offset, bytes per frame) of a row of the workspace table (cpe_debug_workspace_buffer)"""
    buf = C.create_string_buffer(64)
    off, per = C.c_size_t(), C.c_size_t()
    ov, side, pub = C.c_int32(), C.c_int32(), C.c_int32()
    k = 0
    while L.cpe_debug_workspace_buffer(n, h, w, k, buf, 64, C.byref(off), C.byref(per), C.byref(ov), C.byref(side), C.byref(pub)) == 0:
        if buf.value.decode() == name:
            return off.value, per.value
        k += 1
    raise KeyError(name)
