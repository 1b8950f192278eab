"""The tiled one-bit plane layout of cpe_dev.h (bit_tile_cols / bit_plane_words / bit_word), compiled for the host and
checked against a row-major reference restated in numpy: 64 x 8 tiles of 8 consecutive u64 words, word r of tile
(ty, tx) = row 8 ty + r, bit i = pixel 64 (tx - 1) + i; tile columns 0 and last and the rows >= h are zero."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'cylinder-pose-estimation_amd', 'csrc')
HIPCC = os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'bin', 'hipcc')

# packs a u8 mask (h, w, then h * w bytes on stdin) with bit_word and writes bit_plane_words(h, w) u64 words to stdout;
# also reads every pixel back through a 64-column window at each 32-column offset, the way BitWin::load assembles one
PACK = r'''
#include "cpe_dev.h"
#include <cstdio>
#include <vector>
using namespace cpe;
int main()
{
    int h, w;
    if (fread(&h, 4, 1, stdin) != 1 || fread(&w, 4, 1, stdin) != 1) return 2;
    std::vector<unsigned char> m((size_t)h * w);
    if (fread(m.data(), 1, m.size(), stdin) != m.size()) return 2;
    const int tc = bit_tile_cols(w);
    std::vector<unsigned long long> p(bit_plane_words(h, w), 0ull);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++)
            if (m[(size_t)y * w + x]) p[bit_word(tc, y, x >> 6)] |= 1ull << (x & 63);
    for (int y = 0; y < 8 * ((h + 7) / 8); y++)
        for (int k = -2; 32 * k + 63 < 64 * (tc - 1); k++) {
            const int j = k >> 1;
            unsigned long long v = p[bit_word(tc, y, j)];
            if (k & 1) v = (v >> 32) | (p[bit_word(tc, y, j + 1)] << 32);
            for (int b = 0; b < 64; b++) {
                const int x = 32 * k + b;
                const bool ref = y < h && x >= 0 && x < w && m[(size_t)y * w + x];
                if ((((v >> b) & 1ull) != 0) != ref) { fprintf(stderr, "window mismatch y %d x %d\n", y, x); return 1; }
            }
        }
    fwrite(p.data(), 8, p.size(), stdout);
    return 0;
}
'''


@pytest.fixture(scope='module')
def packer(tmp_path_factory):
    d = tmp_path_factory.mktemp('bitplane')
    src, exe = d / 'pack.cpp', d / 'pack'
    src.write_text(PACK)
    subprocess.run([HIPCC, '-std=c++17', '-O1', '--cuda-host-only', '-x', 'hip', '-I', CSRC, str(src), '-o', str(exe)],
                   check=True, capture_output=True)
    return str(exe)


def _reference(mask):
    h, w = mask.shape
    th, ww = (h + 7) // 8, (w + 63) // 64
    pad = np.zeros((8 * th, 64 * (ww + 2)), np.uint8)
    pad[:h, 64:64 + w] = mask != 0
    words = np.packbits(pad.reshape(8 * th, ww + 2, 64), axis=-1, bitorder='little').view('<u8')[..., 0]   # [row, tile column]
    return words.reshape(th, 8, ww + 2).transpose(0, 2, 1).reshape(-1)                                # tile-major, 8 rows each


@pytest.mark.parametrize('w', [640, 650, 801, 1920])
@pytest.mark.parametrize('h', [480, 483, 601, 1199])
def test_tiled_plane_matches_row_major_reference(packer, h, w):
    rng = np.random.default_rng(h * 7919 + w)
    mask = (rng.random((h, w)) < 0.3).astype(np.uint8) * 255
    mask[:, 0] = 255; mask[:, -1] = 255; mask[-1, :] = 255      # the last column / row: next to the zero padding
    p = subprocess.run([packer], input=np.array([h, w], '<i4').tobytes() + mask.tobytes(), capture_output=True)
    assert p.returncode == 0, p.stderr.decode()
    got = np.frombuffer(p.stdout, '<u8')
    ref = _reference(mask)
    assert got.size == ((h + 7) // 8) * ((w + 63) // 64 + 2) * 8 == ref.size   # bit_plane_words
    assert np.array_equal(got, ref)
    tiles = got.reshape((h + 7) // 8, (w + 63) // 64 + 2, 8)
    assert not tiles[:, 0].any() and not tiles[:, -1].any()      # zero tile columns
    assert not tiles[-1, :, h - 8 * (tiles.shape[0] - 1):].any()  # rows >= h of the last tile row
