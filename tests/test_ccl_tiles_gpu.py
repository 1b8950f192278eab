"""The word-level labelling passes (csrc/ccl.hip: k_ccl_init64 labels the components of every 64 x 8 tile from its row masks,
k_ccl_merge64 unites across tile edges) against scipy.ndimage.label: the label of a pixel is the raster index of its
component's first pixel.  Frames are a few tiles large and drawn so that what can go wrong at a tile edge does: components
that close only in a neighbouring tile, contacts that exist only diagonally across an edge or a corner, tiles with more runs
than the in-tile work takes on (these keep per-run first labels), windows off the word grid and off the 8-row strips.

cpe_debug_ccl_tiles (include/cpe.h) runs ccl_components -- first labels, merge, root list -- for both connectivities, reading
the set from the bytes or from its one-bit plane, and hands out the label plane as links plus the root list.
cpe_debug_ccl runs the general pass, whose word-level merge still unites inside the tiles (its first labels are row-wise);
that entry takes frames of 64 rows and more, so it gets the same patterns at 64 + 8, 9, 16, 23 rows."""
import numpy as np
import pytest
import torch
from scipy import ndimage

WIDTHS = (64, 80, 128, 192)
HEIGHTS = (8, 9, 16, 23)


def _expected(mask, conn8):
    """as tests/test_ccl_gpu.py: raster index of the component's first pixel, -1 outside the set"""
    lab, k = ndimage.label(mask, structure=np.ones((3, 3)) if conn8 else None)
    idx = np.arange(mask.size, dtype=np.int64).reshape(mask.shape)
    out = np.full(mask.shape, -1, dtype=np.int64)
    if k:
        first = ndimage.minimum(idx, lab, index=np.arange(1, k + 1)).astype(np.int64)
        out[lab > 0] = first[lab[lab > 0] - 1]
    return out


def _tiled(tile, h, w):
    """one 8 x 64 drawing repeated in every tile of the frame"""
    return np.tile(tile, ((h + 7) // 8, (w + 63) // 64))[:h, :w]


def _serpentine_tile():
    t = np.zeros((8, 64), bool)
    t[0:8:2, 1:63] = True
    t[1, 62] = t[5, 62] = t[3, 1] = True
    return t


def _spiral_tile():
    t = np.zeros((8, 64), bool)
    t[0, 0:63] = True; t[0:8, 62] = True; t[7, 2:63] = True; t[2:8, 2] = True
    t[2, 2:59] = True; t[2:6, 58] = True; t[5, 6:59] = True; t[4, 6] = True
    return t


def _patterns(rng, h, w):
    """bool [k,h,w]: the frames of one call"""
    def z():
        return np.zeros((h, w), bool)
    def put(m, y, x, v=True):
        if 0 <= y < h and 0 <= x < w:
            m[y, x] = v
    out = [_tiled(_serpentine_tile(), h, w), _tiled(_spiral_tile(), h, w)]
    m = z(); m[0:9, 10] = True; m[0:9, 50] = True; m[8:9, 10:51] = True               # a U that closes in the tile below
    m[min(12, h - 1):, 5] = True
    out.append(m)
    m = z(); m[1, 20:65] = True; m[6, 20:65] = True; m[1:7, 64:65] = True              # a U that closes in the tile to the right
    out.append(m)
    m = z()                                                                             # diagonal-only contacts
    for (ya, xa, yb, xb) in ((7, 63, 8, 64), (7, 10, 8, 11), (3, 63, 4, 64), (7, 64, 8, 63), (7, 20, 8, 19), (5, 63, 4, 64),
                             (15, 127, 16, 128), (7, 127, 8, 128), (1, 64, 0, 63)):
        put(m, ya, xa); put(m, yb, xb)
    out.append(m)
    yy, xx = np.mgrid[0:h, 0:w]
    out.append((yy + xx) % 2 == 0)                                                      # checkerboard
    out.append(rng.random((h, w)) < 0.5)
    m = z(); m[:, ::3] = True; out.append(m)                                            # combs: loose teeth, teeth on a spine
    m = z(); m[:, 1::2] = True; m[h - 1, :] = True; out.append(m)
    m = z(); m[h // 2, :] = True; out.append(m)                                         # a row that crosses every word
    out.append(np.ones((h, w), bool))
    out.append(z())
    for d in (0.02, 0.5, 0.98):
        out.append(rng.random((h, w)) < d)
    out.append(ndimage.binary_dilation(rng.random((h, w)) < 0.01, iterations=2))        # blobs a few pixels thick
    m = z()                                                                             # thin slanted lines
    for x0 in range(0, w, 37):
        for y in range(h):
            put(m, y, x0 + y // 3); put(m, y, x0 + 20 - y)
    out.append(m)
    return np.stack(out)


def _windows(rng, n, h, w):
    """one window per frame, x0 y0 x1 y1 inclusive, edges anywhere (off the word grid, off the strips)"""
    r = np.empty((n, 4), np.int32)
    r[:, 0] = rng.integers(1, w // 2, n); r[:, 2] = rng.integers(w // 2, w - 1, n)
    r[:, 1] = rng.integers(0, h // 2, n); r[:, 3] = rng.integers(h // 2, h, n)
    r[0] = (0, 0, w - 1, h - 1)
    r[1] = (63, 1, min(w - 1, 64), h - 1)          # two columns, one on either side of a word edge
    return r


def _flatten(links, inside):
    """roots of the union-find links of one call (i32 [n,h,w], frame-relative indices)"""
    n = links.shape[0]
    L = links.reshape(n, -1).astype(np.int64)
    out = np.full_like(L, -1)
    own = np.arange(L.shape[1], dtype=np.int64)
    for f in range(n):
        p = np.where(L[f] < 0, own, L[f])
        while True:                     # pointer doubling; parents are never larger than their children (asserted by the caller)
            q = p[p]
            if np.array_equal(q, p):
                break
            p = q
        sel = inside[f].ravel()
        out[f, sel] = p[sel]
    return out.reshape(links.shape)


@pytest.mark.gpu
@pytest.mark.parametrize('w', WIDTHS)
@pytest.mark.parametrize('h', HEIGHTS)
def test_component_lists_and_links_match_scipy(cpe, gpu, h, w):
    """ccl_components: links and root list, both connectivities, byte and one-bit source, whole frames and windows"""
    from cpe_amd import api
    rng = np.random.default_rng(100 * h + w)
    frames = _patterns(rng, h, w)
    n = frames.shape[0]
    g = torch.from_numpy(frames.astype(np.uint8) * 200).to(gpu)
    ws = api.DetectWorkspace(n, h, w, gpu)
    L = cpe.lib.load()
    cap = 262144
    lab = torch.empty((n, h, w), dtype=torch.int32, device=gpu)
    roots = torch.empty((n, cap), dtype=torch.int32, device=gpu)
    nr = torch.empty(n, dtype=torch.int32, device=gpu)
    rects = _windows(rng, n, h, w)
    rect_d = torch.from_numpy(rects).to(gpu)
    for windowed in (0, 1):
        inside = frames.copy()
        if windowed:
            for f, (x0, y0, x1, y1) in enumerate(rects):
                keep = np.zeros((h, w), bool); keep[y0:y1 + 1, x0:x1 + 1] = True
                inside[f] &= keep
        for conn8 in (1, 0):
            want = np.stack([_expected(inside[f], conn8) for f in range(n)])
            for bits in (0, 1):
                lab.fill_(-7); roots.fill_(-7)
                cpe.lib.check(L.cpe_debug_ccl_tiles(g.data_ptr(), n, h, w, 100, conn8, bits, rect_d.data_ptr() if windowed else None,
                                                    ws.view.data_ptr(), ws.bytes, lab.data_ptr(), roots.data_ptr(), nr.data_ptr(),
                                                    torch.cuda.current_stream().cuda_stream), 'cpe_debug_ccl_tiles')
                torch.cuda.synchronize()
                links = lab.cpu().numpy()
                tag = (h, w, windowed, conn8, bits)
                assert (links[~inside] == -1).all(), tag                      # nothing written outside the set / the window
                own = np.arange(h * w, dtype=np.int64).reshape(h, w)
                assert ((links >= 0) & (links <= own))[inside].all(), tag     # parents are pixels with smaller indices
                got = _flatten(links, inside)
                bad = [(f, int((got[f] != want[f]).sum())) for f in range(n) if not np.array_equal(got[f], want[f])]
                assert not bad, (tag, bad)
                counts = nr.cpu().numpy()
                rl = roots.cpu().numpy()
                for f in range(n):
                    exp = np.unique(want[f][inside[f]])
                    assert counts[f] == exp.size, (tag, f, int(counts[f]), exp.size)
                    assert np.array_equal(np.sort(rl[f, :counts[f]]), exp), (tag, f)


@pytest.mark.gpu
@pytest.mark.parametrize('w', WIDTHS)
@pytest.mark.parametrize('hh', HEIGHTS)
def test_general_pass_labels_match_scipy(cpe, gpu, hh, w):
    """cpe_debug_ccl (row-wise first labels, word-level merge that unites inside the tiles too, flatten): labels of the same
    patterns, both connectivities"""
    from cpe_amd import api
    h = 64 + hh
    rng = np.random.default_rng(100 * h + w + 1)
    frames = _patterns(rng, h, w)
    n = frames.shape[0]
    g = torch.from_numpy(frames.astype(np.uint8) * 200).to(gpu)
    ws = api.DetectWorkspace(n, h, w, gpu)
    L = cpe.lib.load()
    for conn8 in (1, 0):
        cpe.lib.check(L.cpe_debug_ccl(g.data_ptr(), n, h, w, 100, 0, conn8, 0, 0, 1, ws.view.data_ptr(), ws.bytes,
                                      torch.cuda.current_stream().cuda_stream), 'cpe_debug_ccl')
        torch.cuda.synchronize()
        got = ws.plane('labels').cpu().numpy()
        for f in range(n):
            want = _expected(frames[f], conn8)
            assert np.array_equal(got[f], want), (h, w, conn8, f, int((got[f] != want).sum()))
