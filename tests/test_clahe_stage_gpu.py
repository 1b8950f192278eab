"""LAB-L + CLAHE(4.5, 4 x 4), the front end of the region stage, on its own against the oracle, tolerance 0 (cpe_debug_clahe_planes
for grey frames, cpe_debug_clahe_planes_bgr for true-colour ones, include/cpe.h; fused 1: the passes the detector runs, 0: the
byte-level apply and the planes' own pass).  The CLAHE image must equal `stages.clahe(stages.lab_l(grey))` /
`stages.clahe(stages.lab_l_bgr(bgr))`, and the 17 planes, the bucket sizes and the box must be what the *oracle's* image defines.

The inputs are the generated cases of tests/clahe_cases.py (tile histograms with chosen clip residuals, pixel orders, grey values
that share an L value, neighbouring tiles with very different tables, at the sizes that reach each load path, both apply kernels
and the padded geometries); tests/test_clahe_generators_cpu.py shows that each rule of CLAHE changes a pixel of a named case.
Here: every case in a mixed batch, the batch reversed and each frame alone (cross-frame leaks of hist, nrect, sw); two different
calls on one workspace; frame pointers 0, 1 and 4 bytes off a 16-byte boundary (the dword and byte paths, the refusal of the
fused pass); all 2^24 colours through k_bgr2labl (c_gamma and c_ly entry by entry, the grid-stride loop's second trip);
grey-replicated colours against the grey entry (c_lab_l); true-colour versions of grey cases whose L plane is not LAB-L of the
luma."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clahe_cases as K  # noqa: E402

NTHR = K.NTHR


def _outputs(n, h, w, gpu):
    th8, tc = (h + 7) // 8, (w + 63) // 64 + 2
    return dict(cl=torch.empty((n, h, w), dtype=torch.uint8, device=gpu),
                planes=torch.empty((n, NTHR, th8, tc, 8), dtype=torch.int64, device=gpu),
                buckets=torch.empty((n, NTHR + 1), dtype=torch.int32, device=gpu),
                box=torch.empty((n, 4), dtype=torch.int32, device=gpu))


def _host(o):
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in o.items()}
    out['planes'] = out['planes'].view(np.uint64)
    return out


def _run(cpe, gpu, frames, fused, ws=None):
    """frames: u8 [n,h,w] numpy array, or a device tensor (a view at the address the test wants)"""
    from cpe_amd import api
    g = frames if torch.is_tensor(frames) else torch.from_numpy(np.array(frames, order='C')).to(gpu)
    n, h, w = g.shape
    ws = api.DetectWorkspace(n, h, w, gpu) if ws is None else ws.use(n)
    o = _outputs(n, h, w, gpu)
    L = cpe.lib.load()
    cpe.lib.check(L.cpe_debug_clahe_planes(g.data_ptr(), n, h, w, fused, ws.view.data_ptr(), ws.bytes, o['cl'].data_ptr(),
                                           o['planes'].data_ptr(), o['buckets'].data_ptr(), o['box'].data_ptr(),
                                           torch.cuda.current_stream().cuda_stream), 'cpe_debug_clahe_planes')
    return _host(o)


def _run_bgr(cpe, gpu, bgr, fused, ws=None):
    from cpe_amd import api
    g = bgr if torch.is_tensor(bgr) else torch.from_numpy(np.array(bgr, order='C')).to(gpu)
    n, h, w, c = g.shape
    assert c == 3
    ws = api.DetectWorkspace(n, h, w, gpu) if ws is None else ws.use(n)
    o = _outputs(n, h, w, gpu)
    o['L'] = torch.empty((n, h, w), dtype=torch.uint8, device=gpu)
    L = cpe.lib.load()
    cpe.lib.check(L.cpe_debug_clahe_planes_bgr(g.data_ptr(), n, h, w, fused, ws.view.data_ptr(), ws.bytes, o['L'].data_ptr(),
                                               o['cl'].data_ptr(), o['planes'].data_ptr(), o['buckets'].data_ptr(),
                                               o['box'].data_ptr(), torch.cuda.current_stream().cuda_stream),
                  'cpe_debug_clahe_planes_bgr')
    return _host(o)


def _check(out, refs, what):
    """frame f of the outputs against the oracle's view refs[f] (clahe_cases.ref)"""
    for f, r in enumerate(refs):
        tag = f'{what}, frame {f}'
        if 'L' in out:
            assert np.array_equal(out['L'][f], r['L']), f'{tag}: L plane differs from the oracle'
        bad = out['cl'][f] != r['cl']
        assert not bad.any(), f'{tag}: {int(bad.sum())} CLAHE pixels differ from the oracle, first at {tuple(np.argwhere(bad)[0])}'
        assert np.array_equal(out['planes'][f], r['planes']), f'{tag}: planes differ from oracle image > threshold'
        assert np.array_equal(out['buckets'][f, 1:], r['buckets'][1:]), f'{tag}: bucket sizes'
        assert np.array_equal(out['box'][f], r['box']), f'{tag}: box of the pixels > 50'


def _same(a, b, what):
    for k in a:
        x, y = (a[k][:, 1:], b[k][:, 1:]) if k == 'buckets' else (a[k], b[k])
        assert np.array_equal(x, y), f'{what}: {k} differs'


# ---------------------------------------------------------------- grey: every case, in batches and alone
@pytest.mark.gpu
@pytest.mark.parametrize('fused', [0, 1])
@pytest.mark.parametrize('size', [s for s in K.sizes() if s != K.HUGE], ids=lambda s: f'{s[0]}x{s[1]}')
def test_grey_cases_match_oracle(cpe, orc, gpu, size, fused):
    """the cases of one size as a mixed batch, the batch reversed, and each frame alone: all equal the oracle, so all are
    bit-identical to each other"""
    names = K.names([size])
    assert len(names) >= 2
    refs = [K.ref(n) for n in names]
    frames = np.stack([K.get(n)['gray'] for n in names])
    batch = _run(cpe, gpu, frames, fused)
    _check(batch, refs, f'batch {names}')
    rev = _run(cpe, gpu, frames[::-1], fused)
    _check(rev, refs[::-1], f'reversed batch {names}')
    _same({k: v[::-1] for k, v in rev.items()}, batch, 'reversed batch against batch')
    for f, n in enumerate(names):
        one = _run(cpe, gpu, frames[f:f + 1], fused)
        _check(one, refs[f:f + 1], f'{n} alone')
        _same(one, {k: v[f:f + 1] for k, v in batch.items()}, f'{n} alone against its frame of the batch')


@pytest.mark.gpu
def test_largest_frame(cpe, orc, gpu):
    """the one 4096 x 4096 frame (tiles of 2^20 pixels, clip limit 18432), with both sets of passes"""
    (name,) = K.names([K.HUGE])
    for fused in (0, 1):
        _check(_run(cpe, gpu, K.get(name)['gray'][None], fused), [K.ref(name)], f'{name}, fused {fused}')


# ---------------------------------------------------------------- one workspace, different calls one after the other
@pytest.mark.gpu
def test_workspace_reuse(cpe, orc, gpu):
    """a bright batch, then fewer and darker frames, then colour frames, then the first again, on one workspace: nothing of a
    call (histograms, box, bucket sizes, planes, the L plane in the disc plane) survives into the next"""
    from cpe_amd import api
    ws = api.DetectWorkspace(4, 320, 512, gpu)
    a = ['full_320x512', 'patchA_320x512', 'resid_320x512', 'patchB_320x512']
    b = ['resid2_320x512', 'patchB_320x512']
    fa = np.stack([K.get(n)['gray'] for n in a]); fb = np.stack([K.get(n)['gray'] for n in b])
    first = _run(cpe, gpu, fa, 1, ws)
    _check(first, [K.ref(n) for n in a], 'first call')
    _check(_run(cpe, gpu, fb, 0, ws), [K.ref(n) for n in b], 'second call, fewer frames, byte passes')
    _check(_run(cpe, gpu, fb, 1, ws), [K.ref(n) for n in b], 'third call, fused')
    rc = [K.ref('patchA_320x512', v) for v in range(3)]
    _check(_run_bgr(cpe, gpu, np.stack([r['bgr'] for r in rc]), 1, ws), rc, 'fourth call, colour')
    again = _run(cpe, gpu, fa, 1, ws)
    _same(again, first, 'first call repeated')


# ---------------------------------------------------------------- frame pointers off the 16-byte grid
@pytest.mark.gpu
@pytest.mark.parametrize('fused', [0, 1])
@pytest.mark.parametrize('h,w,names', [(320, 512, ['patchA_320x512', 'resid_320x512']),
                                       (65, 67, ['patchA_65x67', 'patchB_65x67', 'zeros_65x67'])])
def test_base_alignment(cpe, orc, gpu, h, w, names, fused):
    """the frames 0, 1 and 4 bytes into a larger tensor: 4 keeps the dword paths and refuses the 16-byte ones (histogram and the
    fused apply), 1 leaves the byte paths; at 65 x 67 frames 1 and 2 of a batch are unaligned in any case"""
    n = len(names)
    frames = torch.from_numpy(np.stack([K.get(m)['gray'] for m in names]))
    refs = [K.ref(m) for m in names]
    buf = torch.zeros(n * h * w + 64, dtype=torch.uint8, device=gpu)
    assert buf.data_ptr() % 16 == 0
    for off in (0, 1, 4):
        view = buf[off:off + n * h * w].view(n, h, w)
        view.copy_(frames)
        assert view.data_ptr() % 16 == off
        _check(_run(cpe, gpu, view, fused), refs, f'base offset {off}')


# ---------------------------------------------------------------- colour: the L plane of every colour
@pytest.mark.gpu
def test_all_colours_l_plane(cpe, orc, gpu):
    """all 2^24 colours as 16 frames of 1024 x 1024 and a 17th random frame (n h w > 2^24 = 65536 workgroups x 256 threads: the
    grid-stride loop of k_bgr2labl takes a second trip): L equals the oracle's everywhere -- c_gamma and c_ly entry by entry --
    and the CLAHE image is the oracle's CLAHE of it"""
    from oracle import stages as S
    v = np.arange(1 << 24, dtype=np.uint32).reshape(16, 1024, 1024)
    bgr = np.empty((17, 1024, 1024, 3), np.uint8)
    bgr[:16, ..., 0] = v & 255; bgr[:16, ..., 1] = (v >> 8) & 255; bgr[:16, ..., 2] = v >> 16
    bgr[16] = np.random.default_rng(17).integers(0, 256, (1024, 1024, 3))
    out = _run_bgr(cpe, gpu, bgr, 1)
    for f in range(17):
        L = S.lab_l_bgr(bgr[f])
        bad = out['L'][f] != L
        assert not bad.any(), f'frame {f}: {int(bad.sum())} colours with another L, first {bgr[f][tuple(np.argwhere(bad)[0])]}'
        assert np.array_equal(out['cl'][f], S.clahe(L)), f'frame {f}: CLAHE of the L plane'


@pytest.mark.gpu
@pytest.mark.parametrize('fused', [0, 1])
def test_grey_replicated_colours_are_the_grey_path(cpe, orc, gpu, fused):
    """B = G = R = v through the colour entry and v through the grey entry: the same L (= LAB-L of the oracle) and the same
    CLAHE image, on frames that hold all 256 grey values: pins region.hip's c_lab_l against detect.hip's tables"""
    from oracle import stages as S
    for names in (['patchA_320x512', 'patchB_320x512'], ['patchA_317x512'], ['patchA_65x67', 'patchB_65x67'], ['patchA_64x64']):
        grey = np.stack([K.get(m)['gray'] for m in names])
        if grey.shape[1] >= 300:
            assert all(len(np.unique(g)) == 256 for g in grey)
        col = _run_bgr(cpe, gpu, np.repeat(grey[..., None], 3, 3), fused)
        mono = _run(cpe, gpu, grey, fused)
        assert np.array_equal(col['L'], np.stack([S.lab_l(g) for g in grey]))
        _same({k: col[k] for k in mono}, mono, f'{names}: colour entry on grey-replicated frames against the grey entry')


# ---------------------------------------------------------------- colour: CLAHE of a true-colour frame's L plane
@pytest.mark.gpu
@pytest.mark.parametrize('fused', [0, 1])
@pytest.mark.parametrize('name', K.COLOUR_CASES)
def test_colour_cases_match_oracle(cpe, orc, gpu, name, fused):
    """three colour versions of a grey case (a red, a blue and a green dominant) as one batch: L, CLAHE image, planes, bucket
    sizes and box equal the oracle's colour path, and that path is not the luma path in disguise"""
    from oracle import stages as S
    refs = [K.ref(name, v) for v in range(3)]
    for r in refs:
        assert (r['L'] != S.lab_l(S.bgr2gray(r['bgr']))).mean() > 0.2
    _check(_run_bgr(cpe, gpu, np.stack([r['bgr'] for r in refs]), fused), refs, f'{name} in colour')
