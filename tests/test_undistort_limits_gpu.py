"""Row f-3 at its limits: k_undistort_map, k_remap_bilinear4 / k_remap_bilinear1 and k_remap_cubic (csrc/undistort.hip) through
their C entries, against oracle/src/orc_undistort.c and the second statements of tests/undistort_cases.py.  Tolerance 0
everywhere.  What the cases reach is asserted without a GPU in tests/test_undistort_cases_cpu.py.

Every output buffer lies between two guards of 64 bytes and is filled with one sentinel value before the call; after it every
byte outside the defined output still holds the sentinel.  The frame buffers of the remap calls are followed by 8 further
frames that the test owns (sentinel too, and checked): a kernel that lost the bound of its frame loop would be caught by the
guard behind `dst`, not by a fault."""
import functools

import numpy as np
import pytest

import oracle
import test_prestep_gpu as P
import undistort_cases as U

GUARD, SENT = P.GUARD, P.SENT
SPARE_FRAMES = 8                    # REMAP_FRAMES of csrc/undistort.hip
NS = (1, 8, 9, U.NMAX)              # one group of frames, a group plus one, two groups plus one
ERR_ARG = -1                        # CPE_ERR_ARG


# ---------------------------------------------------------------- guarded device memory
def region(nbytes, offset=0, tail=0, data=None):
    """-> (tensor, address): nbytes of device memory at a 64-aligned address + offset, GUARD bytes in front and behind and
    `tail` bytes behind that, all SENT; `data` (any numpy array) is copied to the start of the region"""
    import torch
    buf = torch.full((GUARD + offset + nbytes + GUARD + tail,), SENT, dtype=torch.uint8, device='cuda')
    assert buf.data_ptr() % 64 == 0
    if data is not None:
        b = torch.from_numpy(np.ascontiguousarray(data).view(np.uint8).reshape(-1).copy())
        buf[GUARD + offset:GUARD + offset + b.numel()] = b.cuda()
    return buf, buf.data_ptr() + GUARD + offset


def written(buf, nbytes, offset=0):
    """the region's bytes, after checking that every byte of the buffer outside it is still SENT"""
    import torch
    torch.cuda.synchronize()
    a = buf.cpu().numpy()
    lo = GUARD + offset
    assert (a[:lo] == SENT).all(), 'bytes in front of the output were written'
    assert (a[lo + nbytes:] == SENT).all(), 'bytes behind the output were written'
    return a[lo:lo + nbytes]


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def lib():
    import cpe_amd
    return cpe_amd.lib.load()


def kernels_of(call):
    """-> (what call() returns, names of the kernels it launched)"""
    import cpe_amd
    cpe_amd.lib.profile_report()
    cpe_amd.lib.profile(True)
    try:
        r = call()
    finally:
        cpe_amd.lib.profile(False)
    return r, sorted(k for k, _, _ in cpe_amd.lib.profile_report())


# ---------------------------------------------------------------- cpe_undistort_map
def host_camera(Km, dist):
    """K f64[9] and the coefficients followed by NaN: a read beyond n_dist would poison the map"""
    Kc = np.ascontiguousarray(np.asarray(Km, dtype=np.float64).reshape(9))
    d = np.full(13, np.nan)
    d[:len(dist)] = dist
    return Kc, d


def run_map(Km, dist, h, w, null_dist=False):
    Kc, d = host_camera(Km, dist)
    bxy, pxy = region(h * w * 4)
    bf, pf = region(h * w * 2)
    rc = lib().cpe_undistort_map(Kc.ctypes.data, None if null_dist else d.ctypes.data, len(dist), h, w, pxy, pf, stream())
    assert rc == 0, lib().cpe_last_error_string().decode()
    return written(bxy, h * w * 4).view(np.int16).reshape(h, w, 2), written(bf, h * w * 2).view(np.uint16).reshape(h, w)


@pytest.mark.gpu
@pytest.mark.parametrize('h,w', U.SIZES)
@pytest.mark.parametrize('name', list(U.CAMERAS))
def test_map_kernel_matches_oracle(gpu, orc, name, h, w):
    Km, dist = U.camera(name, h, w)
    mxy, mf = U.oracle_map(name, h, w)
    xy, f = run_map(Km, dist, h, w)
    assert np.array_equal(xy, mxy), f'map_xy differs in {np.count_nonzero((xy != mxy).any(-1))} of {h * w} entries'
    assert np.array_equal(f, mf), f'map_f differs in {np.count_nonzero(f != mf)} of {h * w} entries'
    xy2, f2 = run_map(Km, dist, h, w, null_dist=(name == 'none'))     # `none`: the second call hands over no pointer at all
    assert np.array_equal(xy2, xy) and np.array_equal(f2, f)


@pytest.mark.gpu
def test_map_argument_errors_write_nothing(gpu, orc):
    h, w = 7, 5
    Km, dist = U.camera('barrel5', h, w)
    Kc, d = host_camera(Km, dist)
    sing, _ = host_camera([[1, 2, 3], [2, 4, 6], [0, 0, 1]], [])
    nofx, _ = host_camera([[0, 1, 3], [1, 0, 2], [0, 0, 1]], [])       # not singular, yet 1 / fx is what the model divides by
    nofy, _ = host_camera([[2, 1, 3], [1, 0, 2], [0, 0, 1]], [])
    for m in (sing, nofx, nofy):
        assert (np.linalg.det(m.reshape(3, 3)) == 0) == (m is sing)
    bxy, pxy = region(h * w * 4)
    bf, pf = region(h * w * 2)
    ok = dict(K=Kc.ctypes.data, dist=d.ctypes.data, n_dist=5, h=h, w=w, xy=pxy, f=pf)
    bad = [dict(n_dist=k) for k in (1, 2, 3, 6, 7, 13, -1)] + [dict(K=sing.ctypes.data), dict(K=nofx.ctypes.data), dict(K=nofy.ctypes.data),
           dict(h=0), dict(w=0), dict(h=32768), dict(w=32768), dict(h=-1), dict(K=None), dict(dist=None), dict(xy=None), dict(f=None)]
    L = lib()
    call = lambda a: L.cpe_undistort_map(a['K'], a['dist'], a['n_dist'], a['h'], a['w'], a['xy'], a['f'], stream())
    for b in bad:
        assert call(dict(ok, **b)) == ERR_ARG, b
        assert L.cpe_last_error_string().decode().startswith('cpe_undistort_map'), b
    assert (written(bxy, 0) == SENT).all() and (written(bf, 0) == SENT).all()
    assert call(ok) == 0
    mxy, mf = U.oracle_map('barrel5', h, w)
    assert np.array_equal(written(bxy, h * w * 4).view(np.int16).reshape(h, w, 2), mxy)
    assert np.array_equal(written(bf, h * w * 2).view(np.uint16).reshape(h, w), mf)


@pytest.mark.gpu
def test_map_refuses_a_camera_that_is_singular_in_a_later_stripe(gpu, orc):
    """the bottom row 0 -0.5 1 makes the determinant of the stripe at row y0 equal to 1 - y0 / 2: the first stripe inverts, the
    second (two rows per stripe at w = 2048) does not.  The oracle refuses the camera; so must the entry, before it writes."""
    Km = np.array([[1.0, 0, 0], [0, 1.0, 0], [0, -0.5, 1.0]])
    h, w = 4, 2048
    assert U.stripe_rows(h, w) == 2 and np.linalg.det(Km) == 1.0
    with pytest.raises(ValueError):
        orc.undistort_map(Km, [], h, w)
    Kc, d = host_camera(Km, [])
    bxy, pxy = region(h * w * 4)
    bf, pf = region(h * w * 2)
    assert lib().cpe_undistort_map(Kc.ctypes.data, d.ctypes.data, 0, h, w, pxy, pf, stream()) == ERR_ARG
    assert lib().cpe_last_error_string().decode().startswith('cpe_undistort_map: singular')
    assert (written(bxy, 0) == SENT).all() and (written(bf, 0) == SENT).all()
    mxy, mf = orc.undistort_map(Km, [], 2, w)               # its first stripe alone is a camera like any other
    xy, f = run_map(Km, [], 2, w)
    assert np.array_equal(xy, mxy) and np.array_equal(f, mf)


# ---------------------------------------------------------------- cpe_remap_bilinear_batch
def run_remap(entry, fr, n, maps, extra=(), off_src=0, off_maps=None, off_dst=0):
    """one call of a remap entry -> (u8 [n,h,w], kernels launched).  `maps`: the numpy arrays of the map arguments, in order;
    `extra`: integer arguments between the maps and dst (the cubic entry's fill)."""
    h, w = fr.shape[1:]
    N = h * w
    off_maps = off_maps or (0,) * len(maps)
    bsrc, psrc = region((len(fr) + SPARE_FRAMES) * N, off_src, data=fr)
    dev = [region(m.nbytes, o, data=m) for m, o in zip(maps, off_maps)]
    bdst, pdst = region(n * N, off_dst, tail=SPARE_FRAMES * N)
    args = [psrc, n, h, w] + [p for _, p in dev] + list(extra) + [pdst, stream()]
    rc, kernels = kernels_of(lambda: getattr(lib(), entry)(*args))
    assert rc == 0, lib().cpe_last_error_string().decode()
    return written(bdst, n * N, off_dst).reshape(n, h, w), kernels


def run_bilinear(fr, n, mxy, mf, off_src=0, off_xy=0, off_f=0, off_dst=0):
    return run_remap('cpe_remap_bilinear_batch', fr, n, (mxy, mf), (), off_src, (off_xy, off_f), off_dst)


def bilinear_kernel(h, w, off_xy=0, off_f=0, off_dst=0):
    """the kernel the wrapper picks: 4 pixels per thread where h*w is a multiple of 4 and dst and both maps are 16-aligned"""
    return ['k_remap_bilinear4' if (h * w) % 4 == 0 and off_xy % 16 == 0 and off_f % 16 == 0 and off_dst % 16 == 0 else 'k_remap_bilinear1']


@functools.lru_cache(maxsize=None)
def bilinear_expected(h, w):
    """u8 [M,NMAX,h,w] of oracle.remap_bilinear on the crafted maps, equal to the integer statement; read-only, shared"""
    oracle.build()
    mxy, mf = U.crafted_bilinear(h, w)
    fr = U.frames(h, w)
    e = np.stack([np.stack([oracle.remap_bilinear(f, mxy[k], mf[k]) for f in fr]) for k in range(len(mxy))])
    assert np.array_equal(e, np.stack([np.stack([U.remap_bilinear_np(f, mxy[k], mf[k]) for f in fr]) for k in range(len(mxy))]))
    e.setflags(write=False)
    return e


def same_frames(got, exp, what):
    for f in range(len(got)):
        assert np.array_equal(got[f], exp[f]), f'{what}: frame {f} differs in {np.count_nonzero(got[f] != exp[f])} of {got[f].size} pixels'


@pytest.mark.gpu
@pytest.mark.parametrize('h,w', U.BILINEAR_SIZES)
def test_bilinear_kernels_on_crafted_maps(gpu, h, w):
    mxy, mf = U.crafted_bilinear(h, w)
    fr, exp = U.frames(h, w), bilinear_expected(h, w)
    assert (fr[U.FRAME_255] == 255).all() and not fr[U.FRAME_0].any()
    for k in range(len(mxy)):
        for n in NS:
            got, kernels = run_bilinear(fr, n, mxy[k], mf[k])
            assert kernels == bilinear_kernel(h, w)
            same_frames(got, exp[k], f'map {k}, n={n}')


@pytest.mark.gpu
@pytest.mark.parametrize('h,w', U.BILINEAR_SIZES)
def test_bilinear_kernels_at_every_alignment(gpu, h, w):
    """n = 9 again with one pointer moved: the first six variants take the one-pixel kernel, a moved `src` keeps the 4-pixel one
    where the size allows it; every variant gives the bytes of the aligned call"""
    mxy, mf = U.crafted_bilinear(h, w)
    fr, exp = U.frames(h, w), bilinear_expected(h, w)
    variants = [dict(off_dst=1), dict(off_dst=2), dict(off_dst=4), dict(off_dst=8), dict(off_xy=4), dict(off_f=2), dict(off_src=1)]
    for k in range(len(mxy)):
        for v in variants:
            got, kernels = run_bilinear(fr, 9, mxy[k], mf[k], **v)
            assert kernels == bilinear_kernel(h, w, **{a: o for a, o in v.items() if a != 'off_src'}), v
            same_frames(got, exp[k], f'map {k}, {v}')
    assert bilinear_kernel(h, w, off_dst=8) == ['k_remap_bilinear1'] and bilinear_kernel(h, w) == bilinear_kernel(h, w, 0, 0, 0)


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['pincushion4', 'general', 'wrap', 'saturate'])
def test_bilinear_kernels_on_camera_maps(gpu, orc, name):
    for (h, w) in ((29, 37), (65, 130), (5, 4096)):
        mxy, mf = U.oracle_map(name, h, w)
        fr = U.frames(h, w)
        got, kernels = run_bilinear(fr, 9, mxy, mf)
        assert kernels == bilinear_kernel(h, w)
        same_frames(got, [orc.remap_bilinear(f, mxy, mf) for f in fr[:9]], f'{name} {h}x{w}')


@pytest.mark.gpu
def test_undistorter_and_undistort_image(gpu, orc):
    import torch
    from cpe_amd import iotool
    h, w = 65, 130
    Km, dist = U.camera('pincushion4', h, w)
    cam = dict(IntrinsicMatrix=Km.tolist(), RadialDistortion=dist[:2].tolist(), TangentialDistortion=dist[2:].tolist())
    mxy, mf = U.oracle_map('pincushion4', h, w)
    fr = U.frames(h, w)
    want = np.stack([orc.remap_bilinear(f, mxy, mf) for f in fr[:9]])
    und = iotool.Undistorter(cam, h, w, 'cuda:0')
    assert np.array_equal(und.map_xy.cpu().numpy(), mxy) and np.array_equal(und.map_f.cpu().numpy().view(np.uint16), mf)
    assert np.array_equal(und(torch.from_numpy(np.array(fr[:9])).cuda()).cpu().numpy(), want)
    assert np.array_equal(und(torch.from_numpy(np.array(fr[1])).cuda()).cpu().numpy(), want[1])
    assert np.array_equal(iotool.undistort_image(fr[0], cam), want[0])
    col = np.ascontiguousarray(np.moveaxis(fr[:3], 0, 2))
    got = iotool.undistort_image(col, cam)
    assert got.shape == (h, w, 3) and np.array_equal(got, np.moveaxis(want[:3], 0, 2))


@pytest.mark.gpu
@pytest.mark.parametrize('h,w', U.BILINEAR_SIZES)
def test_bilinear_identity_and_no_frames(gpu, h, w):
    mxy, mf = U.identity_bilinear(h, w)
    fr = U.frames(h, w)
    got, _ = run_bilinear(fr, 9, mxy, mf)
    assert np.array_equal(got, fr[:9])
    got, kernels = run_bilinear(fr, 0, mxy, mf)             # n = 0: returns 0, launches and writes nothing
    assert got.size == 0 and kernels == []


@pytest.mark.gpu
def test_bilinear_argument_errors_write_nothing(gpu):
    h, w, N = 3, 5, 15
    mxy, mf = U.identity_bilinear(h, w)
    fr = U.frames(h, w)
    bsrc, psrc = region(2 * N, data=fr[:2])
    bxy, pxy = region(mxy.nbytes, data=mxy)
    bf, pf = region(mf.nbytes, data=mf)
    bdst, pdst = region(2 * N)
    ok = dict(src=psrc, n=2, h=h, w=w, xy=pxy, f=pf, dst=pdst)
    bad = [dict(dst=psrc), dict(src=None), dict(xy=None), dict(f=None), dict(dst=None), dict(n=-1), dict(h=0), dict(w=0), dict(h=32768),
           dict(w=32768), dict(h=-3)]
    L = lib()
    call = lambda a: L.cpe_remap_bilinear_batch(a['src'], a['n'], a['h'], a['w'], a['xy'], a['f'], a['dst'], stream())
    for b in bad:
        assert call(dict(ok, **b)) == ERR_ARG, b
        assert L.cpe_last_error_string().decode().startswith('cpe_remap_bilinear_batch'), b
    assert call(dict(ok, n=0)) == 0
    assert (written(bdst, 0) == SENT).all()
    assert np.array_equal(written(bsrc, 2 * N), fr[:2].ravel())                                    # src == dst was refused, not run
    assert call(ok) == 0
    assert np.array_equal(written(bdst, 2 * N).reshape(2, h, w), fr[:2])


@pytest.mark.gpu
def test_python_side_refuses_what_the_reference_cannot_mean(gpu):
    import torch
    import cpe_amd
    from cpe_amd import iotool
    h, w = 29, 37
    Km, _ = U.camera('none', h, w)
    cam = lambda rad, tan: dict(IntrinsicMatrix=Km.tolist(), RadialDistortion=rad, TangentialDistortion=tan)
    K2, d = iotool.camera_arrays(cam([1.0, 2.0, 3.0], [4.0, 5.0]))          # iotool.py:33-36: radial first, tangential last
    assert np.array_equal(K2, Km) and d.tolist() == [1.0, 2.0, 3.0, 4.0, 5.0]
    for rad in ([0.1], [0.1, 0.01, 0.001, 0.0, 0.0]):                       # 3 and 7 stacked coefficients
        with pytest.raises(cpe_amd.lib.CpeError):
            iotool.Undistorter(cam(rad, [0.0, 0.0]), h, w, 'cuda:0')
    und = iotool.Undistorter(cam([0.1, 0.01], [0.0, 0.0]), h, w, 'cuda:0')
    good = torch.zeros((2, h, w), dtype=torch.uint8, device='cuda:0')
    assert und(good).shape == (2, h, w)
    for t in (good.to(torch.int16), good.to(torch.float32), torch.zeros((2, h, 2 * w), dtype=torch.uint8, device='cuda:0')[:, :, ::2],
              torch.zeros((2, w, h), dtype=torch.uint8, device='cuda:0'), torch.zeros((2, h, w + 1), dtype=torch.uint8, device='cuda:0'),
              torch.zeros((2, h, w, 1), dtype=torch.uint8, device='cuda:0')):
        with pytest.raises(cpe_amd.lib.CpeError):
            und(t)


# ---------------------------------------------------------------- cpe_remap_cubic_batch on its own
def run_cubic(fr, n, m, fill):
    return run_remap('cpe_remap_cubic_batch', fr, n, (m,), (fill,))


@functools.lru_cache(maxsize=None)
def cubic_expected(h, w, fill, crafted=False):
    oracle.build()
    m = U.crafted_cubic(h, w) if crafted else P.oracle_map(h, w)
    e = np.stack([oracle.remap_cubic(f, m, fill) for f in U.frames(h, w)])
    e.setflags(write=False)
    return e


@pytest.mark.gpu
@pytest.mark.parametrize('h,w', P.SIZES)
def test_cubic_kernel_matches_oracle(gpu, h, w):
    fr, m = U.frames(h, w), P.oracle_map(h, w)
    for fill in (0, 201):
        exp = cubic_expected(h, w, fill)
        assert (exp.reshape(U.NMAX, -1)[:, P.classes(m)['outside'].ravel()] == fill).all()
        for n in NS:
            got, kernels = run_cubic(fr, n, m, fill)
            assert kernels == ['k_remap_cubic']
            same_frames(got, exp, f'fill {fill}, n={n}')


@pytest.mark.gpu
@pytest.mark.parametrize('h,w', [(3, 3), (5, 7), (29, 37)])
def test_cubic_kernels_on_special_map_values(gpu, h, w):
    """NaN, +-inf, -0.0, +-1e30, the last pixel and the floats next to the image's edges in the map: k_remap_cubic alone, then
    k_prestep<uint8_t, 1> and <uint8_t, 3>, which share its map handling"""
    import torch
    m = U.crafted_cubic(h, w)
    fr = U.frames(h, w)
    for fill in (0, 201):
        got, _ = run_cubic(fr, 9, m, fill)
        same_frames(got, cubic_expected(h, w, fill, True), f'fill {fill}')
        m_dev = torch.from_numpy(np.array(m)).cuda()
        for ch in (1, 3):
            raw = P.raw_frames(h, w, 'uint8', ch)[:9]
            rc, buf = P.run(raw, m_dev, 9, h * w, fill=fill)
            assert rc == 0
            P.check_frames(buf, P.compose(raw, m, fill), 9, h * w, 0, f'prestep, {ch} channels, fill {fill}')


@pytest.mark.gpu
def test_cubic_argument_errors_write_nothing(gpu):
    h, w, N = 5, 7, 35
    fr, m = U.frames(h, w), P.oracle_map(h, w)
    bsrc, psrc = region(2 * N, data=fr[:2])
    bm, pm = region(m.nbytes, data=m)
    bdst, pdst = region(2 * N)
    ok = dict(src=psrc, n=2, h=h, w=w, m=pm, fill=201, dst=pdst)
    bad = [dict(dst=psrc), dict(src=None), dict(m=None), dict(dst=None), dict(n=-1), dict(h=2), dict(w=2), dict(fill=-1), dict(fill=256),
           dict(m=pm + 4), dict(h=1 << 16, w=1 << 16)]
    L = lib()
    call = lambda a: L.cpe_remap_cubic_batch(a['src'], a['n'], a['h'], a['w'], a['m'], a['fill'], a['dst'], stream())
    for b in bad:
        assert call(dict(ok, **b)) == ERR_ARG, b
        assert L.cpe_last_error_string().decode().startswith('cpe_remap_cubic_batch'), b
    assert call(dict(ok, n=0)) == 0
    assert (written(bdst, 0) == SENT).all()
    assert call(ok) == 0
    assert np.array_equal(written(bdst, 2 * N).reshape(2, h, w), cubic_expected(h, w, 201)[:2])
