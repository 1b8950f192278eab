"""Stage a-1's f64 planes (cpe_debug_preprocess, include/cpe.h) against the oracle bit for bit, at every strip and border edge.

The 0/255 mask the product entry returns is blind to almost any f64 error: no pixel of a typical frame has its eigenvalue b
within 1e-6 (relative) of its Sauvola threshold T, so a wrong summation order, a lost outer Gaussian tap or a square root
one ulp off changes b and T but no mask byte.  The debug entry runs the same kernel with b and T stored beside the mask.
Every case compares:
  - b and T with oracle.preprocess(want_b=True) / oracle.sauvola_threshold as f64 bits, reporting the first differing pixel
    and its 128-column strip;
  - the debug mask, the product mask (cpe_preprocess_batch) and the oracle mask with each other, and the mask with
    where(b > T, 0, 255) of the kernel's own planes;
  - b with an independent scipy / numpy chain (within 1e-12 max|b|), and T, computed from the kernel's own b, with a
    long-double separable 15 x 15 box (within 1e-13 max|b|; the f64 evaluation is ~1e-15 max|b| from it, a lost box tap
    ~1e-5).
The shapes walk the kernel's branches: heights 8 .. 24 (the reflected first / last row blocks meet, no straight-line P6
row) and 39 .. 44 (the first straight-line rows); widths around the strip edges (one-column last strips, a strip ending
exactly at w, w - sx0 in 136 .. 152 where the LDS-DMA window leaves the frame, odd widths that take the byte loads);
1199 .. 1202 x {1920, 1922}; 2160 x 3840, 8 x 4096 and 4096 x 24; byte-offset (unaligned) bases and a batch of 40
distinct frames.  test_helpers_report_one_ulp runs the same comparison on oracle planes with one ulp changed (no GPU)."""
import numpy as np
import pytest
import torch
from scipy import ndimage

SW = 128                     # csrc/preprocess.hip: output columns per strip
WIDTHS = (8, 9, 23, 24, 127, 128, 129, 152, 153, 255, 256, 257, 264, 265, 276, 277, 279, 280, 284)
B_TOL = 1e-12                # |b - scipy chain| <= B_TOL * max|b|
T_TOL = 1e-13                # |T - long-double box| <= T_TOL * max|b|


# ---------------------------------------------------------------- content (u8 frames)
def edge_columns(w):
    """the columns a strip's windows turn at: sx0 - 24 (gray window start), sx0 - 1, sx0, sx0 + 127 of every strip, and the
    last two"""
    cols = {w - 2, w - 1}
    for sx0 in range(0, w, SW):
        cols |= {sx0 - 24, sx0 - 1, sx0, sx0 + SW - 1}
    return sorted(c for c in cols if 0 <= c < w)


def impulses(h, w, amp):
    """single pixels of `amp` on black: on every edge column (rows 1 and h / 2), along the last two rows and down the last
    two columns.  amp 4 is the smallest impulse the 5 x 5 binomial keeps (as 1 DN at its centre)."""
    f = np.zeros((h, w), np.uint8)
    cols = edge_columns(w)
    for c in cols:
        f[[1, h // 2], c] = amp
    f[h - 2:, cols + [w // 3]] = amp
    f[[0, h // 3, h - 1], w - 2:] = amp
    return f


def seam_steps(h, w):
    """vertical steps on every strip seam (alternating 60 / 190 bands) and a horizontal one at h / 2"""
    x = np.arange(w)
    f = np.where((x // SW) % 2 == 0, 60, 190)[None, :].repeat(h, 0)
    f[h // 2:] += 30
    return f.astype(np.uint8)


def content(h, w, seed, kinds=None):
    """name -> u8[h,w]: distinct frames of one shape (`kinds`: a subset of the names, in their order)"""
    from cpe_amd import synth
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[:h, :w]
    gen = {
        'synth': lambda: synth.render_batch(1, h, w, seed=seed, with_gt=False)['left'][0].numpy(),
        'noise': lambda: rng.integers(0, 256, (h, w), dtype=np.uint8),
        'const0': lambda: np.zeros((h, w), np.uint8),
        'const128': lambda: np.full((h, w), 128, np.uint8),
        'const255': lambda: np.full((h, w), 255, np.uint8),
        'imp4': lambda: impulses(h, w, 4),
        'imp255': lambda: impulses(h, w, 255),
        'steps': lambda: seam_steps(h, w),
        'checker': lambda: np.where(((y // 3) + (x // 3)) % 2 == 0, 40, 220).astype(np.uint8),
        'ramp': lambda: (100 + (x + 2 * y) // 9).astype(np.uint8),       # 1-DN steps: tiny variances
    }
    return {k: gen[k]() for k in (kinds or gen)}


# ---------------------------------------------------------------- references
def oracle_planes(orc, frame):
    _, mask, b = orc.preprocess(frame, want_b=True)
    return dict(mask=mask, b=b, T=orc.sauvola_threshold(b))


def scipy_b(frame):
    """b from scipy / numpy alone: blur5 (binomial, mirror = BORDER_REFLECT_101, rounded half up), img_as_float, Gaussian
    sigma 3 (mode constant, truncate 4), np.gradient twice, the smaller eigenvalue"""
    k = np.array([1, 4, 6, 4, 1], float)
    blurred = np.floor(ndimage.correlate(frame.astype(float), np.outer(k, k), mode='mirror') / 256 + 0.5)
    G = ndimage.gaussian_filter(blurred / 255, 3.0, mode='constant', cval=0, truncate=4.0)
    gy, gx = np.gradient(G)
    m00 = np.gradient(gx, axis=1)
    m01 = np.gradient(gx, axis=0)
    m11 = np.gradient(gy, axis=0)
    return (m00 + m11) / 2 - np.sqrt(4 * m01 * m01 + (m00 - m11) ** 2) / 2


def longdouble_T(b):
    """Sauvola threshold (window 15, k 0.5, R 128) of b with a separable 15-term box, edge padding, in long double"""
    h, w = b.shape
    p = np.pad(b.astype(np.longdouble), 7, mode='edge')

    def box(a):
        r = a[:, 0:w].copy()
        for j in range(1, 15):
            r += a[:, j:j + w]
        s = r[0:h].copy()
        for i in range(1, 15):
            s += r[i:i + h]
        return s / 225

    m, msq = box(p), box(p * p)
    sd = np.sqrt(np.maximum(msq - m * m, 0))
    return m * (1 + (sd / 128 - 1) / 2)


# ---------------------------------------------------------------- comparison
def first_diff(name, got, want):
    """None if the arrays are equal (f64: bit for bit), else (name, y, x, message) for the first differing pixel"""
    if got.dtype == np.float64:
        got, want = got.view(np.uint64), want.view(np.uint64)
        fmt = lambda v: float(np.array(v, np.uint64).view(np.float64)).hex()
    else:
        fmt = int
    bad = got != want
    if not bad.any():
        return None
    y, x = np.unravel_index(np.argmax(bad), bad.shape)
    return (name, int(y), int(x), f'{name}: {int(bad.sum())} px differ, first at y={y} x={x} (strip {x // SW}): '
                                  f'{fmt(got[y, x])} != {fmt(want[y, x])}')


def first_over(name, err, tol):
    """None if every |err| <= tol, else (name, y, x, message) for the first pixel over it"""
    bad = ~(np.abs(err) <= tol)
    if not bad.any():
        return None
    y, x = np.unravel_index(np.argmax(bad), bad.shape)
    return (name, int(y), int(x), f'{name}: {int(bad.sum())} px beyond {tol:.3g}, first at y={y} x={x} (strip {x // SW}): '
                                  f'error {float(err[y, x]):.3g}, worst {float(np.nanmax(np.abs(err))):.3g}')


def plane_errors(frame, got, ref):
    """every check of the module docstring on one frame.  got: mask, b, T (and mask_prod, the product entry's mask, when
    there is one); ref: oracle_planes of the frame.  -> list of (check, y, x, message), empty when all hold."""
    b, T = got['b'], got['T']
    scale = float(np.abs(ref['b']).max())
    out = [first_diff('b', b, ref['b']), first_diff('T', T, ref['T']),
           first_diff('mask', got['mask'], ref['mask']),
           first_diff('mask(b,T)', got['mask'], np.where(b > T, 0, 255).astype(np.uint8))]
    if 'mask_prod' in got:
        out.append(first_diff('mask_prod', got['mask_prod'], got['mask']))
    out.append(first_over('b~scipy', b - scipy_b(frame), B_TOL * scale))
    out.append(first_over('T~longdouble', (T - longdouble_T(b)).astype(np.float64), T_TOL * scale))
    return [e for e in out if e is not None]


def gpu_planes(cpe, dev, frames, offset=0):
    """the product entry and the debug entry on frames u8[n,h,w]; offset: the batch starts `offset` bytes into its buffer.
    Outputs start as sentinels (mask 77, b and T NaN), so a pixel left unwritten fails every comparison."""
    n, h, w = frames.shape
    buf = torch.empty(n * h * w + 4, dtype=torch.uint8, device=dev)
    g = buf[offset:offset + n * h * w].view(n, h, w)
    g.copy_(torch.from_numpy(np.ascontiguousarray(frames)))
    mp = torch.full((n, h, w), 77, dtype=torch.uint8, device=dev)
    md = torch.full((n, h, w), 77, dtype=torch.uint8, device=dev)
    b = torch.full((n, h, w), float('nan'), dtype=torch.float64, device=dev)
    T = torch.full((n, h, w), float('nan'), dtype=torch.float64, device=dev)
    lib = cpe.lib.load()
    st = torch.cuda.current_stream().cuda_stream
    cpe.lib.check(lib.cpe_preprocess_batch(g.data_ptr(), n, h, w, mp.data_ptr(), st), 'cpe_preprocess_batch')
    cpe.lib.check(lib.cpe_debug_preprocess(g.data_ptr(), n, h, w, md.data_ptr(), b.data_ptr(), T.data_ptr(), st),
                  'cpe_debug_preprocess')
    torch.cuda.synchronize()
    mp, md, b, T = (t.cpu().numpy() for t in (mp, md, b, T))
    return [dict(mask_prod=mp[i], mask=md[i], b=b[i], T=T[i]) for i in range(n)]


def check_shape(cpe, orc, dev, h, w, seed, kinds=None):
    """all frames of content(h, w) in one call; -> list of failure messages"""
    frames = content(h, w, seed, kinds)
    got = gpu_planes(cpe, dev, np.stack(list(frames.values())))
    fails = []
    for (name, f), g in zip(frames.items(), got):
        fails += [f'{h}x{w} {name}: {e[3]}' for e in plane_errors(f, g, oracle_planes(orc, f))]
    return fails


def _report(fails, cases):
    assert not fails, f'{len(fails)} failures over {cases} shapes:\n' + '\n'.join(fails[:30])


# ---------------------------------------------------------------- GPU cases
@pytest.mark.gpu
@pytest.mark.parametrize('heights', [range(8, 17), range(17, 25), range(39, 45)], ids=['h8-16', 'h17-24', 'h39-44'])
def test_small_shapes(cpe, orc, gpu, heights):
    """every height of the group against every width of WIDTHS, ten frames each"""
    fails = []
    for h in heights:
        for w in WIDTHS:
            fails += check_shape(cpe, orc, gpu, h, w, seed=1000 * h + w)
    _report(fails, len(heights) * len(WIDTHS))


@pytest.mark.gpu
@pytest.mark.parametrize('w', [1920, 1922])
def test_full_hd_heights(cpe, orc, gpu, w):
    """heights 1199 .. 1202 (every remainder of h / 4 at the bottom row block); at w = 1922 every strip takes the byte loads.
    A rendered frame per shape and one other kind, each kind once over the two widths."""
    others = ['noise', 'imp255', 'steps', 'ramp', 'checker', 'imp4', 'const128', 'const255']
    fails = []
    for i, h in enumerate(range(1199, 1203)):
        fails += check_shape(cpe, orc, gpu, h, w, seed=h + w, kinds=['synth', others[2 * i + (w == 1922)]])
    _report(fails, 4)


@pytest.mark.gpu
@pytest.mark.parametrize('h,w,kinds', [(2160, 3840, ['synth', 'imp255']), (8, 4096, None), (4096, 24, None)],
                         ids=['4k', '8x4096', '4096x24'])
def test_extreme_shapes(cpe, orc, gpu, h, w, kinds):
    _report(check_shape(cpe, orc, gpu, h, w, seed=7, kinds=kinds), 1)


@pytest.mark.gpu
@pytest.mark.parametrize('h,w', [(41, 512), (300, 1024)])
def test_unaligned_base(cpe, orc, gpu, h, w):
    """byte offsets 1, 2, 3 into a buffer with w % 4 == 0: the interior strips take the byte loads instead of the LDS-DMA
    form, and give the aligned call's planes and the oracle's"""
    frames = content(h, w, seed=h, kinds=['synth', 'noise', 'steps'])
    stack = np.stack(list(frames.values()))
    aligned = gpu_planes(cpe, gpu, stack)
    ref = [oracle_planes(orc, f) for f in stack]
    fails = [f'aligned {name}: {e[3]}' for name, f, g, r in zip(frames, stack, aligned, ref) for e in plane_errors(f, g, r)]
    for off in (1, 2, 3):
        for name, f, g, a, r in zip(frames, stack, gpu_planes(cpe, gpu, stack, offset=off), aligned, ref):
            fails += [f'offset {off} {name}: {e[3]}' for e in plane_errors(f, g, r)]
            fails += [f'offset {off} {name}: {e[3]} (against the aligned call)'
                      for e in (first_diff(k, g[k], a[k]) for k in ('mask_prod', 'mask', 'b', 'T')) if e]
    _report(fails, 4)


@pytest.mark.gpu
def test_batch_of_40(cpe, orc, gpu):
    """40 distinct frames in one call: each equals its own single-frame call and the oracle"""
    from cpe_amd import synth
    h, w = 72, 300
    r = synth.render_batch(16, h, w, seed=11, with_gt=False)
    frames = list(r['left'].numpy()) + list(r['right'].numpy())
    frames += list(content(h, w, seed=12, kinds=['noise', 'const0', 'imp4', 'imp255', 'steps', 'checker', 'ramp',
                                                 'const255']).values())
    stack = np.stack(frames)
    assert stack.shape[0] == 40 and len({f.tobytes() for f in frames}) == 40
    batch = gpu_planes(cpe, gpu, stack)
    fails = []
    for i, (f, g) in enumerate(zip(stack, batch)):
        fails += [f'frame {i}: {e[3]}' for e in plane_errors(f, g, oracle_planes(orc, f))]
        one = gpu_planes(cpe, gpu, f[None])[0]
        fails += [f'frame {i}: {e[3]} (against its single-frame call)'
                  for e in (first_diff(k, g[k], one[k]) for k in ('mask_prod', 'mask', 'b', 'T')) if e]
    _report(fails, 40)


@pytest.mark.gpu
def test_debug_bad_args(cpe, gpu):
    lib = cpe.lib.load()
    p = torch.zeros(64 * 64 * 8, dtype=torch.uint8, device=gpu).data_ptr()
    assert lib.cpe_debug_preprocess(p, 1, 64, 64, p, p, None, None) < 0
    assert b'null' in lib.cpe_last_error_string()
    assert lib.cpe_debug_preprocess(p, 1, 7, 64, p, p, p, None) < 0
    assert lib.cpe_debug_preprocess(p, 0, 64, 64, p, p, p, None) == 0


# ---------------------------------------------------------------- the helpers themselves (CPU)
def test_helpers_report_one_ulp(orc):
    """the comparison above catches what the mask cannot: one ulp of G at one pixel, or of b, or a lost outer Gaussian tap,
    leaves the mask as it is and is reported at its pixel"""
    h, w = 97, 300
    frame = content(h, w, seed=3, kinds=['synth'])['synth']
    ref = oracle_planes(orc, frame)
    assert plane_errors(frame, ref, ref) == []

    def planes_from_b(b):
        T = orc.sauvola_threshold(b)
        return dict(mask=orc.sauvola_mask(b), b=b, T=T)

    G = orc.gauss_sigma3(orc.blur5(frame))
    # one ulp of G at a strip seam: b differs from y0 - 2 on, the mask nowhere
    y0, x0 = 50, SW
    G1 = G.copy()
    G1[y0, x0] = np.nextafter(G1[y0, x0], np.inf)
    got = planes_from_b(orc.hessian_eigs(G1)[1])
    assert np.array_equal(got['mask'], ref['mask'])
    errs = {e[0]: e for e in plane_errors(frame, got, ref)}
    assert set(errs) == {'b', 'T'}, errs
    assert errs['b'][1] == y0 - 2 and abs(errs['b'][2] - x0) <= 2, errs['b']
    assert 'strip 0' in errs['b'][3] or 'strip 1' in errs['b'][3]
    # one ulp of b at one pixel: reported exactly there
    b1 = ref['b'].copy()
    b1[y0, x0 + 7] = np.nextafter(b1[y0, x0 + 7], -np.inf)
    got = dict(ref, b=b1)
    errs = {e[0]: e for e in plane_errors(frame, got, ref)}
    assert set(errs) == {'b'} and errs['b'][1:3] == (y0, x0 + 7), errs
    # a lost outer tap (the last 8 columns of G x (1 - 3e-5)): the mask keeps (almost) every byte, the independent
    # reference does not
    G2 = G.copy()
    G2[:, -8:] *= 1 - 3e-5
    got = planes_from_b(orc.hessian_eigs(G2)[1])
    assert (got['mask'] != ref['mask']).sum() <= 8
    errs = {e[0]: e for e in plane_errors(frame, got, ref)}
    assert 'b~scipy' in errs and errs['b~scipy'][2] >= w - 10, errs
    # T off by 1e-12 max|b| at one pixel: the long-double box reports it
    T1 = ref['T'].copy()
    T1[5, 9] += 1e-12 * np.abs(ref['b']).max()
    errs = {e[0]: e for e in plane_errors(frame, dict(ref, T=T1), ref)}
    assert set(errs) == {'T', 'T~longdouble'} and errs['T~longdouble'][1:3] == (5, 9), errs
