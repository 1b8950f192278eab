"""CPU: LAB-L and CLAHE(4.5, 4 x 4) of the oracle against a second statement, and the generators of tests/clahe_cases.py against
the rules they are named for -- so that a passing tests/test_clahe_stage_gpu.py means something.

* `np_clahe`: cv2.createCLAHE(4.5, (4, 4)).apply restated in numpy (reflect padding, bincount, clip and redistribute, f32
  cumulative table with rint, f32 bilinear weights, (a + b) * ya1 + (c + d) * ya with every product and sum rounded to f32)
  equals `stages.clahe` on every case, tolerance 0.
* every rule of that statement is reached: for each mutant of MUTANTS a named case changes at least one pixel.
* the residual tiles have the residual and the step they are built for, computed from the case's own histograms.
* `stages.lab_l` / `stages.lab_l_bgr` (the tables the kernels copy) against the CIE formula in float64 on all 256 greys and
  all 2^24 colours: |dL| <= 0.95 DN / <= 1.6 DN (measured, deterministic: 0.912 / 1.549), monotone in every channel, and
  R = G = B gives the grey table."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clahe_cases as K  # noqa: E402

f32 = np.float32


def _half_up(x):
    return np.floor(x.astype(np.float64) + 0.5)


def np_clahe(src, clip=4.5, mut=None, lab=None):
    """CLAHE(clip, 4 x 4) of a u8 plane.  mut: one deliberate mistake (MUTANTS).  lab (only with the two merge mutants): the
    plane is LAB-L[src] and the table is built from the grey histogram of src."""
    src = np.ascontiguousarray(src, np.uint8)
    h, w = src.shape
    plane = src if lab is None else lab[src]
    eh, ew = h, w
    if h % 4 or w % 4:
        eh, ew = h + 4 - h % 4, w + 4 - w % 4
        if mut == 'ew_w' and w % 4 == 0:
            ew = w
    mode = 'edge' if mut == 'replicate' else 'reflect'
    pad = lambda p: np.pad(p, ((0, eh - h), (0, ew - w)), mode=mode)
    th, tw = eh // 4, ew // 4
    total = th * tw
    x = clip * total / 256
    limit = max(int(np.floor(x + 0.5)) if mut == 'clip_round' else int(x), 1)
    scale = f32(255) / f32(total)

    def hists(p):
        t = pad(p).reshape(4, th, 4, tw).transpose(0, 2, 1, 3).reshape(16, -1)
        return np.stack([np.bincount(r, minlength=256) for r in t]).astype(np.int64)

    def merged(hg):      # counts of grey values -> counts of L values
        out = np.zeros_like(hg)
        for v in range(256):
            out[:, lab[v]] += hg[:, v]
        return out

    hist = hists(src if mut in ('merge_after_clip', 'no_merge') else plane)     # the two merge mutants count grey values
    lut = np.zeros((16, 256), np.uint8)
    for t in range(16):
        hh = hist[t].copy()
        over = hh > limit
        clipped = int((hh[over] - limit).sum())
        hh[over] = limit
        if mut == 'merge_after_clip':
            hh = merged(hh[None])[0]
        batch, residual = divmod(clipped, 256)
        hh += batch
        if residual:
            step = max(256 // residual, 1)
            idx = np.arange(residual) if mut == 'first_r' else np.arange(0, 256, step)[:residual]
            hh[idx] += 1
        v = np.cumsum(hh).astype(f32) * scale
        lut[t] = np.clip(_half_up(v) if mut == 'lut_half_up' else np.rint(v), 0, 255).astype(np.uint8)
    if mut == 'no_merge':    # the table of the grey histogram, looked up with grey values
        plane = src
    lut = lut.reshape(4, 4, 256)

    def axis(nn, t):
        i = np.arange(nn, dtype=np.int64).astype(f32)
        f = (i / f32(t) if mut == 'div' else i * (f32(1) / f32(t))) - f32(0.5)
        t1 = np.floor(f)
        a = f - t1
        t1 = t1.astype(np.int64)
        return np.clip(t1, 0, 3), np.clip(t1 + 1, 0, 3), a.astype(f32), (f32(1) - a).astype(f32)

    ty1, ty2, ya, ya1 = axis(h, th)
    tx1, tx2, xa, xa1 = axis(w, tw)
    out = np.empty((h, w), np.uint8)
    rows = max(1, (1 << 21) // w)
    for y0 in range(0, h, rows):
        y1 = min(h, y0 + rows)
        v = plane[y0:y1]
        r1, r2 = ty1[y0:y1, None], ty2[y0:y1, None]
        a = lut[r1, tx1[None], v].astype(f32) * xa1[None]
        b = lut[r1, tx2[None], v].astype(f32) * xa[None]
        c = lut[r2, tx1[None], v].astype(f32) * xa1[None]
        d = lut[r2, tx2[None], v].astype(f32) * xa[None]
        ab, cd = a + b, c + d
        if mut == 'fma':     # the first product not rounded on its own
            res = (ab.astype(np.float64) * ya1[y0:y1, None].astype(np.float64) + (cd * ya[y0:y1, None]).astype(np.float64)).astype(f32)
        else:
            res = ab * ya1[y0:y1, None] + cd * ya[y0:y1, None]
        assert res.dtype == f32
        out[y0:y1] = np.clip(_half_up(res) if mut == 'half_up' else np.rint(res), 0, 255).astype(np.uint8)
    return out


# mutant -> the named case that must notice it (the smallest that does)
MUTANTS = {
    'half_up': 'patchA_64x64',            # half-up instead of half-even in the interpolation
    'lut_half_up': 'resid_72x80',         # half-up in the table (a tile of 256 or 289 pixels has no sum that rounds to a tie)
    'first_r': 'resid_64x64',             # residual added to the first r bins instead of every step-th
    'div': 'patchB_72x80',                # x / tw instead of x * (1.0f / tw)
    'fma': 'patchB_72x80',                # a fused multiply-add in res
    'replicate': 'patchB_65x67',          # replicate instead of reflect-101 padding
    'ew_w': 'patchA_66x64',               # ew = w when only h % 4 != 0
    'clip_round': 'resid_64x64',          # clip limit rounded instead of truncated
    'merge_after_clip': 'patchA_64x64',   # bins merged by LAB-L after clipping ...
    'no_merge': 'patchA_64x64',           # ... or not at all
}


@pytest.mark.parametrize('name', list(K.CASES))
def test_numpy_statement_equals_oracle(orc, name):
    r = K.ref(name)
    assert np.array_equal(np_clahe(r['L']), r['cl'])


@pytest.mark.parametrize('name', K.COLOUR_CASES)
def test_numpy_statement_equals_oracle_colour(orc, name):
    """the colour versions: CLAHE of an L plane with all 256 values, and the L plane is not LAB-L of the luma"""
    from oracle import stages as S
    for variant in range(3):
        r = K.ref(name, variant)
        assert np.array_equal(np_clahe(r['L']), r['cl'])
        assert (r['L'] != S.lab_l(S.bgr2gray(r['bgr']))).mean() > 0.2


@pytest.mark.parametrize('mut', list(MUTANTS))
def test_mutant_is_noticed(orc, mut):
    name = MUTANTS[mut]
    r = K.ref(name)
    merge = mut in ('merge_after_clip', 'no_merge')
    got = np_clahe(K.get(name)['gray'], mut=mut, lab=K.lab_table()) if merge else np_clahe(r['L'], mut=mut)
    diff = int((got != r['cl']).sum())
    print(f'{mut}: {diff} of {got.size} pixels differ on {name}')
    assert diff > 0, f'no pixel of {name} notices the mutant {mut}'
    if merge:     # the statement itself, from grey values: merged before clipping
        assert np.array_equal(np_clahe(K.lab_table()[K.get(name)['gray']]), r['cl'])


def test_mutants_reach_the_fused_pass_sizes(orc):
    """the rounding and weight rules are also reached at the sizes only k_clahe_apply64 serves"""
    for mut, name in (('half_up', 'patchA_512x512'), ('half_up', 'patchA_320x512'), ('div', 'patchA_317x512'), ('div', 'patchB_328x528'),
                      ('fma', 'patchA_320x512'), ('fma', 'patchA_317x512'), ('fma', 'patchB_328x528'), ('replicate', 'patchB_317x512'),
                      ('ew_w', 'patchB_317x512'), ('first_r', 'resid_320x512'), ('first_r', 'resid_512x512'),
                      ('lut_half_up', 'patchB_320x512'), ('lut_half_up', 'patchB_317x512'), ('lut_half_up', 'patchB_328x528')):
        r = K.ref(name)
        assert (np_clahe(r['L'], mut=mut) != r['cl']).any(), (mut, name)


@pytest.mark.parametrize('name', [n for n in K.CASES if n.startswith('resid')])
def test_residual_tiles(orc, name):
    """every tile has the residual and the step it is built for; the small frames together hold every residual of RESIDUALS"""
    c = K.get(name)
    G = K.geom(*c['gray'].shape)
    hl = K.tile_hists(K.ref(name)['L'])
    steps = {0: 0, 1: 256, 2: 128, 85: 3, 86: 2, 127: 2, 128: 2, 129: 1, 255: 1}
    for t in range(16):
        ex, r, step = K.residual_of(hl[t], G['clip'])
        assert r == c['resid'][t] and step == steps[r], (t, ex, r, step, c['resid'][t])
        assert hl[t].max() <= G['clip'] or ex > 0


def test_residuals_covered(orc):
    """each size without padding holds each residual (64 x 64: all but 255 -- a tile of 256 pixels with clip limit 4 cannot
    clip more than 252), in more than one pixel order"""
    for h, w in K.SMALL + K.MID:
        if h % 4 or w % 4:
            continue
        seen = {}
        for n in (f'resid_{h}x{w}', f'resid2_{h}x{w}'):
            c = K.get(n)
            for (_, order), r in zip(c['tiles'], c['resid']):
                seen.setdefault(r, set()).add(order)
        want = set(K.RESIDUALS) - ({255} if (h, w) == (64, 64) else set())
        assert set(seen) >= want, (h, w, sorted(seen))
        if (h, w) != (64, 64):
            assert len(seen[255]) >= 1
    assert {o for n in K.names(K.SMALL) for _, o in K.get(n)['tiles']} >= set(K.ORDERS)


def test_fill_tile_orders():
    cnt = np.zeros(256, np.int64); cnt[[0, 7, 200]] = [300, 500, 224]
    for order in K.ORDERS:
        t = K.fill_tile(cnt, 32, 32, order, 3)
        assert np.array_equal(np.bincount(t.ravel(), minlength=256), cnt)
    assert K.fill_tile(cnt, 32, 32, 'first0', 3)[0, 0] == 0 and K.fill_tile(cnt, 32, 32, 'first_nz', 3)[0, 0] != 0
    assert K.fill_tile(cnt, 32, 32, 'sorted', 3)[0, 0] == 0 and K.fill_tile(cnt, 32, 32, 'sorted_desc', 3)[0, 0] == 200
    s = K.fill_tile(cnt, 32, 32, 'sorted', 3).ravel()
    assert (np.diff(s.astype(int)) != 0).sum() == 2              # three runs, each longer than a row and than 256 pixels
    sh = K.fill_tile(cnt, 32, 32, 'shuffled', 3).ravel()
    assert (np.diff(sh.astype(int)) != 0).sum() > 500


def test_pairs_tiles_share_l(orc):
    """the 'pairs' tiles hold grey values that share an L value, each at or below the clip limit and together above it"""
    lab = K.lab_table()
    assert lab[75] == lab[76] == 82
    c = K.get('patchA_64x64')
    G = K.geom(64, 64)
    t = [k for k, (kind, _) in enumerate(c['tiles']) if kind == 'pairs'][0]
    ty, tx = divmod(t, 4)
    hg = np.bincount(c['gray'][ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16].ravel(), minlength=256)
    assert 0 < hg[75] <= G['clip'] and 0 < hg[76] <= G['clip'] and hg[75] + hg[76] > G['clip']
    assert 0 < hg[77] <= G['clip'] and lab[77] != lab[78]


def test_geometry_of_the_sizes():
    """the sizes reach the paths they are listed for"""
    g = {s: K.geom(*s) for s in K.sizes()}
    assert (g[(64, 64)]['tw'], g[(64, 64)]['clip']) == (16, 4)
    assert [g[s]['tw'] for s in ((68, 68), (64, 72), (72, 80))] == [17, 18, 20]
    assert (g[(66, 64)]['ew'], g[(66, 64)]['eh']) == (68, 68) and (g[(64, 66)]['ew'], g[(64, 66)]['eh']) == (68, 68)
    ok64 = lambda s: s[1] % 16 == 0 and g[s]['tw'] >= 128 and g[s]['th'] >= 80
    assert ok64((320, 512)) and not ok64((316, 512)) and not ok64((320, 496))
    assert ok64((317, 512)) and (g[(317, 512)]['tw'], g[(317, 512)]['th']) == (129, 80)
    assert ok64((328, 528)) and 528 % 64 == 16 and 328 % 64 != 0
    assert ok64((512, 512)) and g[(512, 512)]['tw'] == 128
    assert ok64((1200, 1920)) and ok64((4096, 4096)) and not ok64((64, 4096)) and not ok64((4096, 64))


# ---------------------------------------------------------------- the tables against the CIE formula
def _cie_l(b, g, r):
    """L* x 2.55 of sRGB values 0 .. 255 in float64"""
    def lin(c):
        c = c / 255.0
        return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)
    y = 0.212671 * lin(r) + 0.715160 * lin(g) + 0.072169 * lin(b)
    fy = np.where(y > 0.008856, np.cbrt(y), 7.787 * y + 16.0 / 116.0)
    return (116.0 * fy - 16.0) * 2.55


def test_lab_l_grey_table(orc):
    from oracle import stages as S
    v = np.arange(256, dtype=np.uint8)
    L = S.lab_l(v[None])[0].astype(np.float64)
    err = np.abs(L - _cie_l(v.astype(np.float64), v.astype(np.float64), v.astype(np.float64))).max()
    print(f'grey table: max |dL| = {err:.4f} DN')
    assert err <= 0.95
    assert (np.diff(L) >= 0).all()
    assert np.array_equal(S.lab_l_bgr(np.repeat(v[None, :, None], 3, 2))[0], S.lab_l(v[None])[0])


def test_lab_l_colour_table_all_colours(orc):
    from oracle import stages as S
    g, r = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing='ij')
    gf, rf = g.astype(np.float64), r.astype(np.float64)
    worst = 0.0
    prev = None
    cube = np.empty((256, 256, 256), np.uint8)       # [b, g, r]
    for b in range(256):
        bgr = np.stack([np.full_like(g, b), g, r], 2)
        L = S.lab_l_bgr(bgr)
        cube[b] = L
        worst = max(worst, float(np.abs(L - _cie_l(np.float64(b), gf, rf)).max()))
    print(f'colour table: max |dL| = {worst:.4f} DN')
    assert worst <= 1.6
    c = cube.astype(np.int16)
    assert (np.diff(c, axis=0) >= 0).all() and (np.diff(c, axis=1) >= 0).all() and (np.diff(c, axis=2) >= 0).all()
    v = np.arange(256)
    assert np.array_equal(cube[v, v, v], S.lab_l(v.astype(np.uint8)[None])[0])
