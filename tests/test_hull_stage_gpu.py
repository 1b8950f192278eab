"""The hull stage on its own (cpe_debug_region_hull, include/cpe.h) against the oracle, with tolerance 0: largest external
contour -> convex hull -> filled polygon -> boundingRect, as k_region_area, k_hull_fill and k_hull_rows (csrc/region.hip) make
them behind region_hull -- the host function both region stages of the product end in -- and, in mode 1, twice with
k_dilate_ellipse in between (region_stage_plane).

Per case (tests/hull_cases.py; tests/test_hull_generators_cpu.py proves what each one reaches) and mode:
  - status, overflow == 0, rect and hull_n;
  - the vertex set equal to stages.convex_hull of the contour the oracle chooses, and the list the kernel leaves in the
    workspace row `hull` in the same cyclic order, up to rotation and direction;
  - mask_contour byte for byte.
The mode-0 reference is what the oracle's largest_hull_mask(need_positive = 1) composes (hull_cases.largest_hull); the mode-1
reference is stages.get_convex_hull(grey, 127, 5) for status, mask and rect, and the same composition for the vertices.

The cases of one frame size go through calls of at most CHUNK frames (a frame takes 92 MiB of workspace at the least) with an
empty frame in the middle, forward and reversed on ONE workspace, and every case alone on another: all three must agree to the
byte and to the order of the vertices, so nothing of one frame or one call (best, hull_n, mask_contour) reaches the next.
Every one-component case runs again with an isolated pixel far away (`+px`): n_roots = 2 sends k_hull_fill to the border
tracer and k_region_area past its one-component shortcut, and the answer must be the one without the pixel.

Three branches of the kernels that no valid mask reaches, and why:
  - k_hull_fill, nv > HULL_LDS_W - 1 (OVF_VERTS), and k_hull_rows, nh > HR_MAXV (vertices read from HBM instead of LDS): a
    convex lattice polygon in an N x N box has O(N^(2/3)) vertices.  The largest count any generator here reaches is 540 (the
    digital disc of radius 2040 in 4096 x 4096; 340 for radius 1020 in 2048 x 2048, the widest frame of the LDS path), under
    HR_MAXV = 1024 and HULL_LDS_W - 1 = 2047 (tests/test_hull_generators_cpu.py::test_vertex_maximum);
  - k_hull_fill, m == 1 (one column, one pixel): a component inside one column has a contour of area 0, so it is never
    chosen -- unless it is a mask's only component in mode 0, which that mode's precondition excludes -- and the second planar
    round sees a set at least 11 columns wide.
A region rectangle one row high is out of reach for the same reason (hull_cases.py)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hull_cases as H  # noqa: E402
from bitplane_util import decode_plane, plane_words, workspace_row  # noqa: E402

CHUNK = 32


def union_of(m):
    """the mode-0 input: non-zero = set, the set pixels running through 1 .. 255"""
    y, x = np.ogrid[:m.shape[0], :m.shape[1]]
    return np.where(m, 1 + (5 * x + y) % 255, 0).astype(np.uint8)


def image_of(m, mode):
    return union_of(m) if mode == 0 else H.grey_of(m)


_REF = {}


def ref_of(name, mode):
    """the oracle's answer for a case, computed once"""
    if (name, mode) not in _REF:
        from oracle import stages as S
        m = H.mask(name)
        r = H.reference(m, mode)
        if mode == 1:
            st, mk, rect = S.get_convex_hull(H.grey_of(m), 127, 5)
            assert st == r['status'] and np.array_equal(mk, r['mask']) and (st != 0 or rect == r['rect']), name
        _REF[(name, mode)] = dict(status=r['status'], mask=r['mask'], rect=r['rect'], hull=r['hull'])
    return _REF[(name, mode)]


def same_cycle(a, b):
    """two vertex lists equal as cycles, up to rotation and direction"""
    a, b = np.asarray(a).reshape(-1, 2), np.asarray(b).reshape(-1, 2)
    if len(a) != len(b):
        return False
    if len(a) == 0:
        return True
    at = np.nonzero((b == a[0]).all(1))[0]
    if len(at) != 1:
        return False
    return np.array_equal(np.roll(b, -at[0], 0), a) or np.array_equal(np.roll(b[::-1], -(len(b) - 1 - at[0]), 0), a)


def run(gpu, imgs, mode, ws=None):
    from cpe_amd import api
    return api.debug_region_hull(torch.from_numpy(np.ascontiguousarray(imgs)).to(gpu), mode, ws)


def frame(res, i):
    st = res['state'][i]
    return dict(status=st['status'], overflow=st['overflow'], hull_n=st['hull_n'], n_roots=st['n_roots'],
                rect=(st['rect0'], st['rect1'], st['rect2'], st['rect3']), hull=res['hull'][i], mask=res['mask'][i])


def check(got, ref, tag):
    """one frame against the oracle, tolerance 0"""
    print(tag, 'status', got['status'], ref['status'], 'overflow', got['overflow'], 'rect', got['rect'], ref['rect'], 'hull_n', got['hull_n'],
          len(ref['hull']), 'mask pixels that differ', int((got['mask'] != ref['mask']).sum()))
    assert got['overflow'] == 0, tag
    assert got['status'] == ref['status'], (tag, got['status'], ref['status'])
    if ref['status'] == 0:
        assert got['rect'] == ref['rect'], (tag, got['rect'], ref['rect'])
        assert got['hull_n'] == len(ref['hull']), (tag, got['hull_n'], len(ref['hull']))
        assert {tuple(v) for v in got['hull'].tolist()} == {tuple(v) for v in ref['hull'].tolist()}, (tag, 'vertex set')
        assert same_cycle(got['hull'], ref['hull']), (tag, 'vertex order', got['hull'].tolist(), ref['hull'].tolist())
    else:
        assert got['hull_n'] == 0, tag
    assert np.array_equal(got['mask'], ref['mask']), (tag, 'mask_contour', int((got['mask'] != ref['mask']).sum()))


def same_frame(a, b, tag):
    """two runs of one case: identical, the order of the vertices included"""
    assert (a['status'], a['overflow'], a['hull_n']) == (b['status'], b['overflow'], b['hull_n']), tag
    if a['status'] == 0:
        assert a['rect'] == b['rect'], tag
    assert np.array_equal(a['hull'], b['hull']), (tag, 'vertices')
    assert np.array_equal(a['mask'], b['mask']), (tag, 'mask_contour')


def chunks_of(shape, mode):
    names = [k for k in H.names_of(shape) if mode == 1 or H.MODE0[k]]
    return [names[i:i + CHUNK] for i in range(0, len(names), CHUNK)]


BATCHED = [s for s in H.SHAPES if s != H.HUGE]
PARAMS = [pytest.param(s, k, mode, id=f'{s[0]}x{s[1]}-{k}-mode{mode}') for s in BATCHED for mode in (0, 1) for k in range(len(chunks_of(s, mode)))]


@pytest.mark.gpu
@pytest.mark.parametrize('shape,k,mode', PARAMS)
def test_hull_stage_matches_oracle(cpe, orc, gpu, shape, k, mode):
    from cpe_amd import api
    names = chunks_of(shape, mode)[k]
    imgs = [image_of(H.mask(nm), mode) for nm in names]
    mid = len(imgs) // 2
    empty = np.zeros(shape, np.uint8) if mode == 0 else H.grey_of(H.blank(shape))
    imgs.insert(mid, empty); names = names[:mid] + ['(empty)'] + names[mid:]
    n = len(imgs)
    ws = api.DetectWorkspace(n, shape[0], shape[1], gpu)
    fwd = run(gpu, np.stack(imgs), mode, ws)
    fwd = [frame(fwd, i) for i in range(n)]
    rev = run(gpu, np.stack(imgs[::-1]), mode, ws)        # the same workspace: frame f now holds what frame n - 1 - f held
    rev = [frame(rev, n - 1 - i) for i in range(n)]
    one = api.DetectWorkspace(1, shape[0], shape[1], gpu)
    for i, nm in enumerate(names):
        tag = (shape, mode, nm)
        if nm == '(empty)':
            assert fwd[i]['status'] == 1 and fwd[i]['overflow'] == 0 and fwd[i]['hull_n'] == 0 and not fwd[i]['mask'].any(), tag
        else:
            check(fwd[i], ref_of(nm, mode), tag)
        same_frame(fwd[i], rev[i], (tag, 'reversed batch'))
        same_frame(fwd[i], frame(run(gpu, imgs[i][None], mode, one), 0), (tag, 'alone'))
        # the labelling finds the components the generator test counts: one component takes the bit-plane column scan and
        # k_region_area's shortcut, more take the border tracer (mode 1 ends on its second round: one dilated component, or none)
        comps = H.claims(nm).get('comps') if nm != '(empty)' else 0
        if comps is not None:
            assert fwd[i]['n_roots'] == (comps if mode == 0 else 1 - fwd[i]['status']), (tag, fwd[i]['n_roots'], comps)
    # the isolated pixel changes nothing: the tracer's column extents are the bit plane's
    for i, nm in enumerate(names):
        base = H.claims(nm).get('same_as') if nm != '(empty)' else None
        if base in names:
            same_frame(fwd[i], fwd[names.index(base)], ((shape, mode, nm), 'with and without the far pixel'))
        elif base:
            check(fwd[i], ref_of(base, mode), ((shape, mode, nm), 'against the oracle of the mask without the far pixel'))


@pytest.mark.gpu
@pytest.mark.parametrize('mode', [0, 1])
def test_hull_stage_largest_frame(cpe, orc, gpu, mode):
    """the digital disc of radius 2040 in 4096 x 4096, one frame, once: the serial chain of the wide frames with the most
    vertices it can get"""
    got = frame(run(gpu, image_of(H.mask('disc_2040'), mode)[None], mode), 0)
    check(got, ref_of('disc_2040', mode), ('disc_2040', mode))
    assert got['hull_n'] >= 480


@pytest.mark.gpu
@pytest.mark.parametrize('mode', [0, 1])
def test_same_vertices_either_side_of_the_lds_width(cpe, orc, gpu, mode):
    """the same shape at the same offset in a 2048 and a 2064 wide frame: the LDS path and the serial chain list the same
    vertices (each is compared with the oracle in test_hull_stage_matches_oracle)"""
    for nm in H.SAME_2048_2064:
        a = frame(run(gpu, image_of(H.mask(nm + '_w2048'), mode)[None], mode), 0)
        b = frame(run(gpu, image_of(H.mask(nm + '_w2064'), mode)[None], mode), 0)
        assert a['status'] == b['status'] == 0 and a['rect'] == b['rect'] and a['hull_n'] == b['hull_n'] > 0, (nm, mode)
        assert same_cycle(a['hull'], b['hull']) and {tuple(v) for v in a['hull'].tolist()} == {tuple(v) for v in b['hull'].tolist()}, (nm, mode)
        assert np.array_equal(a['mask'], b['mask'][:, :2048]) and not b['mask'][:, 2048:].any(), (nm, mode)


@pytest.mark.gpu
def test_more_components_than_the_root_list_holds(cpe, orc, gpu):
    """1026 x 1024 isolated pixels are more than MAXROOTS components: OVF_ROOTS in the state, never a silently truncated answer"""
    m = H.isolated_pixels()
    assert int(m.sum()) > H.MAXROOTS
    for mode in (0, 1):
        got = frame(run(gpu, image_of(m, mode)[None], mode), 0)
        assert got['overflow'] & H.OVF_ROOTS, (mode, got['overflow'])
        assert not got['mask'].any() and got['hull_n'] == 0, mode


@pytest.mark.gpu
def test_matches_detect_path_cylinder(cpe, orc, gpu):
    """the entry fed a detect call's own disc union reproduces that call's rect and mask_contour.  The masks stage reuses the
    one-bit planes, so the union is taken as tests/test_disc_union_bits_gpu.py takes it: the region stage alone
    (cpe_debug_blob_region, identity table) on the call's CLAHE plane, stopped before anything writes over the row `bits`"""
    from cpe_amd import api, synth
    b = synth.render_batch(2, 480, 640, seed=0, with_gt=False)
    frames = torch.cat([b['left'], b['right']])
    n, h, w = frames.shape
    det = api.detect_grid_batch(frames.to(gpu))
    torch.cuda.synchronize()
    state, mc = det['ws'].state(), det['ws'].plane('mask_contour').cpu().numpy()
    cl = det['ws'].plane('clahe').clone()
    L = cpe.lib.load()
    ws = api.DetectWorkspace(n, h, w, gpu)
    cap = 1024
    kp = torch.zeros((n, cap, 3), dtype=torch.float32, device=gpu)
    nkp = torch.zeros(n, dtype=torch.int32, device=gpu)
    bl = torch.zeros((n, 17, 64, 3), dtype=torch.float64, device=gpu)
    nbl = torch.zeros((n, 17), dtype=torch.int32, device=gpu)
    cpe.lib.check(L.cpe_debug_blob_region(cl.data_ptr(), n, h, w, ws.view.data_ptr(), ws.bytes, kp.data_ptr(), cap, nkp.data_ptr(),
                                          bl.data_ptr(), 64, nbl.data_ptr(), torch.cuda.current_stream().cuda_stream),
                  'cpe_debug_blob_region')
    torch.cuda.synchronize()
    off, _ = workspace_row(L, n, h, w, 'bits')
    pw = plane_words(h, w)
    planes = ws.view[off:off + n * pw * 8].cpu().numpy().view('<u8').reshape(n, pw)
    unions = []
    for f in range(n):
        u, clean = decode_plane(planes[f], h, w)
        assert clean and u.any(), f
        unions.append(union_of(u))
    got = run(gpu, np.stack(unions), 0)
    for f in range(n):
        g = frame(got, f)
        print('frame', f, 'rect', g['rect'], 'hull_n', g['hull_n'], state[f]['hull_n'], 'n_roots', g['n_roots'])
        assert g['status'] == 0 and g['overflow'] == 0, f
        assert g['rect'] == (state[f]['rect0'], state[f]['rect1'], state[f]['rect2'], state[f]['rect3']), f
        assert mc[f].any() and np.array_equal(g['mask'], mc[f]), f


@pytest.mark.gpu
def test_matches_detect_path_plane(cpe, orc, gpu):
    """the entry in mode 1 on the grey frames of a planar detect call reproduces that call's rect and mask_contour"""
    from cpe_amd import synth
    sc = synth.Scene(h=483, w=650, radius=5000.0, depth=(5340.0, 5400.0), tilt_deg=4.0)
    b = synth.render_batch(1, 483, 650, seed=9, scene=sc, with_gt=False)
    frames = torch.cat([b['left'], b['right']])
    det = cpe.api.detect_grid_batch(frames.to(gpu), target='plane')
    torch.cuda.synchronize()
    state, mc = det['ws'].state(), det['ws'].plane('mask_contour').cpu().numpy()
    got = run(gpu, frames.numpy(), 1)
    for f in range(frames.shape[0]):
        g = frame(got, f)
        assert g['status'] == 0 and g['overflow'] == 0, f
        assert g['rect'] == (state[f]['rect0'], state[f]['rect1'], state[f]['rect2'], state[f]['rect3']), f
        assert mc[f].any() and np.array_equal(g['mask'], mc[f]), f
