"""What a call computes never depends on what its workspace held on entry (include/cpe.h, "Workspaces").

Every entry that takes a workspace runs on a block that was prepared in one of these ways before the call under test:
    Z  zeros (the clean run: every other run must reproduce it bit for bit)
    A  the leftovers of a completed call on other frames with the same n and layout and the other target
    B  the leftovers of a call on five other frames, then the call under test on three frames inside the same block (the ragged
       last chunk of FramePipeline: another n is another plane-major layout); bytes at or beyond the size the call was given
       must keep what they held
    F  every byte 0xFF
    R  one row of the table 0xFF, the rest zero -- once per row of cpe_debug_workspace_buffer, the row's name is the test id
each with CPE_SERIAL=1 and with the helper streams.  The detect entries (grey and BGR, cylinder and plane, default, sub-pixel,
debug_planes=False) are held to the oracle by the checks of test_detect_gpu._compare / test_plane_gpu._compare and to run Z;
the line tables and the packed records to run Z byte for byte; the stage entries (one case batch of their own tests each) and
the workspaces of the geometric half (B / F and F) to run Z.  Only content the header defines is compared: rows of xy / id
below n_pts, the planes a frame's status defines (include/cpe.h, "Planes of a frame that ends early"), blur19 as `> 240`.

tests/test_workspace_poison_cpu.py shows that the rows cover the block and that the case frames reach their statuses.
The oracle's view of a frame is computed once per session; the file's 144 tests take 16.5 s on an MI355X.
No pattern, row or mode has changed a defined output so far: the library initialises what it reads.
The test can fail.  Tried once on a scratch build: without the hipMemsetAsync of the CLAHE histograms in clahe_front
(region.hip) -- a change of values only: k_clahe_lut clips and sums the 256 counts of a tile into saturated bytes, no count
is a loop bound or an address -- `test_one_row_poisoned[hist]` fails on the CLAHE plane of frame 0 and the rows beside it
(lut, nrect, best, best_spot) pass.  The reset of the largest-contour key in k_state_init was not tried: a stale key is not
only compared, k_hull_fill takes its low 24 bits as the pixel the border walk starts at, which for a 0xFF key lies outside
the frame."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import workspace_poison as P  # noqa: E402
import plane_colour_oracle as PC  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = ('serial', 'overlap')
U8_PLANES = ('binary', 'hmask', 'vmask', 'mask_contour', 'roi_h', 'roi_v', 'exp_h', 'exp_v', 'clahe', 'blur19', 'blur7')
# FrameState words a detect call defines for a frame, by how far the frame gets (the checks of test_detect_gpu._compare and
# test_execution_variants_give_identical_results)
STATE_ALWAYS = ('status', 'overflow')
STATE_REGION = ('rect0', 'rect1', 'rect2', 'rect3', 'n_kp', 'n_groups')
STATE_SPOT = ('r0', 'spot0', 'spot1', 'spot2', 'spot3', 'n_joints', 'n_joints_all')
STATE_LINES = ('n_rows', 'n_cols')


def _set_mode(monkeypatch, mode):
    if mode == 'serial':
        monkeypatch.setenv('CPE_SERIAL', '1')
    else:
        monkeypatch.delenv('CPE_SERIAL', raising=False)


# ---------------------------------------------------------------- detect: running, preparing the block, snapshots
def _frames_of(case, n=None):
    c = P.detect_case(case)
    return torch.from_numpy(c['frames'][:n] if n else c['frames'])


_OTHER = {}


def _other_frames(case, n):
    """n frames of the case's size and kind that the case does not hold (another scene)"""
    c = P.detect_case(case)
    h, w = c['frames'].shape[1:3]
    key = (h, w, c['frames'].ndim, n)
    if key not in _OTHER:
        g = P._stereo(h, w, 41)
        g = np.concatenate([g, P._stereo(h, w, 42), P._stereo(h, w, 43)])[:n]
        if c['frames'].ndim == 4:
            rng = np.random.default_rng(7)
            g = np.stack([PC.tint(f, rng) for f in g])
        _OTHER[key] = torch.from_numpy(g)
    return _OTHER[key]


_WS = {}


def _ws(gpu, h, w):
    """one block of five frames per frame size for the whole file (every test prepares all of it before its call)"""
    if (h, w) not in _WS:
        _WS.clear()                     # one size at a time: the blocks are hundreds of MB
        _WS[(h, w)] = P.workspace(5, h, w, gpu)
    return _WS[(h, w)]


def _prepare(cpe, gpu, ws, pattern, case, n, row=None):
    """the block before the call under test; -> for B, a copy of the bytes the call must not touch"""
    c = P.detect_case(case)
    other_target = 'plane' if c['target'] == 'cylinder' else 'cylinder'
    if pattern == 'Z':
        P.fill(ws, 0)
    elif pattern == 'F':
        P.fill(ws, 0xFF)
    elif pattern == 'R':
        P.fill_row(ws, n, row, 0xFF)
    elif pattern == 'A':
        P.fill(ws, 0)
        cpe.api.detect_grid_batch(_other_frames(case, n).to(gpu), ws, target=other_target)
    elif pattern == 'B':
        P.fill(ws, 0)
        cpe.api.detect_grid_batch(_other_frames(case, 5).to(gpu), ws, target=other_target)
        torch.cuda.synchronize()
        return P.full_view(ws)[P.total_bytes(n, ws.h, ws.w):].clone()
    else:
        raise KeyError(pattern)
    torch.cuda.synchronize()
    return None


def _line_bytes(cpe, det, i, target):
    rows, cols = cpe.api.line_tables(det, i, target=target)
    out = []
    for d in (rows, cols):
        out.append(repr(list(d['equations'])).encode())
        for k in d['equations']:
            out.append(np.asarray(d['equations'][k], np.float64).tobytes())
            out.append(np.asarray(d['points'][k], np.float64).tobytes())
    return np.frombuffer(b'|'.join(out), np.uint8)


def _snapshot(cpe, det, case, opts):
    """-> (defined, extra): flat dicts name -> numpy array of what the call left.  defined: what include/cpe.h defines for the
    frame's status and the call's options (asserted); extra: the rest of the public planes (printed by the measuring job only)"""
    c = P.detect_case(case)
    target, planar, colour = c['target'], c['target'] == 'plane', c['frames'].ndim == 4
    ws = det['ws']
    n = det['n'].shape[0]
    h, w = ws.h, ws.w
    D, X = {}, {}
    status = det['status'].cpu().numpy(); cnt = det['n'].cpu().numpy()
    D['status'] = status; D['n'] = cnt; D['center'] = det['center'].cpu().numpy().view(np.uint64)
    xy = det['xy'].cpu().numpy(); ids = det['id'].cpu().numpy()
    off, payload = cpe.api.pack_results(det)
    D['pack/offsets'] = off; D['pack/payload'] = payload
    declined = cpe.api.DEBUG_PLANES if ws.skipped_debug_planes else ()
    planes = {k: ws.plane(k).cpu().numpy() for k in U8_PLANES if k not in declined}
    joints = ws.plane('joints').cpu().numpy(); sweep = ws.plane('sweep').cpu().numpy(); raw = ws.plane('state').cpu().numpy()
    state = ws.state()
    for i in range(n):
        s = int(status[i]); st = state[i]
        tag = f'frame{i}(status{s})'
        D[f'xy/{tag}'] = xy[i, :cnt[i]].view(np.uint64); D[f'id/{tag}'] = ids[i, :cnt[i]]
        X[f'xy_past_n/{tag}'] = xy[i, cnt[i]:].view(np.uint64)
        D[f'lines/{tag}'] = _line_bytes(cpe, det, i, target)
        if s in (1, 2):                                    # ended in front of the lines stage: 0 / 0 lines, no points
            assert cnt[i] == 0 and D[f'lines/{tag}'].tobytes() == b'[]|[]', tag
        fields = STATE_ALWAYS + (STATE_REGION if s != 1 else ()) + (STATE_SPOT if s not in (1, 2) else ()) + (STATE_LINES if s in (0, 3) else ())
        D[f'state/{tag}'] = np.array([raw[i, cpe.api._STATE_FIELDS.index(k)] for k in fields if not (planar and k in ('n_kp', 'n_groups'))])
        X[f'state_raw/{tag}'] = raw[i]
        for k, p in planes.items():
            if k == 'blur19':
                D[f'{k}>240/{tag}'] = p[i] > 240
                X[f'{k}/{tag}'] = p[i]
            elif k == 'blur7':
                if s == 0:
                    wr = PC.blur7_written(h, w, (st['rect0'], st['rect1'], st['rect2'], st['rect3']), st['r0'])
                    D[f'{k}/written/{tag}'] = p[i][wr]
                X[f'{k}/{tag}'] = p[i]
            elif k == 'clahe':
                (X if planar and not colour else D)[f'{k}/{tag}'] = p[i]
            elif k in ('binary', 'hmask', 'vmask', 'mask_contour'):
                D[f'{k}/{tag}'] = p[i]                     # the chains in front of the join run for every frame
                assert k != 'mask_contour' or s != 1 or not p[i].any(), (tag, k, 'zero for a frame without region')
            else:                                          # roi_*, exp_*: "Planes of a frame that ends early"
                (D if s != 2 else X)[f'{k}/{tag}'] = p[i]
                assert s != 1 or not p[i].any(), (tag, k, 'zero for a frame without region')
        if s not in (1, 2):
            D[f'joints/{tag}'] = joints[i, :min(st['n_joints'], joints.shape[1])]
        if not planar:
            D[f'sweep/{tag}'] = sweep[i, 8:8 + 3 * 17]
        X[f'sweep_raw/{tag}'] = sweep[i]
    return D, X


def _diff(a, b):
    return [k for k in sorted(set(a) | set(b)) if k not in a or k not in b or a[k].shape != b[k].shape or not np.array_equal(a[k], b[k])]


OPTS = {'default': {}, 'subpixel': dict(subpixel=True), 'no_debug_planes': dict(debug_planes=False)}


def _call(cpe, orc, gpu, case, frames, ws, opts):
    """the call under test with the oracle's checks of its own test file -> its result"""
    import test_detect_gpu as TD
    import test_plane_gpu as TP
    from oracle import stages as S
    c = P.detect_case(case)
    keep = {}
    if frames.dim() == 4:
        det = cpe.api.detect_grid_batch(frames.to(gpu), ws, target=c['target'], **OPTS[opts])
        torch.cuda.synchronize()
        clahe = det['ws'].plane('clahe').cpu().numpy()
        for i, f in enumerate(frames.numpy()):           # the checks of test_boundary_gpu.py::test_true_colour_frames
            ref = _bgr_oracle(f)
            assert np.array_equal(clahe[i], ref['clahe']), i
            assert int(det['status'][i]) == ref['status'], i
            m = int(det['n'][i])
            assert m == len(ref['xy']) and np.array_equal(det['id'][i, :m].cpu().numpy(), ref['id']), i
            assert np.array_equal(det['xy'][i, :m].cpu().numpy(), ref['xy']) and np.array_equal(det['center'][i].cpu().numpy(), ref['center']), i
        return det
    if c['target'] == 'plane':
        TP._compare(cpe, orc, gpu, frames, ws=ws, keep=keep)
    else:
        TD._compare(cpe, orc, gpu, frames, ws=ws, keep=keep, **OPTS[opts])
    return keep['det']


_BGR = {}


def _bgr_oracle(f):
    from oracle import stages as S
    key = f.tobytes()
    if key not in _BGR:
        _BGR[key] = dict(S.detect_grid_bgr(f), clahe=S.clahe(S.lab_l_bgr(f)))
    return _BGR[key]


_Z = {}


def _clean(cpe, orc, gpu, case, n, opts):
    """run Z of (case, first n frames, options): once per session, in whatever mode comes first (the modes must agree with it)"""
    key = (case, n, opts)
    if key not in _Z:
        frames = _frames_of(case, n)
        ws = _ws(gpu, *frames.shape[1:3])
        _prepare(cpe, gpu, ws, 'Z', case, n)
        _Z[key] = _snapshot(cpe, _call(cpe, orc, gpu, case, frames, ws, opts), case, opts)
    return _Z[key]


def run_pattern(cpe, orc, gpu, case, pattern, opts='default', row=None):
    """one call under test on a prepared block, against the oracle and run Z; content the header leaves undefined that differs
    from run Z is printed, not asserted"""
    c = P.detect_case(case)
    n = 3 if pattern == 'B' else len(c['frames'])
    want, want_x = _clean(cpe, orc, gpu, case, n, opts)
    frames = _frames_of(case, n)
    ws = _ws(gpu, *frames.shape[1:3])
    kept = _prepare(cpe, gpu, ws, pattern, case, n, row)
    det = _call(cpe, orc, gpu, case, frames, ws, opts)
    got, got_x = _snapshot(cpe, det, case, opts)
    loose = _diff(got_x, want_x)
    if loose:
        print(case, pattern, opts, row, os.environ.get('CPE_SERIAL', '0'), 'undefined content that differs from run Z:', loose)
    bad = _diff(got, want)
    assert not bad, (case, pattern, opts, row, bad)
    if kept is not None:
        assert ws.bytes == P.total_bytes(n, ws.h, ws.w) < ws.capacity
        assert torch.equal(P.full_view(ws)[ws.bytes:], kept), (case, 'bytes at or beyond the size the call was given changed')


# ---------------------------------------------------------------- detect
CASE_OPTS = [(case, 'default') for case in P.DETECT_CASES] + [('grey480', 'subpixel'), ('grey480', 'no_debug_planes'),
                                                               ('grey483', 'subpixel'), ('grey483', 'no_debug_planes')]


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('pattern', ['A', 'B', 'F'])
@pytest.mark.parametrize('case,opts', CASE_OPTS)
def test_detect_on_a_used_block(cpe, orc, gpu, monkeypatch, case, opts, pattern, mode):
    _set_mode(monkeypatch, mode)
    run_pattern(cpe, orc, gpu, case, pattern, opts)


ROW_CASES = ('grey480', 'grey483', 'plane483', 'bgr480')      # word-level, byte-level, planar, colour


@pytest.mark.parametrize('row', P.row_names(64, 64))
def test_one_row_poisoned(cpe, orc, gpu, monkeypatch, row):
    for mode in MODES:
        _set_mode(monkeypatch, mode)
        for case in ROW_CASES:
            run_pattern(cpe, orc, gpu, case, 'R', row=row)


def test_every_row_of_the_library_is_a_parameter(cpe):
    assert P.row_names(64, 64) == P.row_names(483, 650) and len(P.row_names(64, 64)) >= 58


# ---------------------------------------------------------------- the stage entries
def _leftover(cpe, gpu, ws, seed=51):
    """a completed detect call on five rendered frames of the block's size"""
    P.fill(ws, 0)
    f = np.concatenate([P._stereo(ws.h, ws.w, seed), P._stereo(ws.h, ws.w, seed + 1), P._stereo(ws.h, ws.w, seed + 2)])[:5]
    cpe.api.detect_grid_batch(torch.from_numpy(f).to(gpu), ws)
    torch.cuda.synchronize()


def _stage(cpe, gpu, monkeypatch, h, w, run, same):
    """run(ws) -> result, on a zeroed block (Z), then under B and F in both modes; same(got, want, tag) asserts"""
    ws = P.workspace(5, h, w, gpu)
    P.fill(ws, 0)
    want = run(ws)
    for mode in MODES:
        _set_mode(monkeypatch, mode)
        for pattern in ('B', 'F'):
            if pattern == 'B':
                _leftover(cpe, gpu, ws)
            else:
                P.fill(ws, 0xFF)
            same(run(ws), want, (pattern, mode))


def _pad_to(a, H, W):
    return np.pad(a, ((0, H - a.shape[0]), (0, W - a.shape[1])))


@pytest.mark.parametrize('target', ['cylinder', 'plane'])
def test_stage_masks(cpe, orc, gpu, monkeypatch, target):
    import masks_cases as M
    import test_masks_stage_gpu as T
    H, W = 322, 330
    cases = [M.pad(M.get(k), H, W) for k in ('spot_tiles', 'r0_30', 'nested')]
    cases[2] = dict(cases[2], status=1)                        # a frame without a region between the others

    def same(got, want, tag):
        for i in range(3):
            T._same(got[i], want[i], (tag, i))
    _stage(cpe, gpu, monkeypatch, H, W, lambda ws: T._run(cpe, gpu, cases, target, ws=ws), same)


@pytest.mark.parametrize('names', [('groups_row_2_raster', 'status_1', 'one_col'), ('subpixel_corner_row_w7', 'subpixel_tiny_groups', 'subpixel_corner_col_w7')],
                         ids=['plain', 'subpixel'])
def test_stage_lines(cpe, orc, gpu, monkeypatch, names):
    import lines_cases as L
    import test_lines_stage_gpu as T
    cases = [T._padded(L.get(k), 320, 320) for k in names]

    def same(got, want, tag):
        for i in range(3):
            T._same(got[i], want[i], (tag, names[i]))
    _stage(cpe, gpu, monkeypatch, 320, 320, lambda ws: T._run(cpe, gpu, cases, ws=ws), same)


@pytest.mark.parametrize('mode_arg', [0, 1])
def test_stage_region_hull(cpe, orc, gpu, monkeypatch, mode_arg):
    import hull_cases as H
    import test_hull_stage_gpu as T
    shape = (200, 336)
    names = T.chunks_of(shape, mode_arg)[0][:2]
    imgs = np.stack([T.image_of(H.mask(names[0]), mode_arg), np.zeros(shape, np.uint8) if mode_arg == 0 else H.grey_of(H.blank(shape)),
                     T.image_of(H.mask(names[1]), mode_arg)])

    def same(got, want, tag):
        for i in range(3):
            T.same_frame(T.frame(got, i), T.frame(want, i), (tag, i))
    _stage(cpe, gpu, monkeypatch, *shape, lambda ws: T.run(gpu, imgs, mode_arg, ws), same)


def test_stage_blob_region(cpe, orc, gpu, monkeypatch):
    import test_blob_stage_gpu as T
    imgs = np.stack([T._image('small_holes'), T._image('bright_rings'), T._image('median_paths')])

    def same(got, want, tag):
        for i in range(3):
            T._same(T._frame(got, i), T._frame(want, i), (tag, i))
    _stage(cpe, gpu, monkeypatch, 481, 641, lambda ws: T._run(cpe, gpu, imgs, ws=ws), same)


@pytest.mark.parametrize('fused', [0, 1])
@pytest.mark.parametrize('size', [(320, 512), (317, 512)], ids=['320x512', '317x512'])
def test_stage_clahe_planes(cpe, orc, gpu, monkeypatch, size, fused):
    import clahe_cases as K
    import test_clahe_stage_gpu as T
    names = (K.names([size]) * 2)[:3]
    frames = np.stack([K.get(k)['gray'] for k in names])
    _stage(cpe, gpu, monkeypatch, *size, lambda ws: T._run(cpe, gpu, frames, fused, ws), lambda got, want, tag: T._same(got, want, str(tag)))


@pytest.mark.parametrize('path', [0, 1])
@pytest.mark.parametrize('h,w', [(300, 656), (130, 201)])
def test_stage_dark_labels(cpe, orc, gpu, monkeypatch, h, w, path):
    import test_dark_labels_gpu as T
    rng = np.random.default_rng(h * 7 + w)
    frames = T._frames(rng, 3, h, w)
    rects = [[0, 0, w - 1, h - 1], [33, 5, w - 41, h - 9], [64, 8, w - 2, h - 1]]

    def same(got, want, tag):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[3], want[3]), tag
        for i in range(3):                                     # the root list is a set: its order is the atomics'
            k = int(want[3][i])
            assert 0 < k <= T.MAXROOTS and np.array_equal(np.sort(got[2][i, :k]), np.sort(want[2][i, :k])), (tag, i)
    _stage(cpe, gpu, monkeypatch, h, w, lambda ws: T._run(cpe, gpu, frames, rects, path, ws=ws), same)


@pytest.mark.parametrize('h,w', [(96, 192), (130, 201)])
@pytest.mark.parametrize('thr,invert,conn8', [(128, 0, 1), (40, 1, 0)])
def test_stage_ccl(cpe, orc, gpu, monkeypatch, h, w, thr, invert, conn8):
    import test_ccl_gpu as T
    frames = T._masks(np.random.default_rng(h * 1000 + w + thr), 3, h, w)
    g = torch.from_numpy(frames).to(gpu)
    inside = (frames > thr) != bool(invert)

    def run(ws):
        ws.use(3)
        cpe.lib.check(cpe.lib.load().cpe_debug_ccl(g.data_ptr(), 3, h, w, thr, invert, conn8, 0, 0, 1, ws.view.data_ptr(), ws.bytes,
                                                  torch.cuda.current_stream().cuda_stream), 'cpe_debug_ccl')
        torch.cuda.synchronize()
        return ws.plane('labels').cpu().numpy()

    def same(got, want, tag):                                  # labels of the set, and -1 outside it (tests/test_ccl_gpu.py)
        assert np.array_equal(got[inside], want[inside]) and (got[~inside] == -1).all(), tag
    _stage(cpe, gpu, monkeypatch, h, w, run, same)


def test_stage_external_components(cpe, orc, gpu, monkeypatch):
    import test_ccl_gpu as T
    rng = np.random.default_rng(11)
    h, w = 97, 650
    frames = np.stack([((rng.random((h, w)) < 0.5) * 255).astype(np.uint8), T._nested_mask(rng, h, w, 30), T._nested_mask(rng, h, w, 12)])
    d = torch.from_numpy(frames).to(gpu)
    cap = 1 << 16

    def run(ws):
        ws.use(3)
        first = torch.full((3, cap), -1, dtype=torch.int32, device=gpu)
        cnt = torch.zeros(3, dtype=torch.int32, device=gpu)
        cpe.lib.check(cpe.lib.load().cpe_debug_external_components(d.data_ptr(), 3, h, w, ws.view.data_ptr(), ws.bytes, first.data_ptr(), cap,
                                                                  cnt.data_ptr(), torch.cuda.current_stream().cuda_stream), 'cpe_debug_external_components')
        torch.cuda.synchronize()
        return [sorted(first[i, :int(cnt[i])].cpu().tolist()) for i in range(3)]

    def same(got, want, tag):
        assert got == want and all(len(x) > 0 for x in want), tag
    _stage(cpe, gpu, monkeypatch, h, w, run, same)


# ---------------------------------------------------------------- the geometric half: blocks of our own
def _own_block(gpu, nbytes, value):
    buf = torch.empty(nbytes + 512, dtype=torch.uint8, device=gpu)
    buf.fill_(0x5A)
    at = (-buf.data_ptr()) % 256 + 256
    buf[at:at + nbytes].fill_(value)
    return buf, at


def _guards_intact(buf, at, nbytes):
    return bool((buf[:at] == 0x5A).all()) and bool((buf[at + nbytes:] == 0x5A).all())


@pytest.mark.parametrize('selector,th', [(0, 0.3), (1, 0.12), (2, 0.0)])
def test_fit_workspace_content_is_irrelevant(cpe, orc, gpu, selector, th):
    """cpe_select_triangulate_batch and cpe_choose_idx_batch on the selection cases of tests/test_fit_shapes_gpu.py"""
    import test_fit_shapes_gpu as T
    from cpe_amd import fit
    rig = T._rig()
    cases = T._sel_cases(rig)
    g1, g2 = T._table_batch([(t1, t2, c1, c2) for _, t1, t2, c1, c2, _ in cases], True)
    n = len(cases)
    L = cpe.lib.load()
    MAXP = fit.MAXP
    K1, K2, T21 = (fit._dev3(a, gpu, s) for a, s in zip(rig, ((9,), (9,), (16,))))
    nbytes = L.cpe_fit_workspace_bytes(n)
    assert nbytes > 0
    tabs = (g1.xy.data_ptr(), g1.id.data_ptr(), g1.cnt.data_ptr(), g2.xy.data_ptr(), g2.id.data_ptr(), g2.cnt.data_ptr(), n,
            K1.data_ptr(), K2.data_ptr(), T21.data_ptr())
    stream = torch.cuda.current_stream().cuda_stream
    results = []
    for value in (0, 0xFF):
        buf, at = _own_block(gpu, nbytes, value)
        o = dict(p1=torch.zeros((n, MAXP, 2), dtype=torch.float64, device=gpu), p2=torch.zeros((n, MAXP, 2), dtype=torch.float64, device=gpu),
                 idx=torch.zeros((n, MAXP, 2), dtype=torch.int32, device=gpu), X=torch.zeros((n, MAXP, 3), dtype=torch.float64, device=gpu),
                 err=torch.zeros((n, MAXP), dtype=torch.float64, device=gpu), m=torch.zeros(n, dtype=torch.int32, device=gpu),
                 me=torch.zeros(n, dtype=torch.float64, device=gpu), flags=torch.zeros(n, dtype=torch.int32, device=gpu))
        cpe.lib.check(L.cpe_select_triangulate_batch(*tabs, selector, 3, th, buf.data_ptr() + at, nbytes, o['p1'].data_ptr(), o['p2'].data_ptr(),
                                                     o['idx'].data_ptr(), o['X'].data_ptr(), o['err'].data_ptr(), o['m'].data_ptr(),
                                                     o['me'].data_ptr(), o['flags'].data_ptr(), stream), 'cpe_select_triangulate_batch')
        torch.cuda.synchronize()
        assert _guards_intact(buf, at, nbytes)
        out = {k: v.cpu().numpy() for k, v in o.items()}
        if selector == 0:
            buf, at = _own_block(gpu, nbytes, value)
            c = dict(p1=torch.zeros_like(o['p1']), p2=torch.zeros_like(o['p2']), idx=torch.zeros_like(o['idx']), m=torch.zeros_like(o['m']),
                     flags=torch.zeros_like(o['flags']))
            cpe.lib.check(L.cpe_choose_idx_batch(*tabs, 3, th, buf.data_ptr() + at, nbytes, c['p1'].data_ptr(), c['p2'].data_ptr(),
                                                 c['idx'].data_ptr(), c['m'].data_ptr(), c['flags'].data_ptr(), stream), 'cpe_choose_idx_batch')
            torch.cuda.synchronize()
            assert _guards_intact(buf, at, nbytes)
            out.update({'choose_' + k: v.cpu().numpy() for k, v in c.items()})
        results.append(out)
    zero, poisoned = results
    assert int(zero['m'].max()) > 1000
    for k in zero:          # the tables are zeroed by the test and written up to m: every byte of them is defined
        assert np.array_equal(zero[k].view(np.uint8), poisoned[k].view(np.uint8)), k


def test_match_offset_workspace_content_is_irrelevant(cpe, gpu):
    """cpe_match_offset_batch on the largest group of tests/match_offset_cases.py"""
    import match_offset_cases as M
    import test_match_offset_gpu as T
    from cpe_amd import fit
    group = max(T._groups(), key=len)
    n = len(group)
    prm_kw = group[0]['params']
    K1, K2, T21 = (fit._dev3(a, gpu, s) for a, s in zip(M.case_rig(group[0]), ((9,), (9,), (16,))))
    g1, g2 = T._tables(cpe, gpu, group)
    L = cpe.lib.load()
    kw = dict(dict(win_c=4, win_r=4, th=0.3, tau=0.5, hyp_iters=8, min_score=8), **prm_kw)
    prm = cpe.lib.CpeMatchParams(kw['win_c'], kw['win_r'], kw['th'], kw['tau'], kw['hyp_iters'], kw['min_score'])
    ncand = (2 * kw['win_c'] + 1) * (2 * kw['win_r'] + 1)
    nbytes = L.cpe_match_offset_workspace_bytes(n, kw['win_c'], kw['win_r'])
    assert nbytes > 0 and n >= 3
    results = []
    for value in (0, 0xFF):
        buf, at = _own_block(gpu, nbytes, value)
        o = dict(offset=torch.zeros((n, 2), dtype=torch.int32, device=gpu), score=torch.zeros((n, 4), dtype=torch.int32, device=gpu),
                 scores=torch.zeros((n, ncand), dtype=torch.int32, device=gpu), flags=torch.zeros(n, dtype=torch.int32, device=gpu),
                 id1=torch.zeros((n, M.MAXP, 2), dtype=torch.int32, device=gpu))
        cpe.lib.check(L.cpe_match_offset_batch(g1.xy.data_ptr(), g1.id.data_ptr(), g1.cnt.data_ptr(), g2.xy.data_ptr(), g2.id.data_ptr(),
                                               g2.cnt.data_ptr(), n, K1.data_ptr(), K2.data_ptr(), T21.data_ptr(), float(M.R), C.addressof(prm),
                                               buf.data_ptr() + at, nbytes, o['offset'].data_ptr(), o['score'].data_ptr(), o['scores'].data_ptr(),
                                               o['flags'].data_ptr(), o['id1'].data_ptr(), torch.cuda.current_stream().cuda_stream),
                      'cpe_match_offset_batch')
        torch.cuda.synchronize()
        assert _guards_intact(buf, at, nbytes)
        results.append({k: v.cpu().numpy() for k, v in o.items()})
    zero, poisoned = results
    refs = M.references()
    assert all(np.array_equal(zero['offset'][i], refs[c['name']]['offset']) for i, c in enumerate(group))
    for k in zero:
        assert np.array_equal(zero[k], poisoned[k]), k
