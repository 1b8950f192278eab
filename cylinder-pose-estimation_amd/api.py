"""Python face of the image half of the hot path.

`detect_grid_batch` is the MI355X-native form of python_grid_detection_cylinder.py::detect_grid
(:68-112): all frames of a batch go through the HIP kernels behind the C ABI (include/cpe.h) and come
back as padded point tables; `detect_grid(input_img)` keeps the reference's single-image signature and
return shape, `make_json` its JSON (util_cylinder.py:1674-1727, decoded by makePyGridPts.m:39-41), `save_mat`
writes the structs the MATLAB side holds after makePyGridPts / fitSingleCylinder.
There is no CPU fallback: without a GPU and libcpe_hip.so these raise."""
import collections
import ctypes as C
import functools
import json
import threading

import numpy as np
import torch

from . import lib as _lib
from .fit import GridTables, MAXP

_c = _lib.const
PLANES = _lib.const_group('PLANE_')       # 'binary', 'hmask', ..., 'sweep': the CPE_PLANE_* numbers
TARGETS = _lib.TARGETS                    # 'cylinder', 'plane': CPE_TARGET_*
# debug outputs that no stage reads where rows are a multiple of 16 pixels: undefined after detect_grid_batch(debug_planes=False)
DEBUG_PLANES = ('hmask', 'vmask', 'roi_h', 'roi_v')
STATUS_TEXT = {_c.ST_OK: 'ok', _c.ST_NO_REGION: 'no region (cv2.convexHull(None))',
               _c.ST_NO_SPOT: 'no saturated spot (circle_radius0 unbound)', _c.ST_NO_LINES: 'no valid rows/cols',
               _c.ST_EMPTY: 'empty point list', _c.ST_FEW_POINTS: 'too few points', _c.ST_OVERFLOW: 'workspace capacity exceeded',
               _c.ST_SUBPIXEL_RAISED: 'sub-pixel refinement raised (line sample above / left of the image)'}


@functools.lru_cache(maxsize=None)
def state_fields():
    """((name, is_float), ...) of the 32-bit words of the per-frame state record, as the library lists its fields
    (cpe_debug_state_field); an array field `rect` of 4 words gives rect0 .. rect3"""
    L = _lib.load()
    name = C.create_string_buffer(64)
    words, is_float = C.c_int32(), C.c_int32()
    out, k = [], 0
    while L.cpe_debug_state_field(k, name, len(name), C.byref(words), C.byref(is_float)) == 0:
        base = name.value.decode()
        out += [(base if words.value == 1 else f'{base}{i}', bool(is_float.value)) for i in range(words.value)]
        k += 1
    return tuple(out)


def __getattr__(name):
    """api._STATE_FIELDS, the list of names the tests index the state words by: the same listing, made on first use"""
    if name == '_STATE_FIELDS':
        return [k for k, _ in state_fields()]
    raise AttributeError(f'module {__name__!r} has no attribute {name!r}')


class DetectWorkspace:
    """device scratch for cpe_detect_grid_batch, reusable across calls with the same frame size and up to n frames (a
    smaller batch, e.g. the ragged last chunk of a run, is laid out inside the same buffer)"""

    def __init__(self, n, h, w, device):
        self.n, self.h, self.w = n, h, w
        self.capacity_n = n
        L = _lib.load()
        self.bytes = L.cpe_detect_workspace_bytes(n, h, w)
        self.capacity = self.bytes
        self.buf = torch.empty(self.bytes + 256, dtype=torch.uint8, device=device)
        off = (-self.buf.data_ptr()) % 256
        self.view = self.buf[off:off + self.bytes]
        self.skipped_debug_planes = False       # the last call left DEBUG_PLANES unwritten

    def fits(self, n, h, w):
        return (h, w) == (self.h, self.w) and n <= self.capacity_n and \
            _lib.load().cpe_detect_workspace_bytes(n, h, w) <= self.capacity

    def use(self, n):
        """lay the buffer out for a batch of n frames (n <= the n it was made for).  Every use is a new generation of the
        buffer's contents: a result dict remembers the generation it was made in, and the functions that read
        intermediates through it (line_tables, frame_result) refuse a workspace that has served another call since."""
        if n != self.n:
            self.n = n
            self.bytes = _lib.load().cpe_detect_workspace_bytes(n, self.h, self.w)
        self.generation = getattr(self, 'generation', 0) + 1
        return self

    def plane(self, name):
        """intermediate of the last call: u8 [n,h,w] planes, i32 [n,CPE_MAXJ,2] joints, or the state records"""
        if self.skipped_debug_planes and name in DEBUG_PLANES:
            raise RuntimeError(f'plane({name!r}): the last call ran with debug_planes=False and did not write it')
        L = _lib.load()
        off = C.c_size_t(); per = C.c_size_t()
        _lib.check(L.cpe_detect_workspace_plane(self.n, self.h, self.w, PLANES[name], C.byref(off), C.byref(per)),
                   'cpe_detect_workspace_plane')
        raw = self.view[off.value:off.value + per.value * self.n]
        if name == 'joints':
            return raw.view(torch.int32).reshape(self.n, -1, 2)
        if name == 'labels':
            return raw.view(torch.int32).reshape(self.n, self.h, self.w)
        if name in ('state', 'sweep'):
            return raw.view(torch.int32).reshape(self.n, -1)
        return raw.reshape(self.n, self.h, self.w)

    def state(self):
        """list of dicts (one per frame) of the per-frame state record"""
        arr = self.plane('state').cpu().numpy()
        return [{name: float(np.int32(v).view(np.float32)) if is_float else int(v) for (name, is_float), v in zip(state_fields(), row)}
                for row in arr]


def _output_tables(n, dev):
    return dict(xy=torch.zeros((n, MAXP, 2), dtype=torch.float64, device=dev), id=torch.zeros((n, MAXP, 2), dtype=torch.int32, device=dev),
                n=torch.zeros(n, dtype=torch.int32, device=dev), center=torch.zeros((n, 2), dtype=torch.float64, device=dev),
                status=torch.zeros(n, dtype=torch.int32, device=dev))


def detect_grid_batch(frames, ws=None, subpixel=False, subpixel_window=7, subpixel_step=1.0, target='cylinder', out=None,
                      debug_planes=True):
    """frames: u8 tensor [n,h,w] (grey) or [n,h,w,3] (BGR, as cv2.imread delivers) on the GPU -> dict(xy f64[n,MAXP,2],
    id i32[n,MAXP,2], n i32[n], center f64[n,2], status i32[n], ws).  target='plane': the planar-target script
    (python_grid_detection_plane.py, row f-2); ids are (row, col) there.
    out: the tables of an earlier call with the same n on the same device, written again instead of five new zeroed tensors
    (the earlier result changes with them, and rows of xy / id past n[k] keep what they held).
    debug_planes=False: a caller that only wants the tables declines the planes DEBUG_PLANES (CPE_DETECT_SKIP_DEBUG_PLANES):
    where the width is a multiple of 16 they are not written and ws.plane() refuses them; other widths write them anyway."""
    if not (isinstance(frames, torch.Tensor) and frames.is_cuda and frames.dtype == torch.uint8 and
            (frames.dim() == 3 or (frames.dim() == 4 and frames.shape[3] == 3))):
        raise TypeError('frames must be a CUDA uint8 tensor [n,h,w] (grey) or [n,h,w,3] (BGR)')
    frames = frames.contiguous()
    colour = frames.dim() == 4
    if colour and subpixel:
        frames = bgr_to_gray(frames); colour = False       # the sub-pixel stage: luma only
    n, h, w = frames.shape[:3]
    dev = frames.device
    L = _lib.load()
    if ws is None or not ws.fits(n, h, w) or ws.view.device != dev:
        ws = DetectWorkspace(n, h, w, dev)
    ws.use(n)
    if out is None:
        out = _output_tables(n, dev)
    elif out['n'].shape[0] != n or out['n'].device != dev:
        raise ValueError('detect_grid_batch: `out` holds the tables of another batch size or device')
    xy, ids, cnt, center, status = out['xy'], out['id'], out['n'], out['center'], out['status']
    prm = _lib.CpeDetectParams(1 if subpixel else 0, subpixel_window, subpixel_step, TARGETS[target],
                               0 if debug_planes else _lib.DETECT_SKIP_DEBUG_PLANES)
    ws.skipped_debug_planes = False         # (set once the call has gone through)
    entry = L.cpe_detect_grid_bgr_batch_ex if colour else L.cpe_detect_grid_batch_ex
    _lib.check(entry(frames.data_ptr(), n, h, w, C.addressof(prm), ws.view.data_ptr(), ws.bytes,
                     xy.data_ptr(), ids.data_ptr(), cnt.data_ptr(), center.data_ptr(),
                     status.data_ptr(), torch.cuda.current_stream().cuda_stream),
               'cpe_detect_grid_bgr_batch_ex' if colour else 'cpe_detect_grid_batch_ex')
    ws.skipped_debug_planes = not debug_planes and w % 16 == 0
    return dict(xy=xy, id=ids, n=cnt, center=center, status=status, ws=ws, ws_generation=ws.generation)


def debug_masks(binary, gray, mask_contour, rect, region_status, ws=None, target='cylinder'):
    """the masks stage alone on given inputs (cpe_debug_masks, a test aid): binary, gray, mask_contour u8 [n,h,w], rect i32
    [n,4] (x, y, w, h), region_status i32 [n] (0 or 1), all CUDA tensors on one device; mask_contour must be zero outside rect.
    -> the workspace, whose plane() and state() read as after detect_grid_batch"""
    ins = [binary, gray, mask_contour]
    if not all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.dim() == 3 and t.shape == binary.shape
               for t in ins):
        raise TypeError('binary, gray and mask_contour must be CUDA uint8 tensors [n,h,w] of one shape')
    n, h, w = binary.shape
    dev = binary.device
    ins = [t.contiguous() for t in ins]
    rect = rect.to(dev, torch.int32).contiguous().reshape(n, 4)
    region_status = region_status.to(dev, torch.int32).contiguous().reshape(n)
    if ws is None or not ws.fits(n, h, w) or ws.view.device != dev:
        ws = DetectWorkspace(n, h, w, dev)
    ws.use(n)
    ws.skipped_debug_planes = False
    _lib.check(_lib.load().cpe_debug_masks(ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), rect.data_ptr(),
                                           region_status.data_ptr(), n, h, w, TARGETS[target], ws.view.data_ptr(), ws.bytes,
                                           torch.cuda.current_stream().cuda_stream), 'cpe_debug_masks')
    return ws


def debug_lines(exp_h, exp_v, joints, n_joints, rect, r0, stage_status, g7, gray=None, ws=None, subpixel=False, subpixel_window=7,
                subpixel_step=1.0, target='cylinder'):
    """the lines stage alone on given inputs (cpe_debug_lines, a test aid): exp_h, exp_v, g7, gray u8 [n,h,w] CUDA tensors
    (gray: default g7), joints i32 [n,k,2] (k <= CPE_MAXJ; padded to the table), n_joints, r0, stage_status i32 [n], rect i32
    [n,4] (x, y, w, h).  -> what detect_grid_batch returns (tables, ws, ws_generation): line_tables, pack_results and
    ws.state() read it as they read a detect result"""
    gray = g7 if gray is None else gray
    ins = [exp_h, exp_v, g7, gray]
    if not all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.dim() == 3 and t.shape == exp_h.shape
               for t in ins):
        raise TypeError('exp_h, exp_v, g7 and gray must be CUDA uint8 tensors [n,h,w] of one shape')
    n, h, w = exp_h.shape
    dev = exp_h.device
    ins = [t.contiguous() for t in ins]
    maxj = _lib.detect_constants()['max_joints']
    joints = joints.to(dev, torch.int32).reshape(n, -1, 2)
    if joints.shape[1] > maxj:
        raise ValueError(f'debug_lines: more than CPE_MAXJ = {maxj} joints per frame')
    table = torch.zeros((n, maxj, 2), dtype=torch.int32, device=dev)
    table[:, :joints.shape[1]] = joints
    i32 = lambda t, shape: t.to(dev, torch.int32).contiguous().reshape(shape)
    n_joints, r0, stage_status, rect = i32(n_joints, n), i32(r0, n), i32(stage_status, n), i32(rect, (n, 4))
    if ws is None or not ws.fits(n, h, w) or ws.view.device != dev:
        ws = DetectWorkspace(n, h, w, dev)
    ws.use(n)
    ws.skipped_debug_planes = False
    out = _output_tables(n, dev)
    prm = _lib.CpeDetectParams(1 if subpixel else 0, subpixel_window, subpixel_step, TARGETS[target], 0)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().cpe_debug_lines(ins[0].data_ptr(), ins[1].data_ptr(), table.data_ptr(), n_joints.data_ptr(),
                                               rect.data_ptr(), r0.data_ptr(), stage_status.data_ptr(), ins[2].data_ptr(),
                                               ins[3].data_ptr(), n, h, w, C.addressof(prm), ws.view.data_ptr(), ws.bytes,
                                               out['xy'].data_ptr(), out['id'].data_ptr(), out['n'].data_ptr(),
                                               out['center'].data_ptr(), out['status'].data_ptr(),
                                               torch.cuda.current_stream().cuda_stream), 'cpe_debug_lines')
    return dict(out, ws=ws, ws_generation=ws.generation)


def workspace_row(n, h, w, name):
    """(offset, bytes per frame) of a named row of the workspace table of an (n, h, w) call (cpe_debug_workspace_buffer)"""
    L = _lib.load()
    buf = C.create_string_buffer(64)
    off, per = C.c_size_t(), C.c_size_t()
    ov, side, pub = C.c_int32(), C.c_int32(), C.c_int32()
    k = 0
    while L.cpe_debug_workspace_buffer(n, h, w, k, buf, 64, C.byref(off), C.byref(per), C.byref(ov), C.byref(side), C.byref(pub)) == 0:
        if buf.value.decode() == name:
            return off.value, per.value
        k += 1
    raise KeyError(name)


def debug_region_hull(imgs, mode, ws=None):
    """the hull stage alone (cpe_debug_region_hull, a test aid): imgs u8 [n,h,w] CUDA tensor; mode 0: disc-union images
    (non-zero = set), the cylinder target's tail; mode 1: grey frames, the planar target's region stage.
    -> dict(state: list of per-frame dicts, mask: u8 [n,h,w] numpy (mask_contour), hull: list of i32 (hull_n, 2) numpy (x, y)
    in the order the kernel lists them, ws)"""
    if not (isinstance(imgs, torch.Tensor) and imgs.is_cuda and imgs.dtype == torch.uint8 and imgs.dim() == 3):
        raise TypeError('imgs must be a CUDA uint8 tensor [n,h,w]')
    imgs = imgs.contiguous()
    n, h, w = imgs.shape
    dev = imgs.device
    if ws is None or not ws.fits(n, h, w) or ws.view.device != dev:
        ws = DetectWorkspace(n, h, w, dev)
    ws.use(n)
    ws.skipped_debug_planes = False
    with torch.cuda.device(dev):
        _lib.check(_lib.load().cpe_debug_region_hull(imgs.data_ptr(), n, h, w, int(mode), ws.view.data_ptr(), ws.bytes,
                                                     torch.cuda.current_stream().cuda_stream), 'cpe_debug_region_hull')
        torch.cuda.synchronize(dev)
    state = ws.state()
    off, per = workspace_row(n, h, w, 'hull')
    rows = ws.view[off:off + per * n].view(torch.int32).reshape(n, -1)
    hull = [rows[f, :2 * max(state[f]['hull_n'], 0)].cpu().numpy().reshape(-1, 2) for f in range(n)]
    return dict(state=state, mask=ws.plane('mask_contour').cpu().numpy(), hull=hull, ws=ws)


def tables_of(det):
    """detect_grid_batch output -> GridTables (the N x 4 [x y col row] matrices of makePyGridPts.m:41)"""
    return GridTables(det['xy'], det['id'], det['n'])


def make_json(center, xy, ids):
    """the JSON string make_json returns (util_cylinder.py:1674-1727): indent 4, keys id/x/y in this order"""
    pts = [{"id": [int(c), int(r)], "x": float(x), "y": float(y)} for (x, y), (c, r) in zip(xy, ids)]
    return json.dumps({"center_point": [float(center[0]), float(center[1])], "points": pts}, indent=4, ensure_ascii=False)


def bgr_to_gray(bgr):
    """u8 tensor [n,h,w,3] (BGR, interleaved) on the GPU -> u8 [n,h,w]: cv2.cvtColor(BGR2GRAY) of
    load_and_preprocess_image (util_cylinder.py:1781-1789), cpe_bgr2gray_batch"""
    if not (isinstance(bgr, torch.Tensor) and bgr.is_cuda and bgr.dtype == torch.uint8 and bgr.dim() == 4 and bgr.shape[3] == 3):
        raise TypeError('bgr must be a CUDA uint8 tensor [n,h,w,3]')
    bgr = bgr.contiguous()
    n, h, w, _ = bgr.shape
    gray = torch.empty((n, h, w), dtype=torch.uint8, device=bgr.device)
    with torch.cuda.device(bgr.device):
        _lib.check(_lib.load().cpe_bgr2gray_batch(bgr.data_ptr(), n, h, w, gray.data_ptr(), torch.cuda.current_stream().cuda_stream),
                   'cpe_bgr2gray_batch')
    return gray


def frames_to_device(images, device='cuda:0'):
    """list of numpy u8 images of one size, each H x W (grey) or H x W x 3 (BGR as cv2.imread gives it) -> u8 tensor on the
    device: [n,h,w] if every image is grey, else [n,h,w,3] (grey images replicated into the three channels: the colour path
    makes of a grey-replicated frame exactly what the grey path makes of the plane)."""
    arrs = [np.asarray(a) for a in images]
    for a in arrs:
        if a.dtype != np.uint8:
            raise TypeError('detect_grid expects uint8 images')
        if not (a.ndim == 2 or (a.ndim == 3 and a.shape[2] == 3)):
            raise ValueError(f'Unexpected input dimensions: {a.ndim}')        # util_cylinder.py:1788
    if all(a.ndim == 2 for a in arrs):
        return torch.from_numpy(np.stack(arrs)).to(device)
    return torch.from_numpy(np.stack([np.ascontiguousarray(a) if a.ndim == 3 else np.repeat(a[..., None], 3, 2) for a in arrs])).to(device)


def line_tables(det, frame, target='cylinder'):
    """rows_updated, cols_updated of one frame of a detect_grid_batch result: the third and fourth return values of the
    reference's detect_grid (built by find_and_assign_intersections_P + clean_and_relabel, util_cylinder.py:1106-1206):
    {'points': {'row1': [(x, y), ...], ...}, 'equations': {'row1': [a2, a1, a0, lo, hi, span], ...}}"""
    ws = det['ws']
    if det.get('ws_generation', ws.generation) != ws.generation:
        raise RuntimeError('line_tables: the workspace of this result has served another detect call since (its line tables are '
                           'gone); read them before the next call or give every result its own DetectWorkspace')
    dev = det['xy'].device
    ML = _lib.MAXL
    eq = torch.empty((2, ML, 6), dtype=torch.float64, device=dev)
    npts = torch.empty((2, ML), dtype=torch.int32, device=dev)
    pts = torch.empty((2, ML, ML, 2), dtype=torch.float64, device=dev)
    nl = torch.empty(2, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().cpe_detect_line_tables(ws.view.data_ptr(), ws.bytes, ws.n, ws.h, ws.w, int(frame), eq.data_ptr(),
                                                      npts.data_ptr(), pts.data_ptr(), nl.data_ptr(),
                                                      torch.cuda.current_stream().cuda_stream), 'cpe_detect_line_tables')
    eq, npts, pts, nl = eq.cpu().numpy(), npts.cpu().numpy(), pts.cpu().numpy(), nl.cpu().numpy()
    out = []
    for sd, prefix in ((0, 'row'), (1, 'col')):
        d = {'points': {}, 'equations': {}}
        for g in range(int(nl[sd])):
            d['points'][f'{prefix}{g + 1}'] = [(float(x), float(y)) for x, y in pts[sd, g, :npts[sd, g]]]
            d['equations'][f'{prefix}{g + 1}'] = [float(v) for v in eq[sd, g]]
        out.append(d)
    return out[0], out[1]


FrameRecord = collections.namedtuple('FrameRecord', 'status n center xy id rows cols')
FrameRecord.__doc__ = """one frame of unpack_results: status (int, CPE_ST_*), n (int), center f64[2], xy f64[n,2], id i32[n,2] (numpy arrays
that own their data), rows / cols: the dicts line_tables returns"""

_REC_HEAD = 48


def record_bytes(n_pts, n_lines, n_line_pts):
    """bytes of one packed record (include/cpe.h, "Packed results")"""
    return _REC_HEAD + 24 * n_pts + 48 * n_lines + 8 * ((n_lines + 2) // 2) + 16 * n_line_pts


def unpack_results(offsets, payload, target='cylinder'):
    """offsets int64[n+1], payload uint8[>= offsets[n]] as cpe_detect_results_sizes / cpe_detect_results_pack wrote them (numpy,
    on the host) -> list of n FrameRecord.  Pure: needs neither the GPU nor the library.  The record layout is the one of
    include/cpe.h; ids are stored as the detector made them ((col, row), planar target: (row, col)), so `target` only
    has to name a known target.  Raises ValueError on offsets that are not increasing multiples of 8 from 0, on a payload
    shorter than offsets[n], and on a record whose counts do not give exactly its size."""
    if target not in TARGETS:
        raise ValueError(f'unpack_results: unknown target {target!r}')
    off = np.asarray(offsets)
    buf = np.asarray(payload)
    if off.ndim != 1 or off.size < 1 or off.dtype != np.int64:
        raise ValueError('unpack_results: offsets must be an int64 vector of n + 1 entries')
    if buf.ndim != 1 or buf.dtype != np.uint8:
        raise ValueError('unpack_results: payload must be a uint8 vector')
    if off[0] != 0 or np.any(off & 7) or np.any(np.diff(off) <= 0):
        raise ValueError('unpack_results: offsets must start at 0, be multiples of 8 and increase')
    if buf.size < int(off[-1]):
        raise ValueError(f'unpack_results: payload of {buf.size} bytes is shorter than offsets[n] = {int(off[-1])} '
                         '(records that did not fit were not written)')
    raw = np.ascontiguousarray(buf[:int(off[-1])]).tobytes()        # one copy: what is returned owns its data
    out = []
    for k in range(off.size - 1):
        at, end = int(off[k]), int(off[k + 1])
        if end - at < _REC_HEAD + 8:
            raise ValueError(f'unpack_results: record {k} is shorter than an empty record')
        status, m, nr, nc, npr, npc, z0, z1 = np.frombuffer(raw, '<i4', 8, at).tolist()
        nl, npt = nr + nc, npr + npc
        if min(m, nr, nc, npr, npc) < 0 or z0 or z1 or record_bytes(m, nl, npt) != end - at:
            raise ValueError(f'unpack_results: record {k}: counts {(m, nr, nc, npr, npc)} do not fill its {end - at} bytes')
        center = np.frombuffer(raw, '<f8', 2, at + 32).copy()
        p = at + _REC_HEAD
        xy = np.frombuffer(raw, '<f8', 2 * m, p).reshape(m, 2).copy(); p += 16 * m
        ids = np.frombuffer(raw, '<i4', 2 * m, p).reshape(m, 2).copy(); p += 8 * m
        eq = np.frombuffer(raw, '<f8', 6 * nl, p).reshape(nl, 6).tolist(); p += 48 * nl
        nst = 2 * ((nl + 2) // 2)
        start = np.frombuffer(raw, '<i4', nst, p).tolist(); p += 4 * nst
        if start[0] != 0 or start[nr] != npr or start[nl] != npt or any(b < a for a, b in zip(start[:nl], start[1:nl + 1])) or \
                any(start[nl + 1:]):
            raise ValueError(f'unpack_results: record {k}: the start table does not match the counts')
        pts = list(map(tuple, np.frombuffer(raw, '<f8', 2 * npt, p).reshape(npt, 2).tolist()))
        tables = []
        for first, cnt, prefix in ((0, nr, 'row'), (nr, nc, 'col')):
            d = {'points': {}, 'equations': {}}
            for g in range(cnt):
                d['points'][f'{prefix}{g + 1}'] = pts[start[first + g]:start[first + g + 1]]
                d['equations'][f'{prefix}{g + 1}'] = eq[first + g]
            tables.append(d)
        out.append(FrameRecord(status, m, center, xy, ids, tables[0], tables[1]))
    return out


def pack_results(det):
    """the packed records of all frames of a detect_grid_batch result, on the host: (offsets int64[n+1], payload uint8[offsets[n]])
    as include/cpe.h lays them out.  Two kernels (cpe_detect_results_sizes / _pack); the host reads the n + 1 offsets -- the
    only way to size the payload -- then the payload: two copies per batch whatever n is.  Like line_tables it refuses a
    workspace that has served another call."""
    ws = det['ws']
    if det.get('ws_generation', ws.generation) != ws.generation:
        raise RuntimeError('pack_results: the workspace of this result has served another detect call since (its line tables are '
                           'gone); read them before the next call or give every result its own DetectWorkspace')
    dev = det['xy'].device
    n = det['n'].shape[0]
    L = _lib.load()
    offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(L.cpe_detect_results_sizes(ws.view.data_ptr(), ws.bytes, ws.n, ws.h, ws.w, det['n'].data_ptr(), det['status'].data_ptr(),
                                              offsets.data_ptr(), stream), 'cpe_detect_results_sizes')
        off = offsets.cpu().numpy()
        payload = torch.empty(int(off[-1]), dtype=torch.uint8, device=dev)
        _lib.check(L.cpe_detect_results_pack(ws.view.data_ptr(), ws.bytes, ws.n, ws.h, ws.w, det['xy'].data_ptr(), det['id'].data_ptr(),
                                             det['n'].data_ptr(), det['center'].data_ptr(), det['status'].data_ptr(),
                                             offsets.data_ptr(), payload.data_ptr(), payload.numel(), stream), 'cpe_detect_results_pack')
        return off, payload.cpu().numpy()


def batch_results(det, target='cylinder'):
    """everything detect_grid returns beside the picture, for all frames of a detect_grid_batch result: list of FrameRecord
    (status, n, center, xy, id as in det; rows / cols as line_tables(det, k) gives them) = unpack_results(*pack_results(det))"""
    if target not in TARGETS:
        raise ValueError(f'batch_results: unknown target {target!r}')
    return unpack_results(*pack_results(det), target)


def draw_points(gray, xy):
    """the returned picture: BGR copy of the frame with the grid points marked (deterministic; the reference draws random
    colours, util_cylinder.py:1600-1601)"""
    g = np.asarray(gray)
    col_img = g.copy() if g.ndim == 3 else np.repeat(g[..., None], 3, axis=2)
    for (x, y) in xy:
        xi, yi = int(x), int(y)
        col_img[max(yi - 2, 0):yi + 3, max(xi - 2, 0):xi + 3] = (0, 255, 0)
    return col_img


def frame_result(det, k, gray, target='cylinder', results=None):
    """the 4-tuple detect_grid returns for frame k of a batch result, or None (after printing why) for a failed frame.
    results: batch_results(det, target), fetched once by a caller that loops over the frames of a detect call (run_folder,
    detect_grid); without it the frame's status is read and, for a good frame, the batch is fetched for this one call --
    nothing is kept in `det`."""
    st = int(det['status'][k]) if results is None else results[k].status
    if st != 0:
        print(f'Error in detect_grid: {STATUS_TEXT.get(st, st)}')
        return None
    r = (batch_results(det, target) if results is None else results)[k]
    return draw_points(gray, r.xy), make_json(r.center, r.xy, r.id), r.rows, r.cols


# detect_grid(input_img) is called once per image (makePyGridPts.m:29): its workspace and output tables are kept between
# calls, one set per (device, h, w, colour).  Bounded: the _SINGLE_MAX most recently used sets stay on the device
# (cpe_detect_workspace_bytes(1, h, w): 98 MiB at 640 x 480, 162 MiB at 1920 x 1200, 556 MiB at 3840 x 2160, plus 48 KiB
# of tables), until release_detect_grid_cache(); calls are serialised by _single_lock, so two threads never share a set
# in flight.
_SINGLE_MAX = 4
_single_sets = collections.OrderedDict()
_single_lock = threading.Lock()


def release_detect_grid_cache():
    """drop the workspaces and output tables detect_grid keeps between calls (the next call makes its own again)"""
    with _single_lock:
        _single_sets.clear()


def detect_grid(input_img, device='cuda:0', target='cylinder'):
    """detect_grid(input_img) -> (col_img, result_json, rows_updated, cols_updated)
    (python_grid_detection_cylinder.py:68-110; target='plane': python_grid_detection_plane.py:74-119, whose ids are
    (row, col)).  On a per-frame failure prints and returns None (:111-112).  What is returned owns its data: a later
    call does not change it."""
    img = np.asarray(input_img)
    frames = frames_to_device([img], device)
    key = (str(frames.device), frames.shape[1], frames.shape[2], frames.dim() == 4)
    with _single_lock:
        held = _single_sets.pop(key, None)              # a call that raises leaves its set out of the cache
        if held is None:
            held = (DetectWorkspace(1, frames.shape[1], frames.shape[2], frames.device), _output_tables(1, frames.device))
        det = detect_grid_batch(frames, held[0], target=target, out=held[1])
        results = batch_results(det, target)
        _single_sets[key] = held
        while len(_single_sets) > _SINGLE_MAX:
            _single_sets.popitem(last=False)
    return frame_result(det, 0, img, target, results)


def grid_struct(det, k, results=None):
    """gridPts of makePyGridPts.m:39-41 for frame k: center_point (2 x 1), points (N x 4 = [x y colIdx rowIdx]).
    results: batch_results(det) if the caller has it (no copies then); without it the frame's three tables are copied"""
    if results is not None:
        r = results[k]
        return dict(center_point=r.center.copy().reshape(2, 1), points=np.concatenate([r.xy, r.id.astype(np.float64)], 1).reshape(-1, 4))
    m = int(det['n'][k])
    xy = det['xy'][k, :m].cpu().numpy(); ids = det['id'][k, :m].cpu().numpy().astype(np.float64)
    return dict(center_point=det['center'][k].cpu().numpy().reshape(2, 1), points=np.concatenate([xy, ids], 1).reshape(-1, 4))


def save_mat(path, grid_left=None, grid_right=None, fits=None, names=None):
    """the .mat hand-off of SURVEY 8(b): what the MATLAB pipeline holds after makePyGridPts (gridPtsPair) and
    fitSingleCylinder, written with scipy.io.savemat so `load(path)` gives the same variables.

        gridPtsPair  F x 2 struct array, fields center_point (2 x 1), points (N x 4 [x y colIdx rowIdx])
                     (makePyGridPts.m:39-41, pointsStruct2mat.m:16; column 1 = left image, 2 = right)
        frames       1 x F struct array, fields pts3 (3 x N), cylParams (2 x 6 = [cylParams0; cylParams]), cylT (4 x 4),
                     fvals (1 x 2), meanError (scalar), status        (fitSingleCylinder.m:1, fitCylinderWPts3.m:41)
        names        F x 1 cell of the image stems (getUniqueName.m)

    grid_left / grid_right: lists of dict(center_point, points) (api.grid_struct); fits: the dict
    fit.fit_single_cylinder_batch returns."""
    from scipy.io import savemat
    out = {}
    if grid_left is not None:
        F = len(grid_left)
        if grid_right is not None and len(grid_right) != F:
            raise ValueError('save_mat: left and right tables differ in length')
        pair = np.zeros((F, 2 if grid_right is not None else 1), dtype=[('center_point', 'O'), ('points', 'O')])
        for i in range(F):
            for c, g in enumerate((grid_left, grid_right) if grid_right is not None else (grid_left,)):
                pair[i, c]['center_point'] = np.asarray(g[i]['center_point'], np.float64).reshape(2, 1)
                pair[i, c]['points'] = np.asarray(g[i]['points'], np.float64).reshape(-1, 4)
        out['gridPtsPair'] = pair
    if fits is not None:
        m = fits['m'].cpu().numpy(); F = len(m)
        pts3 = fits['pts3'].cpu().numpy(); cyl = fits['cyl'].cpu().numpy(); T = fits['T'].cpu().numpy()
        fv = fits['fvals'].cpu().numpy(); me = fits['mean_err'].cpu().numpy(); st = fits['status'].cpu().numpy()
        fr = np.zeros((1, F), dtype=[(k, 'O') for k in ('pts3', 'cylParams', 'cylT', 'fvals', 'meanError', 'status')])
        for i in range(F):
            fr[0, i]['pts3'] = np.ascontiguousarray(pts3[i, :m[i]].T)
            fr[0, i]['cylParams'] = cyl[i].reshape(2, 6)
            fr[0, i]['cylT'] = T[i].reshape(4, 4)
            fr[0, i]['fvals'] = fv[i].reshape(1, 2)
            fr[0, i]['meanError'] = float(me[i])
            fr[0, i]['status'] = float(st[i])
        out['frames'] = fr
    if names is not None:
        out['names'] = np.array(list(names), dtype=object).reshape(-1, 1)
    savemat(path, out, oned_as='column')
    return path
