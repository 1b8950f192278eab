"""Helpers for the tests of the workspace contract (include/cpe.h, "Workspaces"): what a call computes never depends on what
its workspace held on entry.  No tests here.

rows(n, h, w): the table of buffers of an (n, h, w) layout as cpe_debug_workspace_buffer lists it (host code only).
fill / fill_row: put one byte value into the whole aligned view of a DetectWorkspace, or into one row (n * bytes_per_frame
from its offset) of the layout of the call that follows.
workspace(capacity_n, h, w, device): a DetectWorkspace larger than the call it will serve (the ragged last chunk)."""
import ctypes as C
import functools

CPE_ERR_ARG = -1   # include/cpe.h


def align_up(v, a=256):
    return (v + a - 1) // a * a


@functools.lru_cache(maxsize=None)
def rows(n, h, w):
    """every row of the table for an (n, h, w) call, in table order: dicts of name, off, per (bytes per frame), overlay,
    side, public (CPE_PLANE_* or -1)"""
    import cpe_amd
    L = cpe_amd.lib.load()
    out = []
    while True:
        name = C.create_string_buffer(64)
        off, per = C.c_size_t(), C.c_size_t()
        ov, side, pub = C.c_int32(), C.c_int32(), C.c_int32()
        rc = L.cpe_debug_workspace_buffer(n, h, w, len(out), name, len(name), C.byref(off), C.byref(per), C.byref(ov),
                                          C.byref(side), C.byref(pub))
        if rc != 0:
            assert rc == CPE_ERR_ARG and out, 'the listing ends with CPE_ERR_ARG past its last row'
            return tuple(out)
        out.append(dict(name=name.value.decode(), off=off.value, per=per.value, overlay=ov.value, side=side.value,
                        public=pub.value))


def row_names(h, w):
    """the names of the rows, which do not depend on the frame size (the size only makes the listing callable)"""
    return [r['name'] for r in rows(1, h, w)]


def total_bytes(n, h, w):
    import cpe_amd
    return cpe_amd.lib.load().cpe_detect_workspace_bytes(n, h, w)


def row_span(r, n, padded=False):
    """[first, last) byte of a row of an n-frame layout; padded: up to the 256-byte boundary the next buffer starts at"""
    end = r['off'] + n * r['per']
    return r['off'], align_up(end) if padded else end


def workspace(capacity_n, h, w, device):
    import cpe_amd
    return cpe_amd.api.DetectWorkspace(capacity_n, h, w, device)


def fill(ws, value):
    """every byte of the block the library is given (the aligned view, at the workspace's full capacity)"""
    ws.buf[(-ws.buf.data_ptr()) % 256:][:ws.capacity].fill_(value)


def full_view(ws):
    """the aligned block at its full capacity, whatever n the last call used"""
    return ws.buf[(-ws.buf.data_ptr()) % 256:][:ws.capacity]


def fill_row(ws, n, name, value, rest=0):
    """the bytes of row `name` of the (n, h, w) layout get `value`, every other byte of the block `rest`"""
    fill(ws, rest)
    (r,) = [r for r in rows(n, ws.h, ws.w) if r['name'] == name]
    a, b = row_span(r, n)
    assert b <= ws.capacity
    full_view(ws)[a:b].fill_(value)


# ---------------------------------------------------------------- the frames of the detect cases
ST_OK, ST_NO_REGION, ST_NO_SPOT, ST_NO_LINES = 0, 1, 2, 3      # include/cpe.h CPE_ST_*


def _stereo(h, w, seed):
    """the rendered stereo pair of tests/test_detect_gpu.py::_frames(h, w, 1, seed): u8 [2,h,w] numpy (left, right)"""
    import torch
    from cpe_amd import synth
    b = synth.render_batch(1, h, w, seed=seed, with_gt=False)
    return torch.cat([b['left'], b['right']]).numpy()


def no_spot(frame):
    """tests/test_detect_gpu.py::test_detect_failure_statuses: the grid without its saturated spot"""
    out = frame.copy()
    out[out > 235] = 200
    return out


def no_lines(frame):
    """the frame averaged over 15 columns (integer arithmetic): the blob region and the saturated spot survive, the vertical
    ridges do not, and the reference's indexing returns early.  No generator of the stage tests makes a whole frame that ends
    there (theirs make the inputs of one stage), so this one is made here; the CPU test holds it to its status."""
    import numpy as np
    k = 15
    pad = np.pad(frame.astype(np.int64), ((0, 0), (k // 2, k // 2)), mode='edge')
    c = np.concatenate([np.zeros((frame.shape[0], 1), np.int64), np.cumsum(pad, 1)], 1)
    return ((c[:, k:] - c[:, :-k]) // k).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def detect_case(name):
    """-> dict(frames: u8 numpy [n,h,w] or [n,h,w,3], target, status: what the oracle must make of every frame)
    grey480: the word-level path (w % 16 == 0), two good frames and one of each early ending; grey483: the byte-level path;
    plane*: the planar frames of tests/test_plane_gpu.py with a dark frame between them; bgr480: true-colour frames (the grey
    plane in GRAYIN, the L plane borrowed from DISCS) around a black one"""
    import numpy as np
    import plane_colour_oracle as PC
    if name == 'grey480':
        f = _stereo(480, 640, 0)
        frames = np.stack([f[0], np.zeros_like(f[0]), f[1], no_spot(f[0]), no_lines(f[0])])
        return dict(frames=frames, target='cylinder', status=[ST_OK, ST_NO_REGION, ST_OK, ST_NO_SPOT, ST_NO_LINES])
    if name == 'grey483':
        f = _stereo(483, 650, 8)
        frames = np.stack([f[0], no_spot(f[1]), f[1], np.zeros_like(f[0])])
        return dict(frames=frames, target='cylinder', status=[ST_OK, ST_NO_SPOT, ST_OK, ST_NO_REGION])
    if name.startswith('plane'):
        h, w, seed = {'plane600': (600, 800, 3), 'plane1200': (1200, 1920, 5), 'plane483': (483, 650, 9)}[name]
        f = PC.plane_frames(h, w, 1, seed)
        frames = np.stack([f[0], np.full_like(f[0], 20), f[1]])        # 20: test_plane_failure_and_argument_checks
        return dict(frames=frames, target='plane', status=[ST_OK, ST_NO_REGION, ST_OK])
    if name == 'bgr480':
        f = _stereo(480, 640, 3)
        rng = np.random.default_rng(12)
        a, b = PC.tint(f[0], rng), PC.tint(f[1], rng)
        return dict(frames=np.stack([a, np.zeros_like(a), b]), target='cylinder', status=[ST_OK, ST_NO_REGION, ST_OK])
    raise KeyError(name)


DETECT_CASES = ('grey480', 'grey483', 'plane600', 'plane483', 'plane1200', 'bgr480')


def oracle_status(case):
    """the status the oracle ends every frame of a case with"""
    from oracle import stages as S
    c = detect_case(case)
    if c['frames'].ndim == 4:
        return [S.detect_grid_bgr(f)['status'] for f in c['frames']]
    fn = S.detect_grid_plane if c['target'] == 'plane' else S.detect_grid
    return [fn(f)['status'] for f in c['frames']]
