"""The detect workspace's table of buffers (csrc/workspace.h) through the library's host-only entries: no GPU call.

Totals are held against the layout of the commit before the table (measured from a CPU build of it): the same memory minus
its two dead slots of 16 bytes per frame.  Public planes keep their sizes, every buffer lies inside the block on a 256-byte
boundary, and two buffers share bytes only as sides of one declared overlay."""
import ctypes as C
import functools
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPE_ERR_ARG = -1   # include/cpe.h

# (n, h, w) -> cpe_detect_workspace_bytes of the parent layout; (40, 64, 64): its dead slots are larger than one 256-byte unit
PARENT_BYTES = {
    (1, 64, 64): 94691072,
    (1, 480, 640): 103160064,
    (3, 480, 650): 310070528,
    (5, 65, 801): 480238080,
    (1, 1200, 1920): 170323712,
    (2, 1200, 1920): 340646144,
    (1, 2160, 3840): 583128832,
    (1, 4096, 4096): 1173246208,
    (7, 64, 4096): 725612544,
    (40, 64, 64): 3787593984,
}
SHAPES = sorted(PARENT_BYTES)

# the four overlays, side by side, by row name
OVERLAYS = [
    [{'dists', 'pool'}, {'groups'}],
    [{'bright_nodes', 'bright_counts'},
     {'roi_h', 'roi_v', 'base_h', 'base_v', 'exp_h', 'exp_v', 'tmpa', 'tmpb', 'discs', 'mask_contour', 'blur7'}],
    [{'labels_joints', 'labels_spot'}, {'lines', 'subpix'}, {'blob_ch', 'blob_d'}],
    [{'labels', 'labels_aux'}, {'blobs'}],
]
U8_PLANES = ('binary', 'hmask', 'vmask', 'mask_contour', 'roi_h', 'roi_v', 'exp_h', 'exp_v', 'clahe', 'blur19', 'blur7')


def align_up(v, a):
    return (v + a - 1) // a * a


@functools.lru_cache(maxsize=None)
def listing(n, h, w):
    """every row of the table for an (n, h, w) call, in table order"""
    import cpe_amd
    L = cpe_amd.lib.load()
    rows = []
    while True:
        name = C.create_string_buffer(64)
        off, per = C.c_size_t(), C.c_size_t()
        ov, side, pub = C.c_int32(), C.c_int32(), C.c_int32()
        rc = L.cpe_debug_workspace_buffer(n, h, w, len(rows), name, len(name), C.byref(off), C.byref(per), C.byref(ov),
                                          C.byref(side), C.byref(pub))
        if rc != 0:
            assert rc == CPE_ERR_ARG, 'past the last row'
            assert len(rows) >= 15
            return tuple(rows)
        rows.append(dict(name=name.value.decode(), off=off.value, per=per.value, overlay=ov.value, side=side.value,
                         public=pub.value))


def public_plane(cpe, n, h, w, plane):
    off, per = C.c_size_t(), C.c_size_t()
    cpe.lib.check(cpe.lib.load().cpe_detect_workspace_plane(n, h, w, plane, C.byref(off), C.byref(per)), 'cpe_detect_workspace_plane')
    return off.value, per.value


@pytest.mark.parametrize('shape', SHAPES)
def test_total_is_the_parents_minus_the_dead_slots(cpe, shape):
    n = shape[0]
    assert cpe.lib.load().cpe_detect_workspace_bytes(*shape) == PARENT_BYTES[shape] - 2 * align_up(16 * n, 256)


def test_plane_numbers_in_one_place(cpe):
    hdr = open(os.path.join(ROOT, 'include', 'cpe.h')).read()
    defines = {k.lower(): int(v) for k, v in re.findall(r'#define CPE_PLANE_(\w+) (\d+)\b', hdr)}
    assert sorted(defines.values()) == list(range(15))
    assert cpe.api.PLANES == defines
    by_public = {r['public']: r['name'] for r in listing(1, 64, 64) if r['public'] >= 0}
    assert by_public == {v: k for k, v in cpe.api.PLANES.items()}
    assert sum(r['public'] >= 0 for r in listing(1, 64, 64)) == 15


@pytest.mark.parametrize('shape', SHAPES)
def test_public_planes(cpe, shape):
    n, h, w = shape
    rows = {r['public']: r for r in listing(*shape) if r['public'] >= 0}
    want = {name: h * w for name in U8_PLANES}
    want.update(joints=131072, state=184, labels=4 * h * w, sweep=768)
    assert set(want) == set(cpe.api.PLANES)
    for name, plane in cpe.api.PLANES.items():
        off, per = public_plane(cpe, n, h, w, plane)
        assert per == want[name], name
        assert (off, per) == (rows[plane]['off'], rows[plane]['per']), name
    off, per = C.c_size_t(), C.c_size_t()
    for plane in (-1, 15):
        assert cpe.lib.load().cpe_detect_workspace_plane(n, h, w, plane, C.byref(off), C.byref(per)) == CPE_ERR_ARG


@pytest.mark.parametrize('shape', SHAPES)
def test_structure(cpe, shape):
    n = shape[0]
    rows = listing(*shape)
    total = cpe.lib.load().cpe_detect_workspace_bytes(*shape)
    names = [r['name'] for r in rows]
    assert len(set(names)) == len(names)
    assert not {'tmp16', 'htime', 'hpar'} & set(names)
    for r in rows:
        assert r['off'] % 256 == 0, r['name']
        assert r['per'] > 0 and r['off'] + n * r['per'] <= total, r['name']
    spans = sorted((r['off'], r['off'] + n * r['per'], r) for r in rows)
    for i, (a0, a1, a) in enumerate(spans):
        for b0, b1, b in spans[i + 1:]:
            if b0 >= a1:
                break
            assert a['overlay'] != 0 and a['overlay'] == b['overlay'] and a['side'] != b['side'], (a['name'], b['name'])
    got = {}
    for r in rows:
        if r['overlay']:
            got.setdefault(r['overlay'], {}).setdefault(r['side'], set()).add(r['name'])
    assert [[sides[k] for k in sorted(sides)] for _, sides in sorted(got.items())] == OVERLAYS
    assert all(r['side'] == 0 for r in rows if not r['overlay'])
    # the sides of an overlay start together
    for sides in got.values():
        assert len({min(r['off'] for r in rows if r['name'] in s) for s in sides.values()}) == 1


# the words of the state record by the names tests and tools read them under (DetectWorkspace.state()), in order
STATE_NAMES = ['status', 'rect0', 'rect1', 'rect2', 'rect3', 'r0', 'spot0', 'spot1', 'spot2', 'spot3', 'n_roots',
               'n_comps', 'n_joints_all', 'n_joints', 'n_blobs', 'n_groups', 'n_groups_prev', 'n_kp', 'n_verts',
               'n_dists', 'best_comp', 'n_seg0', 'n_seg1', 'gang0', 'gang1', 'glen0', 'glen1', 'n_rows', 'n_cols',
               'overflow', 'hull_n', 'crect0', 'crect1', 'crect2', 'crect3', 'nrect0', 'nrect1', 'nrect2', 'nrect3',
               'n_roots_p', 'n_roots_s', 'spot_fail', 'srect0', 'srect1', 'srect2', 'srect3']


def test_state_fields_cover_the_record(cpe):
    fields = cpe.api.state_fields()
    assert len(STATE_NAMES) == 46 and [k for k, _ in fields] == STATE_NAMES == cpe.api._STATE_FIELDS
    state = [r for r in listing(1, 64, 64) if r['name'] == 'state']
    assert len(state) == 1 and len(fields) * 4 == state[0]['per']
    assert [k for k, is_float in fields if is_float] == ['gang0', 'gang1', 'glen0', 'glen1']
    L = cpe.lib.load()
    name = C.create_string_buffer(64)
    words, is_float = C.c_int32(), C.c_int32()
    rows = 0
    while L.cpe_debug_state_field(rows, name, len(name), C.byref(words), C.byref(is_float)) == 0:
        rows += 1
    assert rows == 28
    for index in (rows, 46, -1):
        assert L.cpe_debug_state_field(index, name, len(name), C.byref(words), C.byref(is_float)) == CPE_ERR_ARG
    assert L.cpe_debug_state_field(0, name, 0, C.byref(words), C.byref(is_float)) == CPE_ERR_ARG
    short = C.create_string_buffer(4)   # a name longer than the buffer is cut, and still terminated
    assert L.cpe_debug_state_field(0, short, len(short), C.byref(words), C.byref(is_float)) == 0 and short.value == b'sta'
    assert (words.value, is_float.value) == (1, 0)


def test_listing_rejects_bad_arguments(cpe):
    L = cpe.lib.load()
    name = C.create_string_buffer(64)
    v = [C.c_size_t(), C.c_size_t(), C.c_int32(), C.c_int32(), C.c_int32()]
    refs = [C.byref(x) for x in v]
    assert L.cpe_debug_workspace_buffer(1, 64, 64, 0, name, len(name), *refs) == 0
    assert L.cpe_debug_workspace_buffer(1, 64, 64, -1, name, len(name), *refs) == CPE_ERR_ARG
    assert L.cpe_debug_workspace_buffer(0, 64, 64, 0, name, len(name), *refs) == CPE_ERR_ARG
    assert L.cpe_debug_workspace_buffer(1, 64, 64, 0, name, 0, *refs) == CPE_ERR_ARG
    short = C.create_string_buffer(4)   # a name longer than the buffer is cut, and still terminated
    assert L.cpe_debug_workspace_buffer(1, 64, 64, 0, short, len(short), *refs) == 0 and short.value == b'dis'


def test_opening_a_workspace_keeps_its_error_codes(cpe):
    """a short or missing block is CPE_ERR_WORKSPACE from cpe_detect_grid_batch*, CPE_ERR_ARG from every other entry, and a
    misaligned one CPE_ERR_ARG; the checks come before the first GPU call, so the pointers here are never followed"""
    L = cpe.lib.load()
    total = L.cpe_detect_workspace_bytes(1, 64, 64)
    p = 4096   # stands for any non-null, aligned device pointer
    def detect(ws, ws_bytes):
        return L.cpe_detect_grid_batch_ex(p, 1, 64, 64, None, ws, ws_bytes, p, p, p, p, p, None)
    assert detect(None, total) == -3 and detect(p, total - 1) == -3
    assert b'cpe_detect_grid_batch' in L.cpe_last_error_string()
    assert detect(p + 1, total) == CPE_ERR_ARG
    assert L.cpe_debug_ccl(p, 1, 64, 64, 0, 0, 1, 0, 0, 0, p, total - 1, None) == CPE_ERR_ARG
    assert b'cpe_debug_ccl' in L.cpe_last_error_string()
    assert L.cpe_debug_ccl(p, 1, 64, 64, 0, 0, 1, 0, 0, 0, p + 1, total, None) == CPE_ERR_ARG
    assert L.cpe_detect_line_tables(p, total - 1, 1, 64, 64, 0, p, p, p, p, None) == CPE_ERR_ARG
    assert b'cpe_detect_line_tables' in L.cpe_last_error_string()
