"""Packed results of a whole batch (cpe_detect_results_sizes / cpe_detect_results_pack, api.pack_results / batch_results) against
the per-frame interface they stand in for (the result's own tensors, api.line_tables, api.make_json) and against the oracle.
Tolerance 0 everywhere: the kernels only move data."""
import json

import numpy as np
import pytest
import torch


def _frames(h, w, n, seed):
    from cpe_amd import synth
    b = synth.render_batch(n, h, w, seed=seed, with_gt=False)
    return torch.cat([b['left'], b['right']])


def _same_tables(got, want):
    """equal as Python objects: keys, their order, lists of tuples of floats, lists of six floats"""
    assert got == want
    assert list(got) == list(want) == ['points', 'equations']
    assert list(got['points']) == list(want['points']) and list(got['equations']) == list(want['equations'])
    for k, pts in got['points'].items():
        assert type(pts) is list and all(type(p) is tuple and len(p) == 2 and type(p[0]) is float and type(p[1]) is float for p in pts), k
        # == on floats calls -0.0 and 0.0 equal: the bits are compared as well
        assert np.array_equal(np.array(pts, np.float64).view(np.int64), np.array(want['points'][k], np.float64).view(np.int64)), k
    for k, eq in got['equations'].items():
        assert type(eq) is list and len(eq) == 6 and all(type(v) is float for v in eq), k
        assert np.array_equal(np.array(eq).view(np.int64), np.array(want['equations'][k]).view(np.int64)), k


def _check_against_per_frame(cpe, det, target='cylinder', frames=None):
    """every frame of det: record == det's tensors, line_tables, make_json.  -> (records, offsets, payload)"""
    api = cpe.api
    off, payload = api.pack_results(det)
    recs = api.unpack_results(off, payload, target)
    assert len(recs) == det['n'].shape[0]
    again = api.batch_results(det, target)
    status = det['status'].cpu().numpy(); cnt = det['n'].cpu().numpy()
    xy = det['xy'].cpu().numpy(); ids = det['id'].cpu().numpy(); center = det['center'].cpu().numpy()
    for k in (range(len(recs)) if frames is None else frames):
        r = recs[k]
        tag = f'frame {k}'
        assert r.status == int(status[k]) and r.n == int(cnt[k]), tag
        assert r.xy.dtype == np.float64 and r.id.dtype == np.int32 and r.center.dtype == np.float64, tag
        assert np.array_equal(r.xy.view(np.int64), xy[k, :r.n].view(np.int64)), tag
        assert np.array_equal(r.id, ids[k, :r.n]), tag
        assert np.array_equal(r.center.view(np.int64), center[k].view(np.int64)), tag
        rows, cols = api.line_tables(det, k, target)
        _same_tables(r.rows, rows); _same_tables(r.cols, cols)
        assert api.make_json(r.center, r.xy, r.id) == api.make_json(center[k], xy[k, :r.n], ids[k, :r.n]), tag
        b = again[k]
        assert (b.status, b.n, b.rows, b.cols) == (r.status, r.n, r.rows, r.cols) and np.array_equal(b.xy, r.xy), tag
    return recs, off, payload


def _layout_bytes(r):
    nl = len(r.rows['points']) + len(r.cols['points'])
    npt = sum(len(p) for p in r.rows['points'].values()) + sum(len(p) for p in r.cols['points'].values())
    start = 4 * (nl + 1)
    return 48 + 16 * r.n + 8 * r.n + 48 * nl + (start + 7) // 8 * 8 + 16 * npt


def _check_layout(recs, off, payload):
    """offsets: increasing multiples of 8 from 0; each record as long as the documented layout makes it for its decoded
    counts; header words 6, 7 and the padding after an odd-length start table are zero"""
    assert off.dtype == np.int64 and off[0] == 0 and not np.any(off & 7) and np.all(np.diff(off) > 0)
    assert payload.size == int(off[-1])
    for k, r in enumerate(recs):
        at = int(off[k])
        assert int(off[k + 1]) - at == _layout_bytes(r), k
        head = payload[at:at + 32].view('<i4')
        nr, nc = len(r.rows['points']), len(r.cols['points'])
        assert head.tolist() == [r.status, r.n, nr, nc, sum(len(p) for p in r.rows['points'].values()),
                                 sum(len(p) for p in r.cols['points'].values()), 0, 0], k
        p = at + 48 + 24 * r.n + 48 * (nr + nc)
        nst = nr + nc + 1
        st = payload[p:p + 4 * (nst + nst % 2)].view('<i4')
        assert st[0] == 0 and np.all(np.diff(st[:nst]) >= 0), k
        if nst % 2:
            assert st[nst] == 0, (k, 'padding after the start table')


@pytest.mark.gpu
@pytest.mark.parametrize('h,w,n,seed', [(480, 640, 2, 0), (1200, 1920, 1, 3)])
def test_records_equal_the_per_frame_interface(cpe, orc, gpu, h, w, n, seed):
    det = cpe.api.detect_grid_batch(_frames(h, w, n, seed).to(gpu))
    recs, off, payload = _check_against_per_frame(cpe, det)
    _check_layout(recs, off, payload)
    assert sum(r.status == 0 for r in recs) >= 1 and all(len(r.rows['points']) >= 4 for r in recs if r.status == 0)


@pytest.mark.gpu
def test_mixed_batch_with_failed_frames(cpe, orc, gpu):
    """good frames beside a constant-7 frame (fails before the lines stage: 0 / 0 lines) and a frame without the saturated
    spot: every frame has its record, with the status and the line content the per-frame interface reports"""
    f = _frames(480, 640, 1, 2).numpy().copy()
    dark = np.full((480, 640), 7, np.uint8)
    nospot = f[0].copy(); nospot[nospot > 235] = 200
    frames = torch.from_numpy(np.stack([f[0], dark, f[1], nospot, f[0]]))
    det = cpe.api.detect_grid_batch(frames.to(gpu))
    recs, off, payload = _check_against_per_frame(cpe, det)
    _check_layout(recs, off, payload)
    assert recs[1].status == 1 and recs[3].status == 2 and recs[2].status == 0
    for k in (1, 3):
        assert recs[k].n == 0 and recs[k].rows == {'points': {}, 'equations': {}} and recs[k].cols == {'points': {}, 'equations': {}}
        assert int(off[k + 1] - off[k]) == 56
    assert payload[int(off[0]):int(off[1])].tobytes() == payload[int(off[4]):int(off[5])].tobytes()
    # frame_result alone decides that a failed frame becomes None
    assert cpe.api.frame_result(det, 1, dark, results=recs) is None
    out = cpe.api.frame_result(det, 2, f[1], results=recs)
    assert out[1] == cpe.api.make_json(recs[2].center, recs[2].xy, recs[2].id) and out[2] == recs[2].rows and out[3] == recs[2].cols


@pytest.mark.gpu
@pytest.mark.parametrize('n', [1, 65, 130])
def test_batch_sizes_around_the_scan_width(cpe, orc, gpu, n):
    """n = 1, and more frames than one wavefront (65) or two (130) of the offsets scan, made by repeating four frames:
    every frame equals the per-frame interface and repeated frames give byte-identical records"""
    base = _frames(480, 640, 2, 5)
    idx = [k % 4 for k in range(n)]
    det = cpe.api.detect_grid_batch(base[idx].to(gpu))
    recs, off, payload = _check_against_per_frame(cpe, det)
    _check_layout(recs, off, payload)
    first = {}
    for k, src in enumerate(idx):
        raw = payload[int(off[k]):int(off[k + 1])].tobytes()
        assert first.setdefault(src, raw) == raw, (k, src)
    assert any(r.status == 0 for r in recs)


@pytest.mark.gpu
def test_records_match_the_oracle(cpe, orc, gpu):
    """two frames against oracle.stages.detect_grid(img, lines=True), as test_rows_cols_updated_match_oracle does for the
    single-image call"""
    from oracle import stages as S
    b = _frames(480, 640, 2, 4)
    imgs = [b[0].numpy(), b[3].numpy()]
    det = cpe.api.detect_grid_batch(torch.from_numpy(np.stack(imgs)).to(gpu))
    recs = cpe.api.batch_results(det)
    for r, img in zip(recs, imgs):
        ref = S.detect_grid(img, lines=True)
        assert ref['status'] == 0 and r.status == 0
        assert np.array_equal(r.xy, ref['xy']) and np.array_equal(r.id, ref['id']) and np.array_equal(r.center, ref['center'])
        for got, want in ((r.rows, ref['rows']), (r.cols, ref['cols'])):
            assert list(got['points'].keys()) == list(want['points'].keys())
            assert list(got['equations'].keys()) == list(want['equations'].keys())
            for k in want['points']:
                assert got['points'][k] == [tuple(p) for p in want['points'][k]], k
                assert got['equations'][k] == list(want['equations'][k]), k
        assert len(r.rows['points']) >= 4 and len(r.cols['points']) >= 4


@pytest.mark.gpu
def test_options_plane_colour_subpixel(cpe, orc, gpu):
    from cpe_amd import synth
    sc = synth.Scene(h=600, w=800, radius=5000.0, depth=(5340.0, 5400.0), tilt_deg=4.0)
    b = synth.render_batch(1, 600, 800, seed=3, scene=sc, with_gt=False)
    det = cpe.api.detect_grid_batch(torch.cat([b['left'], b['right']]).to(gpu), target='plane')
    recs, off, payload = _check_against_per_frame(cpe, det, target='plane')
    _check_layout(recs, off, payload)
    assert any(r.status == 0 and r.n >= 60 and r.id[:, 1].min() < 0 for r in recs)      # (row, col) ids, negative columns kept
    f = _frames(480, 640, 1, 0).numpy()
    tint = np.stack([np.stack([np.minimum(255, g.astype(np.int32) + 4).astype(np.uint8), g, (g * 0.93).astype(np.uint8)], 2) for g in f])
    det = cpe.api.detect_grid_batch(torch.from_numpy(tint).to(gpu))
    recs, off, payload = _check_against_per_frame(cpe, det)
    _check_layout(recs, off, payload)
    assert any(r.status == 0 for r in recs)
    det = cpe.api.detect_grid_batch(torch.from_numpy(f).to(gpu), subpixel=True)
    recs, off, payload = _check_against_per_frame(cpe, det)
    _check_layout(recs, off, payload)
    assert any(r.status == 0 for r in recs)


def _raw_calls(cpe, det, payload, payload_bytes):
    """the two C calls on a caller-made payload tensor; -> offsets (numpy)"""
    L = cpe.lib.load()
    ws = det['ws']
    n = det['n'].shape[0]
    offsets = torch.empty(n + 1, dtype=torch.int64, device=det['xy'].device)
    stream = torch.cuda.current_stream().cuda_stream
    cpe.lib.check(L.cpe_detect_results_sizes(ws.view.data_ptr(), ws.bytes, ws.n, ws.h, ws.w, det['n'].data_ptr(), det['status'].data_ptr(),
                                             offsets.data_ptr(), stream), 'cpe_detect_results_sizes')
    if payload is not None:
        cpe.lib.check(L.cpe_detect_results_pack(ws.view.data_ptr(), ws.bytes, ws.n, ws.h, ws.w, det['xy'].data_ptr(), det['id'].data_ptr(),
                                                det['n'].data_ptr(), det['center'].data_ptr(), det['status'].data_ptr(),
                                                offsets.data_ptr(), payload.data_ptr(), payload_bytes, stream), 'cpe_detect_results_pack')
    torch.cuda.synchronize()
    return offsets.cpu().numpy()


@pytest.mark.gpu
def test_payload_bounds_are_respected(cpe, orc, gpu):
    """the pack kernel writes [0, offsets[n]) and nothing else: 4 KB of 0xA5 behind offsets[n] stay intact; with payload_bytes
    = half the total nothing at or beyond it is written, the records that end inside it are whole and the others untouched;
    the decoder refuses the short payload.  (Argument handling: the buffer itself is large enough in every call.)"""
    f = _frames(480, 640, 2, 0)
    det = cpe.api.detect_grid_batch(f.to(gpu))
    off = _raw_calls(cpe, det, None, 0)
    total = int(off[-1])
    ref_off, ref_payload = cpe.api.pack_results(det)
    assert np.array_equal(off, ref_off)
    buf = torch.full((total + 4096,), 0xA5, dtype=torch.uint8, device=gpu)
    _raw_calls(cpe, det, buf, total)
    got = buf.cpu().numpy()
    assert np.array_equal(got[:total], ref_payload)
    assert np.all(got[total:] == 0xA5)
    # the same with the canary counted into payload_bytes: a larger payload changes nothing
    buf.fill_(0xA5)
    _raw_calls(cpe, det, buf, total + 4096)
    got = buf.cpu().numpy()
    assert np.array_equal(got[:total], ref_payload) and np.all(got[total:] == 0xA5)
    # half the total
    half = total // 2
    buf.fill_(0xA5)
    _raw_calls(cpe, det, buf, half)
    got = buf.cpu().numpy()
    assert np.all(got[half:] == 0xA5)
    fits = [k for k in range(len(off) - 1) if off[k + 1] <= half]
    assert 0 < len(fits) < len(off) - 1
    for k in range(len(off) - 1):
        a, b = int(off[k]), int(off[k + 1])
        if k in fits:
            assert np.array_equal(got[a:b], ref_payload[a:b]), k
        else:
            assert np.all(got[a:b] == 0xA5), (k, 'a record that does not fit is skipped whole')
    with pytest.raises(ValueError):
        cpe.api.unpack_results(off, got[:half])
    # argument checks of the two entry points
    L = cpe.lib.load()
    ws = det['ws']
    assert L.cpe_detect_results_sizes(ws.view.data_ptr(), ws.bytes, ws.n, ws.h, ws.w, det['n'].data_ptr(), det['status'].data_ptr(), None, None) == -1
    assert L.cpe_detect_results_sizes(ws.view.data_ptr(), 1024, ws.n, ws.h, ws.w, det['n'].data_ptr(), det['status'].data_ptr(),
                                      buf.data_ptr(), None) == -1
    assert L.cpe_detect_results_pack(ws.view.data_ptr(), ws.bytes, ws.n, ws.h, ws.w, det['xy'].data_ptr(), det['id'].data_ptr(),
                                     det['n'].data_ptr(), det['center'].data_ptr(), det['status'].data_ptr(), None, buf.data_ptr(),
                                     buf.numel(), None) == -1
    assert L.cpe_detect_results_pack(ws.view.data_ptr(), ws.bytes, 0, ws.h, ws.w, det['xy'].data_ptr(), det['id'].data_ptr(),
                                     det['n'].data_ptr(), det['center'].data_ptr(), det['status'].data_ptr(), buf.data_ptr(), buf.data_ptr(),
                                     buf.numel(), None) == -1


@pytest.mark.gpu
def test_line_tables_near_their_capacity(cpe, orc, gpu):
    """tools/stress_parity.py seeds 4011 / 9508 (1920x1200, degraded): 220-250 label groups per direction, close to CPE_MAXL.
    Whatever the status, the records equal line_tables"""
    from cpe_amd import synth
    frames = []
    for seed in (4011, 9508):
        rng = np.random.default_rng(seed)
        b = synth.render_batch(1, 1200, 1920, seed=seed, with_gt=False)
        d, _ = synth.degrade(b['left'][0].numpy(), rng)
        frames.append(d)
    det = cpe.api.detect_grid_batch(torch.from_numpy(np.stack(frames)).to(gpu))
    recs, off, payload = _check_against_per_frame(cpe, det)
    _check_layout(recs, off, payload)
    # (test_degraded_full_size_frames_beyond_the_round_2_tables: both frames end with status 0 and 660 / 1220 grid points)
    assert all(r.status == 0 and r.n >= 600 for r in recs), [(r.status, r.n, len(r.rows['points']), len(r.cols['points'])) for r in recs]


@pytest.mark.gpu
def test_batch_results_refuse_a_workspace_that_has_moved_on(cpe, orc, gpu):
    f = _frames(480, 640, 2, 0).to(gpu)
    ws = cpe.api.DetectWorkspace(4, 480, 640, f.device)
    det4 = cpe.api.detect_grid_batch(f, ws)
    recs4 = cpe.api.batch_results(det4)
    rows4, cols4 = cpe.api.line_tables(det4, 3)
    det1 = cpe.api.detect_grid_batch(f[3:4], ws)
    recs1 = cpe.api.batch_results(det1)
    assert recs1[0].rows == recs4[3].rows == rows4 and recs1[0].cols == recs4[3].cols == cols4
    with pytest.raises(RuntimeError):
        cpe.api.batch_results(det4)
    with pytest.raises(RuntimeError):
        cpe.api.pack_results(det4)
    with pytest.raises(RuntimeError):
        cpe.api.line_tables(det4, 3)


def _equals_oracle(out, ref):
    col_img, result_json, rows, cols = out
    d = json.loads(result_json)
    assert [p['id'] for p in d['points']] == ref['id'].tolist()
    assert np.array_equal(np.array([[p['x'], p['y']] for p in d['points']]), ref['xy'])
    assert d['center_point'] == ref['center'].tolist()
    for got, want in ((rows, ref['rows']), (cols, ref['cols'])):
        assert list(got['points'].keys()) == list(want['points'].keys())
        for k in want['points']:
            assert got['points'][k] == [tuple(p) for p in want['points'][k]], k
            assert got['equations'][k] == list(want['equations'][k]), k


@pytest.mark.gpu
def test_single_image_calls_share_a_workspace_and_own_their_results(cpe, orc, gpu):
    """two successive api.detect_grid calls on different images, a call at another frame size in between: every result equals
    the oracle for its image, and the first result is unchanged after the later calls"""
    import copy
    from oracle import stages as S
    b = _frames(480, 640, 2, 4)
    img1, img2 = b[0].numpy(), b[3].numpy()
    other = _frames(600, 800, 1, 4)[0].numpy()
    ref1, ref2, ref3 = (S.detect_grid(i, lines=True) for i in (img1, img2, other))
    assert ref1['status'] == 0 and ref2['status'] == 0 and ref3['status'] == 0
    out1 = cpe.api.detect_grid(img1)
    _equals_oracle(out1, ref1)
    keep = copy.deepcopy(out1)
    out3 = cpe.api.detect_grid(other)
    _equals_oracle(out3, ref3)
    assert out3[0].shape == (600, 800, 3)
    out2 = cpe.api.detect_grid(img2)
    _equals_oracle(out2, ref2)
    assert out2[1] != out1[1]
    assert np.array_equal(out1[0], keep[0]) and out1[1:] == keep[1:]
    _equals_oracle(out1, ref1)
    # a failed frame between good ones: None, and the next call is unaffected
    assert cpe.api.detect_grid(np.full((480, 640), 7, np.uint8)) is None
    _equals_oracle(cpe.api.detect_grid(img1), ref1)
    # the picture marks the points of the JSON on a copy of the frame
    pic = cpe.api.draw_points(img1, [(p['x'], p['y']) for p in json.loads(out1[1])['points']])
    assert np.array_equal(out1[0], pic)
    # argument errors still raise from api.detect_grid (the drop-in module turns them into None) and leave the cache usable
    with pytest.raises(TypeError):
        cpe.api.detect_grid(np.zeros((480, 640), np.float32))
    with pytest.raises(ValueError):
        cpe.api.detect_grid(np.zeros((4, 480, 640, 3), np.uint8))
    with pytest.raises(cpe.lib.CpeError):
        cpe.api.detect_grid(np.zeros((16, 16), np.uint8))
    _equals_oracle(cpe.api.detect_grid(img2), ref2)
