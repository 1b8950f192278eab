"""The lines stage on its own (cpe_debug_lines, include/cpe.h) against the oracle (stages.lines_stage), with tolerance 0.

The entry labels the two expanded masks as masks_stage does (unions only, inside rect + 2 px) and runs k_lines as the detect
call does, on masks, joints, a rectangle, r0, an incoming status, a blurred image and a grey frame of the test's choosing
(tests/lines_cases.py: one idea per generator; the CPU file tests/test_lines_generators_cpu.py checks that each reaches its
edge: 63 .. 257 label groups per direction, 1023 .. 1025 joints in a group, 2048 / 2112 grid points, label planes with long
parent chains at both label-pass paths, the joint lookup, the early exits, exact ties of the two arg-reductions in different
threads, clipped and empty windows, the planar column merge, the sub-pixel path).  Per frame, bit for bit:
  - status, n_pts, id, centre and xy; the state's n_rows, n_cols and overflow (0, or exactly OVF_LINES);
  - api.line_tables against the oracle's line sets: equations as bits, point counts, points in loop order;
  - api.pack_results / unpack_results equal to the dense tables;
  - a frame that ends in status 6: the status, n_pts 0 and the overflow bit only.
Window 15 of the sub-pixel refinement is refused by the entry as by cpe_detect_grid_batch_ex (1 .. 13: the kernel's window
buffer holds 16 values, a window of 13 reads at most 14); 13 is tested, 15 is checked to be refused.
Checks that do not go through the oracle's restatement (lines_cases.fit_diff / residual): every equation against
numpy.polyfit of the joints of the scipy.ndimage.label component it must come from -- which is also the check of every
surviving group's membership -- and every reported intersection against both of its polynomials.  The oracle alone, on the CPU,
reaches 5.06e-10 px (numpy.polyfit difference over the line's domain; the three-point parabolas of the label cases) and
2.16e-12 px (residual) over all cases (lines_cases.ORACLE_FIT_DIFF = 5.1e-10, ORACLE_RESIDUAL = 2.2e-12, asserted by the CPU
file); the GPU is allowed ten times that -- the margin is numpy's LAPACK path against the Householder restatement, the GPU
itself must equal the oracle exactly.
Each case runs alone, inside a mixed batch and with the batch reversed: the three runs are bit-identical.  A workspace that
held the 256-group and the 2048-point frames gives, for sparse and early-exit frames, what a zeroed workspace gives."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lines_cases as L  # noqa: E402

HAVE_LINES = (0, 3, 4)


def _key(c):
    return (c['exp_h'].shape, c['target'], c['subpixel'])


def _run(cpe, gpu, cases, ws=None):
    """cpe_debug_lines on a list of cases of one frame size, target and sub-pixel setting -> per-frame dicts of host results"""
    assert len({_key(c) for c in cases}) == 1
    c0 = cases[0]
    st = lambda k: torch.from_numpy(np.stack([c[k] for c in cases])).to(gpu)
    kmax = max(1, max(len(c['joints']) for c in cases))
    joints = np.zeros((len(cases), kmax, 2), np.int32)
    for i, c in enumerate(cases):
        joints[i, :len(c['joints'])] = c['joints']
    vec = lambda k: torch.tensor([c[k] for c in cases], dtype=torch.int32)
    sp = c0['subpixel']
    det = cpe.api.debug_lines(st('exp_h'), st('exp_v'), torch.from_numpy(joints), vec('n_joints'),
                              torch.tensor([c['rect'] for c in cases], dtype=torch.int32), vec('r0'), vec('status'), st('g7'), st('gray'),
                              ws=ws, subpixel=sp is not None, subpixel_window=sp[0] if sp else 7, subpixel_step=sp[1] if sp else 1.0,
                              target=c0['target'])
    torch.cuda.synchronize()
    state = det['ws'].state()
    recs = cpe.api.unpack_results(*cpe.api.pack_results(det), target=c0['target'])
    n = det['n'].cpu().numpy(); status = det['status'].cpu().numpy(); center = det['center'].cpu().numpy()
    xy = det['xy'].cpu().numpy(); ids = det['id'].cpu().numpy()
    out = []
    for i in range(len(cases)):
        rows, cols = cpe.api.line_tables(det, i, target=c0['target'])
        m = int(n[i])
        out.append(dict(status=int(status[i]), n=m, xy=xy[i, :m].copy(), id=ids[i, :m].copy(), center=center[i].copy(), rows=rows, cols=cols,
                        rec=recs[i], n_rows=state[i]['n_rows'], n_cols=state[i]['n_cols'], overflow=state[i]['overflow'],
                        state_status=state[i]['status']))
    return out


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def _same_tables(a, b):
    """two line-table dicts are the same lines: equations as bits, points in order"""
    if list(a['equations']) != list(b['equations']) or list(a['points']) != list(b['points']):
        return False
    return all(np.array_equal(_bits(a['equations'][k]), _bits(b['equations'][k])) and
               np.array_equal(_bits(np.array(a['points'][k]).reshape(-1, 2)), _bits(np.array(b['points'][k]).reshape(-1, 2)))
               for k in a['equations'])


def _same(a, b, tag):
    """two runs of one frame are bit-identical"""
    for k in ('status', 'n', 'n_rows', 'n_cols', 'overflow', 'state_status'):
        assert a[k] == b[k], (tag, k, a[k], b[k])
    for k in ('xy', 'id', 'center'):
        assert np.array_equal(_bits(a[k]) if a[k].dtype == np.float64 else a[k], _bits(b[k]) if b[k].dtype == np.float64 else b[k]), (tag, k)
    assert _same_tables(a['rows'], b['rows']) and _same_tables(a['cols'], b['cols']), (tag, 'line tables')
    ra, rb = a['rec'], b['rec']
    assert (ra.status, ra.n) == (rb.status, rb.n) and np.array_equal(_bits(ra.xy), _bits(rb.xy)) and np.array_equal(ra.id, rb.id) and \
        np.array_equal(_bits(ra.center), _bits(rb.center)) and _same_tables(ra.rows, rb.rows) and _same_tables(ra.cols, rb.cols), (tag, 'record')


def _check(c, g, ref, tag, ovf):
    """one frame of a cpe_debug_lines result against the oracle, tolerance 0, and against numpy / scipy"""
    assert g['status'] == ref['status'], (tag, 'status', g['status'], ref['status'])
    assert g['overflow'] == ovf, (tag, 'overflow', g['overflow'], ovf)
    # the packed record is the dense tables
    r = g['rec']
    assert (r.status, r.n) == (g['status'], g['n']) and np.array_equal(r.xy, g['xy']) and np.array_equal(r.id, g['id']) and \
        np.array_equal(r.center, g['center']), (tag, 'record')
    assert _same_tables(r.rows, g['rows']) and _same_tables(r.cols, g['cols']), (tag, 'record lines')
    if ref['status'] == 6:
        assert ovf == L.OVF_LINES and g['n'] == 0 and len(r.xy) == 0, tag
        return
    assert g['n'] == len(ref['xy']), (tag, 'n_pts', g['n'], len(ref['xy']))
    assert np.array_equal(g['id'], ref['id']), (tag, 'ids')
    assert np.array_equal(g['center'], ref['center']), (tag, 'center', g['center'], ref['center'])
    assert np.array_equal(g['xy'], ref['xy']), (tag, 'xy', float(np.abs(g['xy'] - ref['xy']).max()) if g['n'] else 0)
    assert (g['n_rows'], g['n_cols']) == (ref['n_rows'], ref['n_cols']), (tag, 'n_rows / n_cols', g['n_rows'], g['n_cols'], ref['n_rows'], ref['n_cols'])
    if c['status'] != 0 or ref['status'] not in HAVE_LINES:      # skipped frame, or the refinement raised: no lines are left behind
        assert len(g['rows']['equations']) == 0 and len(g['cols']['equations']) == 0, tag
        assert g['n'] == 0 and not g['center'].any(), tag
        return
    for side, (prefix, ls) in enumerate((('row', ref['rows']), ('col', ref['cols']))):
        got = L.lines_of_table(g['rows' if side == 0 else 'cols'], prefix)
        want = L.lines_of(ls)
        assert len(got) == len(want), (tag, prefix, 'lines', len(got), len(want))
        for k, ((ge, gp), (we, wp)) in enumerate(zip(got, want)):
            assert np.array_equal(_bits(ge), _bits(we)), (tag, prefix, k, 'equation bits', ge, we)
            assert len(gp) == len(wp) and np.array_equal(_bits(np.array(gp).reshape(-1, 2)), _bits(np.array(wp).reshape(-1, 2))), (tag, prefix, k, 'points')
    rows, cols = L.lines_of_table(g['rows'], 'row'), L.lines_of_table(g['cols'], 'col')
    res = L.residual(c, rows, cols)
    assert res <= 10 * L.ORACLE_RESIDUAL, (tag, 'residual', res)
    if c['subpixel'] is None:       # (refined lines are fitted to samples, not to joints)
        fd = L.fit_diff(c, rows, cols)
        assert fd <= 10 * L.ORACLE_FIT_DIFF, (tag, 'numpy.polyfit difference', fd)


_ALONE = {}
_WS = {}


def _alone(cpe, gpu, name):
    """the case run on its own (once per session; one workspace per frame size)"""
    if name not in _ALONE:
        c = L.get(name)
        shape = c['exp_h'].shape
        if shape not in _WS:
            _WS[shape] = cpe.api.DetectWorkspace(1, shape[0], shape[1], gpu)
        _ALONE[name] = _run(cpe, gpu, [c], ws=_WS[shape])[0]
    return _ALONE[name]


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(L.CASES))
def test_lines_stage_case_alone(cpe, orc, gpu, name):
    _check(L.get(name), _alone(cpe, gpu, name), L.ref(name), name, L.expect_overflow(name))


def _batches(chunk=24):
    groups = {}
    for name in sorted(L.CASES):
        groups.setdefault(_key(L.get(name)), []).append(name)
    out = []
    for key in sorted(groups, key=str):
        names = groups[key]
        out += [names[i:i + chunk] for i in range(0, len(names), chunk)]
    return out


BATCHES = _batches()


@pytest.mark.gpu
@pytest.mark.parametrize('k', range(len(BATCHES)))
def test_lines_stage_batch_equals_alone(cpe, orc, gpu, k):
    """the cases of one frame size, target and sub-pixel setting in one batch and in reversed order: every frame identical to
    its run alone"""
    names = BATCHES[k]
    cases = [L.get(n) for n in names]
    batch = _run(cpe, gpu, cases)
    rev = _run(cpe, gpu, cases[::-1])
    for i, n in enumerate(names):
        alone = _alone(cpe, gpu, n)
        _same(batch[i], alone, (n, 'batch'))
        _same(rev[len(names) - 1 - i], alone, (n, 'reversed batch'))


def test_batches_mix_the_cases(orc):
    assert sum(len(b) for b in BATCHES) == len(L.CASES) and max(len(b) for b in BATCHES) >= 20
    assert any(len({L.ref(n)['status'] for n in b}) >= 3 for b in BATCHES)       # ok, no lines and overflow side by side


def _padded(c, H, W):
    h, w = c['exp_h'].shape
    pad = lambda a: np.pad(a, ((0, H - h), (0, W - w)))
    return dict(c, exp_h=pad(c['exp_h']), exp_v=pad(c['exp_v']), g7=pad(c['g7']), gray=pad(c['gray']))


@pytest.mark.gpu
def test_lines_stage_leaves_nothing_behind_in_the_workspace(cpe, orc, gpu):
    """LinesWS (in, fin_ord, fin_n, eq, ipts) is read after the call by k_line_tables and k_results_pack: sparse and early-exit
    frames on a workspace whose slots just held the 256-group, the 2048-point, the CPE_MAXJ-joint and the 1024-joint frames
    give the tables, line tables and packed records of a zeroed workspace"""
    H = W = 320
    big = [_padded(L.get(n), H, W) for n in ('groups_row_256_raster', 'points_2048', 'groups_col_256_shuffled', 'all_joints',
                                             'group_size_row_1024', 'constant_g7', 'two_maxima')]
    sparse_names = ['one_row', 'no_joints', 'status_1', 'tiny_groups', 'status_2', 'groups_row_2_raster', 'one_col']
    sparse = [_padded(L.get(n), H, W) for n in sparse_names]
    refined = [_padded(L.get(n), H, W) for n in ('subpixel_corner_row_w7', 'subpixel_tiny_groups', 'subpixel_corner_col_w7')]
    refined += [dict(sparse[k], subpixel=(7, 1.0)) for k in (0, 1, 2, 4)]
    ws = cpe.api.DetectWorkspace(len(big), H, W, gpu)
    fresh = cpe.api.DetectWorkspace(len(big), H, W, gpu)
    full = _run(cpe, gpu, big, ws=ws)
    assert [f['status'] for f in full] == [0] * len(big) and full[1]['n'] == L.MAXP and full[0]['n_rows'] == 255
    for cases, tags in ((sparse, sparse_names), (refined, None)):
        fresh.buf.zero_()
        want = _run(cpe, gpu, cases, ws=fresh)
        _run(cpe, gpu, big, ws=ws)
        got = _run(cpe, gpu, cases, ws=ws)
        for i in range(len(cases)):
            _same(got[i], want[i], ('stale workspace', tags[i] if tags else i))
        if tags:
            for i, n in enumerate(tags):
                _check(sparse[i], got[i], L.ref(n), ('stale workspace', n), 0)
            assert sorted({g['status'] for g in got}) == [0, 1, 2, 3]
        else:
            assert [g['status'] for g in got] == [7, 0, 7, 3, 3, 1, 2]


@pytest.mark.gpu
def test_lines_stage_refuses_what_the_detect_call_refuses(cpe, gpu):
    """sub-pixel windows outside 1 .. 13, a non-positive step, and the refinement of the planar target"""
    c = L.get('subpixel_corner_row_w13')
    for bad in (dict(subpixel=(15, 1.0)), dict(subpixel=(0, 1.0)), dict(subpixel=(7, 0.0)), dict(subpixel=(7, 1.0), target='plane')):
        with pytest.raises(cpe.lib.CpeError):
            _run(cpe, gpu, [dict(c, **bad)])
