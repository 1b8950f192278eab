"""k_select_triangulate (csrc/fit.hip) at every patch size 1..8 and on grids with holes, against the C oracle: the cases of
tests/selector_cases.py, whose plain restatement of chooseIdx.m tests/test_selector_cases_cpu.py holds against the same oracle
without a GPU.  Every comparison is exact but the one of mean_err (1e-13 relative to math.fsum, as
test_fit_shapes_gpu.py::test_select_triangulate_shapes has it): the thresholds lie half way between two means that differ
(test_margins), or on one on purpose (the boundary tests), and the kernel's errors have the oracle's bits.

All cases that share a threshold are the frames of one call, padded past their counts with NaN pixels and +-9999 indices."""
import collections
import math

import numpy as np
import pytest
import torch

import selector_cases as SC
from test_fit_shapes_gpu import _np, _table_batch, _three_ways

R = 45.0
PER_POINT = ('p1', 'p2', 'idx', 'pts3', 'err')


def _frames(names):
    return [(SC.case(n).t1, SC.case(n).t2, len(SC.case(n).t1), len(SC.case(n).t2)) for n in names]


def _groups(patch):
    """{th: [case names]}: th is per call"""
    groups = collections.OrderedDict()
    for name in SC.CASE_NAMES:
        groups.setdefault(SC.threshold(name, patch), []).append(name)
    return groups


def _oracle(orc, selector, name, patch, th):
    c = SC.case(name)
    K1, K2, T21 = SC.rig()
    if selector == 0:
        return orc.choose_idx(c.t1, c.t2, K1, K2, T21, patch, th)
    if selector == 1:
        return orc.triangulate_with_threshold(c.t1, c.t2, K1, K2, T21, th)
    return orc.find_correspondences(c.t1, c.t2) + (False,)


def _check_frame(orc, fit, out, i, ref, tag):
    """frame i of a select_triangulate_batch result against the oracle's (p1, p2, idx, fallback)"""
    r1, r2, idx, fb = ref
    m, fl = int(out['m'][i]), int(out['flags'][i])
    assert m == len(r1), (tag, m, len(r1))
    assert not fl & fit.FLAG_OVERFLOW, tag
    assert bool(fl & fit.FLAG_FALLBACK) == fb and not fl & ~fit.FLAG_FALLBACK, (tag, fl)
    assert np.array_equal(out['idx'][i, :m], idx), tag
    assert np.array_equal(out['p1'][i, :m], r1) and np.array_equal(out['p2'][i, :m], r2), tag
    for q in (q for q in PER_POINT if q in out):                  # nothing written past m
        assert not out[q][i, m:].any(), (tag, q)
    if 'pts3' in out:
        X, err = orc.triangulate(r1, r2, *SC.rig())
        assert np.array_equal(out['pts3'][i, :m], X) and np.array_equal(out['err'][i, :m], err), tag
        assert m > 0, tag
        me = math.fsum(out['err'][i, :m]) / m
        assert abs(out['mean_err'][i] - me) <= 1e-13 * me, (tag, out['mean_err'][i], me)


def _select(fit, names, selector, patch, th, poison=True):
    g1, g2 = _table_batch(_frames(names), poison)
    out = _np(fit.select_triangulate_batch(g1, g2, *SC.rig(), selector=selector, patch=patch, th=th))
    torch.cuda.synchronize()
    return out, (g1, g2)


@pytest.mark.gpu
@pytest.mark.parametrize('patch', SC.PATCHES)
def test_choose_idx_at_every_patch_size(cpe, orc, gpu, patch):
    from cpe_amd import fit
    fallbacks = 0
    for th, names in _groups(patch).items():
        out, (g1, g2) = _select(fit, names, 0, patch, th)
        ch = _np(fit.choose_idx_batch(g1, g2, *SC.rig(), patch, th))
        torch.cuda.synchronize()
        for q in ('p1', 'p2', 'idx', 'm', 'flags'):                # the selecting half as an entry of its own: the same numbers
            assert np.array_equal(ch[q], out[q]), (patch, names, q)
        for i, name in enumerate(names):
            ref = _oracle(orc, 0, name, patch, th)
            _check_frame(orc, fit, out, i, ref, (name, patch))
            fallbacks += ref[3]
    assert fallbacks >= (1 if patch < 3 else 2)                     # all_bad at every size; from 3 on thin has no window


@pytest.mark.gpu
@pytest.mark.parametrize('selector', [1, 2])
def test_threshold_and_join_selectors(cpe, orc, gpu, selector):
    from cpe_amd import fit
    groups = collections.OrderedDict()
    for name in SC.CASE_NAMES:
        groups.setdefault(SC.threshold(name) if selector == 1 else 0.0, []).append(name)
    seen_fallback = False
    for th, names in groups.items():
        out, _ = _select(fit, names, selector, 3, th)
        for i, name in enumerate(names):
            ref = _oracle(orc, selector, name, 3, th)
            _check_frame(orc, fit, out, i, ref, (name, selector))
            seen_fallback |= ref[3]
    assert seen_fallback == (selector == 1)                         # all_bad: no pair below 0.3


@pytest.mark.gpu
@pytest.mark.parametrize('patch', [1, 3, 8])
def test_a_frame_does_not_depend_on_its_place(cpe, gpu, patch):
    """the frames in a mixed batch with poison padding, reversed with zero padding, and each alone: the same bytes"""
    from cpe_amd import fit
    for th, names in _groups(patch).items():
        def run(tabs):
            out = _np(fit.select_triangulate_batch(*tabs, *SC.rig(), selector=0, patch=patch, th=th))
            torch.cuda.synchronize()
            return out
        _three_ways(run, _frames(names), _table_batch)


@pytest.mark.gpu
@pytest.mark.parametrize('name,patch', SC.BOUNDARY)
def test_patch_threshold_is_strict(cpe, orc, gpu, name, patch):
    """th on the very double a window's mean is: rejected; on the next double: accepted"""
    from cpe_amd import fit
    th_equal, th_above, _ = SC.boundary(name, patch)
    only = {tuple(k) for k in SC.boundary_keys(name, patch)}
    got = {}
    for th in (th_equal, th_above):
        out, _ = _select(fit, [name], 0, patch, th)
        _check_frame(orc, fit, out, 0, _oracle(orc, 0, name, patch, th), (name, patch, th))
        m = int(out['m'][0])
        got[th] = (m, bool(int(out['flags'][0]) & fit.FLAG_FALLBACK), {tuple(k) for k in out['idx'][0, :m].tolist()})
    (m_eq, fb_eq, keys_eq), (m_ab, fb_ab, keys_ab) = got[th_equal], got[th_above]
    assert not fb_ab and only and only <= keys_ab
    if name.startswith('exact_'):
        assert fb_eq and m_eq == m_ab == patch * patch            # the join: as many, in table-1 order, and the flag
    else:
        assert not fb_eq and not only & keys_eq and keys_ab - keys_eq == only


@pytest.mark.gpu
def test_pair_threshold_is_strict(cpe, orc, gpu):
    from cpe_amd import fit
    name = SC.BOUNDARY_PAIR
    th_equal, th_above, key = SC.boundary_pair()
    keys = {}
    for th in (th_equal, th_above):
        out, _ = _select(fit, [name], 1, 3, th)
        _check_frame(orc, fit, out, 0, _oracle(orc, 1, name, 3, th), (name, th))
        keys[th] = [tuple(k) for k in out['idx'][0, :int(out['m'][0])].tolist()]
    assert key not in keys[th_equal] and key in keys[th_above]
    assert [k for k in keys[th_above] if k != key] == keys[th_equal]


@pytest.mark.gpu
@pytest.mark.parametrize('patch', [2, 5])
def test_patch_reaches_the_kernel_through_the_fit(cpe, orc, gpu, patch):
    """fit_single_cylinder_batch(patch=) selects what select_triangulate_batch does at that patch, which is not what patch 3
    selects (test_selector_cases_cpu.py::test_patch_sizes_are_told_apart)"""
    from cpe_amd import fit
    name = 'holes10'
    th = SC.threshold(name, patch)
    sel, (g1, g2) = _select(fit, [name], 0, patch, th)
    out = _np(fit.fit_single_cylinder_batch(g1, g2, *SC.rig(), R, patch=patch, th=th))
    torch.cuda.synchronize()
    for q in ('m', 'idx', 'flags', 'p1', 'p2', 'pts3'):
        assert np.array_equal(out[q], sel[q]), q
    _check_frame(orc, fit, out, 0, _oracle(orc, 0, name, patch, th), (name, patch))
    default = orc.choose_idx(SC.case(name).t1, SC.case(name).t2, *SC.rig(), 3, th)
    assert int(out['m'][0]) != len(default[0])


@pytest.mark.gpu
@pytest.mark.parametrize('patch', [0, 9, -1])
def test_patch_outside_1_to_8_is_refused(cpe, gpu, patch):
    from cpe_amd import fit
    L = cpe.lib.load()
    MAXP = fit.MAXP
    names = ['full', 'thin']
    n = len(names)
    g1, g2 = _table_batch(_frames(names), True)
    K1, K2, T21 = fit._cameras(*SC.rig(), gpu)
    nbytes = L.cpe_fit_workspace_bytes(n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=gpu)
    tabs = (g1.xy.data_ptr(), g1.id.data_ptr(), g1.cnt.data_ptr(), g2.xy.data_ptr(), g2.id.data_ptr(), g2.cnt.data_ptr(), n,
            K1.data_ptr(), K2.data_ptr(), T21.data_ptr())
    stream = torch.cuda.current_stream().cuda_stream

    def outputs():
        o = dict(p1=torch.empty((n, MAXP, 2), dtype=torch.float64, device=gpu), p2=torch.empty((n, MAXP, 2), dtype=torch.float64, device=gpu),
                 idx=torch.empty((n, MAXP, 2), dtype=torch.int32, device=gpu), X=torch.empty((n, MAXP, 3), dtype=torch.float64, device=gpu),
                 err=torch.empty((n, MAXP), dtype=torch.float64, device=gpu), m=torch.empty(n, dtype=torch.int32, device=gpu),
                 me=torch.empty(n, dtype=torch.float64, device=gpu), flags=torch.empty(n, dtype=torch.int32, device=gpu))
        for t in o.values():
            t.view(torch.uint8).fill_(0x5A)
        return o

    def untouched(o):
        torch.cuda.synchronize()
        return all(bool((t.view(torch.uint8) == 0x5A).all()) for t in o.values())

    o = outputs()
    rc = L.cpe_select_triangulate_batch(*tabs, 0, patch, 0.3, ws.data_ptr(), nbytes, o['p1'].data_ptr(), o['p2'].data_ptr(),
                                        o['idx'].data_ptr(), o['X'].data_ptr(), o['err'].data_ptr(), o['m'].data_ptr(),
                                        o['me'].data_ptr(), o['flags'].data_ptr(), stream)
    assert rc == cpe.lib.const.ERR_ARG
    assert 'cpe_select_triangulate_batch' in L.cpe_last_error_string().decode()
    assert untouched(o)
    o = outputs()
    rc = L.cpe_choose_idx_batch(*tabs, patch, 0.3, ws.data_ptr(), nbytes, o['p1'].data_ptr(), o['p2'].data_ptr(), o['idx'].data_ptr(),
                                o['m'].data_ptr(), o['flags'].data_ptr(), stream)
    assert rc == cpe.lib.const.ERR_ARG
    assert 'cpe_choose_idx_batch' in L.cpe_last_error_string().decode()
    assert untouched(o)
    # a valid call afterwards works: the refusal left nothing behind
    assert int(_np(fit.select_triangulate_batch(g1, g2, *SC.rig(), patch=1))['m'][0]) > 0
    with pytest.raises(cpe.lib.CpeError, match='cpe_select_triangulate_batch'):
        fit.select_triangulate_batch(g1, g2, *SC.rig(), patch=patch)
    with pytest.raises(cpe.lib.CpeError, match='cpe_choose_idx_batch'):
        fit.choose_idx_batch(g1, g2, *SC.rig(), patch, 0.3)
    with pytest.raises(cpe.lib.CpeError, match='patch must be 1..8'):
        fit.fit_single_cylinder_batch(g1, g2, *SC.rig(), R, patch=patch)
