"""The call plumbing in front of the fit kernels, without a GPU and without the library: the slab carver of fit.py, its
table and line-count checks, the output specs of pipeline.py and the table of modes FramePipeline's options resolve to.
The expected error texts and dicts are literal copies of what the code held before these pieces were shared."""
import itertools

import pytest
import torch

import cpe_amd  # noqa: F401
from cpe_amd import fit, pipeline
from cpe_amd import lib as _lib

MAXP, MAXL = fit.MAXP, _lib.MAXL
F64, I32, U8 = torch.float64, torch.int32, torch.uint8
SHAPES = [('a', ()), ('b', (2,)), ('c', (MAXP, 3)), ('d', (2, 2, 4)), ('e', ())]


@pytest.mark.parametrize('dtype', [F64, I32])
@pytest.mark.parametrize('zero', [True, False])
@pytest.mark.parametrize('n', [0, 1, 3, None])
def test_slab_views_are_contiguous_ordered_disjoint_and_cover_the_allocation(dtype, zero, n):
    fields = SHAPES if n is not None else [('P', (2, 5, 4)), ('centre', (4,)), ('one', (1,))]
    views = fit._slab(torch.device('cpu'), dtype, zero, n, fields)
    assert list(views) == [name for name, _ in fields]
    at, total = None, 0
    for (name, shape), v in zip(fields, views.values()):
        assert v.dtype == dtype and v.is_contiguous(), name
        assert tuple(v.shape) == (() if n is None else (n,)) + shape, name
        total += v.numel() * v.element_size()
        if v.numel():
            assert at is None or v.data_ptr() == at, f'{name} does not start where the view before it ends'
            at = v.data_ptr() + v.numel() * v.element_size()
            if zero:
                assert not v.any(), name
    first = next(iter(views.values()))
    assert first.untyped_storage().nbytes() == total, 'the views do not cover the allocation exactly'
    assert all(v.untyped_storage().data_ptr() == first.untyped_storage().data_ptr() for v in views.values()), 'more than one allocation'
    if total:
        assert next(v for v in views.values() if v.numel()).data_ptr() == first.untyped_storage().data_ptr()
    for k, v in enumerate(views.values()):
        v.fill_(k + 1)
    for k, (name, v) in enumerate(views.items()):
        assert bool((v == k + 1).all()), f'a write through another view reached {name}'


def _tables(n=2, dev='cpu'):
    return fit.GridTables(torch.zeros((n, MAXP, 2), dtype=F64, device=dev), torch.zeros((n, MAXP, 2), dtype=I32, device=dev),
                          torch.zeros(n, dtype=I32, device=dev))


def test_check_tables_accepts_good_tables():
    fit._check_tables('x', _tables())
    fit._check_tables('x', _tables(0))
    fit._check_tables('x', _tables(3), 3, 'gp2.', torch.device('cpu'))


@pytest.mark.parametrize('what', ['grid_relabel_batch', 'table_triangulate_batch', 'grid_assign_batch'])
def test_check_tables_refuses_dtype_shape_and_device_with_the_callers_texts(what):
    g = _tables()
    g.xy = g.xy.float()
    with pytest.raises(TypeError) as e:
        fit._check_tables(what, g)
    assert str(e.value) == f'{what}: xy must be torch.float64 [2, {MAXP}, 2] on cpu, got torch.float32 [2, {MAXP}, 2] on cpu'
    g = _tables()
    g.id = torch.zeros((2, MAXP, 3), dtype=I32)
    with pytest.raises(TypeError) as e:
        fit._check_tables(what, g)
    assert str(e.value) == f'{what}: id must be torch.int32 [2, {MAXP}, 2] on cpu, got torch.int32 [2, {MAXP}, 3] on cpu'
    g = _tables()
    g.cnt = g.cnt.to('meta')
    with pytest.raises(TypeError) as e:
        fit._check_tables(what, g)
    assert str(e.value) == f'{what}: cnt must be torch.int32 [2] on cpu, got torch.int32 [2] on meta'
    g = _tables()
    g.cnt = g.cnt.long()
    with pytest.raises(TypeError) as e:
        fit._check_tables(what, g)
    assert str(e.value) == f'{what}: cnt must be torch.int32 [2] on cpu, got torch.int64 [2] on cpu'


def test_check_tables_of_the_fused_call_names_the_table_and_holds_both_to_the_first():
    cpu = torch.device('cpu')
    g = _tables()
    g.id = g.id.long()
    with pytest.raises(TypeError) as e:
        fit._check_tables('fused_triangulate_batch', g, 2, 'gp1.', cpu)
    assert str(e.value) == (f'fused_triangulate_batch: gp1.id must be torch.int32 [2, {MAXP}, 2] on cpu, got torch.int64 '
                            f'[2, {MAXP}, 2] on cpu')
    with pytest.raises(TypeError) as e:                   # table 2 with another frame count than table 1
        fit._check_tables('fused_triangulate_batch', _tables(3), 2, 'gp2.', cpu)
    assert str(e.value) == (f'fused_triangulate_batch: gp2.xy must be torch.float64 [2, {MAXP}, 2] on cpu, got torch.float64 '
                            f'[3, {MAXP}, 2] on cpu')
    with pytest.raises(TypeError) as e:                   # table 2 wholly on another device than table 1
        fit._check_tables('fused_triangulate_batch', _tables(2, 'meta'), 2, 'gp2.', cpu)
    assert str(e.value) == (f'fused_triangulate_batch: gp2.xy must be torch.float64 [2, {MAXP}, 2] on cpu, got torch.float64 '
                            f'[2, {MAXP}, 2] on meta')


@pytest.mark.parametrize('what', ['index_planes_batch', 'fit_projector_model', 'ProjectorModel.table', 'LaserTable'])
def test_line_count_is_one_to_maxl(what):
    assert fit._line_count(what, 3, 3) == 1
    assert fit._line_count(what, -4, MAXL - 5) == MAXL
    assert fit._line_count(what, '-1', 1.0) == 3          # as the callers' int(lo), int(hi)
    with pytest.raises(ValueError) as e:
        fit._line_count(what, 3, 2)
    assert str(e.value) == f'{what}: 0 indices in [3, 2], must be 1..{MAXL}'
    with pytest.raises(ValueError) as e:
        fit._line_count(what, 0, MAXL)
    assert str(e.value) == f'{what}: {MAXL + 1} indices in [0, {MAXL}], must be 1..{MAXL}'


def test_laser_table_still_checks_its_range_and_shapes():
    z = lambda *s: torch.zeros(s, dtype=F64)
    with pytest.raises(ValueError) as e:
        fit.LaserTable(z(2, 1, 4), torch.zeros((2, 1), dtype=I32), 0, MAXL, z(4), torch.zeros(1, dtype=I32))
    assert str(e.value) == f'LaserTable: {MAXL + 1} indices in [0, {MAXL}], must be 1..{MAXL}'
    with pytest.raises(ValueError) as e:
        fit.LaserTable(z(2, 2, 4), torch.zeros((2, 3), dtype=I32), -1, 1, z(4), torch.zeros(1, dtype=I32))
    assert str(e.value) == 'LaserTable: P must be [2,3,4] and status [2,3], got [2, 2, 4] and [2, 3]'


def test_ptr_is_null_for_none_and_for_empty_tensors():
    t = torch.zeros(3)
    assert fit._ptr(None) is None and fit._ptr(torch.zeros((0, 4))) is None and fit._ptr(t) == t.data_ptr()


# ---- pipeline.py: the output specs, literally as they were written out before they were built from a common core ----
EXPECTED = dict(
    FIT_OUTPUTS=dict(pts3=((MAXP, 3), F64), m=((), I32), cyl_raw=((2, 6), F64), cyl=((2, 6), F64), T=((4, 4), F64), fvals=((2,), F64),
                     mean_err=((), F64), status=((), I32), offset=((2,), I32), match_score=((4,), I32), match_flags=((), I32)),
    PLANE_FIT_OUTPUTS=dict(pts3=((MAXP, 3), F64), idx=((MAXP, 2), I32), m=((), I32), P=((4,), F64), T=((4, 4), F64), grid=((3, 3), F64),
                           stats=((8,), F64), n_inliers=((), I32), inlier_mask=((MAXP,), U8), plane_flags=((), I32), mean_err=((), F64),
                           status=((), I32)),
    RELABEL_OUTPUTS=dict(relabel_counts=((2, 2, 4), I32), relabel_flags=((2,), I32)),
    MONO_FIT_OUTPUTS=dict(pts3=((MAXP, 3), F64), idx=((MAXP, 2), I32), m=((), I32), cyl_raw=((2, 6), F64), cyl=((2, 6), F64),
                          T=((4, 4), F64), fvals=((2,), F64), mean_err=((), F64), status=((), I32), counts=((4,), I32),
                          res=((MAXP, 2), F64), src=((MAXP, 2), I32), stats=((2,), F64)),
    FUSED_FIT_OUTPUTS=dict(pts3=((MAXP, 3), F64), idx=((MAXP, 2), I32), m=((), I32), cyl_raw=((2, 6), F64), cyl=((2, 6), F64),
                           T=((4, 4), F64), fvals=((2,), F64), mean_err=((), F64), status=((), I32), counts=((6,), I32),
                           res=((MAXP, 4), F64), src=((MAXP, 3), I32), stats=((4,), F64), flags=((), I32)),
    REFINED_FIT_OUTPUTS=dict(pts3=((MAXP, 3), F64), idx=((MAXP, 2), I32), m=((), I32), cyl_raw=((2, 6), F64), cyl=((2, 6), F64),
                             T=((4, 4), F64), fvals=((2,), F64), mean_err=((), F64), status=((), I32), round_taken=((), I32),
                             renumbered=((2,), I32)))


@pytest.mark.parametrize('name', list(EXPECTED))
def test_output_specs_are_what_they_were(name):
    assert list(getattr(pipeline, name).items()) == list(EXPECTED[name].items())


def _spec_before(target, source, refine):
    """alloc_fits' choice as it was written with nested conditionals"""
    if source == 'fused':
        return 'REFINED_FIT_OUTPUTS' if refine else 'FUSED_FIT_OUTPUTS'
    return dict(cylinder='FIT_OUTPUTS', plane='PLANE_FIT_OUTPUTS')[target] if source == 'stereo' else 'MONO_FIT_OUTPUTS'


@pytest.mark.parametrize('target, source, refine', list(itertools.product(('cylinder', 'plane'), ('stereo', 'left', 'right', 'fused'),
                                                                          (False, True))))
def test_alloc_fits_is_a_lookup_of_the_same_spec(target, source, refine):
    spec = EXPECTED[_spec_before(target, source, refine)]
    got = pipeline.alloc_fits(2, 'cpu', target, source, refine)
    assert list(got) == list(spec)
    for k, (shape, dt) in spec.items():
        assert tuple(got[k].shape) == (2,) + shape and got[k].dtype == dt and got[k].device.type == 'cpu' and not got[k].any(), k
    if not refine:
        assert list(pipeline.alloc_fits(2, 'cpu', target, source)) == list(spec)
    if source == 'stereo' and not refine and target == 'cylinder':
        assert list(pipeline.alloc_fits(2, 'cpu')) == list(spec)


# ---- pipeline.py: the options FramePipeline refuses, in the order its constructor looked at them, and the mode of the rest ----
def _laser_table(lo=-1, hi=1):
    L = hi - lo + 1
    return fit.LaserTable(torch.zeros((2, L, 4), dtype=F64), torch.zeros((2, L), dtype=I32), lo, hi, torch.zeros(4, dtype=F64),
                          torch.zeros(1, dtype=I32))


def _pipe(**kw):
    return pipeline.FramePipeline(480, 640, torch.eye(3), torch.eye(3), torch.eye(4), 45.0, device='cpu', **kw)


PLANE_CYL = "target='plane': match and ransac score with the cylinder's radius and do not apply (radius is not read)"
RELABEL = ("relabel= re-labels straight grid lines: target='plane' only (the cylinder's lines are curved, and the cylinder script "
           "numbers them differently)")
ONE_CAMERA = "laser_table= and table= belong to one camera: source='left' or 'right'"
REFINE_SOURCE = "refine= re-numbers against the laser-plane table and fits fused points: source='fused' only"
LT = 'a small table'
REFUSED = [
    (dict(stage='fit'), "stage is 'full' or 'detect'"),
    (dict(stage='fit', target='board', source='both'), "stage is 'full' or 'detect'"),
    (dict(target='board'), "target is 'cylinder' or 'plane'"),
    (dict(target='plane', match={}), PLANE_CYL),
    (dict(target='plane', ransac={}), PLANE_CYL),
    (dict(target='plane', ransac={}, source='left'), PLANE_CYL),
    (dict(plane={}), "plane= holds keywords of the planar fit: target='plane' only"),
    (dict(plane=dict(tau=1.0), relabel={}), "plane= holds keywords of the planar fit: target='plane' only"),
    (dict(relabel={}), RELABEL),
    (dict(relabel={}, source='fused', laser_table=LT), RELABEL),
    (dict(source='both'), "source is 'stereo', 'left', 'right' or 'fused'"),
    (dict(laser_table=LT), ONE_CAMERA),
    (dict(table={}), ONE_CAMERA),
    (dict(target='plane', laser_table=LT), ONE_CAMERA),
    (dict(source='left'), "source='left' needs laser_table= (a fit.LaserTable): one camera has no other way to a 3-D point"),
    (dict(source='right', table={}), "source='right' needs laser_table= (a fit.LaserTable): one camera has no other way to a 3-D point"),
    (dict(source='fused'), "source='fused' needs laser_table= (a fit.LaserTable)"),
    (dict(source='fused', refine={}), "source='fused' needs laser_table= (a fit.LaserTable)"),
    (dict(source='left', laser_table=LT, match={}), "source='left': match searches the index shift between two tables, there is one"),
    (dict(source='right', laser_table=LT, match={}), "source='right': match searches the index shift between two tables, there is one"),
    (dict(source='fused', laser_table=LT, match={}),
     "source='fused': match feeds the stereo selector; repair the numbering first (fit.match_offset_batch)"),
    (dict(source='left', laser_table=LT, target='plane'),
     "source='left': target='plane' builds the table from stereo points and does not read one"),
    (dict(source='fused', laser_table=LT, target='plane', stage='detect'),
     "source='fused': target='plane' builds the table from stereo points and does not read one"),
    (dict(source='right', laser_table=LT, stage='detect'), "source='right': stage='detect' ends at the stereo selector"),
    (dict(source='fused', laser_table=LT, stage='detect'), "source='fused': stage='detect' ends at the stereo selector"),
    (dict(refine={}), REFINE_SOURCE),
    (dict(refine={}, target='plane'), REFINE_SOURCE),
    (dict(refine={}, source='left', laser_table=LT), REFINE_SOURCE),
    (dict(refine={}, source='fused', laser_table=LT, ransac={}), 'refine= fits every round with fit_cylinder_batch: ransac does not apply'),
]


@pytest.mark.parametrize('kw, text', REFUSED)
def test_refused_options_keep_their_type_and_text(kw, text):
    kw = {k: _laser_table() if v is LT else v for k, v in kw.items()}
    with pytest.raises(ValueError) as e:
        _pipe(**kw)
    assert type(e.value) is ValueError and str(e.value) == text


def test_refine_refuses_a_table_with_more_nodes_than_one_prediction_holds():
    half = (MAXL - 1) // 2
    nodes = (2 * half + 1) ** 2
    assert nodes > fit.PRED_MAXN, 'the largest table fits one prediction: this refusal cannot occur'
    with pytest.raises(ValueError) as e:
        _pipe(source='fused', laser_table=_laser_table(-half, half), refine={})
    assert str(e.value) == f'refine=: the table holds {nodes} nodes, more than {fit.PRED_MAXN}: give window='
    p = _pipe(source='fused', laser_table=_laser_table(-half, half), refine=dict(window=((-2, 2), (-2, 2))))
    assert p.mode == 'fused refined'


ACCEPTED = [
    (dict(), 'stereo cylinder'),
    (dict(match={}, ransac=dict(hypotheses=8), fit_mode=fit.FIT_LM, lanes=2), 'stereo cylinder'),
    (dict(stage='detect'), 'stereo detect-only'),
    (dict(stage='detect', match={}), 'stereo detect-only'),
    (dict(stage='detect', target='plane'), 'stereo detect-only'),
    (dict(target='plane'), 'stereo plane'),
    (dict(target='plane', plane=dict(tau=1.0), relabel={}), 'stereo plane'),
    (dict(source='left', laser_table=LT), 'mono left'),
    (dict(source='right', laser_table=LT, table=dict(max_res=0.5), ransac={}), 'mono right'),
    (dict(source='fused', laser_table=LT), 'fused'),
    (dict(source='fused', laser_table=LT, ransac={}, table=dict(max_res=0.5)), 'fused'),
    (dict(source='fused', laser_table=LT, refine={}), 'fused refined'),
    (dict(source='fused', laser_table=LT, refine=dict(rounds=1), table=dict(max_px=2.0)), 'fused refined'),
]


@pytest.mark.parametrize('kw, mode', ACCEPTED)
def test_accepted_options_resolve_to_their_mode(kw, mode):
    kw = {k: _laser_table() if v is LT else v for k, v in kw.items()}
    p = _pipe(**kw)
    assert p.mode == mode and p.mode in pipeline._MODES
    assert (p.laser_table is None) == ('laser_table' not in kw)
    if 'refine' in kw:                                    # the defaults the constructor adds, the caller's keywords on top
        assert p.refine == dict(dict(image_size=(480, 640), first=dict(selector=fit.SEL_CHOOSE_IDX, th=0.3, mode=p.fit_mode)), **kw['refine'])
    else:
        assert p.refine is None


def test_the_mode_table_names_cameras_fit_record_and_outputs():
    M = pipeline._MODES
    assert list(M) == ['stereo cylinder', 'stereo detect-only', 'stereo plane', 'mono left', 'mono right', 'fused', 'fused refined']
    assert [m.cameras for m in M.values()] == ['LR', 'LR', 'LR', 'L', 'R', 'LR', 'LR']
    assert [m.outputs for m in M.values()] == [pipeline.FIT_OUTPUTS, None, pipeline.PLANE_FIT_OUTPUTS, pipeline.MONO_FIT_OUTPUTS,
                                               pipeline.MONO_FIT_OUTPUTS, pipeline.FUSED_FIT_OUTPUTS, pipeline.REFINED_FIT_OUTPUTS]
    plane = [name for name, m in M.items() if m.record is pipeline._plane_record]
    assert plane == ['stereo plane'] and all(m.record is pipeline._cylinder_record for name, m in M.items() if name != 'stereo plane')
    assert len({m.fit for m in M.values()}) == 6          # the two one-camera modes share theirs


def test_split_detect_covers_interleaved_concatenated_and_one_camera():
    c = 3
    det = dict(xy=torch.arange(2 * c * MAXP * 2, dtype=F64).view(2 * c, MAXP, 2), id=torch.arange(2 * c * MAXP * 2, dtype=I32).view(2 * c, MAXP, 2),
               n=torch.arange(2 * c, dtype=I32), status=torch.arange(2 * c, dtype=I32) % 3, center=torch.arange(4 * c, dtype=F64).view(2 * c, 2))
    for inter, (a, b) in ((True, (slice(0, None, 2), slice(1, None, 2))), (False, (slice(None, c), slice(c, None)))):
        g1, g2, st_l, st_r, (c1, c2) = pipeline._split_detect(det, 'LR', inter)
        for g, s, st, ctr in ((g1, a, st_l, c1), (g2, b, st_r, c2)):
            assert torch.equal(g.xy, det['xy'][s]) and torch.equal(g.id, det['id'][s]) and torch.equal(g.cnt, det['n'][s])
            assert g.xy.is_contiguous() and g.id.is_contiguous() and g.cnt.is_contiguous() and ctr.is_contiguous()
            assert torch.equal(st, det['status'][s]) and torch.equal(ctr, det['center'][s])
        if not inter:                                     # concatenated: views, no copy
            assert g1.xy.data_ptr() == det['xy'].data_ptr() and g2.xy.data_ptr() == det['xy'][c:].data_ptr()
    g1, g2, st_l, st_r, (c1, c2) = pipeline._split_detect(det, 'L')
    assert g2 is None and c2 is None and g1.xy.data_ptr() == det['xy'].data_ptr() and torch.equal(g1.cnt, det['n'])
    assert torch.equal(st_l, det['status']) and not st_r.any() and st_r.shape == st_l.shape and st_r.dtype == st_l.dtype
    g1, g2, st_l, st_r, (c1, c2) = pipeline._split_detect(det, 'R')
    assert g1 is None and c1 is None and g2.id.data_ptr() == det['id'].data_ptr() and torch.equal(c2, det['center'])
    assert torch.equal(st_r, det['status']) and not st_l.any()
