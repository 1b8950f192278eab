"""The plumbing of the one-camera repair without a GPU and without the library: `repair` travels through FramePipeline's table=
to fit.fit_single_cylinder_mono_repaired_batch, run_experiment refuses it for the sources that have two tables, and
pipeline.MONO_REPAIR_OUTPUTS names what run_raw can keep."""
import numpy as np
import pytest
import torch

import cpe_amd  # noqa: F401
from cpe_amd import experiment, fit, pipeline

I32 = torch.int32


def _table():
    return fit.LaserTable(torch.zeros((2, 3, 4), dtype=torch.float64), torch.zeros((2, 3), dtype=I32), -1, 1,
                          torch.zeros(4, dtype=torch.float64), torch.zeros(1, dtype=I32))


def _pipe(source, **kw):
    K = np.eye(3)
    return pipeline.FramePipeline(480, 640, K, 2 * K, np.eye(4), 45.0, chunk=2, device='cpu', source=source, laser_table=_table(),
                                  fit_mode=fit.FIT_LM, **kw)


@pytest.fixture
def calls(monkeypatch):
    seen = []
    monkeypatch.setattr(fit, 'fit_single_cylinder_mono_batch', lambda *a, **kw: seen.append(('plain', a, kw)) or 'plain')
    monkeypatch.setattr(fit, 'fit_single_cylinder_mono_repaired_batch', lambda *a, **kw: seen.append(('repaired', a, kw)) or 'repaired')
    return seen


def test_without_repair_the_plain_call_gets_the_table_keywords(calls):
    p = _pipe('left', table=dict(need_both=True, max_res=0.3))
    assert pipeline._fit_mono(p, 'g1', None, None, 0) == 'plain'
    (which, a, kw), = calls
    assert which == 'plain' and a[0] == 'g1' and a[2] is None and kw == dict(ransac=None, mode=fit.FIT_LM, need_both=True, max_res=0.3)
    assert p.table == dict(need_both=True, max_res=0.3)


@pytest.mark.parametrize('source, cam', [('left', 1), ('right', 2)])
def test_repair_travels_through_table(calls, source, cam):
    p = _pipe(source, table=dict(repair={}))
    g = ('g1', None) if cam == 1 else (None, 'g2')
    assert pipeline._fit_mono(p, g[0], g[1], None, 0) == 'repaired'
    (which, a, kw), = calls
    assert which == 'repaired' and a[0] == f'g{cam}' and a[1] == cam and a[2] is p.K1 and a[3] is p.K2 and a[4] is p.T21
    assert a[5] is p.laser_table and a[6] == 45.0
    assert kw == dict(shift={}, image_size=(480, 640), mode=fit.FIT_LM), 'the defaults: the search on, the frame\'s size, the fit mode'
    assert p.table == dict(repair={}), 'the pipeline keeps its options: a second chunk finds them again'
    assert p.mode == ('mono left' if cam == 1 else 'mono right')


def test_repair_keywords_override_and_max_res_goes_along(calls):
    p = _pipe('left', table=dict(max_res=0.4, repair=dict(shift=dict(win=(2, 2)), rounds=2, image_size=None, mode=fit.FIT_NELDER_MEAD)))
    pipeline._fit_mono(p, 'g1', None, None, 0)
    assert calls[0][2] == dict(shift=dict(win=(2, 2)), rounds=2, image_size=None, mode=fit.FIT_NELDER_MEAD, max_res=0.4)


def test_repair_refuses_ransac(calls):
    p = _pipe('left', table=dict(repair={}), ransac=dict(hypotheses=8))
    with pytest.raises(ValueError, match='ransac does not apply'):
        pipeline._fit_mono(p, 'g1', None, None, 0)
    assert not calls


@pytest.mark.parametrize('source', ['stereo', 'fused'])
def test_run_experiment_refuses_repair_for_two_tables(source, tmp_path):
    with pytest.raises(ValueError, match="repair= .* source must be 'left' or 'right'"):
        experiment.run_experiment(str(tmp_path), None, np.eye(3), np.eye(3), np.eye(4), source=source, repair={})


def test_repair_is_the_last_keyword_of_run_experiment():
    import inspect
    prm = list(inspect.signature(experiment.run_experiment).parameters.values())
    assert prm[-1].name == 'repair' and prm[-1].default is None


def test_mono_repair_outputs():
    assert pipeline.MONO_REPAIR_OUTPUTS == dict(shift=((2,), I32), shift_flags=((), I32), shift_score=((4,), I32), round_taken=((), I32),
                                                renumbered=((), I32))
    assert not set(pipeline.MONO_REPAIR_OUTPUTS) & set(pipeline.MONO_FIT_OUTPUTS), 'they are added to the mono outputs, not part of them'
    f = pipeline.alloc_fits(3, 'cpu', source='left')
    assert set(f) == set(pipeline.MONO_FIT_OUTPUTS), 'alloc_fits is unchanged: the caller adds the repair outputs it wants kept'


def test_repair_listing():
    names = ['a', 'b', 'c', 'd']
    got = experiment.repair_listing(names, torch.tensor([[0, 0], [-1, 0], [0, 0], [0, 0]], dtype=I32), torch.tensor([0, 1, 2, 0], dtype=I32),
                                    torch.tensor([1, 1, 0, 1], dtype=I32), torch.tensor([0, 0, 0, 3], dtype=I32))
    assert got == [dict(index=1, name='b', shift=(-1, 0), flags=1, round=1, renumbered=0),
                   dict(index=2, name='c', shift=(0, 0), flags=2, round=0, renumbered=0),
                   dict(index=3, name='d', shift=(0, 0), flags=0, round=1, renumbered=3)]


def test_the_repaired_call_refuses_what_does_not_apply():
    gp = fit.GridTables(torch.zeros((1, fit.MAXP, 2), dtype=torch.float64), torch.zeros((1, fit.MAXP, 2), dtype=I32), torch.zeros(1, dtype=I32))
    K = np.eye(3)
    for kw, text in ((dict(rounds=-1), 'rounds < 0'), (dict(need_both=False), 'need_both does not apply'), (dict(ransac={}), 'ransac does not'),
                     (dict(min_sin=0.1), 'min_sin does not apply'), (dict(rms_ratio=0.5), 'rms_ratio >= 1')):
        with pytest.raises(ValueError, match=text):
            fit.fit_single_cylinder_mono_repaired_batch(gp, 1, K, K, np.eye(4), _table(), 45.0, **kw)
    with pytest.raises(ValueError, match='cam is 1 or 2'):
        fit.fit_single_cylinder_mono_repaired_batch(gp, 3, K, K, np.eye(4), _table(), 45.0)
