"""The curvature calls in front of the library, without a GPU: the header declares them and parses into the argument types the
binding passes (k, mode and the gate are plain arguments, so there is no structure whose layout could differ), and the Python
wrappers refuse bad arguments before the library is loaded."""
import ctypes as C
import math
import re

import pytest
import torch

import cpe_amd  # noqa: F401
from cpe_amd import fit
from cpe_amd import lib as _lib

MAXP = _lib.MAXP
F64, I32, U8 = torch.float64, torch.int32, torch.uint8


def test_header_declares_the_calls_and_the_version():
    names = _lib.declared_symbols()
    assert 'cpe_est_curvatures_batch' in names and 'cpe_curvature_consensus_batch' in names
    hdr = open(_lib.HEADER_PATH).read()
    assert int(re.search(r'#define CPE_VERSION (\d+)', hdr).group(1)) >= 128
    assert '128: cpe_est_curvatures_batch, cpe_curvature_consensus_batch' in hdr
    P, I, D = C.c_void_p, C.c_int32, C.c_double
    assert _lib._SIGS['cpe_est_curvatures_batch'] == (I, [P, P, I, I, I, P, P, P, P, P, P, P])
    assert _lib._SIGS['cpe_curvature_consensus_batch'] == (I, [P, P, I, P, P, P, P, D, D, D, P, P, P, P, P])


def test_constants():
    c = _lib.const
    assert (c.CURV_REFERENCE, c.CURV_INTERCEPT, c.CURV_MAXK, c.CURV_K) == (0, 1, 32, 20)
    assert (fit.CURV_REFERENCE, fit.CURV_INTERCEPT, fit.CURV_MAXK) == (0, 1, 32)
    assert not any(name.startswith('CpeCurv') for name in _lib._STRUCTS)


@pytest.fixture
def no_library(monkeypatch):
    def boom():
        raise AssertionError('the library was loaded before the arguments were checked')
    monkeypatch.setattr(_lib, 'load', boom)


def _pts(n=2, dtype=F64, shape=None):
    return torch.zeros(shape or (n, MAXP, 3), dtype=dtype), torch.zeros(n, dtype=I32)


def test_est_curvatures_refuses_bad_tensors(no_library):
    X, cnt = _pts()
    with pytest.raises(TypeError) as e:
        fit.est_curvatures_batch(X.float(), cnt)
    assert str(e.value) == f'est_curvatures_batch: pts3 must be torch.float64 [2, {MAXP}, 3] on cpu, got torch.float32 [2, {MAXP}, 3] on cpu'
    with pytest.raises(TypeError) as e:
        fit.est_curvatures_batch(X[:, :100], cnt)
    assert str(e.value) == f'est_curvatures_batch: pts3 must be torch.float64 [2, {MAXP}, 3] on cpu, got torch.float64 [2, 100, 3] on cpu'
    with pytest.raises(TypeError) as e:
        fit.est_curvatures_batch(X, cnt.long())
    assert str(e.value) == 'est_curvatures_batch: cnt must be torch.int32 [2] on cpu, got torch.int64 [2] on cpu'
    with pytest.raises(TypeError) as e:
        fit.est_curvatures_batch(X, cnt.to('meta'))
    assert str(e.value) == 'est_curvatures_batch: cnt must be torch.int32 [2] on cpu, got torch.int32 [2] on meta'
    with pytest.raises(TypeError):
        fit.est_curvatures_batch(X, [3, 4])


@pytest.mark.parametrize('k,mode,text', [
    (4, 0, 'est_curvatures_batch: k 4 must be 5..32 in mode 0'), (5, 1, 'est_curvatures_batch: k 5 must be 6..32 in mode 1'),
    (33, 0, 'est_curvatures_batch: k 33 must be 5..32 in mode 0'), (20.5, 1, 'est_curvatures_batch: k 20.5 must be 6..32 in mode 1'),
    (20, 2, 'est_curvatures_batch: mode 2 must be CURV_REFERENCE (0) or CURV_INTERCEPT (1)')])
def test_est_curvatures_refuses_bad_k_and_mode(no_library, k, mode, text):
    X, cnt = _pts()
    with pytest.raises(ValueError) as e:
        fit.est_curvatures_batch(X, cnt, k=k, mode=mode)
    assert str(e.value) == text


def _curv(n=2):
    return dict(Kdir=torch.zeros((n, MAXP, 2, 3), dtype=F64), L=torch.zeros((n, MAXP, 2), dtype=F64),
                normal=torch.zeros((n, MAXP, 3), dtype=F64), pt_status=torch.zeros((n, MAXP), dtype=U8))


def test_consensus_refuses_bad_tensors_and_gates(no_library):
    X, cnt = _pts()
    cv = _curv()
    cv['L'] = cv['L'].float()
    with pytest.raises(TypeError) as e:
        fit.curvature_consensus_batch(X, cnt, cv)
    assert str(e.value) == (f"curvature_consensus_batch: curv['L'] must be torch.float64 [2, {MAXP}, 2] on cpu, "
                            f"got torch.float32 [2, {MAXP}, 2] on cpu")
    cv = _curv(3)
    with pytest.raises(TypeError) as e:
        fit.curvature_consensus_batch(X, cnt, cv)
    assert "curv['Kdir'] must be torch.float64 [2, " in str(e.value)
    for bad in (dict(rho_max=-1.0), dict(r_min=-1.0), dict(r_min=50.0, r_max=50.0), dict(rho_max=math.nan), dict(r_max=math.nan)):
        with pytest.raises(ValueError) as e:
            fit.curvature_consensus_batch(X, cnt, _curv(), **bad)
        assert str(e.value).startswith('curvature_consensus_batch: rho_max ')


def test_gated_fit_and_experiment_options(no_library):
    assert fit._curvature_options('x', None, 45.0) == (20, fit.CURV_INTERCEPT, 0.25, 45.0 * (1 - 1 / 3), 45.0 * (1 + 1 / 3))
    assert fit._curvature_options('x', dict(k=12, mode=0, band=0.5, r_max=70.0), 40.0) == (12, 0, 0.25, 20.0, 70.0)
    with pytest.raises(ValueError) as e:
        fit._curvature_options('fit_single_cylinder_gated_batch', dict(kk=3), 45.0)
    assert str(e.value) == "fit_single_cylinder_gated_batch: unknown curvature options ['kk']"
    g = fit.GridTables(torch.zeros((1, MAXP, 2), dtype=F64), torch.zeros((1, MAXP, 2), dtype=I32), torch.zeros(1, dtype=I32))
    with pytest.raises(ValueError) as e:
        fit.fit_single_cylinder_gated_batch(g, g, None, None, None, 45.0, curvature=dict(k=40))
    assert str(e.value) == 'fit_single_cylinder_gated_batch: k 40 must be 6..32 in mode 1'


def test_compact_gated_keeps_table_order_and_zeroes_the_rest():
    X = torch.arange(2 * 6 * 3, dtype=F64).reshape(2, 6, 3)
    X[0, 0] = math.nan                                           # a slot that is not gated in may hold anything
    gate = torch.tensor([[0, 1, 1, 0, 1, 0], [1, 1, 1, 1, 1, 1]], dtype=U8)
    kept, m = fit.compact_gated(X, gate)
    assert m.dtype == I32 and m.tolist() == [3, 6]
    assert torch.equal(kept[0, :3], X[0, [1, 2, 4]]) and not kept[0, 3:].any()
    assert torch.equal(kept[1], X[1])                            # all gated in: the table as it stands
