"""The scenes of multiframe_cases.py keep their simplex path when sin / cos move by a few ulp.

The resident multi-frame fit calls the device math library where the oracle calls glibc, so its objective differs from the
oracle's in the last bits.  x and the iteration counts can be compared with the oracle bit for bit only on scenes where no
comparison of the simplex is that close.  This file establishes that on the CPU, before a scene is used on the GPU: fminsearch
(multiframe.nelder_mead6) from the oracle's initial pose, once with exact trig and 16 times with cos / sin each moved by a
random -4..+4 ulp (OpenCL's full-profile bound for f64 sin / cos; the ROCm documents at hand state no tighter one for ocml),
must take the same path to the same x.  A scene that fails is replaced by another seed in multiframe_cases.CASES."""
import numpy as np
import pytest

import multiframe_cases as mc

RUNS = 16


@pytest.fixture(scope='module')
def oracle_x0(orc):
    cache = {}

    def make(name):
        if name not in cache:
            cache[name] = compute(name)
        return cache[name]

    def compute(name):
        P, cnt, angles, _ = mc.case_scene(name)
        TAGV = np.stack([orc.get_TAGVcyl(*a) for a in angles])
        raw = np.zeros((len(cnt), 2, 6))
        for i in range(len(cnt)):
            r = orc.fit_cylinder(P[i, :cnt[i]], mc.RADIUS)
            raw[i, 0], raw[i, 1] = r['cyl0'], r['cyl']
        x0 = np.empty(6)
        import ctypes as C
        orc.lib().orc_multi_init(raw.ctypes.data_as(C.POINTER(C.c_double)), P.ctypes.data_as(C.POINTER(C.c_double)),
                                 cnt.ctypes.data_as(C.POINTER(C.c_int)), C.c_int(P.shape[1]),
                                 TAGV.ctypes.data_as(C.POINTER(C.c_double)), x0.ctypes.data_as(C.POINTER(C.c_double)))
        return P, cnt, TAGV, x0
    return make


def test_case_table():
    assert sorted(c['F'] for c in mc.CASES.values()) == [2, 3, 17, 33]
    assert sum(1 for c in mc.CASES.values() if c['noise'] == 0) == 1
    used = set()
    for c in mc.CASES.values():
        used |= set(mc.counts(c['F'], c['start']))
    assert used == set(mc.COUNT_CYCLE) == {5, 63, 64, 65, 160, 2048}


def test_numpy_objective_is_the_oracles(orc, oracle_x0):
    """the host objective used below is the oracle's up to summation order"""
    P, cnt, TAGV, x0 = oracle_x0('F3')
    for x in (x0, x0 + 0.01):
        want = orc.multi_objective(x, P, cnt, TAGV, mc.RADIUS)
        assert abs(mc.NumpyObjective(P, cnt, TAGV)(list(x)) - want) <= 1e-12 * want


def test_move_ulps():
    for v in (0.3, -0.3, 1.0):
        assert mc.move_ulps(v, 0) == v
        assert mc.move_ulps(v, 1) == np.nextafter(v, np.inf) and mc.move_ulps(v, -1) == np.nextafter(v, -np.inf)
        assert mc.move_ulps(v, 4) == np.nextafter(np.nextafter(np.nextafter(np.nextafter(v, np.inf), np.inf), np.inf), np.inf)


@pytest.mark.parametrize('name', sorted(mc.CASES))
def test_simplex_path_survives_trig_ulps(cpe, oracle_x0, name):
    from cpe_amd import multiframe
    P, cnt, TAGV, x0 = oracle_x0(name)
    x, f, iters, evals = multiframe.nelder_mead6(mc.NumpyObjective(P, cnt, TAGV), list(x0))
    assert np.isfinite(f) and iters > 10
    fs = [f]
    for run in range(RUNS):
        rng = np.random.default_rng(1000 + run)
        xr, fr, ir, er = multiframe.nelder_mead6(mc.NumpyObjective(P, cnt, TAGV, rng=rng), list(x0))
        assert (ir, er) == (iters, evals), f'{name}: run {run} left the iteration path ({ir}, {er}) != ({iters}, {evals})'
        assert xr == x, f'{name}: run {run} ended in another x'
        fs.append(fr)
    spread = (max(fs) - min(fs)) / abs(f)
    print(f'{name}: iters {iters} evals {evals} f {f!r} relative spread of f {spread:.3g}')
    assert spread <= 1e-13
