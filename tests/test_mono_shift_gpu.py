"""cpe_mono_shift_batch (csrc/fit.hip k_mono_vote, k_mono_pick) against the numpy reference of tests/mono_shift_cases.py.

Every case's margin is > 1e-6 (tests/test_mono_shift_cases_cpu.py), so scores, cand, cand_score, score and flags are compared
exactly; rms at (2 m + 18) eps rms.  The C entry point is called with every output filled with poison first: what the call leaves
untouched shows."""
import numpy as np
import pytest
import torch

import mono_shift_cases as MC
import table_tri_cases as TC

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A
KEYS = MC.INT_KEYS + ('rms',)


def _raw(cpe, gpu, xy, I, cnt, cam, table, win=(4, 4), tau=0.1, min_sin=0.01, min_score=8, swap=0, top_k=4, lo=None, hi=None,
         alias=None):
    """the C call on poisoned outputs -> rc, dict of numpy arrays.  alias: (output name, input name): that output is the input"""
    t = lambda a, dt=None: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(gpu)
    n = len(cnt)
    K, Tc = TC.camera(cam)
    ins = dict(xy=t(xy), id=t(I), cnt=t(cnt), K=t(K, np.float64).reshape(9), Tc=None if Tc is None else t(Tc, np.float64).reshape(16),
               P=t(table['P'], np.float64), status=t(table['status'], np.int32))
    ncand = (2 * abs(win[0]) + 1) * (2 * abs(win[1]) + 1)         # (a refused call still gets buffers that would hold it)
    kk = min(max(top_k, 1), 16)
    full = lambda *shape: torch.full(shape, POISON, dtype=torch.int32, device=gpu)
    o = dict(scores=full(n, ncand), cand=full(n, kk, 2), cand_score=full(n, kk), score=full(n, 4), flags=full(n),
             rms=torch.full((n, 2), 1e300, dtype=torch.float64, device=gpu))
    ptr = lambda a: None if a is None or a.numel() == 0 else a.data_ptr()
    arg = dict(o)
    if alias is not None:
        arg[alias[0]] = ins[alias[1]]
    rc = cpe.lib.load().cpe_mono_shift_batch(ptr(ins['xy']), ptr(ins['id']), ptr(ins['cnt']), n, ptr(ins['K']), ptr(ins['Tc']), ptr(ins['P']),
                                             ptr(ins['status']), table['lo'] if lo is None else lo, table['hi'] if hi is None else hi,
                                             win[0], win[1], tau, min_sin, min_score, swap, top_k, ptr(arg['scores']), ptr(arg['cand']),
                                             ptr(arg['cand_score']),
                                             ptr(arg['score']), ptr(arg['rms']), ptr(arg['flags']), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in o.items()}


def _call(cpe, gpu, case, poison=None, **kw):
    xy, I, cnt = MC.arrays(case, poison)
    rc, out = _raw(cpe, gpu, xy, I, cnt, case['cam'], case['table'], **dict(MC.params(case), **kw))
    assert rc == 0, cpe.lib.load().cpe_last_error_string()
    return out


def _compare(name, g, refs):
    worst = 0.0
    for f, ref in enumerate(refs):
        worst = max(worst, MC.compare_frame({k: g[k][f] for k in KEYS}, ref, f'{name}, frame {f}'))
    print(f'{name}: rms error at most {worst:.3f} of its tolerance, margin {min(r["margin"] for r in refs):.2e}')


@pytest.mark.parametrize('name', list(MC.cases()))
def test_case(cpe, gpu, name):
    """every case and batch of mono_shift_cases.cases() against ref_mono_shift; poison in the inputs past every count changes no
    bit; a second call gives the same bits"""
    case = MC.cases()[name]
    a = _call(cpe, gpu, case, poison=41)
    b = _call(cpe, gpu, case)
    for k in KEYS:
        assert a[k].tobytes() == b[k].tobytes(), f'{name}: {k} depends on slots past the count'
    _compare(name, a, MC.reference(name))


def test_repeat_gives_the_same_bits(cpe, gpu):
    case = MC.cases()['65 frames']
    outs = [_call(cpe, gpu, case) for _ in range(3)]
    for o in outs[1:]:
        for k in KEYS:
            assert o[k].tobytes() == outs[0][k].tobytes(), f'{k} does not repeat'


def test_top_k_slots_only(cpe, gpu):
    """cand and cand_score are written for top_k slots and no further"""
    case = MC.cases()['top_k 1']
    xy, I, cnt = MC.arrays(case)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    K, _ = TC.camera(1)
    tab = case['table']
    n = len(cnt)
    ins = [t(xy), t(I), t(cnt), t(K).reshape(9), t(tab['P']), t(tab['status'].astype(np.int32))]
    cand = torch.full((n * 2 + 2,), POISON, dtype=torch.int32, device=gpu)
    cs = torch.full((n + 1,), POISON, dtype=torch.int32, device=gpu)
    rest = [torch.zeros(s, dtype=torch.int32, device=gpu) for s in ((n, 81), (n, 4), (n,))]
    rms = torch.zeros((n, 2), dtype=torch.float64, device=gpu)
    rc = cpe.lib.load().cpe_mono_shift_batch(ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), n, ins[3].data_ptr(), None,
                                             ins[4].data_ptr(), ins[5].data_ptr(), tab['lo'], tab['hi'], 4, 4, 0.1, 0.01, 8, 0, 1,
                                             rest[0].data_ptr(),
                                             cand.data_ptr(), cs.data_ptr(), rest[1].data_ptr(), rms.data_ptr(), rest[2].data_ptr(),
                                             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    refs = MC.reference('top_k 1')
    assert np.array_equal(cand.cpu().numpy()[:2 * n].reshape(n, 2), np.stack([r['cand'][0] for r in refs]))
    assert (cand.cpu().numpy()[2 * n:].view(np.uint32) == POISON).all() and cs.cpu().numpy()[n:].view(np.uint32)[0] == POISON


def test_refused_arguments(cpe, gpu):
    """a window above CPE_SHIFT_MAX_WIN, tau <= 0 or NaN, top_k 0 or 9, a negative min_score or min_sin, swap 2, L outside
    1..CPE_MAXL, an output that is an input: CPE_ERR_ARG and nothing written"""
    case = MC.cases()['three frames']
    xy, I, cnt = MC.arrays(case)
    rig = case['table']
    big = dict(P=np.zeros((2, 257, 4)), status=np.zeros((2, 257), np.int32), lo=0, hi=256)
    calls = [(what, kw, rig if rng is None else (big if rng == (0, 256) else dict(rig, lo=rng[0], hi=rng[1])))
             for what, (rng, kw) in MC.REFUSED_CALLS.items()]
    calls += [(f'{o} is {i}', dict(alias=(o, i)), rig) for o, i in (('scores', 'id'), ('cand', 'cnt'), ('rms', 'xy'), ('flags', 'status'),
                                                                    ('score', 'K'), ('cand_score', 'P'))]
    for what, kw, tab in calls:
        rc, g = _raw(cpe, gpu, xy, I, cnt, 1, tab, **kw)
        assert rc == -1, what
        for k in MC.INT_KEYS:
            assert (g[k].view(np.uint32) == POISON).all(), f'{what}: {k} written'
        assert (g['rms'] == 1e300).all(), what
    rc, g = _raw(cpe, gpu, xy, I, cnt, 2, rig, alias=('score', 'Tc'))
    assert rc == -1
    tab = cpe.fit.LaserTable(*(torch.from_numpy(rig[k]).to(gpu) for k in ('P', 'status')), rig['lo'], rig['hi'],
                             torch.zeros(4, dtype=torch.float64, device=gpu), torch.zeros(1, dtype=torch.int32, device=gpu))
    gp = cpe.fit.GridTables(*(torch.from_numpy(a).to(gpu) for a in (xy, I, cnt)))
    K, _ = TC.camera(1)
    for kw in (dict(win=(9, 4)), dict(win=(4, 9)), dict(tau=0.0), dict(tau=float('nan')), dict(top_k=0), dict(top_k=9),
               dict(min_score=-1), dict(min_sin=-0.5)):
        with pytest.raises(ValueError):
            cpe.fit.mono_shift_batch(gp, K, None, tab, **kw)


def test_n_zero(cpe, gpu):
    rig = TC.rig_table(-16, 16)
    rc, g = _raw(cpe, gpu, np.zeros((0, MC.MAXP, 2)), np.zeros((0, MC.MAXP, 2), np.int32), np.zeros(0, np.int32), 1, rig)
    assert rc == 0
    tab = cpe.fit.LaserTable(*(torch.from_numpy(rig[k]).to(gpu) for k in ('P', 'status')), -16, 16,
                             torch.zeros(4, dtype=torch.float64, device=gpu), torch.zeros(1, dtype=torch.int32, device=gpu))
    gp = cpe.fit.GridTables(torch.zeros((0, MC.MAXP, 2), dtype=torch.float64, device=gpu),
                            torch.zeros((0, MC.MAXP, 2), dtype=torch.int32, device=gpu), torch.zeros(0, dtype=torch.int32, device=gpu))
    out = cpe.fit.mono_shift_batch(gp, TC.camera(1)[0], None, tab)
    assert tuple(out['scores'].shape) == (0, 81) and tuple(out['cand'].shape) == (0, 4, 2) and tuple(out['rms'].shape) == (0, 2)


def test_python_layer_equals_the_c_call(cpe, gpu):
    """fit.mono_shift_batch: the same bits as the C call, and swap from the table's family0"""
    for name, family0, ids, transposed in (('three frames', 'col', 'col_row', False), ('transposed swap 1', 'row', 'col_row', True),
                                           ('transposed swap 1', 'col', 'row_col', True), ('camera 2', 'col', 'col_row', False),
                                           ('window (8, 8)', 'row', 'row_col', False), ('top_k 8', 'col', 'col_row', False)):
        case = MC.cases()[name]
        xy, I, cnt = MC.arrays(case)
        raw = _call(cpe, gpu, case)
        t = case['table']
        tab = cpe.fit.LaserTable(torch.from_numpy(t['P']).to(gpu), torch.from_numpy(t['status']).to(gpu), t['lo'], t['hi'],
                                 torch.zeros(4, dtype=torch.float64, device=gpu), torch.zeros(1, dtype=torch.int32, device=gpu), family0)
        p = MC.params(case)
        assert tab.swap_for(ids) == p['swap'] == int(transposed)
        K, Tc = TC.camera(case['cam'])
        out = cpe.fit.mono_shift_batch(cpe.fit.GridTables(*(torch.from_numpy(a).to(gpu) for a in (xy, I, cnt))), K, Tc, tab, win=p['win'],
                                       tau=p['tau'], min_score=p['min_score'], min_sin=p['min_sin'], top_k=p['top_k'], ids=ids)
        torch.cuda.synchronize()
        assert set(out) == set(KEYS) | {'win'}
        for k in KEYS:
            assert out[k].cpu().numpy().tobytes() == raw[k].tobytes(), f'{name}: {k}'
