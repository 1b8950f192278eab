"""cpe_multi_frame_consensus_batch (csrc/fit.hip k_multi_frame_hyp, k_multi_frame_consensus) / multiframe.fit_multi_frame_consensus_gpu /
experiment.run_experiment(multi_frame='consensus') against the numpy reference and the case table of multiframe_consensus_cases.

Yardsticks:
  decisions  info (winning hypothesis, its two frames, rounds), inlier, n_inliers, n_used, flags, status: equal to ref_consensus.
             Every case takes its decisions with inlier_margin > 1e-3 and key_gap > 1e-6 (test_multiframe_consensus_cpu.py), the
             kernels' terms and the restatement's agree to about 1e-12
  exact      frame_terms and T against cpe_pose_vec2T_batch + cpe_multi_frame_terms at the returned x; with max_rounds = 1 x,
             T, fvals, iters against cpe_multi_frame_fit_lm_batch(frame_ok = inlier == 1, x0_in = x0) -- the same device code
             on the same list; a second call, a poisoned workspace, a group of a batch against its single call: bit for bit
  optimum    with more rounds f over the final list <= scipy's optimum on that list (1 + 1e-6), the bound of the LM tests; on
             the 24-frame scenes the pose within NOISY_CONSENSUS_BOUNDS of Ttrue"""
import ctypes as C
import json
import math

import numpy as np
import pytest

import multiframe_cases as mc
import multiframe_consensus_cases as cc
import multiframe_lm_cases as lc

R = cc.RADIUS
NAMES = sorted(cc.CASES)
OK_NAMES = [n for n in NAMES if cc.CASES[n].get('expect', 'bad') != 'few']
GROUP_KEYS = ('x0', 'x', 'T', 'fvals', 'iters', 'n_used', 'n_inliers', 'info', 'flags', 'status')
FRAME_KEYS = ('inlier', 'frame_terms')


def host(res):
    return {k: v.cpu().numpy() for k, v in res.items() if k != 'TAGV'}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def bits_equal(a, b, keys):
    return all(np.array_equal(bits(a[k]), bits(b[k])) for k in keys)


def assert_failed_group(r, g, status):
    assert r['status'][g] == status
    for k in GROUP_KEYS[:-1]:
        assert not r[k][g].any(), f'{k} of a group with status {status} must be zero'


def on_device(s, gpu):
    import torch
    d = dict(s, Pd=torch.from_numpy(s['P']).to(gpu), cd=torch.from_numpy(np.asarray(s['cnt'], np.int32)).to(gpu),
             rawd=torch.from_numpy(s['raw']).to(gpu), TAGVd=torch.from_numpy(s['TAGV']).to(gpu))
    d['okd'] = None if s['keep'] is None else torch.from_numpy(s['keep']).to(gpu)
    return d


@pytest.fixture(scope='module')
def built(orc, cpe, gpu):
    """name -> the case on the host and the device with its reference: computed once"""
    return {name: on_device(cc.build(name, orc), gpu) for name in NAMES}


def run(s, **over):
    from cpe_amd import multiframe
    kw = dict(s['cons'], **over)
    kw.setdefault('frame_ok', s['okd'])
    return host(multiframe.fit_multi_frame_consensus_gpu(s['Pd'], s['cd'], s['rawd'], s['TAGVd'], R, **kw))


def run_lm(s, **kw):
    from cpe_amd import multiframe
    return host(multiframe.fit_multi_frame_gpu(s['Pd'], s['cd'], s['rawd'], s['TAGVd'], R, method='lm', **kw))


@pytest.fixture(scope='module')
def results(built):
    return {name: run(built[name]) for name in NAMES}


def kept_of(s):
    return np.arange(len(s['cnt'])) if s['keep'] is None else np.flatnonzero(s['keep'])


def pieces(cpe, s, x):
    """-> vec2T(x) on the device (flat 16) and every frame's term at it"""
    import torch
    dev, n = s['Pd'].device, len(s['cnt'])
    T = cpe.multiframe.vec2T_batch(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64).reshape(1, 6)).to(dev))
    terms = torch.zeros(n, dtype=torch.float64, device=dev)
    assert cpe.lib.load().cpe_multi_frame_terms(s['Pd'].data_ptr(), s['cd'].data_ptr(), n, s['TAGVd'].data_ptr(), T.data_ptr(), R,
                                                terms.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
    return T.cpu().numpy()[0], terms.cpu().numpy()


# ------------------------------------------------------------------------------------------------------- 1 the decisions
@pytest.mark.gpu
@pytest.mark.parametrize('name', NAMES)
def test_decisions_equal_the_reference(built, results, name):
    s, got, ref = built[name], results[name], built[name]['ref']
    print(f'{name}: status {got["status"][0]} info {got["info"][0].tolist()} flags {got["flags"][0]} inliers {got["n_inliers"][0]} of '
          f'{got["n_used"][0]} fvals {got["fvals"][0].tolist()} iters {got["iters"][0].tolist()} | reference info {ref["info"]} iters '
          f'{ref.get("iters")} margin {ref["inlier_margin"]:.3g} gap {ref["key_gap"]:.3g}')
    assert ref['inlier_margin'] > 1e-3 and ref['key_gap'] > 1e-6
    if s['expect'] == 'few':
        assert ref['status'] == cc.ST_FEW
        assert_failed_group(got, 0, cc.ST_FEW)
        assert (got['inlier'] == -1).all() and np.isnan(got['frame_terms']).all()
        return
    assert got['status'][0] == cc.ST_OK == ref['status']
    assert got['info'][0].tolist() == ref['info']
    assert got['n_used'][0] == ref['n_used'] == len(kept_of(s))
    assert got['n_inliers'][0] == ref['n_inliers'] == (got['inlier'] == 1).sum()
    assert got['flags'][0] == ref['flags']
    assert np.array_equal(got['inlier'], ref['inlier'])
    assert np.flatnonzero(got['inlier'] == 0).tolist() == s['out']
    assert all(np.isfinite(got[k]).all() for k in ('x0', 'x', 'T', 'fvals'))
    # the winning key's sum -- the terms of S_0 at the closed-form pose x0 -- against the restatement's (LAPACK and numpy's
    # summation order there, Jacobi sweeps and the lane tree here): three orders inside the margins the decisions have
    assert abs(got['fvals'][0, 0] - ref['fvals'][0]) <= 1e-6 * ref['fvals'][0]
    if s['cons']['max_rounds'] == 0:
        assert np.array_equal(bits(got['x']), bits(got['x0'])) and got['fvals'][0, 0] == got['fvals'][0, 1]
        assert got['iters'][0].tolist() == [0, 0] and got['flags'][0] == 0 and got['info'][0, 3] == 0
    if name.startswith('F24') and s['cons']['max_rounds'] > 0:
        rot, tr = cc.pose_errors(got['T'][0], s['Ttrue'])
        print(f'{name}: {rot:.4f} deg {tr:.4f} mm off Ttrue')
        assert rot <= cc.NOISY_CONSENSUS_BOUNDS['rot_deg'] and tr <= cc.NOISY_CONSENSUS_BOUNDS['tr_mm']


# ------------------------------------------------------------------------------------------------------------- 2 exact
@pytest.mark.gpu
@pytest.mark.parametrize('name', OK_NAMES)
def test_terms_and_pose_matrix_equal_the_exported_pieces(cpe, built, results, name):
    s, got = built[name], results[name]
    T, terms = pieces(cpe, s, got['x'][0])
    kept = kept_of(s)
    assert np.array_equal(bits(got['T'][0]), bits(T))
    assert np.array_equal(bits(got['frame_terms'][kept]), bits(terms[kept]))
    rest = np.setdiff1d(np.arange(len(s['cnt'])), kept)
    assert np.isnan(got['frame_terms'][rest]).all() and (got['inlier'][rest] == -1).all()
    fitted = np.flatnonzero(got['inlier'] == 1)
    v = 0.0
    for t in terms[fitted].tolist():
        v = v + t
    assert got['fvals'][0, 1] == v, 'the objective of x over the list it was fitted to: its terms added in order'
    tau2 = s['cons']['tau'] ** 2
    if got['flags'][0] & cc.CONVERGED:
        assert np.array_equal(fitted, kept[(terms[kept] < tau2) & (s['cnt'][kept] >= 1)])
    assert bits_equal(run(s), got, GROUP_KEYS + FRAME_KEYS), 'a second call repeats the bits'


@pytest.mark.gpu
@pytest.mark.parametrize('name', OK_NAMES)
def test_one_round_is_the_lm_call_on_the_inliers(built, name):
    import torch
    s = built[name]
    got = run(s, max_rounds=1)
    assert got['status'][0] == cc.ST_OK and got['info'][0, 3] == 1
    lm = run_lm(s, frame_ok=torch.from_numpy((got['inlier'] == 1).astype(np.int32)).to(s['Pd'].device), x0=got['x0'])
    assert lm['status'][0] == cc.ST_OK and lm['n_used'][0] == got['n_inliers'][0]
    assert bits_equal(got, lm, ('x0', 'x', 'T', 'fvals', 'iters'))
    if name == 'F24_clean':
        assert (got['inlier'] == 1).all()
    if (got['inlier'] == 1).all():              # every frame agrees with x0: the call is the LM form on all frames from x0
        assert bits_equal(got, run_lm(s, x0=got['x0']), ('x0', 'x', 'T', 'fvals', 'iters'))


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['F24_3bad', 'F24_8bad', 'F45_5bad', 'two_rounds', 'F9_unusable'])
def test_rounds_reach_the_optimum_of_the_final_list(built, results, name):
    s, got = built[name], results[name]
    fitted = np.flatnonzero(got['inlier'] == 1)
    prob = lc.Problem(s['P'][fitted], s['cnt'][fitted], s['TAGV'][fitted])
    _, f_ls = lc.scipy_optimum(prob, s['Ttrue'])
    print(f'{name}: f {got["fvals"][0, 1]!r} scipy on the same {len(fitted)} frames {f_ls!r} rounds {got["info"][0, 3]}')
    assert got['fvals'][0, 1] <= f_ls * (1 + 1e-6)
    assert got['fvals'][0, 1] <= got['fvals'][0, 0] or got['info'][0, 3] > 1


@pytest.mark.gpu
def test_the_two_round_case(built, results):
    s, got = built['two_rounds'], results['two_rounds']
    at_x0 = run(s, max_rounds=0)
    late = np.flatnonzero((got['inlier'] == 1) & (at_x0['inlier'] == 0))
    tau = s['cons']['tau']
    assert got['info'][0, 3] == 2 and got['flags'][0] == cc.CONVERGED and len(late) == 1 and late[0] not in s['bad']
    a, b = math.sqrt(at_x0['frame_terms'][late[0]]) / tau, math.sqrt(got['frame_terms'][late[0]]) / tau
    print(f'frame {late[0]}: rms / tau {a:.4f} at x0, {b:.4f} at x; iters {got["iters"][0].tolist()}')
    assert 1.0 < a < 1.25 and b < 1.0
    assert got['n_inliers'][0] == at_x0['n_inliers'][0] + 1
    one = run(s, max_rounds=1)                         # stopped after the first round: fitted to S_0, neither flag
    assert one['flags'][0] == 0 and np.array_equal(one['inlier'], at_x0['inlier']) and one['iters'][0, 0] < got['iters'][0, 0]


# ------------------------------------------------------------------------------------------------------------ 3 batching
@pytest.mark.gpu
def test_groups_equal_single_calls(built, orc):
    import torch
    parts = [built[n] for n in ('F4_1bad', 'F24_3bad', 'F14_holes')]
    s = {k: torch.cat([p[k] for p in parts]).contiguous() for k in ('Pd', 'cd', 'rawd', 'TAGVd')}
    ok = np.ones(42, np.int32)
    ok[28:] = parts[2]['keep']
    s.update(okd=torch.from_numpy(ok).to(s['Pd'].device), cons=cc.DEFAULTS)
    # the 24 frames alone, a range that runs backwards, the 4 + 24 frames as one experiment (they share Ttrue), the 14 with their
    # holes, backwards again, an empty group
    gs = [4, 28, 0, 28, 42, 4, 4]
    what = ['F24_3bad', cc.ST_OVERFLOW, 'union', 'F14_holes', cc.ST_OVERFLOW, cc.ST_FEW]
    got = run(s, group_start=gs)
    host_tables = {k: np.concatenate([p[k] for p in parts]) for k in ('P', 'cnt', 'raw', 'TAGV')}
    union = cc.ref_consensus(host_tables['P'], host_tables['cnt'], host_tables['TAGV'], host_tables['raw'], np.arange(42) < 28)
    print(f'union: info {union["info"]} margin {union["inlier_margin"]:.3g} gap {union["key_gap"]:.3g}')
    assert union['inlier_margin'] > 1e-3 and union['key_gap'] > 1e-6 and union['status'] == cc.ST_OK
    assert got['info'][2].tolist() == union['info'] and got['n_inliers'][2] == union['n_inliers'] == 24
    expected = {f: set() for f in range(42)}
    for g, w in enumerate(what):
        if isinstance(w, int):
            assert_failed_group(got, g, w)
            continue
        a, b = gs[g], gs[g + 1]
        one = run(s, group_start=[a, b])
        assert one['status'][0] == cc.ST_OK
        assert bits_equal({k: got[k][g:g + 1] for k in GROUP_KEYS}, one, GROUP_KEYS), f'group {g} {w} differs from its single-group call'
        if w != 'union':
            ref = built[w]['ref']
            assert got['info'][g].tolist() == [ref['info'][0], ref['info'][1] + a, ref['info'][2] + a, ref['info'][3]]
            assert np.array_equal(one['inlier'][a:b], ref['inlier'])
        for f in np.flatnonzero(one['inlier'] >= 0):
            expected[f].add((int(one['inlier'][f]), float(one['frame_terms'][f])))
    for f in range(42):
        if not ok[f]:
            assert got['inlier'][f] == -1 and np.isnan(got['frame_terms'][f])
        else:
            assert (int(got['inlier'][f]), float(got['frame_terms'][f])) in expected[f], f'frame {f}'
            assert len({e[0] for e in expected[f]}) == 1, 'the groups that keep a frame agree on it'


@pytest.mark.gpu
def test_more_kept_frames_than_a_group_holds(gpu):
    import torch
    n = cc.MAXF + 1
    pts = torch.zeros((mc.MAXP, 3), dtype=torch.float64)
    pts[:5] = torch.tensor([[40.0, -50, 400], [45, -20, 395], [50, 0, 400], [42, 20, 398], [48, 50, 402]])
    s = dict(Pd=pts.to(gpu).expand(n, -1, -1).contiguous(), cd=torch.full((n,), 5, dtype=torch.int32, device=gpu),
             rawd=torch.zeros((n, 2, 6), dtype=torch.float64, device=gpu),
             TAGVd=torch.eye(4, dtype=torch.float64, device=gpu).reshape(1, 16).expand(n, -1).contiguous(), okd=None, cons=cc.DEFAULTS)
    got = run(s)
    assert_failed_group(got, 0, cc.ST_OVERFLOW)
    assert (got['inlier'] == -1).all() and np.isnan(got['frame_terms']).all()
    ok = torch.ones(n, dtype=torch.int32, device=gpu)
    ok[3] = 0
    assert_failed_group(run(s, frame_ok=ok), 0, cc.ST_FEW)          # 1024 kept frames fit; none of them is usable
    for gs in ([3, 0], [-1, 3], [0, n + 1]):
        assert_failed_group(run(s, group_start=gs), 0, cc.ST_OVERFLOW)


# ------------------------------------------------------------------------------------------------ 4 the C ABI: scratch, refusals
def raw_call(cpe, s, cons=None, params=None, ws_fill=None, ws_bytes=None, null=None, G=1, frame_terms=True, fill=None):
    """the entry point itself on one group of all frames -> rc, outputs (host), the tensors"""
    import torch
    L, dev, n = cpe.lib.load(), s['Pd'].device, len(s['cnt'])
    gs = torch.tensor([0, n], dtype=torch.int32, device=dev)
    f64 = lambda *shape: torch.full(shape, 7.25 if fill is None else fill, dtype=torch.float64, device=dev)
    i32 = lambda *shape: torch.full(shape, 77, dtype=torch.int32, device=dev)
    outs = dict(x0=f64(1, 6), x=f64(1, 6), T=f64(1, 16), fvals=f64(1, 2), iters=i32(1, 2), n_used=i32(1), n_inliers=i32(1), info=i32(1, 4),
                flags=i32(1), status=i32(1), inlier=i32(n), frame_terms=f64(n))
    max_hyp = cons.max_hyp if cons is not None else 2048
    need = L.cpe_multi_frame_consensus_workspace_bytes(1, max_hyp)
    ws = torch.full((max(need, 1024),), 0 if ws_fill is None else ws_fill, dtype=torch.uint8, device=dev)
    ptrs = {k: t.data_ptr() for k, t in outs.items()}
    if null is not None:
        ptrs[null] = None
    if not frame_terms:
        ptrs['frame_terms'] = None
    rc = L.cpe_multi_frame_consensus_batch(
        s['Pd'].data_ptr(), s['cd'].data_ptr(), s['TAGVd'].data_ptr(), s['rawd'].data_ptr(), s['okd'].data_ptr() if s['okd'] is not None else None,
        gs.data_ptr(), G, n, R, C.addressof(params) if params is not None else None, C.addressof(cons) if cons is not None else None,
        ws.data_ptr() if ws_bytes != 'null' else None, need if ws_bytes in (None, 'null') else ws_bytes,
        *(ptrs[k] for k in GROUP_KEYS + FRAME_KEYS), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, {k: t.cpu().numpy() for k, t in outs.items()}


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['F24_3bad', 'F14_holes', 'F3_1bad_min3'])
def test_poisoned_workspace_and_outputs(cpe, built, results, name):
    s, got = built[name], results[name]
    cons = cpe.lib.CpeConsensusParams(*(s['cons'][k] for k in ('tau', 'max_hyp', 'max_rounds', 'min_inliers')))
    for ws_fill, fill in ((0xFF, float('nan')), (0x00, -1e300), (0x7F, 7.25)):
        rc, out = raw_call(cpe, s, cons=cons, ws_fill=ws_fill, fill=fill)
        assert rc == 0
        assert bits_equal(out, got, GROUP_KEYS)
        kept = kept_of(s) if got['status'][0] == cc.ST_OK else []
        assert bits_equal({k: out[k][kept] for k in FRAME_KEYS}, {k: got[k][kept] for k in FRAME_KEYS}, FRAME_KEYS)
        rest = np.setdiff1d(np.arange(len(s['cnt'])), kept)
        assert (out['inlier'][rest] == 77).all(), 'frames that are not kept, and those of a failed group, are not written'
        assert np.array_equal(bits(out['frame_terms'][rest]), bits(np.full(len(rest), fill)))


@pytest.mark.gpu
def test_null_arguments_and_refusals(cpe, built, results):
    s, got = built['F24_clean'], results['F24_clean']
    P = cpe.lib.CpeConsensusParams
    untouched = lambda out: all((v == (7.25 if v.dtype == np.float64 else 77)).all() for v in out.values())
    rc, out = raw_call(cpe, s)                                           # NULL cons = the defaults, NULL params
    assert rc == 0 and bits_equal(out, got, GROUP_KEYS + FRAME_KEYS)
    rc, out = raw_call(cpe, s, frame_terms=False)
    assert rc == 0 and bits_equal(out, got, GROUP_KEYS + ('inlier',)) and (out['frame_terms'] == 7.25).all()
    for k in GROUP_KEYS + ('inlier',):
        rc, out = raw_call(cpe, s, null=k)
        assert rc == -1 and untouched(out), f'NULL output {k}'
    bad = [P(0.0, 2048, 4, 3), P(-1.0, 2048, 4, 3), P(float('nan'), 2048, 4, 3), P(float('inf'), 2048, 4, 3), P(0.5, 0, 4, 3),
           P(0.5, cc.MAX_HYP + 1, 4, 3), P(0.5, 2048, -1, 3), P(0.5, 2048, 17, 3), P(0.5, 2048, 4, 1)]
    for c in bad:
        rc, out = raw_call(cpe, s, cons=c)
        assert rc == -1 and untouched(out), f'cons {c.tau} {c.max_hyp} {c.max_rounds} {c.min_inliers}'
    assert b'cpe_multi_frame_consensus_batch' in cpe.lib.load().cpe_last_error_string()
    rc, out = raw_call(cpe, s, params=cpe.lib.CpeFitParams(1e-5, 1e-5, 100000, 100000, 0, 0))      # CPE_FIT_NELDER_MEAD
    assert rc == -1 and untouched(out)
    rc, out = raw_call(cpe, s, params=cpe.lib.CpeFitParams(1e-5, 1e-5, 0, 100000, 1, 0))
    assert rc == -1 and untouched(out)
    need = cpe.lib.load().cpe_multi_frame_consensus_workspace_bytes(1, 2048)
    assert need == 2048 * 60 and cpe.lib.load().cpe_multi_frame_consensus_workspace_bytes(3, 130) == 3 * 130 * 60
    assert cpe.lib.load().cpe_multi_frame_consensus_workspace_bytes(0, 2048) == 0
    assert cpe.lib.load().cpe_multi_frame_consensus_workspace_bytes(1, cc.MAX_HYP + 1) == 0
    for ws_bytes in (need - 1, 'null'):
        rc, out = raw_call(cpe, s, ws_bytes=ws_bytes)
        assert rc == -3 and untouched(out)
    rc, out = raw_call(cpe, s, G=-1)
    assert rc == -1 and untouched(out)
    rc, out = raw_call(cpe, s, G=0)
    assert rc == 0 and untouched(out)
    # the largest allowed values run
    rc, out = raw_call(cpe, s, cons=P(0.5, cc.MAX_HYP, 16, 2))
    assert rc == 0 and out['status'][0] == cc.ST_OK and bits_equal(out, got, ('x', 'inlier'))
    from cpe_amd import multiframe
    with pytest.raises(cpe.lib.CpeError):
        multiframe.fit_multi_frame_consensus_gpu(s['Pd'], s['cd'], s['rawd'], s['TAGVd'], R, max_hyp=0)


# ---------------------------------------------------------------------------------- 5 run_experiment(multi_frame='consensus')
H, W, NF = 480, 640, 6


@pytest.mark.gpu
def test_run_experiment_consensus_mode(cpe, gpu, tmp_path):
    """the folder of test_multiframe_lm_gpu.py::test_run_experiment_lm_mode"""
    import torch
    import warnings
    from PIL import Image
    from cpe_amd import experiment, multiframe, synth
    b = synth.render_batch(NF, H, W, seed=0, with_gt=False)
    stems = ['-10', '-21', '00', '1-2', '11', '2-1']
    L, Rr = b['left'].numpy(), b['right'].numpy()
    for i, st in enumerate(stems):
        Image.fromarray(L[i]).save(tmp_path / f'{st}L.png')
        Image.fromarray(Rr[i]).save(tmp_path / f'{st}R.png')
    for side in 'LR':
        Image.fromarray(np.zeros((H, W), np.uint8)).save(tmp_path / f'3-3{side}.png')
    lens = lambda K: dict(IntrinsicMatrix=np.asarray(K, dtype=np.float64).tolist(), RadialDistortion=[0.012, -0.004],
                          TangentialDistortion=[0.0002, -0.0001])
    (tmp_path / 'cam.json').write_text(json.dumps(dict(LeftCamera=lens(b['K1']), RightCamera=lens(b['K2']))))
    args = (str(tmp_path), str(tmp_path / 'cam.json'), b['K1'], b['K2'], b['T21'], b['radius'])
    lm = experiment.run_experiment(*args, chunk=4, multi_frame='lm')
    # the rendered frames do not share one AGV pose (the LM form leaves about 13 mm rms per frame): a wide tau, under which a pose
    # is returned, and a tighter one
    seen = []
    for tau in (25.0, 8.0):
        opts = dict(tau=tau, min_inliers=2, max_rounds=3)
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter('always')
            res = experiment.run_experiment(*args, chunk=4, multi_frame='consensus', consensus=opts, frame_angles=True)
        # the layers by hand
        names = res['names']
        bad = {s['index'] for s in res['skipped']}
        ok = torch.tensor([0 if i in bad else 1 for i in range(len(names))], dtype=torch.int32, device=gpu)
        by_hand = multiframe.group_result(multiframe.fit_multi_frame_consensus_gpu(res['pts3'], res['cnt'], res['cyl_raw'], res['angles'],
                                                                                   b['radius'], frame_ok=ok, **opts))
        c = res['consensus']
        print(f'tau {tau}: consensus {c}; fval {res["fval"]!r}; lm fval {lm["fval"]!r}; warnings {[str(w.message) for w in caught]}')
        assert set(res) - set(lm) == {'consensus', 'angles_est', 'angles_status', 'angles_delta_deg'}
        assert set(c) == {'inliers', 'rejected', 'n_inliers', 'rounds', 'flags', 'status'}
        assert c['status'] == by_hand['status'] and c['n_inliers'] == by_hand['n_inliers'] and c['flags'] == by_hand['flags']
        assert c['rounds'] == by_hand['info'][3]
        if c['status'] == 0:
            assert res['T_cam_agv'] == by_hand['T'] and res['fval'] == by_hand['fvals'][1]
            assert c['inliers'] == [names[i] for i in range(len(names)) if by_hand['inlier'][i] == 1]
            assert [r['index'] for r in c['rejected']] == [i for i in range(len(names)) if by_hand['inlier'][i] == 0]
            assert all(r['name'] == names[r['index']] and r['rms'] == math.sqrt(by_hand['frame_terms'][r['index']]) and r['rms'] >= tau
                       for r in c['rejected'])
            assert len(c['inliers']) + len(c['rejected']) + len(bad) == len(names)
            assert bool(c['rejected']) == any('left out' in str(w.message) for w in caught)
            assert res['angles_est'] is not None and res['angles_est'].shape == (len(names), 2)
        else:
            assert res['T_cam_agv'] is None and res['angles_est'] is None and any('status' in str(w.message) for w in caught)
        seen.append((c['status'], len(c['rejected'])))
    assert seen[0] == (0, 0), 'at 25 mm all six frames agree with one pose'
    assert seen[1] == (0, 3), 'at 8 mm three frames agree (about 3 mm rms) and three are 25-31 mm off'
    # the other modes are as they were: no new key, and the LM pose is the LM call's
    assert 'consensus' not in lm
    by_hand_lm = multiframe.group_result(multiframe.fit_multi_frame_gpu(lm['pts3'], lm['cnt'], lm['cyl_raw'], lm['angles'], b['radius'],
                                                                        frame_ok=ok, method='lm'))
    assert lm['T_cam_agv'] == by_hand_lm['T'] and lm['fval'] == by_hand_lm['fvals'][1]
    with pytest.raises(ValueError):
        experiment.run_experiment(*args, chunk=4, multi_frame='lm', consensus={})
