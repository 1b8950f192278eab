"""The build-defined LM form of the resident multi-frame fit: cpe_multi_frame_fit_lm_batch /
multiframe.fit_multi_frame_gpu(method='lm') / experiment.run_experiment(multi_frame='lm').

Scenes: multiframe_cases.CASES -- point counts 5, 63, 64, 65, 160, 2048 (lane tails, a full table), frame counts 2, 3, 17, 33
(one past one and two rounds of a workgroup of up to 16 wavefronts).  Yardsticks:
  exact    f(x0), f(x), T, frame_terms against the exported pieces (cpe_pose_vec2T_batch + cpe_multi_frame_terms, the terms
           added on the host in frame order), a second call, a group of a batch against its single call: bit for bit
  optimum  scipy's least_squares(method='lm', xtol = ftol = 1e-14) from Ttrue (multiframe_lm_cases.scipy_optimum): f <= f_ls
           (1 + 1e-6) (<= tol_f 1e-3 = 1e-8 on the noise-free scene), rotation within 1e-4 rad -- the per-frame LM test's figures
           -- and translation within 1e-4 |t_ls|, the displacement that rotation bound allows; f <= f(Ttrue) with noise
  x0       the numpy restatement's initial pose (LAPACK eigenvectors and solver, numpy's summation order).  Measured on one
           MI355X, rotation ||R1' R2 - I||_F / sqrt(2) / translation relative to |t|: F17 4.05e-14 / 6.99e-16, F2 4.84e-15 /
           6.17e-10, F3 1.01e-14 / 1.09e-15, F33 2.02e-13 / 1.12e-13.  The bounds are 100 times the largest: 2.02e-11 and
           6.17e-8.  (F2's translation stands out because the fitted origin of its 2048-point frame lies 1e10 mm along the
           axis -- the per-frame simplex does not hold it -- so (I - d d') o carries about 1e-6 mm of rounding.)"""
import ctypes as C
import json

import numpy as np
import pytest

import multiframe_cases as mc
import multiframe_lm_cases as lc

R = mc.RADIUS
ST_OK, ST_FEW, ST_OVERFLOW = 0, 5, 6
NAMES = sorted(mc.CASES)
KEYS = ('x0', 'x', 'T', 'fvals', 'iters', 'n_used', 'status')
X0_ROT_BOUND, X0_TR_BOUND = 2.02e-11, 6.17e-8     # 100 x the largest difference measured (module docstring)


def host(res):
    return {k: v.cpu().numpy() for k, v in res.items() if k != 'TAGV'}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def bits_equal(a, b, keys=KEYS):
    return all(np.array_equal(bits(a[k]), bits(b[k])) for k in keys)


def group_of(r, g):
    return {k: r[k][g:g + 1] for k in KEYS}


def assert_failed_group(r, g, status):
    assert r['status'][g] == status
    for k in ('x0', 'x', 'T', 'fvals', 'iters', 'n_used'):
        assert not r[k][g].any(), f'{k} of a group with status {status} must be zero'


@pytest.fixture(scope='module')
def scenes(cpe, gpu):
    """name -> the scene on the host and the device, its per-frame fits (on the GPU), the numpy restatement's fit and scipy's
    optimum: computed once"""
    import torch
    from cpe_amd import fit
    out = {}
    for name in NAMES:
        P, cnt, angles, Ttrue = mc.case_scene(name)
        TAGV = np.stack([mc.get_TAGVcyl(*a).ravel() for a in angles])
        Pd, cd = torch.from_numpy(P).to(gpu), torch.from_numpy(cnt).to(gpu)
        per = fit.fit_cylinder_batch(Pd, cd, R)
        assert not per['status'].any()
        raw = per['cyl_raw'].cpu().numpy()
        prob = lc.Problem(P, cnt, TAGV)
        x_ls, f_ls = lc.scipy_optimum(prob, Ttrue)
        out[name] = dict(P=P, cnt=cnt, TAGV=TAGV, raw=raw, Ttrue=Ttrue, Pd=Pd, cd=cd, rawd=per['cyl_raw'].contiguous(),
                         TAGVd=torch.from_numpy(TAGV).to(gpu), prob=prob, ref=lc.fit(prob, raw), x_ls=x_ls, f_ls=f_ls,
                         f_true=prob.f(lc.T2vec(Ttrue)), noise=mc.CASES[name]['noise'])
    return out


def fit_lm(s, **kw):
    from cpe_amd import multiframe
    return host(multiframe.fit_multi_frame_gpu(s['Pd'], s['cd'], s['rawd'], s['TAGVd'], R, method='lm', **kw))


@pytest.fixture(scope='module')
def single(scenes):
    return {name: fit_lm(scenes[name]) for name in NAMES}


def pieces(cpe, s, x):
    """-> vec2T(x) on the device (flat 16), the frames' terms at it, the objective with the terms added in frame order"""
    import torch
    dev = s['Pd'].device
    T = cpe.multiframe.vec2T_batch(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64).reshape(1, 6)).to(dev))
    terms = torch.zeros(len(s['cnt']), dtype=torch.float64, device=dev)
    rc = cpe.lib.load().cpe_multi_frame_terms(s['Pd'].data_ptr(), s['cd'].data_ptr(), len(s['cnt']), s['TAGVd'].data_ptr(), T.data_ptr(), R,
                                              terms.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    terms = terms.cpu().numpy()
    v = 0.0
    for t in terms.tolist():
        v = v + t
    return T.cpu().numpy()[0], terms, v


def check_optimum(s, got, name):
    f = got['fvals'][0, 1]
    T, T_ls = got['T'][0].reshape(4, 4), lc.vec2T(s['x_ls'])
    rot = lc.rotation_between(T[:3, :3], T_ls[:3, :3])
    dt = np.linalg.norm(T[:3, 3] - T_ls[:3, 3]) / np.linalg.norm(T_ls[:3, 3])
    print(f'{name}: f {f!r} f_ls {s["f_ls"]!r} f(Ttrue) {s["f_true"]!r} rotation to scipy {rot:.3g} rad translation {dt:.3g} relative; '
          f'iters {got["iters"][0].tolist()}')
    assert got['status'][0] == ST_OK
    if s['noise'] == 0:
        assert f <= 1e-8
    else:
        assert f <= s['f_ls'] * (1 + 1e-6)
        assert f <= s['f_true']
    assert rot <= 1e-4
    assert dt <= 1e-4


# ------------------------------------------------------------------------------------------------------------ 1 exact
@pytest.mark.gpu
@pytest.mark.parametrize('name', NAMES)
def test_outputs_equal_the_exported_pieces(cpe, scenes, single, name):
    s, got = scenes[name], single[name]
    assert got['status'][0] == ST_OK and got['n_used'][0] == len(s['cnt'])
    _, _, f0 = pieces(cpe, s, got['x0'][0])
    T, terms, f = pieces(cpe, s, got['x'][0])
    print(f'{name}: fvals {got["fvals"][0].tolist()} pieces {[f0, f]} iters {got["iters"][0].tolist()}')
    assert got['fvals'][0].tolist() == [f0, f]
    assert np.array_equal(bits(got['T'][0]), bits(T))
    assert np.array_equal(bits(got['frame_terms']), bits(terms))
    again = fit_lm(s)
    assert bits_equal(again, got, KEYS + ('frame_terms',))


# ---------------------------------------------------------------------------------------------------- 2, 3 optimum, iterations
@pytest.mark.gpu
@pytest.mark.parametrize('name', NAMES)
def test_reaches_the_optimum(scenes, single, name):
    s, got = scenes[name], single[name]
    check_optimum(s, got, name)
    print(f'{name}: iterations {got["iters"][0, 0]} (numpy restatement {s["ref"]["iters"]})')
    assert got['iters'][0, 0] <= 3 * s['ref']['iters']
    assert got['iters'][0, 1] >= got['iters'][0, 0] + 2


# ------------------------------------------------------------------------------------------------------ 4 the initial pose
@pytest.mark.gpu
@pytest.mark.parametrize('name', NAMES)
def test_initial_pose_against_the_restatement(scenes, single, name):
    s, got = scenes[name], single[name]
    T0, T0_ref = lc.vec2T(got['x0'][0]), lc.vec2T(s['ref']['x0'])
    rot = lc.rotation_between(T0[:3, :3], T0_ref[:3, :3])
    dt = np.linalg.norm(T0[:3, 3] - T0_ref[:3, 3]) / np.linalg.norm(T0_ref[:3, 3])
    print(f'{name}: initial pose against the restatement: rotation {rot:.3g} translation {dt:.3g} relative; f0 {got["fvals"][0, 0]!r} '
          f'restatement {s["ref"]["fvals"][0]!r}')
    assert rot <= X0_ROT_BOUND
    assert dt <= X0_TR_BOUND
    given = fit_lm(s, x0=s['ref']['x0'].reshape(1, 6))
    assert np.array_equal(given['x0'][0], s['ref']['x0'])
    check_optimum(s, given, name + ' from the restatement\'s x0')


# --------------------------------------------------------------------------------------------------------------- 5 batching
@pytest.mark.gpu
@pytest.mark.parametrize('masked', [False, True], ids=['all_frames', 'frame_ok'])
def test_groups_equal_single_calls(scenes, single, masked):
    import torch
    s = {k: torch.cat([scenes[n][k] for n in NAMES]).contiguous() for k in ('Pd', 'cd', 'rawd', 'TAGVd')}
    off = np.concatenate([[0], np.cumsum([len(scenes[n]['cnt']) for n in NAMES])]).tolist()        # F17 F2 F3 F33 -> 0 17 19 22 55
    assert off == [0, 17, 19, 22, 55]
    # groups out of order, two ranges that run backwards, an empty one, and one that overlaps three others
    gs = [22, 55, 0, 17, 17, 19, 22, 18, 55]
    what = ['F33', ST_OVERFLOW, 'F17', ST_FEW, 'F2', 'F3', ST_OVERFLOW, (18, 55)]
    kw = {}
    if masked:
        ok = np.ones(55, np.int32)
        ok[[0, 5, 16, 20, 30, 54]] = 0
        kw['frame_ok'] = torch.from_numpy(ok).to(s['Pd'].device)
    got = fit_lm(s, group_start=gs, **kw)
    assert len(got['status']) == len(what)
    allowed = {}                                                      # frame -> the terms a group may have written for it
    for g, w in enumerate(what):
        if isinstance(w, int):
            assert_failed_group(got, g, w)
            continue
        a, b = gs[g], gs[g + 1]
        one = fit_lm(s, group_start=[a, b], **kw)
        assert one['status'][0] == ST_OK
        assert bits_equal(group_of(got, g), one), f'group {g} {w} differs from its single-group call'
        if not masked and isinstance(w, str):
            assert bits_equal(one, single[w]), f'{w} inside the table differs from {w} alone'
            assert np.array_equal(bits(one['frame_terms'][a:b]), bits(single[w]['frame_terms']))
        for f in range(a, b):
            allowed.setdefault(f, []).append(one['frame_terms'][f])
    for f in range(55):
        t = got['frame_terms'][f]
        if masked and not ok[f]:
            assert np.isnan(t), 'a frame no group keeps is left as the wrapper initialised it'
        else:
            assert any(np.array_equal(bits(np.float64(t)), bits(np.float64(v))) for v in allowed[f]), f'frame_terms[{f}]'
            if f < 18:
                assert len(allowed[f]) == 1
    if masked:                                                        # F17 with the mask = its kept frames gathered
        keep = torch.from_numpy(np.flatnonzero(ok[:17])).to(s['Pd'].device)
        gathered = {k: scenes['F17'][k][keep].contiguous() for k in ('Pd', 'cd', 'rawd', 'TAGVd')}
        assert bits_equal(group_of(got, 2), fit_lm(gathered)) and got['n_used'][2] == 14


# --------------------------------------------------------------------------------------------------------------- 6 statuses
@pytest.mark.gpu
def test_statuses(scenes, gpu):
    import torch
    s = scenes['F3']
    for gs in ([3, 0], [-1, 3], [0, 4]):
        assert_failed_group(fit_lm(s, group_start=gs), 0, ST_OVERFLOW)
    ok = torch.tensor([0, 1, 0], dtype=torch.int32, device=gpu)
    assert_failed_group(fit_lm(s, frame_ok=ok), 0, ST_FEW)                                   # one kept frame
    assert_failed_group(fit_lm(s, frame_ok=ok, x0=[[0.0] * 6]), 0, ST_FEW)
    raw = s['rawd'].clone()
    raw[[0, 2]] = 0
    blind = dict(s, rawd=raw)
    got = fit_lm(blind)                                                                       # one usable frame of three kept
    assert_failed_group(got, 0, ST_FEW)
    assert np.isnan(got['frame_terms']).all()
    raw[0, 1, 3] = float('nan')
    assert_failed_group(fit_lm(dict(s, rawd=raw)), 0, ST_FEW)
    # with x0_in the fitted rows are not read: the same table is fitted
    assert fit_lm(blind, x0=scenes['F3']['ref']['x0'].reshape(1, 6))['status'][0] == ST_OK


@pytest.mark.gpu
def test_more_kept_frames_than_a_group_holds(gpu):
    import torch
    MAXF = 1024
    n = MAXF + 1
    pts = torch.zeros((mc.MAXP, 3), dtype=torch.float64)
    pts[:5] = torch.tensor([[40.0, -50, 400], [45, -20, 395], [50, 0, 400], [42, 20, 398], [48, 50, 402]])
    s = dict(Pd=pts.to(gpu).expand(n, -1, -1).contiguous(), cd=torch.full((n,), 5, dtype=torch.int32, device=gpu),
             rawd=torch.zeros((n, 2, 6), dtype=torch.float64, device=gpu),
             TAGVd=torch.eye(4, dtype=torch.float64, device=gpu).reshape(1, 16).expand(n, -1).contiguous())
    x0 = [[0.0] * 6]
    assert_failed_group(fit_lm(s, x0=x0, max_iter=2), 0, ST_OVERFLOW)
    ok = torch.ones(n, dtype=torch.int32, device=gpu)
    ok[3] = 0
    got = fit_lm(s, x0=x0, max_iter=2, frame_ok=ok)                  # exactly CPE_MULTI_MAXF kept frames are fitted
    assert got['status'][0] == ST_OK and got['n_used'][0] == MAXF and np.isfinite(got['fvals']).all()
    assert got['iters'][0, 0] <= 2 and np.isnan(got['frame_terms'][3]) and np.isfinite(np.delete(got['frame_terms'], 3)).all()


# -------------------------------------------------------------------------------------------------------------- 7 far start
@pytest.mark.gpu
@pytest.mark.parametrize('name', NAMES)
def test_far_start_ends_within_the_caps(scenes, name):
    from cpe_amd import multiframe
    s = scenes[name]
    quirk = host(multiframe.fit_multi_frame_gpu(s['Pd'], s['cd'], s['rawd'], s['TAGVd'], R, max_fun_evals=10))
    assert quirk['status'][0] == ST_OK
    got = fit_lm(s, x0=quirk['x0'])
    print(f'{name}: from the two-frame initial pose f0 {got["fvals"][0, 0]:.4g} -> status {got["status"][0]} f {got["fvals"][0, 1]:.6g} '
          f'iters {got["iters"][0].tolist()}')
    assert got['iters'][0, 0] <= 200 and got['iters'][0, 1] <= 1 + 12 * 200
    if got['status'][0] == ST_OK:
        assert all(np.isfinite(got[k]).all() for k in ('x0', 'x', 'T', 'fvals'))
        assert got['fvals'][0, 1] <= got['fvals'][0, 0]
        assert np.array_equal(got['x0'], quirk['x0'])
    else:
        assert_failed_group(got, 0, ST_FEW)


# --------------------------------------------------------------------------------------------------------------- 8 arguments
@pytest.mark.gpu
def test_bad_arguments_launch_nothing(cpe, scenes):
    import torch
    s = scenes['F2']
    L = cpe.lib.load()
    dev = s['Pd'].device
    gs = torch.tensor([0, 2], dtype=torch.int32, device=dev)
    SENT = 7.25
    f64 = lambda *shape: torch.full(shape, SENT, dtype=torch.float64, device=dev)
    i32 = lambda *shape: torch.full(shape, 77, dtype=torch.int32, device=dev)
    outs = [f64(1, 6), f64(1, 6), f64(1, 16), f64(1, 2), i32(1, 2), i32(1), i32(1)]
    terms = f64(2)

    def call(G=1, params=None, null_out=None, raw=True, x0=None):
        ptrs = [t.data_ptr() for t in outs]
        if null_out is not None:
            ptrs[null_out] = None
        return L.cpe_multi_frame_fit_lm_batch(s['Pd'].data_ptr(), s['cd'].data_ptr(), s['TAGVd'].data_ptr(),
                                              s['rawd'].data_ptr() if raw else None, None, gs.data_ptr(), G, 2, R,
                                              C.addressof(params) if params is not None else None, x0, *ptrs, terms.data_ptr(),
                                              torch.cuda.current_stream().cuda_stream)

    for k in range(len(outs)):
        assert call(null_out=k) == -1, f'NULL output {k}'
    assert call(G=-1) == -1
    assert call(raw=False) == -1                                                                # cyl_raw NULL without x0_in
    assert call(params=cpe.lib.CpeFitParams(1e-5, 1e-5, 0, 100000, 1, 0)) == -1
    assert call(params=cpe.lib.CpeFitParams(1e-5, 1e-5, 100000, 100000, 0, 0)) == -1          # CPE_FIT_NELDER_MEAD
    assert b'cpe_multi_frame_fit_lm_batch' in L.cpe_last_error_string()
    assert call(G=0) == 0                                                                       # a no-op
    torch.cuda.synchronize()
    for t in outs + [terms]:
        assert (t == (SENT if t.dtype == torch.float64 else 77)).all(), 'an output was written by a call that must launch nothing'
    # NULL frame_terms and NULL cyl_raw beside x0_in are accepted
    x0 = torch.from_numpy(scenes['F2']['ref']['x0'].reshape(1, 6)).to(dev)
    ptrs = [t.data_ptr() for t in outs]
    assert L.cpe_multi_frame_fit_lm_batch(s['Pd'].data_ptr(), s['cd'].data_ptr(), s['TAGVd'].data_ptr(), None, None, gs.data_ptr(), 1, 2, R,
                                          None, x0.data_ptr(), *ptrs, None, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert outs[6].item() == ST_OK and (terms == SENT).all()


# ------------------------------------------------------------------------------------------- 9 run_experiment(multi_frame='lm')
H, W, NF = 480, 640, 6


@pytest.mark.gpu
def test_run_experiment_lm_mode(cpe, gpu, tmp_path):
    """the folder of test_multiframe_fit_gpu.py::test_run_experiment_gpu_mode"""
    from PIL import Image
    from cpe_amd import experiment, synth
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
    nm = experiment.run_experiment(*args, chunk=4, multi_frame='gpu')
    print(f'fval: lm {lm["fval"]!r} gpu {nm["fval"]!r}')
    assert lm['T_cam_agv'] is not None and len(lm['T_cam_agv']) == 16 and np.isfinite(lm['T_cam_agv']).all()
    assert lm['fval'] <= nm['fval']
