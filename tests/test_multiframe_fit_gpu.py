"""The resident multi-frame camera-AGV fit: cpe_multi_frame_fit_batch / multiframe.fit_multi_frame_gpu, the pose utilities
cpe_pose_vec2T_batch / cpe_pose_T2vec_batch and experiment.run_experiment(multi_frame='gpu').

Two yardsticks (the kernel calls the device math library for sin / cos / acos, the oracle glibc):
  A  bit for bit, no tolerance: the kernel against its own pieces driven from the host -- multiframe.nelder_mead6 around
     cpe_pose_vec2T_batch + cpe_multi_frame_terms, the terms added on the host in frame order, from the kernel's x0.
  B  against the oracle (orc.multi_fit) from the oracle's x0, on the scenes test_multiframe_cases_cpu.py found stable:
     x, iterations and evaluations equal, fvals to 1e-12 relative, rotation of T to 1e-14, translation of T equal; and with
     the device's own initial pose: x0 to 1e-9, fvals against orc.multi_objective at the returned poses to 1e-12 relative,
     f <= f0, |f - oracle's f| <= 1e-5 (the optimiser's TolFun)."""
import ctypes as C
import json
import math

import numpy as np
import pytest

import multiframe_cases as mc

R = mc.RADIUS
ST_OK, ST_FEW, ST_OVERFLOW = 0, 5, 6
NAMES = sorted(mc.CASES)


def host(res):
    """a result of fit_multi_frame_gpu as numpy arrays (synchronises)"""
    return {k: v.cpu().numpy() for k, v in res.items() if k != 'TAGV'}


def bits_equal(a, b, keys=('x0', 'x', 'T', 'fvals', 'iters', 'n_used', 'status')):
    return all(np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)) for k in keys)


def group_of(r, g):
    return {k: v[g:g + 1] for k, v in r.items()}


def assert_failed_group(r, g, status):
    assert r['status'][g] == status
    for k in ('x0', 'x', 'T', 'fvals', 'iters', 'n_used'):
        assert not r[k][g].any(), f'{k} of a group with status {status} must be zero'


@pytest.fixture(scope='module')
def scenes(cpe, orc, gpu):
    """name -> the scene on the host and on the device, its per-frame fits (fitCylinderWPts3 on the GPU, which the existing
    tests pin to the oracle's) and the oracle's multi-frame fit: computed once"""
    import torch
    from cpe_amd import fit
    out = {}
    for name in NAMES:
        P, cnt, angles, _ = mc.case_scene(name)
        TAGV = np.stack([orc.get_TAGVcyl(*a) for a in angles])
        Pd, cd = torch.from_numpy(P).to(gpu), torch.from_numpy(cnt).to(gpu)
        per = fit.fit_cylinder_batch(Pd, cd, R)
        assert not per['status'].any()
        raw = per['cyl_raw'].cpu().numpy()
        out[name] = dict(P=P, cnt=cnt, angles=angles, TAGV=TAGV, raw=raw, Pd=Pd, cd=cd, rawd=per['cyl_raw'].contiguous(),
                         TAGVd=torch.from_numpy(TAGV).to(gpu), ref=orc.multi_fit(P, cnt, TAGV, raw, R))
    return out


def fit_gpu(s, **kw):
    from cpe_amd import multiframe
    return host(multiframe.fit_multi_frame_gpu(s['Pd'], s['cd'], s['rawd'], s['TAGVd'], R, **kw))


@pytest.fixture(scope='module')
def single(scenes):
    """name -> the one-group call with the device's initial pose: shared by the tests that compare against it"""
    return {name: fit_gpu(scenes[name]) for name in NAMES}


class PiecesObjective:
    """dist() from the exported pieces: cpe_pose_vec2T_batch, cpe_multi_frame_terms, the terms added on the host in frame order"""

    def __init__(self, cpe, s):
        import torch
        self.torch, self.mf, self.L, self.s = torch, cpe.multiframe, cpe.lib.load(), s
        self.F = len(s['cnt'])
        self.terms = torch.zeros(self.F, dtype=torch.float64, device=s['Pd'].device)

    def __call__(self, x):
        torch, s = self.torch, self.s
        T = self.mf.vec2T_batch(torch.tensor([x], dtype=torch.float64).to(s['Pd'].device))
        rc = self.L.cpe_multi_frame_terms(s['Pd'].data_ptr(), s['cd'].data_ptr(), self.F, s['TAGVd'].data_ptr(), T.data_ptr(), R,
                                          self.terms.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        v = 0.0
        for t in self.terms.tolist():
            v = v + t
        return v


def check_against_pieces(cpe, s, got, **tol):
    import torch
    assert got['status'][0] == ST_OK and got['n_used'][0] == len(s['cnt'])
    obj = PiecesObjective(cpe, s)
    x0 = got['x0'][0].tolist()
    nm = dict(tolx=tol.get('tol_x', 1e-5), tolf=tol.get('tol_f', 1e-5), maxiter=tol.get('max_iter', 100000),
              maxfun=tol.get('max_fun_evals', 100000))
    f0 = obj(x0)
    x, f, iters, evals = cpe.multiframe.nelder_mead6(obj, x0, **nm)
    print(f'pieces: iters {iters} evals {evals} f0 {f0!r} f {f!r}; kernel: {got["iters"][0].tolist()} {got["fvals"][0].tolist()}')
    assert got['iters'][0].tolist() == [iters, evals]
    assert got['fvals'][0].tolist() == [f0, f]
    assert got['x'][0].tolist() == x
    T = cpe.multiframe.vec2T_batch(torch.from_numpy(got['x']).to(s['Pd'].device)).cpu().numpy()
    assert np.array_equal(got['T'], T)
    return iters, evals


# ---------------------------------------------------------------------------------------------------------- yardstick A
@pytest.mark.gpu
@pytest.mark.parametrize('name', NAMES)
def test_kernel_equals_its_pieces_driven_from_the_host(cpe, scenes, single, name):
    check_against_pieces(cpe, scenes[name], single[name])


@pytest.mark.gpu
def test_kernel_equals_its_pieces_early_stop_and_tolerances(cpe, scenes, single):
    s = scenes['F3']
    iters, evals = check_against_pieces(cpe, s, fit_gpu(s, max_fun_evals=20), max_fun_evals=20)
    assert 20 <= evals <= 27                      # fminsearch looks at the bound once per iteration (an iteration that shrinks makes 8 evaluations)
    s = scenes['F17']
    loose = fit_gpu(s, tol_x=1e-2, tol_f=1e-2)
    iters, evals = check_against_pieces(cpe, s, loose, tol_x=1e-2, tol_f=1e-2)
    assert iters < single['F17']['iters'][0, 0]


# ---------------------------------------------------------------------------------------------------------- yardstick B
@pytest.mark.gpu
@pytest.mark.parametrize('name', NAMES)
def test_from_the_oracles_x0(scenes, name):
    s = scenes[name]
    ref = s['ref']
    got = fit_gpu(s, x0=ref['x0'].reshape(1, 6))
    assert got['status'][0] == ST_OK
    assert np.array_equal(got['x0'][0], ref['x0'])
    rel = np.abs(got['fvals'][0] - ref['fvals']) / np.abs(ref['fvals'])
    dT = np.abs(got['T'][0] - ref['T']).reshape(4, 4)
    print(f'{name}: iters {got["iters"][0].tolist()} oracle {[ref["iters"], ref["evals"]]} fvals rel {rel} dR {dT[:3, :3].max():.3g}')
    assert got['iters'][0].tolist() == [ref['iters'], ref['evals']]
    assert np.array_equal(got['x'][0], ref['x'])
    assert (rel <= 1e-12).all()
    assert dT[:3, :3].max() <= 1e-14
    assert np.array_equal(got['T'][0].reshape(4, 4)[:, 3], ref['T'].reshape(4, 4)[:, 3])
    assert np.array_equal(got['T'][0][12:], [0, 0, 0, 1])


@pytest.mark.gpu
@pytest.mark.parametrize('name', NAMES)
def test_device_initial_pose(orc, scenes, single, name):
    s, got = scenes[name], single[name]
    ref = s['ref']
    assert got['status'][0] == ST_OK and got['n_used'][0] == len(s['cnt'])
    x0, x, fv = got['x0'][0], got['x'][0], got['fvals'][0]
    d_rot = np.abs(x0[:3] - ref['x0'][:3]).max()
    d_tr = (np.abs(x0[3:] - ref['x0'][3:]) / np.abs(ref['x0'][3:])).max()
    want = [orc.multi_objective(x0, s['P'], s['cnt'], s['TAGV'], R), orc.multi_objective(x, s['P'], s['cnt'], s['TAGV'], R)]
    rel = [abs(fv[k] - want[k]) / abs(want[k]) for k in range(2)]
    print(f'{name}: x0 rotation {d_rot:.3g} translation {d_tr:.3g}; fvals {fv.tolist()} rel to oracle objective {rel}; '
          f'oracle fit f {ref["fvals"][1]!r} diff {abs(fv[1] - ref["fvals"][1]):.3g}; iters {got["iters"][0].tolist()}')
    assert d_rot <= 1e-9 and d_tr <= 1e-9
    assert max(rel) <= 1e-12
    assert fv[1] <= fv[0]
    assert abs(fv[1] - ref['fvals'][1]) <= 1e-5


# --------------------------------------------------------------------------------------------------------------- groups
def stacked(scenes, order):
    """the scenes of `order` in one table; None = an empty group.  -> scene-like dict, group_start, names per group"""
    import torch
    parts = [scenes[n] for n in order if n is not None]
    s = {k: torch.cat([p[k] for p in parts]).contiguous() for k in ('Pd', 'cd', 'rawd', 'TAGVd')}
    gs = [0]
    for n in order:
        gs.append(gs[-1] + (len(scenes[n]['cnt']) if n is not None else 0))
    return s, gs


@pytest.mark.gpu
@pytest.mark.parametrize('order', [NAMES, [NAMES[3], None, NAMES[0], NAMES[2], NAMES[1]]], ids=['in_order', 'reordered_with_empty'])
def test_groups_equal_single_calls(scenes, single, order):
    s, gs = stacked(scenes, order)
    got = fit_gpu(s, group_start=gs)
    assert len(got['status']) == len(order)
    for g, name in enumerate(order):
        if name is None:
            assert_failed_group(got, g, ST_FEW)
        else:
            assert bits_equal(group_of(got, g), single[name]), f'group {g} ({name}) differs from its single call'


# ------------------------------------------------------------------------------------------------------------- frame_ok
@pytest.mark.gpu
def test_frame_ok_equals_gathered_frames(scenes):
    import torch
    s = scenes['F17']
    F = len(s['cnt'])
    ok = np.ones(F, np.int32)
    ok[[0, 5, 16]] = 0
    got = fit_gpu(s, frame_ok=torch.from_numpy(ok).to(s['Pd'].device))
    keep = torch.from_numpy(np.flatnonzero(ok)).to(s['Pd'].device)
    gathered = {k: s[k][keep].contiguous() for k in ('Pd', 'cd', 'rawd', 'TAGVd')}
    want = fit_gpu(gathered)
    assert want['status'][0] == ST_OK and got['n_used'][0] == F - 3
    assert bits_equal(got, want)
    ok[:] = 0
    ok[7] = 1
    assert_failed_group(fit_gpu(s, frame_ok=torch.from_numpy(ok).to(s['Pd'].device)), 0, ST_FEW)


# ------------------------------------------------------------------------------------------------ statuses and arguments
@pytest.mark.gpu
def test_group_ranges(scenes, single):
    s = scenes['F3']
    got = fit_gpu(s, group_start=[3, 0])
    assert_failed_group(got, 0, ST_OVERFLOW)                        # runs backwards
    got = fit_gpu(s, group_start=[0, 3, 4])
    assert bits_equal(group_of(got, 0), single['F3'])
    assert_failed_group(got, 1, ST_OVERFLOW)                        # ends past n
    assert_failed_group(fit_gpu(s, group_start=[-1, 3]), 0, ST_OVERFLOW)


@pytest.mark.gpu
def test_more_kept_frames_than_a_group_holds(cpe, gpu):
    import torch
    MAXF = 1024
    n = MAXF + 1
    pts = torch.zeros((mc.MAXP, 3), dtype=torch.float64)
    pts[:5] = torch.tensor([[40.0, -50, 400], [45, -20, 395], [50, 0, 400], [42, 20, 398], [48, 50, 402]])
    s = dict(Pd=pts.to(gpu).expand(n, -1, -1).contiguous(), cd=torch.full((n,), 5, dtype=torch.int32, device=gpu),
             rawd=torch.zeros((n, 2, 6), dtype=torch.float64, device=gpu),
             TAGVd=torch.eye(4, dtype=torch.float64, device=gpu).reshape(1, 16).expand(n, -1).contiguous())
    x0 = [[0.0] * 6]
    assert_failed_group(fit_gpu(s, x0=x0, max_fun_evals=10), 0, ST_OVERFLOW)
    ok = torch.ones(n, dtype=torch.int32, device=gpu)
    ok[3] = 0
    got = fit_gpu(s, x0=x0, max_fun_evals=10, frame_ok=ok)          # exactly CPE_MULTI_MAXF kept frames are fitted
    assert got['status'][0] == ST_OK and got['n_used'][0] == MAXF and np.isfinite(got['fvals']).all()


@pytest.mark.gpu
def test_second_kept_frame_without_points(scenes, single):
    import torch
    s, gs = stacked(scenes, ['F2', 'F3', 'F3'])
    s['cd'] = s['cd'].clone()
    s['cd'][gs[1] + 1] = 0
    got = fit_gpu(s, group_start=gs)
    assert bits_equal(group_of(got, 0), single['F2']) and bits_equal(group_of(got, 2), single['F3'])
    assert_failed_group(got, 1, ST_FEW)
    # a frame without points beyond the first two is kept and contributes the term 0 (documented deviation)
    s['cd'][gs[1] + 1] = scenes['F3']['cd'][1]
    s['cd'][gs[1] + 2] = 0
    got = fit_gpu(s, group_start=gs[1:3])
    assert got['status'][0] == ST_OK and got['n_used'][0] == 3


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

    def call(G=1, params=None, null_out=None):
        ptrs = [t.data_ptr() for t in outs]
        if null_out is not None:
            ptrs[null_out] = None
        return L.cpe_multi_frame_fit_batch(s['Pd'].data_ptr(), s['cd'].data_ptr(), s['TAGVd'].data_ptr(), s['rawd'].data_ptr(), None,
                                           gs.data_ptr(), G, 2, R, C.addressof(params) if params is not None else None, None, *ptrs,
                                           torch.cuda.current_stream().cuda_stream)

    for k in range(len(outs)):
        assert call(null_out=k) == -1, f'NULL output {k}'
    assert call(G=-1) == -1
    assert call(params=cpe.lib.CpeFitParams(1e-5, 1e-5, 100000, 100000, 1, 0)) == -1          # CPE_FIT_LM
    assert call(params=cpe.lib.CpeFitParams(1e-5, 1e-5, 0, 100000, 0, 0)) == -1
    assert b'cpe_multi_frame_fit_batch' in L.cpe_last_error_string()
    assert call(G=0) == 0                                                                       # a no-op
    torch.cuda.synchronize()
    for t in outs:
        assert (t == (SENT if t.dtype == torch.float64 else 77)).all(), 'an output was written by a call that must launch nothing'


# ---------------------------------------------------------------------------------------------------------- cpe_pose_*
def rotvec_T(v, t=(0.0, 0.0, 0.0)):
    """exact-enough 4x4 of a rotation vector, built on the host with the oracle-independent Rodrigues formula"""
    v = np.asarray(v, dtype=np.float64)
    th = np.linalg.norm(v)
    K = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]]) / th
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)
    T[:3, 3] = t
    return T


@pytest.fixture(scope='module')
def poses():
    rng = np.random.default_rng(5)
    x = []
    while len(x) < 64:
        v = rng.standard_normal(3)
        th = rng.uniform(0.0, math.pi)
        if math.sin(th) >= 0.1:
            x.append(np.concatenate([v / np.linalg.norm(v) * th, rng.uniform(-500, 500, 3)]))
    return np.array(x)


@pytest.mark.gpu
def test_pose_vec2T_and_T2vec_against_the_oracle(cpe, orc, gpu, poses):
    import torch
    mf = cpe.multiframe
    T = mf.vec2T_batch(torch.from_numpy(poses).to(gpu))
    back = mf.T2vec_batch(T).cpu().numpy()
    T = T.cpu().numpy()
    wantT = np.stack([orc.vec2T(x) for x in poses])
    assert np.abs(T - wantT).max() <= 1e-14
    assert np.array_equal(T[:, [3, 7, 11]], poses[:, 3:]) and np.array_equal(T[:, 12:], np.tile([0.0, 0, 0, 1], (64, 1)))
    x = mf.T2vec_batch(torch.from_numpy(wantT).to(gpu)).cpu().numpy()
    wantx = np.stack([orc.T2vec(t) for t in wantT])
    assert np.abs(x[:, :3] - wantx[:, :3]).max() <= 1e-13 and np.array_equal(x[:, 3:], wantx[:, 3:])
    # the round trip T2vec(vec2T(x)) on the same poses
    assert np.abs(back[:, :3] - poses[:, :3]).max() <= 1e-13 and np.array_equal(back[:, 3:], poses[:, 3:])


@pytest.mark.gpu
def test_pose_small_angles_and_half_turns(cpe, orc, gpu):
    import torch
    mf = cpe.multiframe
    small = np.array([[0.0, 0, 0, 1, 2, 3], [5e-7, -5e-7, 5e-7, -1, 0, 4], [0, 9.9e-7, 0, 0, 0, 0]])
    T = mf.vec2T_batch(torch.from_numpy(small).to(gpu)).cpu().numpy().reshape(-1, 4, 4)
    for k in range(3):
        assert np.array_equal(T[k, :3, :3], np.eye(3)) and np.array_equal(T[k, :3, 3], small[k, 3:])     # |theta| < 1e-6: exactly I
    # the near-0 branch of T2vec
    near0 = np.stack([orc.vec2T([2e-5, -1e-5, 3e-5, 1, 2, 3]), np.eye(4).ravel()])
    x = mf.T2vec_batch(torch.from_numpy(near0).to(gpu)).cpu().numpy()
    assert np.abs(x - np.stack([orc.T2vec(t) for t in near0])).max() <= 1e-13
    # rotations by exactly pi: about each axis and about (1, -1, 0) / sqrt(2) -- the near-pi branch and its a / b / c selection
    axes = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1 / math.sqrt(2), -1 / math.sqrt(2), 0)]
    Ts = np.stack([rotvec_T(np.array(a) * math.pi, (1.0, -2.0, 3.0)).ravel() for a in axes])
    x = mf.T2vec_batch(torch.from_numpy(Ts).to(gpu)).cpu().numpy()
    want = np.stack([orc.T2vec(t) for t in Ts])
    assert np.abs(x - want).max() <= 1e-13
    for k, a in enumerate(axes):                                        # (the half turn itself, up to the sign of the axis)
        assert min(np.abs(x[k, :3] - np.array(a) * math.pi).max(), np.abs(x[k, :3] + np.array(a) * math.pi).max()) <= 1e-7
    # n = 0
    L = cpe.lib.load()
    assert L.cpe_pose_vec2T_batch(None, 0, None, None) == 0 and L.cpe_pose_T2vec_batch(None, 0, None, None) == 0
    assert L.cpe_pose_vec2T_batch(None, -1, None, None) == -1
    assert mf.vec2T_batch(torch.zeros((0, 6), dtype=torch.float64, device=gpu)).shape == (0, 16)
    assert mf.T2vec_batch(torch.zeros((0, 16), dtype=torch.float64, device=gpu)).shape == (0, 6)


# ----------------------------------------------------------------------------------------- run_experiment(multi_frame='gpu')
H, W, NF = 480, 640, 6


@pytest.mark.gpu
def test_run_experiment_gpu_mode(cpe, gpu, tmp_path):
    import torch
    from PIL import Image
    from cpe_amd import experiment, multiframe, pipeline, synth
    b = synth.render_batch(NF, H, W, seed=0, with_gt=False)
    stems = ['-10', '-21', '00', '1-2', '11', '2-1']
    L, Rr = b['left'].numpy(), b['right'].numpy()
    for i, st in enumerate(stems):
        Image.fromarray(L[i]).save(tmp_path / f'{st}L.png')
        Image.fromarray(Rr[i]).save(tmp_path / f'{st}R.png')
    for side in 'LR':
        Image.fromarray(np.zeros((H, W), np.uint8)).save(tmp_path / f'3-3{side}.png')                   # sorts last: a black pair
    lens = lambda K: dict(IntrinsicMatrix=np.asarray(K, dtype=np.float64).tolist(), RadialDistortion=[0.012, -0.004],
                          TangentialDistortion=[0.0002, -0.0001])
    (tmp_path / 'cam.json').write_text(json.dumps(dict(LeftCamera=lens(b['K1']), RightCamera=lens(b['K2']))))
    args = (str(tmp_path), str(tmp_path / 'cam.json'), b['K1'], b['K2'], b['T21'], b['radius'])
    res = experiment.run_experiment(*args, chunk=4, multi_frame='gpu')
    plain = experiment.run_experiment(*args, chunk=4, multi_frame=False)
    assert plain['T_cam_agv'] is None and torch.equal(res['records'].view(torch.int64), plain['records'].view(torch.int64))
    assert res['skipped'] == plain['skipped'] and res['skipped'][-1]['index'] == NF
    good = [i for i in range(NF + 1) if i not in {s['index'] for s in res['skipped']}]
    assert len(good) >= 2, 'the scene must hold frames that are fitted'
    # the direct call on the gathered good frames
    g = torch.tensor(good, device=gpu)
    want = multiframe.group_result(multiframe.fit_multi_frame_gpu(res['pts3'][g], res['cnt'][g], res['cyl_raw'][g], res['angles'][good],
                                                                  b['radius']))
    assert want['status'] == ST_OK and want['n_used'] == len(good)
    assert res['T_cam_agv'] == want['T'] and res['fval'] == want['fvals'][1] and len(res['T_cam_agv']) == 16
    assert sorted(want) == sorted(['T', 'x', 'x0', 'fvals', 'iters', 'evals', 'TAGV', 'n_used', 'status'])
    # fewer than two fitted frames: the host path's warning, no result
    for st in stems[1:]:
        for side in 'LR':
            Image.fromarray(np.zeros((H, W), np.uint8)).save(tmp_path / f'{st}{side}.png')
    with pytest.warns(UserWarning, match='fitted frame'):
        few = experiment.run_experiment(*args, chunk=4, multi_frame='gpu')
    assert few['T_cam_agv'] is None and few['fval'] is None
