"""Time the build-defined frame-angle solver (cpe_frame_angles_lm_batch: pan and tilt of every frame from a calibrated
camera-AGV pose) on the experiment's own size and on a run-time batch -- 45 and 4096 frames of 250 points each, from the scene
generator of tests/multiframe_cases.py, the pose the scenes were made with, the start from the frames' own per-frame fits.

    python tools/time_frame_angles.py [--frames 45 4096] [--points 250] [--reps 21] [--procs 3] [--child-timeout 300] [--out FILE]

Per size, timed by the protocol of tools/timing.py between device events, one call on preallocated outputs:
    solver   cpe_frame_angles_lm_batch (start, LM, chain and T * chain of the result)
    terms    cpe_multi_frame_terms on the same tables at the solver's result: one pass over the points, for scale -- the solver
             should cost about its objective evaluations + Jacobian passes (one per iteration) times that
The line of a size also carries the statuses, the iteration and evaluation counts (mean and maximum over the frames) and
passes = mean evaluations + mean iterations.
The scenes come from tests/multiframe_cases.py (the generator the GPU tests use): this file has to stay beside the tests."""
import argparse
import json
import sys

import timing

RADIUS = 45.0
SCENE_FRAMES = 45


def child(sizes, points, reps):
    import numpy as np
    import torch
    import cpe_amd  # noqa: F401
    import multiframe_cases as mc
    from cpe_amd import fit, lib, multiframe
    dev = torch.device('cuda:0')
    L = lib.load()
    for n in sizes:
        scenes = [mc.make_scene(SCENE_FRAMES, seed, noise=0.05, npts=points) for seed in range((n + SCENE_FRAMES - 1) // SCENE_FRAMES)]
        P = torch.from_numpy(np.concatenate([s[0] for s in scenes])[:n]).to(dev)
        cnt = torch.from_numpy(np.concatenate([s[1] for s in scenes])[:n]).to(dev)
        truth = np.concatenate([s[2] for s in scenes])[:n]
        T = torch.from_numpy(scenes[0][3].reshape(1, 16)).to(dev)               # the generator's pose does not depend on the seed
        raw = fit.fit_cylinder_batch(P, cnt, RADIUS)['cyl_raw'].contiguous()
        first = multiframe.estimate_frame_angles_gpu(P, cnt, raw, T, RADIUS)      # warm-up, and the figures of the line
        out = {k: torch.empty_like(v) for k, v in first.items()}
        terms = torch.empty(n, dtype=torch.float64, device=dev)
        stream = torch.cuda.current_stream().cuda_stream

        def solver():
            lib.check(L.cpe_frame_angles_lm_batch(P.data_ptr(), cnt.data_ptr(), raw.data_ptr(), T.data_ptr(), None, 1, n, RADIUS, None, None,
                                                  out['angles0'].data_ptr(), out['angles'].data_ptr(), out['fvals'].data_ptr(),
                                                  out['iters'].data_ptr(), out['TAGV'].data_ptr(), out['Tcyl'].data_ptr(),
                                                  out['status'].data_ptr(), stream), 'cpe_frame_angles_lm_batch')

        def one_pass():
            lib.check(L.cpe_multi_frame_terms(P.data_ptr(), cnt.data_ptr(), n, first['TAGV'].data_ptr(), T.data_ptr(), RADIUS,
                                              terms.data_ptr(), stream), 'cpe_multi_frame_terms')

        variants = dict(solver=solver, terms=one_pass)
        for f in variants.values():
            f()
        torch.cuda.synchronize()
        assert all(torch.equal(out[k], first[k]) for k in out), 'the call on preallocated outputs differs from the wrapper\'s'
        ms = timing.event_loop(variants, reps)
        it = first['iters'].cpu().numpy().astype(np.float64)
        ok = first['status'].cpu().numpy() == 0
        err = np.abs(first['angles'].cpu().numpy() - truth)[ok]
        med = timing.medians(ms)
        print(json.dumps(dict(kind='case', frames=n, points=points, reps=reps, median_ms=med, ratio=med['solver'] / med['terms'],
                              status_ok=int(ok.sum()), iters_mean=float(it[ok, 0].mean()), iters_max=int(it[ok, 0].max()),
                              evals_mean=float(it[ok, 1].mean()), evals_max=int(it[ok, 1].max()),
                              passes=float(it[ok, 0].mean() + it[ok, 1].mean()), max_error_rad=float(err.max()),
                              f_max=float(first['fvals'][:, 1].max()), ms=ms)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, nargs='+', default=[45, 4096])
    ap.add_argument('--points', type=int, default=250)
    a = timing.parse(ap, reps=21, child_timeout=300.0)
    if a.child:
        return child(a.frames, a.points, a.reps)
    lines, emit = timing.run_children(__file__, a)
    for n in a.frames:
        rows = [d for d in lines if d['kind'] == 'case' and d['frames'] == n]
        med, spread = timing.reduce(rows)
        emit(dict(kind='summary', frames=n, points=a.points, procs=a.procs, solver_ms=med['solver'], terms_ms=med['terms'],
                  solver_spread_ms=spread['solver'], terms_spread_ms=spread['terms'], ratio=med['solver'] / med['terms'],
                  passes=rows[0]['passes'], iters_mean=rows[0]['iters_mean'], iters_max=rows[0]['iters_max'],
                  evals_mean=rows[0]['evals_mean'], evals_max=rows[0]['evals_max'], status_ok=rows[0]['status_ok'],
                  max_error_rad=rows[0]['max_error_rad']))
    return 0


if __name__ == '__main__':
    sys.exit(main())
