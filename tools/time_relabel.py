"""Time the per-image re-labelling of the planar tables (cpe_grid_relabel_batch) at the Python layer: the call alone, and
fit.fit_single_plane_batch with and without relabel=.  The yardstick is the same call without the option.

    python tools/time_relabel.py [--frames 45 4096] [--reps 11] [--procs 3] [--child-timeout 400] [--out FILE]

Tables: analytic boards (the rig of cpe_amd.synth, 17 x 25 grid = 425 points, 16 seeded poses of up to 25 deg tilt repeated
over the frames, 0.25 px noise per frame), ids (row, col) with the true indices in both images, so that the selector and the
fit behind the re-labelling do the same work with and without it; the centre is the pixel of the grid point (0, 0).  Per size,
timed by the protocol of tools/timing.py between device events, one call:
    relabel          fit.grid_relabel_batch(both images' tables, 2 n images)
    plane            fit.fit_single_plane_batch(g1, g2, ...)
    plane_relabel    fit.fit_single_plane_batch(g1, g2, ..., relabel={}, center1=, center2=)"""
import argparse
import json
import sys

import timing


def make_boards(n, dev, seed=0, poses=16):
    """-> g1, g2 (fit.GridTables, ids (row, col)), c1, c2 (f64[n,2] centres), K1, K2, T21"""
    import numpy as np
    import torch
    from cpe_amd import fit, synth
    scene = synth.Scene(h=1200, w=1920)
    K1, K2, T21, Tp = synth.make_rig(scene)
    delta = scene.pitch_px / scene.focal
    Op = -Tp[:3, :3].T @ Tp[:3, 3]
    ii, jj = np.meshgrid(np.arange(-8, 9), np.arange(-12, 13), indexing='ij')
    d = np.stack([ii.ravel() * delta, jj.ravel() * delta, np.ones(ii.size)], 1) @ Tp[:3, :3]
    ids = np.stack([jj.ravel(), ii.ravel()], 1).astype(np.int32)
    zero = int(np.nonzero((ii.ravel() == 0) & (jj.ravel() == 0))[0][0])
    rng = np.random.default_rng(seed)
    uv = []
    for _ in range(poses):
        nrm = synth._rot(np.radians(rng.uniform(-25, 25)), np.radians(rng.uniform(-25, 25)), 0.0) @ np.array([0, 0, 1.0])
        c = np.array([27.0 + rng.uniform(-10, 10), rng.uniform(-10, 10), rng.uniform(330, 400)])
        X = Op + (((c - Op) @ nrm) / (d @ nrm))[:, None] * d
        p, q = X @ K1.T, (X @ T21[:3, :3].T + T21[:3, 3]) @ K2.T
        uv.append((p[:, :2] / p[:, 2:], q[:, :2] / q[:, 2:]))
    m = ids.shape[0]
    xy = np.zeros((2, n, fit.MAXP, 2)); idx = np.zeros((n, fit.MAXP, 2), np.int32); ctr = np.zeros((2, n, 2))
    for f in range(n):
        for k in range(2):
            xy[k, f, :m] = uv[f % poses][k] + rng.normal(0, 0.25, (m, 2))
            ctr[k, f] = uv[f % poses][k][zero]
        idx[f, :m] = ids
    cnt = torch.full((n,), m, dtype=torch.int32, device=dev)
    t = lambda a: torch.from_numpy(a).to(dev)
    tid = t(idx)
    return fit.GridTables(t(xy[0]), tid, cnt), fit.GridTables(t(xy[1]), tid.clone(), cnt.clone()), t(ctr[0]), t(ctr[1]), K1, K2, T21


def child(sizes, reps):
    import torch
    import cpe_amd  # noqa: F401
    from cpe_amd import fit
    dev = torch.device('cuda:0')
    for n in sizes:
        g1, g2, c1, c2, K1, K2, T21 = make_boards(n, dev)
        both, ctr = fit._cat_tables(g1, g2), torch.cat([c1, c2])
        first, ms = timing.time_variants(dict(
            relabel=lambda: fit.grid_relabel_batch(both, ctr),
            plane=lambda: fit.fit_single_plane_batch(g1, g2, K1, K2, T21, tau=1.0),
            plane_relabel=lambda: fit.fit_single_plane_batch(g1, g2, K1, K2, T21, tau=1.0, relabel={}, center1=c1, center2=c2)), reps)
        med = timing.medians(ms)
        same = bool(torch.equal(first['plane']['idx'], first['plane_relabel']['idx']) and torch.equal(first['plane']['P'], first['plane_relabel']['P']))
        print(json.dumps(dict(kind='relabel', frames=n, points=float(g1.cnt.double().mean()), reps=reps, median_ms=med,
                              relabel_over_plane=med['relabel'] / med['plane'], plane_relabel_over_plane=med['plane_relabel'] / med['plane'],
                              kept_all=int((first['relabel']['tables'].cnt == both.cnt).sum()), flagged=int(first['relabel']['flags'].ne(0).sum()),
                              same_planes=same, ms=ms)), flush=True)
        del first, g1, g2, both
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, nargs='*', default=[45, 4096])
    a = timing.parse(ap, reps=11, child_timeout=400.0)
    if a.child:
        return child(a.frames, a.reps)
    lines, emit = timing.run_children(__file__, a)
    for n in a.frames:
        rows = [d for d in lines if d['kind'] == 'relabel' and d['frames'] == n]
        emit(timing.ratio_summary(dict(kind='relabel_summary', frames=n, procs=a.procs), rows,
                                  (('relabel_over_plane', 'relabel', 'plane'), ('plane_relabel_over_plane', 'plane_relabel', 'plane'))))
    return 0


if __name__ == '__main__':
    sys.exit(main())
