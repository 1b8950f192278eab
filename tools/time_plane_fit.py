"""Time the planar target's geometric half (cpe_fit_plane_batch, cpe_index_planes_batch) at the Python layer, with the
cylinder's Levenberg-Marquardt fit on the same point tables as the yardstick.  The tables are analytic: the 17 x 25 grid of
the projector of cpe_amd.synth.make_rig on seeded boards (tilts +-25 deg, depth 330-400 mm), 0.25 px noise, every 20th point
lifted 5-40 mm off the board, triangulated by fit.triangulate_batch; for the per-frame fit thinned to `--points` points.

    python tools/time_plane_fit.py [--frames 45 4096] [--points 250] [--table-frames 45 1024] [--reps 11] [--procs 3]
                                   [--child-timeout 400] [--out FILE]

Per size, timed by the protocol of tools/timing.py between device events, one call:
    plane       fit.fit_plane_batch(X, idx, cnt)                       fitplane, grid map, pose
    plane_trim  fit.fit_plane_batch(X, idx, cnt, tau=1.0)              the same behind the trimming loop
    lm          fit.fit_cylinder_batch(X, cnt, 45, mode=FIT_LM)        the yardstick
and for the table sizes (all 425 points of a frame)
    table       fit.index_planes_batch(X, idx, cnt, -12, 12)
    lm          as above, on these tables"""
import argparse
import json
import sys

import timing

RADIUS = 45.0


def make_tables(n, points, dev, seed=0, lift=True):
    """-> X f64[n,MAXP,3], idx i32[n,MAXP,2], cnt i32[n] on dev; lift=False leaves every point on its board"""
    import numpy as np
    import torch
    from cpe_amd import fit, synth
    scene = synth.Scene(h=1200, w=1920)
    K1, K2, T21, Tp = synth.make_rig(scene)
    delta = scene.pitch_px / scene.focal
    Op = -Tp[:3, :3].T @ Tp[:3, 3]
    ii, jj = np.meshgrid(np.arange(-8, 9), np.arange(-12, 13), indexing='ij')
    d = np.stack([ii.ravel() * delta, jj.ravel() * delta, np.ones(ii.size)], 1) @ Tp[:3, :3]
    ids = np.stack([ii.ravel(), jj.ravel()], 1).astype(np.int32)
    rng = np.random.default_rng(seed)
    p1 = np.zeros((n, fit.MAXP, 2)); p2 = np.zeros_like(p1); idx = np.zeros((n, fit.MAXP, 2), np.int32); cnt = np.zeros(n, np.int32)
    for f in range(n):
        ax, ay = np.radians(rng.uniform(-25, 25, 2))
        nrm = synth._rot(ax, ay, 0.0) @ np.array([0, 0, 1.0])
        c = np.array([27.0 + rng.uniform(-10, 10), rng.uniform(-10, 10), rng.uniform(330, 400)])
        keep = np.sort(rng.permutation(len(ids))[:points])
        X = Op + (((c - Op) @ nrm) / (d[keep] @ nrm))[:, None] * d[keep]
        if lift:
            X[::20] += (rng.uniform(5, 40, len(X[::20])) * rng.choice([-1, 1], len(X[::20])))[:, None] * nrm
        a = X @ K1.T
        b = (X @ T21[:3, :3].T + T21[:3, 3]) @ K2.T
        m = len(keep)
        p1[f, :m] = a[:, :2] / a[:, 2:] + 0.25 * rng.standard_normal((m, 2))
        p2[f, :m] = b[:, :2] / b[:, 2:] + 0.25 * rng.standard_normal((m, 2))
        idx[f, :m] = ids[keep]
        cnt[f] = m
    cnt_d = torch.from_numpy(cnt).to(dev)
    tri = fit.triangulate_batch(torch.from_numpy(p1).to(dev), torch.from_numpy(p2).to(dev), cnt_d, K1, K2, T21)
    return tri['pts3'], torch.from_numpy(idx).to(dev), cnt_d


def child(sizes, points, table_sizes, reps):
    import torch
    import cpe_amd  # noqa: F401
    from cpe_amd import fit
    dev = torch.device('cuda:0')
    for n in sizes:
        X, idx, cnt = make_tables(n, points, dev)
        first, ms = timing.time_variants(dict(plane=lambda: fit.fit_plane_batch(X, idx, cnt),
                                              plane_trim=lambda: fit.fit_plane_batch(X, idx, cnt, tau=1.0),
                                              lm=lambda: fit.fit_cylinder_batch(X, cnt, RADIUS, mode=fit.FIT_LM)), reps)
        med = timing.medians(ms)
        print(json.dumps(dict(kind='fit', frames=n, points=float(cnt.double().mean()), reps=reps, median_ms=med,
                              plane_over_lm=med['plane'] / med['lm'], trim_over_lm=med['plane_trim'] / med['lm'],
                              status_ok=int((first['plane']['status'] == 0).sum()), status_ok_trim=int((first['plane_trim']['status'] == 0).sum()),
                              inliers_trim=float(first['plane_trim']['n_inliers'].double().mean()),
                              refits_trim=float(first['plane_trim']['stats'][:, 6].mean()),
                              rms=float(first['plane']['stats'][:, 0].mean()), rms_trim=float(first['plane_trim']['stats'][:, 0].mean()),
                              lm_iters=float(first['lm']['iters'][:, 0].double().mean()), ms=ms)), flush=True)
        del first, X, idx, cnt
        torch.cuda.empty_cache()
    for n in table_sizes:
        X, idx, cnt = make_tables(n, 425, dev)
        first, ms = timing.time_variants(dict(table=lambda: fit.index_planes_batch(X, idx, cnt, -12, 12),
                                              lm=lambda: fit.fit_cylinder_batch(X, cnt, RADIUS, mode=fit.FIT_LM)), reps)
        med = timing.medians(ms)
        c = first['table']['centre'].cpu().tolist()
        print(json.dumps(dict(kind='table', frames=n, points=425.0, reps=reps, median_ms=med, table_over_lm=med['table'] / med['lm'],
                              lines_ok=int((first['table']['status'] == 0).sum()), centre_status=int(first['table']['centre_status']),
                              centre=c, ms=ms)), flush=True)
        del first, X, idx, cnt
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, nargs='*', default=[45, 4096])
    ap.add_argument('--points', type=int, default=250)
    ap.add_argument('--table-frames', type=int, nargs='*', default=[45, 1024])
    a = timing.parse(ap, reps=11, child_timeout=400.0)
    if a.child:
        return child(a.frames, a.points, a.table_frames, a.reps)
    lines, emit = timing.run_children(__file__, a)
    for kind, sizes, keys in (('fit', a.frames, ('plane', 'plane_trim')), ('table', a.table_frames, ('table',))):
        for n in sizes:
            rows = [d for d in lines if d['kind'] == kind and d['frames'] == n]
            emit(timing.ratio_summary(dict(kind=kind + '_summary', frames=n, points=rows[0]['points'], procs=a.procs), rows,
                                      [(f'{k}_over_lm', k, 'lm') for k in keys], skip=('trim_over_lm',)))   # the row's name for plane_trim_over_lm
    return 0


if __name__ == '__main__':
    sys.exit(main())
