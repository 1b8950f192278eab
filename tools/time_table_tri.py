"""Time single-camera triangulation from the laser-plane table (cpe_table_triangulate_batch) at the Python layer against the
stereo path it replaces, on the same grid-point tables, and FramePipeline with one camera against the stereo pipeline on the same
rendered frames.  The tables are analytic: the 17 x 25 grid of the projector of cpe_amd.synth.make_rig on seeded cylinders
(R = 45 mm, axis tilts +-8 deg, depth 330-400 mm) seen by both cameras with 0.25 px noise, thinned to `--points` points; the
laser-plane table is the rig's true one, -12..12.

    python tools/time_table_tri.py [--frames 45 4096] [--points 250] [--pipeline-frames 64] [--chunk 32] [--reps 11] [--procs 3]
                                   [--child-timeout 400] [--out FILE]

Per size, timed by the protocol of tools/timing.py between device events, one call:
    table_tri    fit.table_triangulate_batch(gp1, K1, None, table)               one camera
    select_tri   fit.select_triangulate_batch(gp1, gp2, K1, K2, T21)             chooseIdx + DLT: the step it replaces
    mono_fit     fit.fit_single_cylinder_mono_batch(gp1, K1, None, table, 45)    FIT_LM
    stereo_fit   fit.fit_single_cylinder_batch(gp1, gp2, K1, K2, T21, 45)        FIT_LM
and on `--pipeline-frames` rendered 1920 x 1200 pairs (0 = skip), in chunks of `--chunk`:
    pipe_left    FramePipeline(source='left', laser_table=table).run(left, None)
    pipe_stereo  FramePipeline().run(left, right)"""
import argparse
import json
import sys

import timing

RADIUS = 45.0


def rig_table(scene, lo, hi, dev):
    """the true laser planes of the scene's projector as a fit.LaserTable, family 0 = col"""
    import numpy as np
    import torch
    from cpe_amd import fit, synth
    Tp = synth.make_rig(scene)[3]
    delta = scene.pitch_px / scene.focal
    Op = -Tp[:3, :3].T @ Tp[:3, 3]
    P = np.zeros((2, hi - lo + 1, 4))
    for j, v in enumerate(range(lo, hi + 1)):
        for k, nn in enumerate((np.array([1.0, 0, -v * delta]), np.array([0, 1.0, -v * delta]))):
            w = nn @ Tp[:3, :3]
            w /= np.linalg.norm(w)
            P[k, j] = [*w, -w @ Op]
    return fit.LaserTable(torch.from_numpy(P).to(dev), torch.zeros((2, hi - lo + 1), dtype=torch.int32, device=dev), lo, hi,
                          torch.tensor([*Op, 0.0], dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev), 'col')


def make_tables(n, points, dev, seed=0):
    """-> gp1, gp2 (fit.GridTables of both cameras), K1, K2, T21, table"""
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
    xy = np.zeros((2, n, fit.MAXP, 2)); idx = np.zeros((n, fit.MAXP, 2), np.int32); cnt = np.zeros(n, np.int32)
    for f in range(n):
        az, ax = np.radians(rng.uniform(-8, 8, 2))
        a = np.array([np.sin(az), np.cos(az) * np.cos(ax), np.sin(ax) * np.cos(az)])
        a /= np.linalg.norm(a)
        c = np.array([27.0 + rng.uniform(-12, 12), rng.uniform(-10, 10), rng.uniform(330, 400)])
        wv = Op - c
        dp = d - (d @ a)[:, None] * a
        wp = wv - (wv @ a) * a
        A, B, Cc = (dp * dp).sum(1), 2 * dp @ wp, wp @ wp - RADIUS ** 2
        disc = B * B - 4 * A * Cc
        hit = np.nonzero(disc > 0)[0]
        keep = np.sort(rng.permutation(hit)[:points])
        s = (-B[keep] - np.sqrt(disc[keep])) / (2 * A[keep])
        X = Op + s[:, None] * d[keep]
        p = X @ K1.T
        q = (X @ T21[:3, :3].T + T21[:3, 3]) @ K2.T
        m = len(keep)
        xy[0, f, :m] = p[:, :2] / p[:, 2:] + 0.25 * rng.standard_normal((m, 2))
        xy[1, f, :m] = q[:, :2] / q[:, 2:] + 0.25 * rng.standard_normal((m, 2))
        idx[f, :m] = ids[keep]
        cnt[f] = m
    t = lambda a: torch.from_numpy(a).to(dev)
    idx_d, cnt_d = t(idx), t(cnt)
    return fit.GridTables(t(xy[0]), idx_d, cnt_d), fit.GridTables(t(xy[1]), idx_d, cnt_d), K1, K2, T21, rig_table(scene, -12, 12, dev)


def child(sizes, points, pipeline_frames, chunk, reps):
    import torch
    import cpe_amd  # noqa: F401
    from cpe_amd import fit, pipeline, synth
    dev = torch.device('cuda:0')
    for n in sizes:
        g1, g2, K1, K2, T21, tab = make_tables(n, points, dev)
        first, ms = timing.time_variants(dict(
            table_tri=lambda: fit.table_triangulate_batch(g1, K1, None, tab),
            select_tri=lambda: fit.select_triangulate_batch(g1, g2, K1, K2, T21),
            mono_fit=lambda: fit.fit_single_cylinder_mono_batch(g1, K1, None, tab, RADIUS, mode=fit.FIT_LM),
            stereo_fit=lambda: fit.fit_single_cylinder_batch(g1, g2, K1, K2, T21, RADIUS, mode=fit.FIT_LM)), reps)
        med = timing.medians(ms)
        print(json.dumps(dict(kind='tables', frames=n, points=float(g1.cnt.double().mean()), reps=reps, median_ms=med,
                              tri_over_select=med['table_tri'] / med['select_tri'], mono_over_stereo=med['mono_fit'] / med['stereo_fit'],
                              m_table=float(first['table_tri']['m'].double().mean()), m_select=float(first['select_tri']['m'].double().mean()),
                              res_rms=float(first['table_tri']['stats'][:, 0].mean()),
                              status_ok_mono=int((first['mono_fit']['status'] == 0).sum()),
                              status_ok_stereo=int((first['stereo_fit']['status'] == 0).sum()), ms=ms)), flush=True)
        del first, g1, g2, tab
        torch.cuda.empty_cache()
    if pipeline_frames > 0:
        b = synth.render_batch(pipeline_frames, 1200, 1920, seed=1, device=dev, with_gt=False)
        tab = rig_table(b['scene'], -max(b['scene'].half_lines, b['scene'].half_lines_v), max(b['scene'].half_lines, b['scene'].half_lines_v), dev)
        args = (1200, 1920, b['K1'], b['K2'], b['T21'], b['radius'])
        left, right = b['left'], b['right']
        mono = pipeline.FramePipeline(*args, chunk=chunk, device=dev, fit_mode=fit.FIT_LM, source='left', laser_table=tab)
        stereo = pipeline.FramePipeline(*args, chunk=chunk, device=dev, fit_mode=fit.FIT_LM)
        first, ms = timing.time_variants(dict(pipe_left=lambda: mono.run(left, None), pipe_stereo=lambda: stereo.run(left, right)), reps)
        med = timing.medians(ms)
        ok = lambda rec: int((pipeline.unpack_counters(rec[:, 15])[2] == 0).sum())
        print(json.dumps(dict(kind='pipeline', frames=pipeline_frames, chunk=chunk, reps=reps, median_ms=med,
                              left_over_stereo=med['pipe_left'] / med['pipe_stereo'], fit_ok_left=ok(first['pipe_left']),
                              fit_ok_stereo=ok(first['pipe_stereo']), ms=ms)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, nargs='*', default=[45, 4096])
    ap.add_argument('--points', type=int, default=250)
    ap.add_argument('--pipeline-frames', type=int, default=64)
    ap.add_argument('--chunk', type=int, default=32)
    a = timing.parse(ap, reps=11, child_timeout=400.0)
    if a.child:
        return child(a.frames, a.points, a.pipeline_frames, a.chunk, a.reps)
    lines, emit = timing.run_children(__file__, a)
    ratios = dict(tables=(('tri_over_select', 'table_tri', 'select_tri'), ('mono_over_stereo', 'mono_fit', 'stereo_fit')),
                  pipeline=(('left_over_stereo', 'pipe_left', 'pipe_stereo'),))
    for kind, sizes in (('tables', a.frames), ('pipeline', [a.pipeline_frames] if a.pipeline_frames > 0 else [])):
        for n in sizes:
            rows = [d for d in lines if d['kind'] == kind and d['frames'] == n]
            emit(timing.ratio_summary(dict(kind=kind + '_summary', frames=n, procs=a.procs), rows, ratios[kind]))
    return 0


if __name__ == '__main__':
    sys.exit(main())
