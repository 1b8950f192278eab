"""Time fused triangulation (cpe_fused_triangulate_batch: both cameras' rays and the laser planes in one solve) at the Python
layer against the two routes it joins, on the same grid-point tables: those of tools/time_table_tri.py (the 17 x 25 grid of the
projector of cpe_amd.synth.make_rig on seeded cylinders, 0.25 px noise, thinned to `--points` points, the same points in both
cameras, so every fused point is a pair; the rig's true table, -12..12).

    python tools/time_fused_tri.py [--frames 45 4096] [--points 250] [--reps 11] [--procs 3] [--child-timeout 400] [--out FILE]

Per size, timed by the protocol of tools/timing.py between device events, one call:
    fused_tri    fit.fused_triangulate_batch(gp1, gp2, K1, K2, T21, table)
    select_tri   fit.select_triangulate_batch(gp1, gp2, K1, K2, T21)             chooseIdx + DLT
    table_tri    fit.table_triangulate_batch(gp1, K1, None, table)               one camera
    fused_fit    fit.fit_single_cylinder_fused_batch(gp1, gp2, K1, K2, T21, table, 45)   FIT_LM
    stereo_fit   fit.fit_single_cylinder_batch(gp1, gp2, K1, K2, T21, 45)                FIT_LM"""
import argparse
import json
import sys

import timing

RADIUS = 45.0


def child(sizes, points, reps):
    import torch
    import cpe_amd  # noqa: F401
    from cpe_amd import fit
    from time_table_tri import make_tables
    dev = torch.device('cuda:0')
    for n in sizes:
        g1, g2, K1, K2, T21, tab = make_tables(n, points, dev)
        first, ms = timing.time_variants(dict(
            fused_tri=lambda: fit.fused_triangulate_batch(g1, g2, K1, K2, T21, tab),
            select_tri=lambda: fit.select_triangulate_batch(g1, g2, K1, K2, T21),
            table_tri=lambda: fit.table_triangulate_batch(g1, K1, None, tab),
            fused_fit=lambda: fit.fit_single_cylinder_fused_batch(g1, g2, K1, K2, T21, tab, RADIUS, mode=fit.FIT_LM),
            stereo_fit=lambda: fit.fit_single_cylinder_batch(g1, g2, K1, K2, T21, RADIUS, mode=fit.FIT_LM)), reps)
        med = timing.medians(ms)
        mean = lambda t: float(t.double().mean())
        print(json.dumps(dict(kind='tables', frames=n, points=mean(g1.cnt), reps=reps, median_ms=med,
                              fused_over_select=med['fused_tri'] / med['select_tri'], fused_over_table=med['fused_tri'] / med['table_tri'],
                              fused_fit_over_stereo_fit=med['fused_fit'] / med['stereo_fit'],
                              m_fused=mean(first['fused_tri']['m']), m_select=mean(first['select_tri']['m']), m_table=mean(first['table_tri']['m']),
                              ray_rms_px=mean(first['fused_tri']['stats'][:, 0]), plane_rms_mm=mean(first['fused_tri']['stats'][:, 2]),
                              status_ok_fused=int((first['fused_fit']['status'] == 0).sum()),
                              status_ok_stereo=int((first['stereo_fit']['status'] == 0).sum()), ms=ms)), flush=True)
        del first, g1, g2, tab
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, nargs='*', default=[45, 4096])
    ap.add_argument('--points', type=int, default=250)
    a = timing.parse(ap, reps=11, child_timeout=400.0)
    if a.child:
        return child(a.frames, a.points, a.reps)
    lines, emit = timing.run_children(__file__, a)
    ratios = (('fused_over_select', 'fused_tri', 'select_tri'), ('fused_over_table', 'fused_tri', 'table_tri'),
              ('fused_fit_over_stereo_fit', 'fused_fit', 'stereo_fit'))
    for n in a.frames:
        rows = [d for d in lines if d['kind'] == 'tables' and d['frames'] == n]
        emit(timing.ratio_summary(dict(kind='tables_summary', frames=n, procs=a.procs), rows, ratios))
    return 0


if __name__ == '__main__':
    sys.exit(main())
