"""Time the predicted grid and the re-numbering against it (cpe_grid_predict_batch, cpe_grid_assign_batch) and the refinement
loop built on them at the Python layer, on the grid-point tables of tools/time_table_tri.py (the 17 x 25 grid of the projector of
cpe_amd.synth.make_rig on seeded cylinders, 0.25 px noise, thinned to `--points` points; the rig's true table, -12..12: 625 nodes).

    python tools/time_grid_refine.py [--frames 45 4096] [--points 250 425] [--reps 11] [--procs 3] [--child-timeout 400] [--out FILE]

Per size, timed by the protocol of tools/timing.py between device events, one call:
    predict      fit.grid_predict_batch(cyl, 45, K1, K2, T21, table)                      the poses of stereo_fit
    assign       fit.grid_assign_batch(gp1, pred, 1)                                      one image against 625 nodes
    fused_fit    fit.fit_single_cylinder_fused_batch(gp1, gp2, K1, K2, T21, table, 45)    FIT_LM
    stereo_fit   fit.fit_single_cylinder_batch(gp1, gp2, K1, K2, T21, 45)                 FIT_LM
    refined_1    fit.fit_single_cylinder_refined_batch(..., rounds=1)                     first and rounds FIT_LM
    refined_2    fit.fit_single_cylinder_refined_batch(..., rounds=2)"""
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
        for pts in points:
            g1, g2, K1, K2, T21, tab = make_tables(n, pts, dev)
            cyl = fit.fit_single_cylinder_batch(g1, g2, K1, K2, T21, RADIUS, mode=fit.FIT_LM)['cyl'][:, 1].contiguous()
            pred = fit.grid_predict_batch(cyl, RADIUS, K1, K2, T21, tab)
            lm = dict(first=dict(mode=fit.FIT_LM), mode=fit.FIT_LM)
            first, ms = timing.time_variants(dict(
                predict=lambda: fit.grid_predict_batch(cyl, RADIUS, K1, K2, T21, tab),
                assign=lambda: fit.grid_assign_batch(g1, pred, 1),
                fused_fit=lambda: fit.fit_single_cylinder_fused_batch(g1, g2, K1, K2, T21, tab, RADIUS, mode=fit.FIT_LM),
                stereo_fit=lambda: fit.fit_single_cylinder_batch(g1, g2, K1, K2, T21, RADIUS, mode=fit.FIT_LM),
                refined_1=lambda: fit.fit_single_cylinder_refined_batch(g1, g2, K1, K2, T21, tab, RADIUS, rounds=1, **lm),
                refined_2=lambda: fit.fit_single_cylinder_refined_batch(g1, g2, K1, K2, T21, tab, RADIUS, rounds=2, **lm)), reps)
            med = timing.medians(ms)
            mean = lambda t: float(t.double().mean())
            print(json.dumps(dict(kind='tables', frames=n, points=mean(g1.cnt), nodes=pred['Nu'] * pred['Nv'], reps=reps, median_ms=med,
                                  refined_1_over_fused_fit=med['refined_1'] / med['fused_fit'],
                                  refined_2_over_fused_fit=med['refined_2'] / med['fused_fit'],
                                  visible_1=mean(first['predict']['counts'][:, 1]), kept=mean(first['assign']['m']),
                                  renumbered=mean(first['assign']['counts'][:, 2]), dist_rms_px=mean(first['assign']['stats'][:, 0]),
                                  taken_2=int((first['refined_2']['round_taken'] == 2).sum()),
                                  status_ok_refined=int((first['refined_2']['status'] == 0).sum()),
                                  status_ok_fused=int((first['fused_fit']['status'] == 0).sum()), ms=ms)), flush=True)
            del first, g1, g2, tab, pred, cyl
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, nargs='*', default=[45, 4096])
    ap.add_argument('--points', type=int, nargs='*', default=[250, 425])
    a = timing.parse(ap, reps=11, child_timeout=400.0)
    if a.child:
        return child(a.frames, a.points, a.reps)
    lines, emit = timing.run_children(__file__, a)
    ratios = (('refined_1_over_fused_fit', 'refined_1', 'fused_fit'), ('refined_2_over_fused_fit', 'refined_2', 'fused_fit'))
    for n in a.frames:
        for i in range(len(a.points)):
            rows = [d for d in lines if d['kind'] == 'tables' and d['frames'] == n][i::len(a.points)]
            emit(timing.ratio_summary(dict(kind='tables_summary', frames=n, procs=a.procs), rows, ratios))
    return 0


if __name__ == '__main__':
    sys.exit(main())
