"""Time the predicted grid and the re-numbering against it (cpe_grid_predict_batch, cpe_grid_assign_batch) and the refinement
loop built on them at the Python layer, on the grid-point tables of tools/time_table_tri.py (the 17 x 25 grid of the projector of
cpe_amd.synth.make_rig on seeded cylinders, 0.25 px noise, thinned to `--points` points; the rig's true table, -12..12: 625 nodes).

    python tools/time_grid_refine.py [--frames 45 4096] [--points 250 425] [--reps 11] [--procs 3] [--child-timeout 400] [--out FILE]

Per size, alternated inside one process, the time between two device events around one call:
    predict      fit.grid_predict_batch(cyl, 45, K1, K2, T21, table)                      the poses of stereo_fit
    assign       fit.grid_assign_batch(gp1, pred, 1)                                      one image against 625 nodes
    fused_fit    fit.fit_single_cylinder_fused_batch(gp1, gp2, K1, K2, T21, table, 45)    FIT_LM
    stereo_fit   fit.fit_single_cylinder_batch(gp1, gp2, K1, K2, T21, 45)                 FIT_LM
    refined_1    fit.fit_single_cylinder_refined_batch(..., rounds=1)                     first and rounds FIT_LM
    refined_2    fit.fit_single_cylinder_refined_batch(..., rounds=2)
The parent starts `--procs` fresh children one after the other, each under --child-timeout seconds, and reports the median over
the children's medians with the run-to-run spread (max - min of the children's medians).  A child that fails or outlives its
limit ends the run: nothing more is started on the GPU after it."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
RADIUS = 45.0


def child(sizes, points, reps):
    import torch
    import cpe_amd  # noqa: F401
    from cpe_amd import fit
    from time_table_tri import make_tables, time_variants
    dev = torch.device('cuda:0')
    for n in sizes:
        for pts in points:
            g1, g2, K1, K2, T21, tab = make_tables(n, pts, dev)
            cyl = fit.fit_single_cylinder_batch(g1, g2, K1, K2, T21, RADIUS, mode=fit.FIT_LM)['cyl'][:, 1].contiguous()
            pred = fit.grid_predict_batch(cyl, RADIUS, K1, K2, T21, tab)
            lm = dict(first=dict(mode=fit.FIT_LM), mode=fit.FIT_LM)
            first, ms = time_variants(dict(
                predict=lambda: fit.grid_predict_batch(cyl, RADIUS, K1, K2, T21, tab),
                assign=lambda: fit.grid_assign_batch(g1, pred, 1),
                fused_fit=lambda: fit.fit_single_cylinder_fused_batch(g1, g2, K1, K2, T21, tab, RADIUS, mode=fit.FIT_LM),
                stereo_fit=lambda: fit.fit_single_cylinder_batch(g1, g2, K1, K2, T21, RADIUS, mode=fit.FIT_LM),
                refined_1=lambda: fit.fit_single_cylinder_refined_batch(g1, g2, K1, K2, T21, tab, RADIUS, rounds=1, **lm),
                refined_2=lambda: fit.fit_single_cylinder_refined_batch(g1, g2, K1, K2, T21, tab, RADIUS, rounds=2, **lm)), reps)
            med = {k: statistics.median(v) for k, v in ms.items()}
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
    ap.add_argument('--reps', type=int, default=11)
    ap.add_argument('--procs', type=int, default=3)
    ap.add_argument('--child-timeout', type=float, default=400.0, help='seconds one child may take')
    ap.add_argument('--out', default=None, help='also append every raw line to this file')
    ap.add_argument('--child', action='store_true')
    a = ap.parse_args()
    if a.child:
        return child(a.frames, a.points, a.reps)
    lines = []

    def emit(d):
        lines.append(d)
        print(json.dumps(d), flush=True)
        if a.out:
            with open(a.out, 'a') as f:
                f.write(json.dumps(d) + '\n')
    for p in range(a.procs):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', '--reps', str(a.reps), '--points'] +
                           [str(n) for n in a.points] + ['--frames'] + [str(n) for n in a.frames], stdout=subprocess.PIPE, text=True,
                           check=True, timeout=a.child_timeout)
        for ln in r.stdout.splitlines():
            if ln.startswith('{'):
                emit(dict(json.loads(ln), process=p))
    ratios = (('refined_1_over_fused_fit', 'refined_1', 'fused_fit'), ('refined_2_over_fused_fit', 'refined_2', 'fused_fit'))
    for n in a.frames:
        for i in range(len(a.points)):
            rows = [d for d in lines if d['kind'] == 'tables' and d['frames'] == n][i::len(a.points)]
            keys = list(rows[0]['median_ms'])
            med = {k: statistics.median(d['median_ms'][k] for d in rows) for k in keys}
            spread = {k: max(d['median_ms'][k] for d in rows) - min(d['median_ms'][k] for d in rows) for k in keys}
            skip = ('kind', 'frames', 'reps', 'median_ms', 'ms', 'process') + tuple(r[0] for r in ratios)
            extra = {k: v for k, v in rows[0].items() if k not in skip}
            emit(dict(kind='tables_summary', frames=n, procs=a.procs, median_ms=med, spread_ms=spread,
                      **{name: med[num] / med[den] for name, num, den in ratios}, **extra))
    return 0


if __name__ == '__main__':
    sys.exit(main())
