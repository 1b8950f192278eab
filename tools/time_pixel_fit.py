"""Time the pixel fit (cpe_fit_cylinder_pixels_batch) at the Python layer against the two paths it stands beside, on the same tensors.

    python tools/time_pixel_fit.py [--sizes 45x250 4096x250 64x2048] [--reps 11] [--procs 3] [--child-timeout 400] [--out FILE]

Tables: the analytic cylinders of tools/time_table_tri.py (17 x 25 grid, thinned to the wanted points per image, 0.25 px noise), the
rig's true table; a size with more points per image than the grid has nodes repeats the nodes, each time with noise of its own
(several detections of one node are legitimate here).  The start of every variant is the fused LM fit's cyl[:, 1], made before the
timed calls.  Per size, timed by the protocol of tools/timing.py between device events, one call each:
    pixels        fit.fit_cylinder_pixels_batch(gp1, gp2, cyl0, R, K1, K2, T21, table)                   one launch
    fused_lm      fit.fused_triangulate_batch(...) + fit.fit_cylinder_batch(mode=FIT_LM)                   two launches
    refine_round  fit.grid_predict_batch + fit.grid_assign_batch x 2 + fused_triangulate_batch + fit_cylinder_batch(FIT_LM): one
                  round of fit.fit_single_cylinder_refined_batch without its torch.where
The kernel alone and hardware counters are not measured here: that takes a profiler run."""
import argparse
import json
import sys

import timing


def _tables(n, points, dev):
    import torch
    import time_table_tri
    from cpe_amd import fit
    g1, g2, K1, K2, T21, tab = time_table_tri.make_tables(n, min(points, 424), dev)
    if points > 424:
        gen = torch.Generator(device='cpu').manual_seed(5)
        m = int(g1.cnt.min())
        reps = -(-points // m)

        def grow(g):
            xy = g.xy[:, :m].repeat(1, reps, 1)[:, :points]
            xy = xy + (0.25 * torch.randn(xy.shape, generator=gen, dtype=torch.float64)).to(dev) * (torch.arange(points, device=dev) >= m)[None, :, None]
            out = torch.zeros_like(g.xy)
            out[:, :points] = xy
            ids = torch.zeros_like(g.id)
            ids[:, :points] = g.id[:, :m].repeat(1, reps, 1)[:, :points]
            return fit.GridTables(out, ids, torch.full_like(g.cnt, points))
        g1, g2 = grow(g1), grow(g2)
    return g1, g2, K1, K2, T21, tab


def child(sizes, reps):
    import torch
    import cpe_amd  # noqa: F401
    from cpe_amd import fit
    import time_table_tri
    dev = torch.device('cuda:0')
    R = time_table_tri.RADIUS
    for n, points in sizes:
        g1, g2, K1, K2, T21, tab = _tables(n, points, dev)
        tab.has_centre()                                   # (the one look at the table's centre, outside the timed calls)
        start = fit.fit_single_cylinder_fused_batch(g1, g2, K1, K2, T21, tab, R, mode=fit.FIT_LM)
        cyl0 = start['cyl'][:, 1].contiguous()

        def fused_lm():
            tri = fit.fused_triangulate_batch(g1, g2, K1, K2, T21, tab)
            return fit.fit_cylinder_batch(tri['pts3'], tri['m'], R, mode=fit.FIT_LM)

        def refine_round():
            pred = fit.grid_predict_batch(cyl0, R, K1, K2, T21, tab)
            a1, a2 = fit.grid_assign_batch(g1, pred, 1), fit.grid_assign_batch(g2, pred, 2)
            tri = fit.fused_triangulate_batch(a1['tables'], a2['tables'], K1, K2, T21, tab)
            return fit.fit_cylinder_batch(tri['pts3'], tri['m'], R, mode=fit.FIT_LM)

        first, ms = timing.time_variants(dict(pixels=lambda: fit.fit_cylinder_pixels_batch(g1, g2, cyl0, R, K1, K2, T21, tab, want=()),
                                              fused_lm=fused_lm, refine_round=refine_round), reps)
        med = timing.medians(ms)
        px = first['pixels']
        print(json.dumps(dict(kind='pixel_fit', frames=n, points=points, reps=reps, median_ms=med,
                              pixels_over_fused_lm=med['pixels'] / med['fused_lm'], pixels_over_refine_round=med['pixels'] / med['refine_round'],
                              pixels_ok=int((px['status'] == 0).sum()), fused_ok=int((first['fused_lm']['status'] == 0).sum()),
                              iterations_mean=float(px['iters'][:, 0].double().mean()), iterations_max=int(px['iters'][:, 0].max()),
                              evaluations_mean=float(px['iters'][:, 1].double().mean()), used_mean=float(px['counts'][:, :2].sum(1).double().mean()),
                              px_rms_mean=float(px['stats'][:, 2].mean()), ms=ms)), flush=True)
        del first, px, start
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', nargs='*', default=['45x250', '4096x250', '64x2048'], help='frames x points per image')
    a = timing.parse(ap, reps=11, child_timeout=400.0)
    sizes = [tuple(int(v) for v in s.split('x')) for s in a.sizes]
    if a.child:
        return child(sizes, a.reps)
    lines, emit = timing.run_children(__file__, a)
    ratios = (('pixels_over_fused_lm', 'pixels', 'fused_lm'), ('pixels_over_refine_round', 'pixels', 'refine_round'))
    for n, points in sizes:
        rows = [d for d in lines if d['frames'] == n and d['points'] == points]
        emit(timing.ratio_summary(dict(kind='pixel_fit_summary', frames=n, points=points, procs=a.procs), rows, ratios))
    return 0


if __name__ == '__main__':
    sys.exit(main())
