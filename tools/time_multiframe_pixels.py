"""Time the multi-frame pixel fit (cpe_multi_frame_fit_pixels_batch) at the Python layer against the two calls it stands beside, on
the same tensors.

    python tools/time_multiframe_pixels.py [--shapes 1x45 16x45 1x1024] [--points 250] [--reps 11] [--procs 3] [--child-timeout 500]
                                           [--so FILE] [--out FILE]

Tables: the scenes of tests/multiframe_pixel_cases.py (pan +-0.35 rad, tilt +-0.2 rad, 0.25 px noise, the rig's true table), groups x
frames per shape, the first `points` detections of every image.  Made before the timed calls: the fused LM fit of every frame and the
point-based multi-frame pose the pixel fit starts from.  Per shape, timed by the protocol of tools/timing.py between device events,
one call each:
    pixels_mf      multiframe.fit_multi_frame_pixels_gpu(..., x0 = the point-based pose)                   one launch, one workgroup per group
    points_lm      multiframe.fit_multi_frame_gpu(method='lm') on the fused points of the same tables        one launch
    pixels_frames  fit.fit_cylinder_pixels_batch over the same frames from their fused fits                  one launch, one wave per frame
--so: another build of the library (csrc/fit.hip with another CPE_MFPX_WAVES), loaded in place of the package's.
The kernel alone and hardware counters are not measured here: that takes a profiler run."""
import argparse
import json
import sys

import timing


def _group_tensors(groups, frames, points, dev):
    import numpy as np
    import torch
    import multiframe_pixel_cases as M
    import plane_fit_cases as PC
    import table_tri_cases as TC
    from cpe_amd import fit
    scenes = [M.scene(frames, 100 + g) for g in range(groups)]
    mats = lambda k: [np.concatenate([f['xy'][:points], f['id'][:points]], 1) for sc in scenes for f in sc[k]]
    g1, g2 = fit.GridTables.from_lists(mats('fr1'), dev), fit.GridTables.from_lists(mats('fr2'), dev)
    t = TC.rig_table(TC.LO, TC.HI)
    tab = fit.LaserTable(torch.from_numpy(t['P']).to(dev), torch.from_numpy(t['status'].astype(np.int32)).to(dev), t['lo'], t['hi'],
                         torch.from_numpy(np.concatenate([PC.rig()[5], [0.0]])).to(dev), torch.zeros(1, dtype=torch.int32, device=dev))
    TAGV = torch.from_numpy(np.concatenate([sc['TAGV'] for sc in scenes]).reshape(-1, 16)).to(dev)
    gs = torch.arange(0, groups * frames + 1, frames, dtype=torch.int32, device=dev)
    return g1, g2, PC.rig()[:3], tab, TAGV, gs, M.RADIUS


def child(shapes, points, reps, so):
    import torch
    import cpe_amd
    if so:
        cpe_amd.lib.SO_PATH = so
    from cpe_amd import fit, multiframe
    dev = torch.device('cuda:0')
    for groups, frames in shapes:
        g1, g2, K, tab, TAGV, gs, R = _group_tensors(groups, frames, points, dev)
        tab.has_centre()
        fused = fit.fit_single_cylinder_fused_batch(g1, g2, *K, tab, R, mode=fit.FIT_LM)
        ok = (fused['status'] == 0).to(torch.int32)
        cyl0 = fused['cyl'][:, 1].contiguous()
        points_lm = lambda: multiframe.fit_multi_frame_gpu(fused['pts3'], fused['m'], fused['cyl_raw'], TAGV, R, frame_ok=ok, group_start=gs,
                                                           method='lm')
        x0 = points_lm()['x'].clone()
        variants = dict(pixels_mf=lambda: multiframe.fit_multi_frame_pixels_gpu(g1.xy, g1.id, g1.cnt, g2.xy, g2.id, g2.cnt, TAGV, x0, R, *K, tab,
                                                                                frame_ok=ok, group_start=gs),
                        points_lm=points_lm,
                        pixels_frames=lambda: fit.fit_cylinder_pixels_batch(g1, g2, cyl0, R, *K, tab, use=ok, want=()))
        first, ms = timing.time_variants(variants, reps)
        med = timing.medians(ms)
        px = first['pixels_mf']
        print(json.dumps(dict(kind='multiframe_pixels', groups=groups, frames=frames, points=points, reps=reps, median_ms=med,
                              pixels_mf_over_points_lm=med['pixels_mf'] / med['points_lm'],
                              pixels_mf_over_pixels_frames=med['pixels_mf'] / med['pixels_frames'], ok=int((px['status'] == 0).sum()),
                              points_ok=int((first['points_lm']['status'] == 0).sum()), iterations_max=int(px['iters'][:, 0].max()),
                              evaluations_max=int(px['iters'][:, 1].max()), used_mean=float(px['counts'][:, :2].sum(1).double().mean()),
                              px_rms_mean=float(px['stats'][:, 2].mean()), points_iterations_max=int(first['points_lm']['iters'][:, 0].max()),
                              ms=ms)), flush=True)
        del first, px, fused
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', nargs='*', default=['1x45', '16x45', '1x1024'], help='groups x frames per group')
    ap.add_argument('--points', type=int, default=250, help='detections per image')
    ap.add_argument('--so', default=None, help='a library file to load in place of the package\'s')
    a = timing.parse(ap, reps=11, child_timeout=500.0)
    shapes = [tuple(int(v) for v in s.split('x')) for s in a.shapes]
    if a.child:
        return child(shapes, a.points, a.reps, a.so)
    lines, emit = timing.run_children(__file__, a)
    ratios = (('pixels_mf_over_points_lm', 'pixels_mf', 'points_lm'), ('pixels_mf_over_pixels_frames', 'pixels_mf', 'pixels_frames'))
    for groups, frames in shapes:
        rows = [d for d in lines if d['groups'] == groups and d['frames'] == frames]
        emit(timing.ratio_summary(dict(kind='multiframe_pixels_summary', groups=groups, frames=frames, points=a.points, procs=a.procs, so=a.so),
                                  rows, ratios))
    return 0


if __name__ == '__main__':
    sys.exit(main())
