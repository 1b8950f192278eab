"""Time the joint pose-and-angles fit (cpe_multi_frame_fit_pixels_angles_batch) at the Python layer against the fixed-angle pixel fit
on the same tensors.

    python tools/time_multiframe_joint.py [--shapes 1x45 16x45 1x256] [--points 250] [--reps 11] [--procs 3] [--child-timeout 500]
                                          [--so FILE] [--out FILE]

Tables: the perturbed scenes of tests/multiframe_joint_cases.py (the nominal angles + N(0, 0.003 rad), 0.25 px noise, the rig's true
table), groups x frames per shape, the first `points` detections of every image.  Made before the timed calls: the fixed-angle fit
from the scenes' starts, whose pose both timed calls start from.  Per shape, timed by the protocol of tools/timing.py between
device events, one call each:
    joint          multiframe.fit_multi_frame_pixels_angles_gpu(..., the nominal angles)     one launch, one workgroup per group
    pixels_mf      multiframe.fit_multi_frame_pixels_gpu(..., the nominal chains): the yardstick, same launch shape
There is no pass mark: the line holds the ratio, and the iterations and evaluations of both.
--so: another build of the library (another form of the kernel), loaded in place of the package's.
The kernel alone and hardware counters are not measured here: that takes a profiler run."""
import argparse
import json
import sys

import timing


def _group_tensors(groups, frames, points, dev):
    import numpy as np
    import torch
    import multiframe_joint_cases as J
    import plane_fit_cases as PC
    import table_tri_cases as TC
    from cpe_amd import fit
    scenes = [J.joint_scene(frames, 100 + g) for g in range(groups)]
    mats = lambda k: [np.concatenate([f['xy'][:points], f['id'][:points]], 1) for sc in scenes for f in sc[k]]
    g1, g2 = fit.GridTables.from_lists(mats('fr1'), dev), fit.GridTables.from_lists(mats('fr2'), dev)
    t = TC.rig_table(TC.LO, TC.HI)
    tab = fit.LaserTable(torch.from_numpy(t['P']).to(dev), torch.from_numpy(t['status'].astype(np.int32)).to(dev), t['lo'], t['hi'],
                         torch.from_numpy(np.concatenate([PC.rig()[5], [0.0]])).to(dev), torch.zeros(1, dtype=torch.int32, device=dev))
    angles = torch.from_numpy(np.concatenate([sc['angles'] for sc in scenes])).to(dev)
    TAGV = torch.from_numpy(np.concatenate([sc['TAGV'] for sc in scenes]).reshape(-1, 16)).to(dev)
    x0 = torch.from_numpy(np.stack([sc['x0'] for sc in scenes])).to(dev)
    gs = torch.arange(0, groups * frames + 1, frames, dtype=torch.int32, device=dev)
    return g1, g2, PC.rig()[:3], tab, angles, TAGV, x0, gs, J.RADIUS


def child(shapes, points, reps, so):
    import torch
    import cpe_amd
    if so:
        cpe_amd.lib.SO_PATH = so
    from cpe_amd import multiframe
    dev = torch.device('cuda:0')
    for groups, frames in shapes:
        g1, g2, K, tab, angles, TAGV, x0, gs, R = _group_tensors(groups, frames, points, dev)
        tab.has_centre()
        cams = (g1.xy, g1.id, g1.cnt, g2.xy, g2.id, g2.cnt)
        x1 = multiframe.fit_multi_frame_pixels_gpu(*cams, TAGV, x0, R, *K, tab, group_start=gs)['x'].clone()
        variants = dict(joint=lambda: multiframe.fit_multi_frame_pixels_angles_gpu(*cams, angles, x1, R, *K, tab, group_start=gs),
                        pixels_mf=lambda: multiframe.fit_multi_frame_pixels_gpu(*cams, TAGV, x1, R, *K, tab, group_start=gs))
        first, ms = timing.time_variants(variants, reps)
        med = timing.medians(ms)
        jt, px = first['joint'], first['pixels_mf']
        print(json.dumps(dict(kind='multiframe_joint', groups=groups, frames=frames, points=points, reps=reps, median_ms=med,
                              joint_over_pixels_mf=med['joint'] / med['pixels_mf'], ok=int((jt['status'] == 0).sum()),
                              pixels_ok=int((px['status'] == 0).sum()), iterations_max=int(jt['iters'][:, 0].max()),
                              evaluations_max=int(jt['iters'][:, 1].max()), pixels_iterations_max=int(px['iters'][:, 0].max()),
                              pixels_evaluations_max=int(px['iters'][:, 1].max()), used_mean=float(jt['counts'][:, :2].sum(1).double().mean()),
                              px_rms_mean=float(jt['stats'][:, 2].mean()), pixels_px_rms_mean=float(px['stats'][:, 2].mean()), ms=ms)), flush=True)
        del first, jt, px
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', nargs='*', default=['1x45', '16x45', '1x256'], help='groups x frames per group')
    ap.add_argument('--points', type=int, default=250, help='detections per image')
    ap.add_argument('--so', default=None, help='a library file to load in place of the package\'s')
    a = timing.parse(ap, reps=11, child_timeout=500.0)
    shapes = [tuple(int(v) for v in s.split('x')) for s in a.shapes]
    if a.child:
        return child(shapes, a.points, a.reps, a.so)
    lines, emit = timing.run_children(__file__, a)
    for groups, frames in shapes:
        rows = [d for d in lines if d['groups'] == groups and d['frames'] == frames]
        emit(timing.ratio_summary(dict(kind='multiframe_joint_summary', groups=groups, frames=frames, points=a.points, procs=a.procs, so=a.so),
                                  rows, (('joint_over_pixels_mf', 'joint', 'pixels_mf'),)))
    return 0


if __name__ == '__main__':
    sys.exit(main())
