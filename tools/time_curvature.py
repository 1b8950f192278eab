"""Time the curvatures of every point (cpe_est_curvatures_batch) and their consensus (cpe_curvature_consensus_batch) at the
Python layer against the per-frame fit of the same tensors.

    python tools/time_curvature.py [--cases 45x250 4096x250 64x2048] [--reps 11] [--procs 3] [--child-timeout 400] [--out FILE]

Points: the seeded cylinders of tests/curvature_cases.py (0.05 mm noise), `frames x points` per case, every frame its own seed
up to 64 and repeated beyond.  Per case and mode, timed by the protocol of tools/timing.py between device events, one call each:
    curvatures   fit.est_curvatures_batch(pts3, cnt, k=20, mode=mode)            20-NN + quadric at every point
    consensus    fit.curvature_consensus_batch(pts3, cnt, curv)                   on the curvatures of the warm-up call
    fit_lm       fit.fit_cylinder_batch(pts3, cnt, R, mode=FIT_LM)                the yardstick: 20-NN + quadric at ONE point, then LM
curv_over_fit is what the curvatures of all points cost in units of one LM fit of the same frames."""
import argparse
import json
import sys

import timing


def child(cases, reps):
    import numpy as np
    import torch
    import cpe_amd  # noqa: F401
    from cpe_amd import fit
    import curvature_cases as cc
    dev = torch.device('cuda:0')
    for frames, points in cases:
        base = [cc.cylinder_points(100 + s, points, noise=0.05) for s in range(min(frames, 64))]
        X, cnt = cc.pack([(points, base[i % len(base)]) for i in range(frames)])
        X, cnt = torch.from_numpy(X).to(dev), torch.from_numpy(cnt).to(dev)
        for mode in (fit.CURV_REFERENCE, fit.CURV_INTERCEPT):
            curv = fit.est_curvatures_batch(X, cnt, k=20, mode=mode)
            first, ms = timing.time_variants(dict(
                curvatures=lambda: fit.est_curvatures_batch(X, cnt, k=20, mode=mode),
                consensus=lambda: fit.curvature_consensus_batch(X, cnt, curv),
                fit_lm=lambda: fit.fit_cylinder_batch(X, cnt, cc.R, mode=fit.FIT_LM)), reps)
            med = timing.medians(ms)
            con = first['consensus']
            ok = con['status'] == 0
            print(json.dumps(dict(kind='curvature', frames=frames, points=points, mode=mode, reps=reps, median_ms=med,
                                  curv_over_fit=med['curvatures'] / med['fit_lm'],
                                  us_per_point=1e3 * med['curvatures'] / (frames * points),
                                  bad_points=int(first['curvatures']['pt_status'].sum()), consensus_ok=int(ok.sum()),
                                  gated_share=float(con['n_gated'].double().mean()) / points,
                                  median_radius=float(con['axis'][ok, 6].median()) if bool(ok.any()) else None,
                                  fit_ok=int((first['fit_lm']['status'] == 0).sum()), ms=ms)), flush=True)
            del first, con, curv
            torch.cuda.empty_cache()


def _case(text):
    frames, points = text.lower().split('x')
    return int(frames), int(points)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', type=_case, nargs='*', default=[(45, 250), (4096, 250), (64, 2048)])
    a = timing.parse(ap, reps=11, child_timeout=400.0)
    if a.child:
        return child(a.cases, a.reps)
    lines, emit = timing.run_children(__file__, a)
    for frames, points in a.cases:
        for mode in (0, 1):
            rows = [d for d in lines if (d['frames'], d['points'], d['mode']) == (frames, points, mode)]
            emit(timing.ratio_summary(dict(kind='curvature_summary', frames=frames, points=points, mode=mode, procs=a.procs), rows,
                                      (('curv_over_fit', 'curvatures', 'fit_lm'),)))
    return 0


if __name__ == '__main__':
    sys.exit(main())
