"""Time the projector model (cpe_fit_projector_model) at the Python layer against the free laser-plane table
(cpe_index_planes_batch) on the same point tables: the analytic boards of tools/time_plane_fit.py (17 x 25 grid, seeded poses,
0.25 px noise, triangulated by fit.triangulate_batch) WITHOUT the lifted points, all 425 points of every frame.

    python tools/time_projector_model.py [--frames 45 1024] [--reps 11] [--procs 3] [--child-timeout 400] [--out FILE]

Per size, timed by the protocol of tools/timing.py between device events, one call:
    table       fit.index_planes_batch(X, idx, cnt, -12, 12)
    model       fit.fit_projector_model(X, idx, cnt, -12, 12)               one moments pass, one solve
    model_trim  fit.fit_projector_model(X, idx, cnt, -12, 12, tau=1.0)      the same behind the trimming loop (on clean tables
                                                                            round 1 finds no change: two moments passes, one solve)"""
import argparse
import json
import sys

import timing


def child(sizes, reps):
    import torch
    import cpe_amd  # noqa: F401
    from cpe_amd import fit
    from time_plane_fit import make_tables
    dev = torch.device('cuda:0')
    for n in sizes:
        X, idx, cnt = make_tables(n, 425, dev, lift=False)
        first, ms = timing.time_variants(dict(table=lambda: fit.index_planes_batch(X, idx, cnt, -12, 12),
                                              model=lambda: fit.fit_projector_model(X, idx, cnt, -12, 12),
                                              model_trim=lambda: fit.fit_projector_model(X, idx, cnt, -12, 12, tau=1.0)), reps)
        med = timing.medians(ms)
        print(json.dumps(dict(kind='projector', frames=n, points=425.0, reps=reps, median_ms=med, model_over_table=med['model'] / med['table'],
                              trim_over_table=med['model_trim'] / med['table'], lines_ok=int((first['table']['status'] == 0).sum()),
                              info=first['model']['info'].cpu().tolist(), info_trim=first['model_trim']['info'].cpu().tolist(),
                              model=first['model']['model'].cpu().tolist(), ms=ms)), flush=True)
        del first, X, idx, cnt
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, nargs='*', default=[45, 1024])
    a = timing.parse(ap, reps=11, child_timeout=400.0)
    if a.child:
        return child(a.frames, a.reps)
    lines, emit = timing.run_children(__file__, a)
    for n in a.frames:
        rows = [d for d in lines if d['kind'] == 'projector' and d['frames'] == n]
        emit(timing.ratio_summary(dict(kind='projector_summary', frames=n, points=425.0, procs=a.procs), rows,
                                  (('model_over_table', 'model', 'table'), ('trim_over_table', 'model_trim', 'table')), skip=('model',)))
    return 0


if __name__ == '__main__':
    sys.exit(main())
