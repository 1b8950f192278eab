"""Time the index-shift search of stereo frames (cpe_index_shift_batch) at the Python layer against single-camera triangulation
from a table of the same size (cpe_table_triangulate_batch: like it one wavefront per frame's points, reading the same table),
and the renumbered projector fit against the trimmed fit it extends.

    python tools/time_index_shift.py [--frames 45 4096] [--points 250] [--fit-frames 45] [--reps 11] [--procs 3]
                                     [--child-timeout 400] [--out FILE]

Tables: the analytic cylinders of tools/time_table_tri.py (17 x 25 grid, thinned to `--points` points, 0.25 px noise), their
stereo points from fit.select_triangulate_batch(selector=SEL_JOIN) (every pair, so every point), every third frame numbered
one column up or one row down; the table is the rig's true one, -16..16.  Per size, timed by the protocol of tools/timing.py
between device events, one call:
    index_shift  fit.index_shift_batch(X, idx, m, table, win=(4, 4))
    table_tri    fit.table_triangulate_batch(gp1, K1, None, table)
Fit: the `--fit-frames` analytic boards of tools/time_projector_model.py (425 points each), clean and with every ninth frame
numbered one column up:
    model_trim           fit.fit_projector_model(X, idx, cnt, -12, 12, tau=1.0)
    renumbered           fit.fit_projector_model_renumbered(X, idx, cnt, -12, 12, tau=1.0)      fit, table, search, refit
    model_trim_shifted, renumbered_shifted                                                      the same on the shifted tables"""
import argparse
import json
import sys

import timing


def child(sizes, points, fit_frames, reps):
    import torch
    import cpe_amd  # noqa: F401
    from cpe_amd import fit, synth
    import time_plane_fit
    import time_table_tri
    dev = torch.device('cuda:0')
    for n in sizes:
        g1, g2, K1, K2, T21, _ = time_table_tri.make_tables(n, points, dev)
        tab = time_table_tri.rig_table(synth.Scene(h=1200, w=1920), -16, 16, dev)
        sel = fit.select_triangulate_batch(g1, g2, K1, K2, T21, selector=fit.SEL_JOIN)   # every pair: all `points` points
        X, m = sel['pts3'], sel['m']
        move = torch.zeros((n, 2), dtype=torch.int32, device=dev)
        move[0::6, 0] = 1
        move[3::6, 1] = -1
        idx = (sel['idx'] + move[:, None, :]).contiguous()
        first, ms = timing.time_variants(dict(index_shift=lambda: fit.index_shift_batch(X, idx, m, tab, win=(4, 4)),
                                              table_tri=lambda: fit.table_triangulate_batch(g1, K1, None, tab)), reps)
        med = timing.medians(ms)
        print(json.dumps(dict(kind='tables', frames=n, points=float(m.double().mean()), reps=reps, median_ms=med,
                              shift_over_tri=med['index_shift'] / med['table_tri'],
                              shifts_right=int((first['index_shift']['shift'] == -move).all(1).sum()),
                              flagged=int((first['index_shift']['flags'] & ~fit.SHIFT_SHIFTED).ne(0).any(1).sum()), ms=ms)), flush=True)
        del first, g1, g2, sel, X, idx
        torch.cuda.empty_cache()
    if fit_frames > 0:
        X, idx, cnt = time_plane_fit.make_tables(fit_frames, 425, dev, lift=False)
        move = torch.zeros((fit_frames, 2), dtype=torch.int32, device=dev)
        move[4::9, 0] = 1
        off = (idx + move[:, None, :]).contiguous()
        first, ms = timing.time_variants(dict(
            model_trim=lambda: fit.fit_projector_model(X, idx, cnt, -12, 12, tau=1.0),
            renumbered=lambda: fit.fit_projector_model_renumbered(X, idx, cnt, -12, 12, tau=1.0),
            model_trim_shifted=lambda: fit.fit_projector_model(X, off, cnt, -12, 13, tau=1.0),
            renumbered_shifted=lambda: fit.fit_projector_model_renumbered(X, off, cnt, -12, 13, tau=1.0)), reps)
        med = timing.medians(ms)
        rs = first['renumbered_shifted']
        print(json.dumps(dict(kind='fit', frames=fit_frames, points=425.0, reps=reps, median_ms=med,
                              renumbered_over_trim=med['renumbered'] / med['model_trim'],
                              renumbered_over_trim_shifted=med['renumbered_shifted'] / med['model_trim_shifted'],
                              shifts_right=int((rs['shift']['shift'] == -move).all(1).sum()),
                              info_trim_shifted=first['model_trim_shifted']['info'].cpu().tolist(), info_refit_shifted=rs['fit']['info'].cpu().tolist(),
                              info_refit=first['renumbered']['fit']['info'].cpu().tolist(), ms=ms)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, nargs='*', default=[45, 4096])
    ap.add_argument('--points', type=int, default=250)
    ap.add_argument('--fit-frames', type=int, default=45)
    a = timing.parse(ap, reps=11, child_timeout=400.0)
    if a.child:
        return child(a.frames, a.points, a.fit_frames, a.reps)
    lines, emit = timing.run_children(__file__, a)
    ratios = dict(tables=(('shift_over_tri', 'index_shift', 'table_tri'),),
                  fit=(('renumbered_over_trim', 'renumbered', 'model_trim'),
                       ('renumbered_over_trim_shifted', 'renumbered_shifted', 'model_trim_shifted')))
    for kind, sizes in (('tables', a.frames), ('fit', [a.fit_frames] if a.fit_frames > 0 else [])):
        for n in sizes:
            rows = [d for d in lines if d['kind'] == kind and d['frames'] == n]
            emit(timing.ratio_summary(dict(kind=kind + '_summary', frames=n, procs=a.procs), rows, ratios[kind]))
    return 0


if __name__ == '__main__':
    sys.exit(main())
