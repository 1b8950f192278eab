"""Time the one-camera index-shift search (cpe_mono_shift_batch) at the Python layer against ONE single-camera triangulation of
the same tables (cpe_table_triangulate_batch), and the repaired one-camera fit against the plain one it extends.

    python tools/time_mono_shift.py [--frames 45 4096] [--points 250] [--windows 4 8] [--reps 11] [--procs 3]
                                    [--child-timeout 400] [--out FILE]

Tables: the analytic cylinders of tools/time_table_tri.py (17 x 25 grid, thinned to `--points` points, 0.25 px noise), camera 1;
every sixth frame numbered one column up, every sixth one row down; the table is the rig's true one, -24..24, so that it covers
window 8 around every index.  Per size and window w, timed by the protocol of tools/timing.py between device events, one call each:
    mono_shift   fit.mono_shift_batch(gp, K1, None, table, win=(w, w))            C = (2 w + 1)^2 candidate solves per point
    table_tri    fit.table_triangulate_batch(gp, K1, None, table, need_both=True)  one solve per point, and it writes the points
    repaired     fit.fit_single_cylinder_mono_repaired_batch(gp, 1, K1, K2, T21, table, R, shift=dict(win=(w, w)), rounds=1)
    plain        fit.fit_single_cylinder_mono_batch(gp, K1, None, table, R, mode=FIT_LM, need_both=True, max_res=0.25)
shift_over_tri is what the search costs in units of one triangulation call; C of them is what C separate calls would cost."""
import argparse
import json
import sys

import timing


def child(sizes, points, windows, reps):
    import torch
    import cpe_amd  # noqa: F401
    from cpe_amd import fit, synth
    import time_table_tri
    dev = torch.device('cuda:0')
    for n in sizes:
        g1, _, K1, K2, T21, _ = time_table_tri.make_tables(n, points, dev)
        tab = time_table_tri.rig_table(synth.Scene(h=1200, w=1920), -24, 24, dev)
        tab.has_centre()                                   # (the one look at the table's centre, outside the timed calls)
        move = torch.zeros((n, 2), dtype=torch.int32, device=dev)
        move[0::6, 0] = 1
        move[3::6, 1] = -1
        gp = fit.GridTables(g1.xy, (g1.id + move[:, None, :]).contiguous(), g1.cnt)
        R = time_table_tri.RADIUS
        for w in windows:
            first, ms = timing.time_variants(dict(
                mono_shift=lambda: fit.mono_shift_batch(gp, K1, None, tab, win=(w, w)),
                table_tri=lambda: fit.table_triangulate_batch(gp, K1, None, tab, need_both=True),
                repaired=lambda: fit.fit_single_cylinder_mono_repaired_batch(gp, 1, K1, K2, T21, tab, R, shift=dict(win=(w, w)), rounds=1),
                plain=lambda: fit.fit_single_cylinder_mono_batch(gp, K1, None, tab, R, mode=fit.FIT_LM, need_both=True, max_res=0.25)), reps)
            med = timing.medians(ms)
            rp = first['repaired']
            print(json.dumps(dict(kind='tables', frames=n, window=w, candidates=(2 * w + 1) ** 2, points=float(g1.cnt.double().mean()),
                                  reps=reps, median_ms=med, shift_over_tri=med['mono_shift'] / med['table_tri'],
                                  repaired_over_plain=med['repaired'] / med['plain'],
                                  votes_right=int((first['mono_shift']['cand'][:, 0] == -move).all(1).sum()),
                                  shifts_right=int((rp['shift'] == -move).all(1).sum()),
                                  weak=int((rp['shift_flags'] & fit.SHIFT_WEAK).ne(0).sum()),
                                  wrong_and_trusted=int(((rp['shift'] != -move).any(1) & (rp['shift_flags'] & fit.SHIFT_WEAK).eq(0)).sum()),
                                  weak_and_moved=int(((rp['shift_flags'] & fit.SHIFT_WEAK).ne(0) & (move != 0).any(1)).sum()),
                                  plain_ok=int((first['plain']['status'] == 0).sum()), repaired_ok=int((rp['status'] == 0).sum()),
                                  plain_points=float(first['plain']['m'].double().mean()), repaired_points=float(rp['m'].double().mean()),
                                  ms=ms)), flush=True)
            del first, rp
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, nargs='*', default=[45, 4096])
    ap.add_argument('--points', type=int, default=250)
    ap.add_argument('--windows', type=int, nargs='*', default=[4, 8])
    a = timing.parse(ap, reps=11, child_timeout=400.0)
    if a.child:
        return child(a.frames, a.points, a.windows, a.reps)
    lines, emit = timing.run_children(__file__, a)
    ratios = (('shift_over_tri', 'mono_shift', 'table_tri'), ('repaired_over_plain', 'repaired', 'plain'))
    for n in a.frames:
        for w in a.windows:
            rows = [d for d in lines if d['frames'] == n and d['window'] == w]
            emit(timing.ratio_summary(dict(kind='tables_summary', frames=n, window=w, procs=a.procs), rows, ratios))
    return 0


if __name__ == '__main__':
    sys.exit(main())
