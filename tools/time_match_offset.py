"""Time the build-defined index-shift search (cpe_match_offset_batch) as the per-frame fit runs it: fit_single_cylinder_batch
with the search off and on, window 4 x 4, on the experiment's own size and on a run-time batch -- 45 and 4096 frames of about
250 points each.  The tables are ground-truth tables of cpe_amd.synth at 1920 x 1200 (no rendering) thinned to `--points`
points, with 0.25 px noise; every eighth frame has its left table numbered one column too high, the defect the search is for.

    python tools/time_match_offset.py [--frames 45 4096] [--points 250] [--reps 11] [--procs 3] [--child-timeout 400] [--out FILE]

Per size, timed by the protocol of tools/timing.py between device events, one call:
    off      fit.fit_single_cylinder_batch(...)                 chooseIdx + triangulate + Nelder-Mead fit, as the pipeline calls it
    on       fit.fit_single_cylinder_batch(..., match={})       the same behind the search
    search   fit.match_offset_batch(..., want_scores=False)     the search alone
The number to read is cost = on - off relative to off: what the search adds to the call it sits in.  The line of a size also
carries how many frames came out SHIFTED / WEAK / EDGE and whether every shifted frame got its (-1, 0)."""
import argparse
import json
import sys

import timing

RADIUS = 45.0
SHIFT_EVERY = 8


def make_tables(n, points, seed=0):
    import numpy as np
    from cpe_amd import synth
    scene = synth.Scene(h=1200, w=1920)
    K1, K2, T21, Tp = synth.make_rig(scene)
    fp = synth._frame_params(scene, n, seed)
    gt = synth.ground_truth(scene, K1, K2, T21, Tp, fp, scene.pitch_px / scene.focal)
    rng = np.random.default_rng(seed + 1)
    left, right = [], []
    for i, g in enumerate(gt):
        keep = np.sort(rng.permutation(len(g['idx']))[:points])
        sh = np.array([1, 0]) if i % SHIFT_EVERY == 1 else np.array([0, 0])
        left.append(np.concatenate([g['uv1'][keep] + 0.25 * rng.standard_normal((len(keep), 2)), g['idx'][keep] + sh], 1))
        right.append(np.concatenate([g['uv2'][keep] + 0.25 * rng.standard_normal((len(keep), 2)), g['idx'][keep]], 1))
    return left, right, K1, K2, T21


def child(sizes, points, reps):
    import numpy as np
    import torch
    import cpe_amd  # noqa: F401
    from cpe_amd import fit
    dev = torch.device('cuda:0')
    for n in sizes:
        left, right, K1, K2, T21 = make_tables(n, points)
        g1, g2 = fit.GridTables.from_lists(left, dev), fit.GridTables.from_lists(right, dev)
        variants = dict(off=lambda: fit.fit_single_cylinder_batch(g1, g2, K1, K2, T21, RADIUS),
                        on=lambda: fit.fit_single_cylinder_batch(g1, g2, K1, K2, T21, RADIUS, match={}),
                        search=lambda: fit.match_offset_batch(g1, g2, K1, K2, T21, RADIUS, want_scores=False))
        first, ms = timing.time_variants(variants, reps)
        fl = first['on']['match_flags'].cpu().numpy()
        off = first['on']['offset'].cpu().numpy()
        want = np.array([[-1, 0] if i % SHIFT_EVERY == 1 else [0, 0] for i in range(n)])
        med = timing.medians(ms)
        print(json.dumps(dict(kind='case', frames=n, points=float(np.mean([len(t) for t in left])), window=[4, 4], reps=reps, median_ms=med,
                              cost_ms=med['on'] - med['off'], cost_over_off=(med['on'] - med['off']) / med['off'],
                              shifted=int((fl & fit.MATCH_SHIFTED != 0).sum()), weak=int((fl & fit.MATCH_WEAK != 0).sum()),
                              edge=int((fl & fit.MATCH_EDGE != 0).sum()), offsets_right=bool((off == want).all()),
                              status_ok_off=int((first['off']['status'] == 0).sum()), status_ok_on=int((first['on']['status'] == 0).sum()),
                              ms=ms)), flush=True)
        del first, g1, g2
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, nargs='+', default=[45, 4096])
    ap.add_argument('--points', type=int, default=250)
    a = timing.parse(ap, reps=11, child_timeout=400.0)
    if a.child:
        return child(a.frames, a.points, a.reps)
    lines, emit = timing.run_children(__file__, a)
    for n in a.frames:
        rows = [d for d in lines if d['kind'] == 'case' and d['frames'] == n]
        med, spread = timing.reduce(rows)
        emit(timing.carry(dict(kind='summary', frames=n, points=rows[0]['points'], window=[4, 4], procs=a.procs, median_ms=med, spread_ms=spread,
                               cost_ms=med['on'] - med['off'], cost_over_off=(med['on'] - med['off']) / med['off']), rows))
    return 0


if __name__ == '__main__':
    sys.exit(main())
