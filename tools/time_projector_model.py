"""Time the projector model (cpe_fit_projector_model) at the Python layer against the free laser-plane table
(cpe_index_planes_batch) on the same point tables: the analytic boards of tools/time_plane_fit.py (17 x 25 grid, seeded poses,
0.25 px noise, triangulated by fit.triangulate_batch) WITHOUT the lifted points, all 425 points of every frame.

    python tools/time_projector_model.py [--frames 45 1024] [--reps 11] [--procs 3] [--child-timeout 400] [--out FILE]

Per size, alternated inside one process, the time between two device events around one call:
    table       fit.index_planes_batch(X, idx, cnt, -12, 12)
    model       fit.fit_projector_model(X, idx, cnt, -12, 12)               one moments pass, one solve
    model_trim  fit.fit_projector_model(X, idx, cnt, -12, 12, tau=1.0)      the same behind the trimming loop (on clean tables
                                                                            round 1 finds no change: two moments passes, one solve)
The parent starts `--procs` fresh children one after the other and reports the median over the children's medians with the
run-to-run spread (max - min of the children's medians).  A child that fails or outlives --child-timeout seconds ends the run:
nothing more is started on the GPU after it."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
KEYS = ('table', 'model', 'model_trim')


def child(sizes, reps):
    import torch
    import cpe_amd  # noqa: F401
    from cpe_amd import fit
    from time_plane_fit import make_tables, time_variants
    dev = torch.device('cuda:0')
    for n in sizes:
        X, idx, cnt = make_tables(n, 425, dev, lift=False)
        first, ms = time_variants(dict(table=lambda: fit.index_planes_batch(X, idx, cnt, -12, 12),
                                       model=lambda: fit.fit_projector_model(X, idx, cnt, -12, 12),
                                       model_trim=lambda: fit.fit_projector_model(X, idx, cnt, -12, 12, tau=1.0)), reps)
        med = {k: statistics.median(v) for k, v in ms.items()}
        print(json.dumps(dict(kind='projector', frames=n, points=425.0, reps=reps, median_ms=med, model_over_table=med['model'] / med['table'],
                              trim_over_table=med['model_trim'] / med['table'], lines_ok=int((first['table']['status'] == 0).sum()),
                              info=first['model']['info'].cpu().tolist(), info_trim=first['model_trim']['info'].cpu().tolist(),
                              model=first['model']['model'].cpu().tolist(), ms=ms)), flush=True)
        del first, X, idx, cnt
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, nargs='*', default=[45, 1024])
    ap.add_argument('--reps', type=int, default=11)
    ap.add_argument('--procs', type=int, default=3)
    ap.add_argument('--child-timeout', type=float, default=400.0, help='seconds one child may take')
    ap.add_argument('--out', default=None, help='also append every raw line to this file')
    ap.add_argument('--child', action='store_true')
    a = ap.parse_args()
    if a.child:
        return child(a.frames, a.reps)
    lines = []

    def emit(d):
        lines.append(d)
        print(json.dumps(d), flush=True)
        if a.out:
            with open(a.out, 'a') as f:
                f.write(json.dumps(d) + '\n')
    for p in range(a.procs):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', '--reps', str(a.reps), '--frames'] + [str(n) for n in a.frames],
                           stdout=subprocess.PIPE, text=True, check=True, timeout=a.child_timeout)
        for ln in r.stdout.splitlines():
            if ln.startswith('{'):
                emit(dict(json.loads(ln), process=p))
    for n in a.frames:
        rows = [d for d in lines if d['kind'] == 'projector' and d['frames'] == n]
        med = {k: statistics.median(d['median_ms'][k] for d in rows) for k in KEYS}
        spread = {k: max(d['median_ms'][k] for d in rows) - min(d['median_ms'][k] for d in rows) for k in KEYS}
        emit(dict(kind='projector_summary', frames=n, points=425.0, procs=a.procs, median_ms=med, spread_ms=spread,
                  model_over_table=med['model'] / med['table'], trim_over_table=med['model_trim'] / med['table'],
                  lines_ok=rows[0]['lines_ok'], info=rows[0]['info'], info_trim=rows[0]['info_trim']))
    return 0


if __name__ == '__main__':
    sys.exit(main())
