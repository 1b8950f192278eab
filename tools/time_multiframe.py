"""Row f-1: time the multi-frame camera-AGV fit (fitCylinderWPts3sAngs) in its forms on the experiment's own size --
45 frames of about 250 points each, from the scene generator of tests/multiframe_cases.py.

    python tools/time_multiframe.py [--frames 45] [--points 250] [--reps 7] [--procs 3] [--child-timeout 300] [--out FILE]

Variants, alternated inside one process, wall time around every repetition from the call to the results on the host:
    host     multiframe.fit_multi_frame: simplex in Python, one copy + launch + read-back per objective evaluation
    gpu      multiframe.fit_multi_frame_gpu + one read-back of T and fvals: the whole fit resident, one launch
    gpu16    the same call for 16 groups (16 scenes of the same size with different seeds), one launch
    lm       the same call with method='lm' (build-defined: all-frame initial pose + Levenberg-Marquardt), one group
    lm16     the same for the 16 groups
For the resident variants the time between two device events around the launch is reported as well (the kernel alone).
Both forms must walk the same simplex path (equal iterations and evaluations) before anything is timed; if they do not, the
line says so and the times are still reported (the resident form evaluates sin / cos with the device library).
The parent process starts `--procs` fresh children one after the other and reports the median over the children's medians
and the run-to-run spreads (max - min of the children's medians) of the host form and of the two one-group resident forms;
`lm_faster` says whether LM resident beats Nelder-Mead resident by more than the larger of those two.  A child that fails or
outlives --child-timeout seconds ends the run: nothing more is started on the GPU after it.
The scenes come from tests/multiframe_cases.py (the generator the GPU tests use), which this file imports by putting tests/
on sys.path: it has to stay beside the tests."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
RADIUS = 45.0
GROUPS = 16


def child(frames, points, reps):
    import numpy as np
    import torch
    import cpe_amd  # noqa: F401
    import multiframe_cases as mc
    from cpe_amd import fit, multiframe
    dev = torch.device('cuda:0')
    scenes = [mc.make_scene(frames, seed, noise=0.05, npts=points) for seed in range(GROUPS)]
    P = torch.from_numpy(np.concatenate([s[0] for s in scenes])).to(dev)
    cnt = torch.from_numpy(np.concatenate([s[1] for s in scenes])).to(dev)
    angles = np.concatenate([s[2] for s in scenes])
    raw = fit.fit_cylinder_batch(P, cnt, RADIUS)['cyl_raw'].contiguous()
    TAGV = torch.tensor([multiframe.get_TAGVcyl(float(a[0]), float(a[1])) for a in angles], dtype=torch.float64).to(dev)
    P1, c1, r1, A1 = P[:frames].contiguous(), cnt[:frames].contiguous(), raw[:frames].contiguous(), TAGV[:frames].contiguous()
    starts = torch.arange(0, (GROUPS + 1) * frames, frames, dtype=torch.int32, device=dev)
    event_ms = {}

    def resident(key, *args, **kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = multiframe.fit_multi_frame_gpu(*args, **kw)
        e1.record()
        back = torch.cat([res['T'].ravel(), res['fvals'].ravel(), res['iters'].ravel().to(torch.float64)]).cpu()
        event_ms.setdefault(key, []).append(e0.elapsed_time(e1))
        return res, back

    variants = dict(host=lambda: multiframe.fit_multi_frame(P1, c1, r1, angles[:frames], RADIUS),
                    gpu=lambda: resident('gpu', P1, c1, r1, A1, RADIUS),
                    gpu16=lambda: resident('gpu16', P, cnt, raw, TAGV, RADIUS, group_start=starts),
                    lm=lambda: resident('lm', P1, c1, r1, A1, RADIUS, method='lm'),
                    lm16=lambda: resident('lm16', P, cnt, raw, TAGV, RADIUS, group_start=starts, method='lm'))
    first = {k: f() for k, f in variants.items()}                # warm-up
    torch.cuda.synchronize()
    h, g = first['host'], multiframe.group_result(first['gpu'][0])
    same_path = (h['iters'], h['evals']) == (g['iters'], g['evals'])
    info = dict(host_iters=h['iters'], host_evals=h['evals'], gpu_iters=g['iters'], gpu_evals=g['evals'], same_path=same_path,
                host_fvals=h['fvals'], gpu_fvals=g['fvals'], gpu16_status=first['gpu16'][0]['status'].tolist(),
                gpu16_evals=first['gpu16'][0]['iters'][:, 1].tolist(), lm_fvals=first['lm'][0]['fvals'][0].tolist(),
                lm_iters=first['lm'][0]['iters'][0].tolist(), lm16_status=first['lm16'][0]['status'].tolist(),
                lm16_iters=first['lm16'][0]['iters'].tolist(), lm16_fvals=first['lm16'][0]['fvals'][:, 1].tolist())
    event_ms.clear()
    ms = {k: [] for k in variants}
    for _ in range(reps):
        for k, f in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    print(json.dumps(dict(kind='case', frames=frames, points=points, groups=GROUPS, reps=reps,
                          median_ms={k: statistics.median(v) for k, v in ms.items()},
                          median_event_ms={k: statistics.median(v) for k, v in event_ms.items()}, ms=ms, **info)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=45)
    ap.add_argument('--points', type=int, default=250)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--procs', type=int, default=3)
    ap.add_argument('--child-timeout', type=float, default=300.0, help='seconds one child may take')
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
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', '--frames', str(a.frames), '--points', str(a.points),
                            '--reps', str(a.reps)], stdout=subprocess.PIPE, text=True, check=True, timeout=a.child_timeout)
        for ln in r.stdout.splitlines():
            if ln.startswith('{'):
                emit(dict(json.loads(ln), process=p))
    rows = [d for d in lines if d['kind'] == 'case']
    med = {k: statistics.median(d['median_ms'][k] for d in rows) for k in ('host', 'gpu', 'gpu16', 'lm', 'lm16')}
    ev = {k: statistics.median(d['median_event_ms'][k] for d in rows) for k in ('gpu', 'gpu16', 'lm', 'lm16')}
    spreads = {k: max(d['median_ms'][k] for d in rows) - min(d['median_ms'][k] for d in rows) for k in ('host', 'gpu', 'lm')}
    spread = spreads['host']
    emit(dict(kind='summary', frames=a.frames, points=a.points, groups=GROUPS, host_ms=med['host'], gpu_ms=med['gpu'], gpu16_ms=med['gpu16'],
              gpu_kernel_ms=ev['gpu'], gpu16_kernel_ms=ev['gpu16'], host_spread_ms=spread, gpu_faster=med['gpu'] + spread < med['host'],
              evals=rows[0]['host_evals'], same_path=all(d['same_path'] for d in rows),
              lm_ms=med['lm'], lm16_ms=med['lm16'], lm_kernel_ms=ev['lm'], lm16_kernel_ms=ev['lm16'], gpu_spread_ms=spreads['gpu'],
              lm_spread_ms=spreads['lm'], lm_faster=med['lm'] + max(spreads['gpu'], spreads['lm']) < med['gpu'],
              lm_iters=rows[0]['lm_iters'], lm_fvals=rows[0]['lm_fvals'], gpu_fvals=rows[0]['gpu_fvals']))
    return 0


if __name__ == '__main__':
    sys.exit(main())
