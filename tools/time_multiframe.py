"""Row f-1: time the multi-frame camera-AGV fit (fitCylinderWPts3sAngs) in its forms on the experiment's own size --
45 frames of about 250 points each, from the scene generator of tests/multiframe_cases.py.

    python tools/time_multiframe.py [--frames 45] [--points 250] [--reps 7] [--procs 3] [--child-timeout 300] [--out FILE]

Variants, timed by the protocol of tools/timing.py on the host clock, from the call to the results on the host:
    host     multiframe.fit_multi_frame: simplex in Python, one copy + launch + read-back per objective evaluation
    gpu      multiframe.fit_multi_frame_gpu + one read-back of T and fvals: the whole fit resident, one launch
    gpu16    the same call for 16 groups (16 scenes of the same size with different seeds), one launch
    lm       the same call with method='lm' (build-defined: all-frame initial pose + Levenberg-Marquardt), one group
    lm16     the same for the 16 groups
For the resident variants the time between two device events around the launch is reported as well (the kernel alone).
Both forms must walk the same simplex path (equal iterations and evaluations) before anything is timed; if they do not, the
line says so and the times are still reported (the resident form evaluates sin / cos with the device library).
The summary carries the run-to-run spreads of the host form and of the two one-group resident forms; `lm_faster` says whether
LM resident beats Nelder-Mead resident by more than the larger of those two.
The scenes come from tests/multiframe_cases.py (the generator the GPU tests use): this file has to stay beside the tests."""
import argparse
import json
import sys

import timing

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
        return timing.resident(event_ms, key, multiframe.fit_multi_frame_gpu, *args, **kw)

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
    ms = timing.host_loop(variants, reps)
    print(json.dumps(dict(kind='case', frames=frames, points=points, groups=GROUPS, reps=reps, median_ms=timing.medians(ms),
                          median_event_ms=timing.medians(event_ms), ms=ms, **info)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=45)
    ap.add_argument('--points', type=int, default=250)
    a = timing.parse(ap, reps=7, child_timeout=300.0)
    if a.child:
        return child(a.frames, a.points, a.reps)
    lines, emit = timing.run_children(__file__, a)
    rows = [d for d in lines if d['kind'] == 'case']
    med, spreads = timing.reduce(rows)
    ev, _ = timing.reduce(rows, field='median_event_ms')
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
