"""Row f-1: time the consensus form of the multi-frame fit (multiframe.fit_multi_frame_consensus_gpu) against its yardstick, the LM
form on the same tensors, on the experiment's own size -- 45 frames of 250 points, one group and 16 groups, with no frame and
with 5 frames of every group displaced (tests/multiframe_consensus_cases.py: a perfect cylinder in the wrong place).

    python tools/time_multiframe_consensus.py [--frames 45] [--points 250] [--bad 5] [--reps 7] [--procs 3] [--child-timeout 300]
                                              [--out FILE]

Variants, timed by the protocol of tools/timing.py: the time between two device events around the Python call (wrapper, launches
and kernels) and the host clock from the call to the results on the host:
    lm / lm16          fit_multi_frame_gpu(method='lm'), one group / 16 groups
    cons / cons16      fit_multi_frame_consensus_gpu with its defaults (990 hypotheses per group at 45 usable frames)
each on the clean tables (suffix 0) and on the tables with displaced frames (suffix the number of them).  With the profile
timers of the library on (one extra warm-up call) the share of the two kernels is reported as well.
The scenes come from tests/: this file has to stay beside the tests."""
import argparse
import json
import sys

import timing

RADIUS = 45.0
GROUPS = 16


def child(frames, points, bad, reps):
    import numpy as np
    import torch
    import cpe_amd  # noqa: F401
    import multiframe_consensus_cases as cc
    from cpe_amd import fit, lib, multiframe
    dev = torch.device('cuda:0')
    tables = {}
    for nb in (0, bad):
        scenes = [cc.displaced_scene(frames, seed, nb, noise=0.1, npts=points) for seed in range(GROUPS)]
        P = torch.from_numpy(np.concatenate([s[0] for s in scenes])).to(dev)
        cnt = torch.from_numpy(np.concatenate([s[1] for s in scenes])).to(dev)
        angles = np.concatenate([s[2] for s in scenes])
        raw = fit.fit_cylinder_batch(P, cnt, RADIUS)['cyl_raw'].contiguous()
        TAGV = torch.tensor([multiframe.get_TAGVcyl(float(a[0]), float(a[1])) for a in angles], dtype=torch.float64).to(dev)
        tables[nb] = dict(all=(P, cnt, raw, TAGV), one=tuple(t[:frames].contiguous() for t in (P, cnt, raw, TAGV)),
                          bad=[s[4] for s in scenes])
    starts = torch.arange(0, (GROUPS + 1) * frames, frames, dtype=torch.int32, device=dev)
    event_ms = {}

    def timed(key, fn, *args, **kw):
        return timing.resident(event_ms, key, fn, *args, RADIUS, **kw)

    variants = {}
    for nb in sorted(tables):
        t = tables[nb]
        variants[f'lm_{nb}'] = lambda t=t, nb=nb: timed(f'lm_{nb}', multiframe.fit_multi_frame_gpu, *t['one'], method='lm')
        variants[f'cons_{nb}'] = lambda t=t, nb=nb: timed(f'cons_{nb}', multiframe.fit_multi_frame_consensus_gpu, *t['one'])
        variants[f'lm16_{nb}'] = lambda t=t, nb=nb: timed(f'lm16_{nb}', multiframe.fit_multi_frame_gpu, *t['all'], group_start=starts,
                                                          method='lm')
        variants[f'cons16_{nb}'] = lambda t=t, nb=nb: timed(f'cons16_{nb}', multiframe.fit_multi_frame_consensus_gpu, *t['all'],
                                                            group_start=starts)
    first = {k: f() for k, f in variants.items()}                # warm-up
    torch.cuda.synchronize()
    info = {}
    for nb in sorted(tables):
        r = first[f'cons16_{nb}'][0]
        inl = r['inlier'].cpu().numpy().reshape(GROUPS, frames)
        info[f'cons16_{nb}'] = dict(status=r['status'].tolist(), n_inliers=r['n_inliers'].tolist(), rounds=r['info'][:, 3].tolist(),
                                    iters=r['iters'].tolist(),
                                    rejected_are_the_displaced=[np.flatnonzero(inl[g] == 0).tolist() == tables[nb]['bad'][g]
                                                                for g in range(GROUPS)])
        info[f'lm16_{nb}'] = dict(status=first[f'lm16_{nb}'][0]['status'].tolist(), iters=first[f'lm16_{nb}'][0]['iters'].tolist())
    lib.profile(True)                                            # the library's per-kernel timers: one call of each consensus variant
    shares = {}
    for k in [k for k in variants if k.startswith('cons')]:
        lib.profile_report()
        variants[k]()
        torch.cuda.synchronize()
        shares[k] = {name: ms for name, calls, ms in lib.profile_report() if name.startswith('k_multi_frame')}
    lib.profile(False)
    event_ms.clear()
    ms = timing.host_loop(variants, reps)
    print(json.dumps(dict(kind='case', frames=frames, points=points, bad=bad, groups=GROUPS, reps=reps, median_ms=timing.medians(ms),
                          median_event_ms=timing.medians(event_ms), kernel_ms=shares, info=info)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=45)
    ap.add_argument('--points', type=int, default=250)
    ap.add_argument('--bad', type=int, default=5)
    a = timing.parse(ap, reps=7, child_timeout=300.0)
    if a.child:
        return child(a.frames, a.points, a.bad, a.reps)
    lines, emit = timing.run_children(__file__, a)
    rows = [d for d in lines if d['kind'] == 'case']
    keys = sorted(rows[0]['median_event_ms'])
    event, event_spread = timing.reduce(rows, keys, 'median_event_ms')
    wall, wall_spread = timing.reduce(rows, keys)
    emit(dict(kind='summary', frames=a.frames, points=a.points, bad=a.bad, groups=GROUPS, event_ms=event, event_spread_ms=event_spread,
              wall_ms=wall, wall_spread_ms=wall_spread, kernel_ms=rows[0]['kernel_ms'],
              all_rejections_exact=all(all(d['info'][k]['rejected_are_the_displaced']) for d in rows for k in d['info'] if k.startswith('cons'))))
    return 0


if __name__ == '__main__':
    sys.exit(main())
