"""Timing of the result export after a detect call, and of the drop-in single-image call.
    python tools/time_results.py [--tree DIR] [--sizes 64,456] [--reps 11]
--tree DIR: import cpe_amd from a built checkout of another commit (the parent, for the comparison) instead of this tree.
On the same warm `det` of n images 1920x1200, after torch.cuda.synchronize(), median / min / max of `reps` repetitions of
  per_frame  the per-frame interface as frame_result used it before the packed records, without the picture: status and n
             read per frame, xy / id / center copied per frame, line_tables, make_json            (every tree)
  packed     batch_results (two kernels, two copies) + make_json of every good frame              (trees that have it)
             and its parts: packed_copies = pack_results alone (kernels and the two copies), packed_decoded = batch_results
             (+ the numpy decoding into the per-frame objects, without the JSON text)
and of a warm api.detect_grid on one 1920x1200 image (whatever path the tree takes).  One JSON line per figure."""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument('--tree', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument('--sizes', default='64,456')
ap.add_argument('--reps', type=int, default=11)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))

import torch  # noqa: E402
import cpe_amd  # noqa: E402
from cpe_amd import api, synth  # noqa: E402

assert torch.cuda.is_available(), 'time_results.py measures on the GPU'
cpe_amd.lib.load()
reps = max(10, args.reps)
tree = os.path.basename(os.path.abspath(args.tree))
has_packed = hasattr(api, 'batch_results')


def per_frame(det):
    out = []
    for k in range(det['n'].shape[0]):
        if int(det['status'][k]) != 0:
            out.append(None)
            continue
        m = int(det['n'][k])
        xy = det['xy'][k, :m].cpu().numpy(); ids = det['id'][k, :m].cpu().numpy(); center = det['center'][k].cpu().numpy()
        rows, cols = api.line_tables(det, k)
        out.append((api.make_json(center, xy, ids), rows, cols))
    return out


def packed(det):
    return [None if r.status != 0 else (api.make_json(r.center, r.xy, r.id), r.rows, r.cols) for r in api.batch_results(det)]


def timed(fn, *a):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize(); t = time.perf_counter()
        fn(*a)
        torch.cuda.synchronize(); ts.append(1e3 * (time.perf_counter() - t))
    return dict(median_ms=round(statistics.median(ts), 3), min_ms=round(min(ts), 3), max_ms=round(max(ts), 3), reps=reps)


for n in [int(v) for v in args.sizes.split(',') if v]:
    b = synth.render_batch((n + 1) // 2, 1200, 1920, seed=1, device='cuda', with_gt=False)
    frames = torch.cat([b['left'], b['right']])[:n].contiguous()
    det = api.detect_grid_batch(frames, api.DetectWorkspace(n, 1200, 1920, frames.device))
    torch.cuda.synchronize()
    ok = int((det['status'] == 0).sum())
    want = per_frame(det)                                   # warm-up of the path, and the yardstick of the packed one
    print(json.dumps(dict(tree=tree, what='per_frame', n=n, ok_frames=ok, **timed(per_frame, det))), flush=True)
    if has_packed:
        assert packed(det) == want, 'the packed export differs from the per-frame interface'
        off, payload = api.pack_results(det)
        sizes = (off[1:] - off[:-1]).tolist()
        print(json.dumps(dict(tree=tree, what='packed', n=n, ok_frames=ok, payload_bytes=int(off[-1]), record_bytes_min=min(sizes),
                              record_bytes_median=int(statistics.median(sizes)), record_bytes_max=max(sizes), **timed(packed, det))), flush=True)
        print(json.dumps(dict(tree=tree, what='packed_copies', n=n, **timed(api.pack_results, det))), flush=True)
        print(json.dumps(dict(tree=tree, what='packed_decoded', n=n, **timed(api.batch_results, det))), flush=True)
    del det, frames, b
    torch.cuda.empty_cache()

img = synth.render_batch(1, 1200, 1920, seed=1, with_gt=False)['left'][0].numpy()
for _ in range(3):
    out = api.detect_grid(img)
assert out is not None
print(json.dumps(dict(tree=tree, what='detect_grid_one_image', packed_path=has_packed, **timed(api.detect_grid, img))), flush=True)
