"""The measuring protocol of the tools/time_*.py scripts that compare variants of one call (profiles/README.md, "The timing
protocol"): a parent that starts fresh child processes one after the other and stops at the first that fails, the loops a child
times its variants with, and the reduction of the children's lines to a summary.  A script keeps what it measures, this file how.
Nothing here imports torch or cpe_amd outside a function only a child calls: the parent runs without the library built."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'tests'), ROOT]      # the children import cpe_amd and the scene generators of tests/


def parse(ap, reps, child_timeout):
    """adds the protocol's arguments to a script's own, with that script's defaults -> the parsed command line"""
    ap.add_argument('--reps', type=int, default=reps)
    ap.add_argument('--procs', type=int, default=3)
    ap.add_argument('--child-timeout', type=float, default=child_timeout, help='seconds one child may take')
    ap.add_argument('--out', default=None, help='also append every raw line to this file')
    ap.add_argument('--child', action='store_true')
    return ap.parse_args()


def run_children(script, a, args=None):
    """Starts a.procs children strictly one after the other: `script --child` with the parent's own arguments, each under
    a.child_timeout seconds.  Their stdout lines that begin with '{' are tagged with the process number and emitted.  A child
    that exits non-zero or outlives its limit raises (CalledProcessError / TimeoutExpired) out of here: no further child is
    started on the GPU and the caller never reaches its summary.
    -> rows (every emitted line, in order), emit (prints a line, flushes, appends it to a.out; the caller's summaries go through it)"""
    rows = []

    def emit(d):
        rows.append(d)
        print(json.dumps(d), flush=True)
        if a.out:
            with open(a.out, 'a') as f:
                f.write(json.dumps(d) + '\n')
    cmd = [sys.executable, os.path.abspath(script), '--child'] + (sys.argv[1:] if args is None else args)
    for p in range(a.procs):
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, check=True, timeout=a.child_timeout)
        for ln in r.stdout.splitlines():
            if ln.startswith('{'):
                emit(dict(json.loads(ln), process=p))
    return rows, emit


def reduce(rows, keys=None, field='median_ms'):
    """rows: one case's line from every child -> (median over the children's medians, spread = max - min of them), per key"""
    keys = list(rows[0][field]) if keys is None else keys
    med = {k: statistics.median(d[field][k] for d in rows) for k in keys}
    spread = {k: max(d[field][k] for d in rows) - min(d[field][k] for d in rows) for k in keys}
    return med, spread


def carry(summary, rows, skip=()):
    """the summary, then every figure it does not have yet from the first process's row -- the counts, statuses and errors, which
    do not depend on the process -- but not that row's reps, raw times and process number"""
    return dict(summary, **{k: v for k, v in rows[0].items() if k not in summary and k not in ('reps', 'ms', 'process') + tuple(skip)})


def ratio_summary(head, rows, ratios, skip=()):
    """head, median_ms, spread_ms, name = median[num] / median[den] for (name, num, den) in ratios, the carried figures"""
    med, spread = reduce(rows)
    return carry(dict(head, median_ms=med, spread_ms=spread, **{name: med[num] / med[den] for name, num, den in ratios}), rows, skip)


def medians(ms):
    return {k: statistics.median(v) for k, v in ms.items()}


def event_loop(variants, reps):
    """variants: {name: callable}, already warm -> {name: [ms of every repetition]}, the variants alternated inside every
    repetition, each call between two device events.  The queue is empty at e0 (every repetition ends in a synchronise), so this
    is the window of `e0.record(); f(); e1.record(); torch.cuda.synchronize()` after a synchronised warm-up as well."""
    import torch
    ms = {k: [] for k in variants}
    for _ in range(reps):
        for k, f in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return ms


def time_variants(variants, reps):
    """-> first ({name: result of the one warm-up call}: the figures of the line), ms (event_loop)"""
    import torch
    first = {k: f() for k, f in variants.items()}
    torch.cuda.synchronize()
    return first, event_loop(variants, reps)


def host_loop(variants, reps):
    """as event_loop, on the host clock: for calls that end with their results on the host (a device-to-host copy)"""
    import torch
    ms = {k: [] for k in variants}
    for _ in range(reps):
        for k, f in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    return ms


def resident(event_ms, key, fn, *args, **kw):
    """a host_loop variant around one resident multi-frame fit: fn(*args, **kw), then T, fvals and iters pulled back to the host;
    the device-event time of the same call is appended to event_ms[key] -> (fn's result, the host copy)"""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    res = fn(*args, **kw)
    e1.record()
    back = torch.cat([res['T'].ravel(), res['fvals'].ravel(), res['iters'].ravel().to(torch.float64)]).cpu()
    event_ms.setdefault(key, []).append(e0.elapsed_time(e1))
    return res, back
