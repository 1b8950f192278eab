#!/usr/bin/env python3
"""Record the output bits of the two Levenberg-Marquardt kernels (cpe_multi_frame_fit_lm_batch, cpe_frame_angles_lm_batch)
for tests/test_lm_recorded_bits_gpu.py.  Run it on the GPU at the commit BEFORE a change to those kernels:

    python tools/record_lm_bits.py [--out tests/golden/lm_parent_bits.npz]

The calls are tests/lm_recorded_cases.py::collect.  Every output array is stored as its uint64 / int32 bits, beside the commit
hash (HEAD; the recorder refuses a work tree whose csrc/ or include/ differ from it, so the hash names what was built) and the
`hipcc --version` text of the build.  Before writing, the recorded set is checked not to be trivial: each kernel
has a call with a rejected trial, one that ends at max_iter, and the angle solver a frame that starts beyond the tilt limit."""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]


def toolchain():
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    return subprocess.run([hipcc, '--version'], check=True, capture_output=True, text=True).stdout.strip()


def check_coverage(out, runs):
    import frame_angles_cases as fc
    import lm_recorded_cases as rc
    for kernel, calls in runs.items():
        rejected = [c for c, it, start, _ in calls if ((it.reshape(-1, 2)[:, 1] - it.reshape(-1, 2)[:, 0]) > start).any()]
        capped = [c for c, it, _, cap in calls if cap is not None and (it.reshape(-1, 2)[:, 0] == cap).any()]
        print(f'{kernel}: {len(calls)} calls, {len(rejected)} with a rejected trial, {len(capped)} ending at max_iter')
        assert rejected, f'{kernel}: no recorded call has a rejected trial'
        assert capped, f'{kernel}: no recorded call ends at max_iter'
    beyond = 0
    for key in out:
        if key.startswith('fa/') and key.endswith('/far/angles0'):
            st = out[key[:-len('angles0')] + 'status']
            F = len(st)
            tilt0 = np.array((rc.FAR_STARTS * 17)[:F])[:, 1]
            sel = np.abs(tilt0) >= fc.TILT_LIMIT
            assert np.isin(st[sel], (0, 5)).all()
            beyond += int(sel.sum())
            print(f'{key[:-len("/angles0")]}: statuses of the starts beyond the tilt limit {st[sel].tolist()}')
    assert beyond, 'no recorded angle frame starts beyond the tilt limit'


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'lm_parent_bits.npz'))
    a = ap.parse_args()
    git = lambda *args: subprocess.run(['git', '-C', ROOT] + list(args), check=True, capture_output=True, text=True).stdout.strip()
    commit = git('rev-parse', 'HEAD')
    dirty = git('status', '--porcelain', '--', 'cylinder-pose-estimation_amd/csrc', 'include')
    if dirty:
        sys.exit(f'the kernels differ from {commit}: commit or stash first, and rebuild\n{dirty}')
    import torch
    import cpe_amd
    import lm_recorded_cases as rc
    cpe_amd.lib.load()
    out, runs = rc.collect(torch.device('cuda:0'))
    check_coverage(out, runs)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, __commit__=np.array(commit), __toolchain__=np.array(toolchain()), **out)
    print(f'{a.out}: {len(out)} arrays, {os.path.getsize(a.out)} bytes, commit {commit}')


if __name__ == '__main__':
    main()
