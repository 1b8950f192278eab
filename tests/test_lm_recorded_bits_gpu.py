"""Every output bit of cpe_multi_frame_fit_lm_batch and cpe_frame_angles_lm_batch against the bits recorded before the change
under test (tests/golden/lm_parent_bits.npz, written by tools/record_lm_bits.py from the calls of lm_recorded_cases.collect).
The other tests of these two kernels compare the result with the exported pieces and with an optimum, which a changed sequence
of trials can still satisfy; this one pins the iterates: x, f, the iteration and evaluation counts, every status."""
import os
import subprocess

import numpy as np
import pytest

import lm_recorded_cases as rc
from conftest import GOLDEN


@pytest.mark.gpu
def test_outputs_equal_the_recorded_bits(cpe, gpu):
    rec = np.load(os.path.join(GOLDEN, 'lm_parent_bits.npz'))
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    toolchain = subprocess.run([hipcc, '--version'], check=True, capture_output=True, text=True).stdout.strip()
    assert toolchain == str(rec['__toolchain__']), (
        'the bits were recorded with another compiler: check out the commit before the change under test (the file was last '
        f'recorded at {rec["__commit__"]}), run tools/record_lm_bits.py there on the GPU, and test again')
    got, _ = rc.collect(gpu)
    keys = sorted(k for k in rec.files if not k.startswith('__'))
    assert sorted(got) == keys
    differ = [k for k in keys if got[k].dtype != rec[k].dtype or not np.array_equal(got[k], rec[k])]
    assert not differ, f'{len(differ)} of {len(keys)} outputs differ from the recorded bits: {differ[:12]}'
