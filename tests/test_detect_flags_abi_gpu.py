"""CpeDetectParams.flags at the C ABI (include/cpe.h): a bit the build does not know is refused with CPE_ERR_ARG before
anything is launched -- outputs and workspace keep what they held -- and flags = 0 is a NULL params."""
import ctypes as C

import numpy as np
import pytest
import torch

CPE_ERR_ARG = -1
TABLES = ('xy', 'id', 'n', 'center', 'status')


def _call(cpe, frames, ws, out, prm):
    n, h, w = frames.shape
    L = cpe.lib.load()
    return L.cpe_detect_grid_batch_ex(frames.data_ptr(), n, h, w, C.addressof(prm) if prm is not None else None, ws.view.data_ptr(), ws.bytes,
                                      out['xy'].data_ptr(), out['id'].data_ptr(), out['n'].data_ptr(), out['center'].data_ptr(),
                                      out['status'].data_ptr(), torch.cuda.current_stream().cuda_stream)


def _tables(n, gpu, fill):
    from cpe_amd.fit import MAXP
    return dict(xy=torch.full((n, MAXP, 2), float(fill), dtype=torch.float64, device=gpu), id=torch.full((n, MAXP, 2), fill, dtype=torch.int32, device=gpu),
                n=torch.full((n,), fill, dtype=torch.int32, device=gpu), center=torch.full((n, 2), float(fill), dtype=torch.float64, device=gpu),
                status=torch.full((n,), fill, dtype=torch.int32, device=gpu))


@pytest.fixture(scope='module')
def frames(gpu):
    from cpe_amd import synth
    b = synth.render_batch(1, 480, 640, seed=0, with_gt=False)
    return torch.cat([b['left'], b['right']]).to(gpu).contiguous()


@pytest.mark.gpu
@pytest.mark.parametrize('flags', [2, -1, 3])
def test_unknown_flag_bits_are_refused_before_any_launch(cpe, gpu, frames, flags):
    n, h, w = frames.shape
    ws = cpe.api.DetectWorkspace(n, h, w, gpu)
    ws.buf.fill_(0x5a)
    out = _tables(n, gpu, 77)
    prm = cpe.lib.CpeDetectParams(0, 7, 1.0, 0, flags)
    rc = _call(cpe, frames, ws, out, prm)
    torch.cuda.synchronize()
    assert rc == CPE_ERR_ARG
    assert b'flags' in cpe.lib.load().cpe_last_error_string()
    assert bool((ws.buf == 0x5a).all()), 'the workspace was written'
    ref = _tables(n, gpu, 77)
    for k in TABLES:
        assert torch.equal(out[k], ref[k]), k


@pytest.mark.gpu
def test_null_params_and_zero_flags_agree(cpe, gpu, frames):
    n, h, w = frames.shape
    res = []
    for prm in (None, cpe.lib.CpeDetectParams(0, 7, 1.0, 0, 0)):
        ws = cpe.api.DetectWorkspace(n, h, w, gpu)
        out = _tables(n, gpu, 0)
        assert _call(cpe, frames, ws, out, prm) == 0
        torch.cuda.synchronize()
        res.append((out, {k: ws.plane(k).cpu().numpy() for k in ('hmask', 'vmask', 'roi_h', 'roi_v', 'exp_h', 'exp_v', 'mask_contour')}, ws.state()))
    (a, pa, sa), (b, pb, sb) = res
    assert int((a['status'] == 0).sum()) >= 1
    for k in TABLES:
        assert torch.equal(a[k], b[k]), k
    for k in pa:
        assert np.array_equal(pa[k], pb[k]), k
    assert pa['hmask'].any() and pa['roi_h'].any()
    assert sa == sb
