"""The MATLAB experiment, exp_gridDetection.m:22-94 without its figures, on a folder of raw stereo images:

    getUniqueName -> parseImgInfo -> per image pair: imread, preProcessing, makePyGridPts L/R, fitSingleCylinder
                  -> fitCylinderWPts3sAngs over the frames that were fitted

Image pairs are read in windows of `chunk`; a window is uploaded as it was decoded (uint8 / uint16, grey or RGB) and goes
through FramePipeline.run_raw: the fused pre-step (iotool.StereoPrestep), one detect call for both cameras and the batched
fitSingleCylinder, all resident on the GPU."""
import os
import re
import warnings

import numpy as np
import torch

from . import api, fit, iotool, multiframe, pipeline
from . import lib as _lib


def unique_names(input_path):
    """getUniqueName.m: the stems of the `*.png` files whose name ends in `L.png` (at least 5 characters), sorted, unique"""
    stems = {f[:-5] for f in os.listdir(input_path) if f.endswith('.png') and len(f) >= 5 and f[-5:] == 'L.png'}
    return sorted(stems)


def parse_img_info(stems):
    """parseImgInfo.m:19: '<pan><tilt>' -> F x 2 array of degrees by ^(-?\\d+)(-?\\d+)$, greedy as MATLAB's regexp
    ('123' -> 12, 3); a stem that does not match gives [0, 0] and a warning, as there"""
    ang = np.zeros((len(stems), 2), dtype=np.float64)
    for i, s in enumerate(stems):
        m = re.match(r'^(-?\d+)(-?\d+)$', s)
        if m is None:
            warnings.warn(f'image name {s!r} is not <pan><tilt>: angles set to [0, 0]')
        else:
            ang[i] = float(m.group(1)), float(m.group(2))
    return ang


def read_raw_image(path):
    """decoded as MATLAB's imread hands the file to im2uint8: 8-bit grey -> uint8 [h,w], 16-bit grey -> uint16 [h,w], colour
    -> uint8 RGB [h,w,3].  An alpha channel is dropped (imread returns it as a separate output).
    PNG kinds that differ from imread, because of the decoder: 16-bit RGB arrives reduced to 8 bits (imread gives uint16
    RGB, so im2uint8's rounding of the 16-bit value is lost: up to 1 grey level), 16-bit grey with alpha likewise; a palette
    file arrives as its RGB colours (imread's first output is the index matrix)."""
    from PIL import Image
    if not os.path.isfile(path):
        raise FileNotFoundError(path)
    with Image.open(path) as im:
        if im.mode in ('L', '1', 'LA'):
            return np.array(im.convert('L'), dtype=np.uint8)
        if im.mode.startswith('I;16') or im.mode == 'I':      # (a 16-bit PNG; older decoders widen it to 32-bit 'I')
            a = np.array(im)
            if a.size and (int(a.min()) < 0 or int(a.max()) > 65535):
                raise _lib.CpeError(f'{path}: {im.mode} image holds values outside 0..65535 ({int(a.min())}..{int(a.max())})')
            return a.astype(np.uint16)
        if im.mode in ('RGB', 'RGBA', 'P'):
            return np.array(im.convert('RGB'), dtype=np.uint8)
        raise _lib.CpeError(f'{path}: image mode {im.mode} is not one the experiment reads (8/16-bit grey, RGB)')


def _upload(images, device):
    a = np.stack(images)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(device)     # (uint16 bits: iotool.StereoPrestep)


def run_experiment(input_path, camera_json, K1, K2, T21, radius=45.0, device='cuda:0', chunk=32, multi_frame=True, mat_path=None,
                   frame_angles=False, match_offset=None):
    """-> dict(names, angles (rad, F x 2), records f64 [F,16] (pipeline.REC layout), pts3 f64 [F,MAXP,3] / cnt i32 [F],
               cyl_raw f64 [F,2,6] ([cylParams0; cylParams] of every frame, the multi-frame fit's third input), skipped,
               T_cam_agv (4x4 row-major list) / fval -- None without multi_frame or with fewer than 2 fitted frames)

    multi_frame: True = multiframe.fit_multi_frame (simplex on the host, bit-identical to the oracle); 'gpu' =
    multiframe.fit_multi_frame_gpu (the whole fit resident, device sin / cos: fval agrees to ~1e-12 relative); 'lm' = the same
    call with method='lm' (build-defined: all-frame initial pose + Levenberg-Marquardt, not the reference's path); False = none.
    The 'gpu' and 'lm' modes fit at most CPE_MULTI_MAXF = 1024 good frames: with more they warn (status 6, CPE_ST_OVERFLOW) and return
    None results, where the host mode would fit them.

    Every `<stem>L.png` needs its `<stem>R.png`: the reference fails in imread on a missing partner, this raises
    FileNotFoundError naming the file, before any frame is processed.
    A frame whose left or right detect status or fit status is non-zero is listed in `skipped` as dict(index, name,
    det_left, det_right, fit) and left out of the multi-frame fit (the script's try / warning leaves such a frame's cell
    empty).  mat_path: the per-frame results are also written there by api.save_mat (frames, names).

    match_offset: None, or a dict of fit.match_offset_batch keywords ({} = its defaults; build-defined, nothing like it in the
    reference): every frame's index shift between the two tables is searched before the selector (FramePipeline(match=...)).
    The dict gains offset i32 [F,2], match_score i32 [F,4] and match_flags i32 [F].  A frame
    flagged fit.MATCH_WEAK -- no shift gave a cylinder worth trusting -- is listed in `skipped` (every entry then has a `match`
    key: the frame's flags) and left out of the multi-frame fit; a frame flagged MATCH_SHIFTED is used.

    frame_angles=True (build-defined, nothing like it in the reference): with a multi-frame result, the good frames go through
    multiframe.estimate_frame_angles_gpu with T_cam_agv, a self-check of the calibration in degrees.  The dict gains
    angles_est (F x 2, rad; NaN for a skipped or failed frame), angles_status (F; the solver's status, -1 for a frame that was
    not given to it) and angles_delta_deg (estimated - nominal); all three are None without a multi-frame result."""
    names = unique_names(input_path)
    if not names:
        raise FileNotFoundError(f'no <name>L.png in {input_path}')
    paths = [(os.path.join(input_path, s + 'L.png'), os.path.join(input_path, s + 'R.png')) for s in names]
    for pair in paths:
        for p in pair:
            if not os.path.isfile(p):
                raise FileNotFoundError(p)
    angles = np.deg2rad(parse_img_info(names))          # exp_gridDetection.m:26-27
    cam_l, cam_r = iotool.load_camera_data(camera_json)
    F, chunk = len(names), max(1, int(chunk))
    dev = torch.device(device)
    pipe = pre = None
    recs = torch.empty((F, pipeline.REC), dtype=torch.float64, device=dev)
    fits = pipeline.alloc_fits(F, dev)
    for w0 in range(0, F, chunk):
        imgs = [(read_raw_image(l), read_raw_image(r)) for l, r in paths[w0:w0 + chunk]]
        if pipe is None:
            h, w = imgs[0][0].shape[:2]
            pre = iotool.StereoPrestep(cam_l, cam_r, h, w, dev)
            pipe = pipeline.FramePipeline(h, w, K1, K2, T21, radius, chunk=chunk, device=dev, match=match_offset)
        kinds = [tuple((a.dtype, a.shape) for a in pair) for pair in imgs]
        for kd, s in zip(kinds, names[w0:]):
            if any(shape[:2] != (pipe.h, pipe.w) for _, shape in kd):
                raise _lib.CpeError(f'{s}: image size differs from the first pair ({pipe.w}x{pipe.h})')
        i0 = 0
        while i0 < len(imgs):                           # frames of one element type and channel count go together
            i1 = i0 + 1
            while i1 < len(imgs) and kinds[i1] == kinds[i0]:
                i1 += 1
            left = _upload([p[0] for p in imgs[i0:i1]], dev)
            right = _upload([p[1] for p in imgs[i0:i1]], dev)
            recs[w0 + i0:w0 + i1] = pipe.run_raw(left, right, pre, {k: t[w0 + i0:w0 + i1] for k, t in fits.items()})
            i0 = i1
    _, _, d_fit, d_l, d_r = pipeline.unpack_counters(recs[:, 15])          # device tensors: the 'gpu' mode masks with them
    st_fit, st_l, st_r = (t.cpu().tolist() for t in (d_fit, d_l, d_r))
    if match_offset is None:
        skipped = [dict(index=i, name=names[i], det_left=st_l[i], det_right=st_r[i], fit=st_fit[i])
                   for i in range(F) if st_l[i] or st_r[i] or st_fit[i]]
    else:
        d_weak = fits['match_flags'] & fit.MATCH_WEAK
        mfl = fits['match_flags'].cpu().tolist()
        skipped = [dict(index=i, name=names[i], det_left=st_l[i], det_right=st_r[i], fit=st_fit[i], match=mfl[i])
                   for i in range(F) if st_l[i] or st_r[i] or st_fit[i] or (mfl[i] & fit.MATCH_WEAK)]
    res = dict(names=names, angles=angles, records=recs, pts3=fits['pts3'], cnt=fits['m'], cyl_raw=fits['cyl_raw'], skipped=skipped,
               T_cam_agv=None, fval=None)
    if match_offset is not None:
        res.update(offset=fits['offset'], match_score=fits['match_score'], match_flags=fits['match_flags'])
    if mat_path is not None:
        api.save_mat(mat_path, fits=fits, names=names)
    if multi_frame in ('gpu', 'lm'):
        # resident: the kept frames are named by a device mask made from the records' status words, the whole tables go in
        # as one group, and T, fval, status and the count of kept frames come back in one copy
        frame_ok = (d_fit == 0) & (d_l == 0) & (d_r == 0)
        if match_offset is not None:
            frame_ok = frame_ok & (d_weak == 0)
        frame_ok = frame_ok.to(torch.int32)
        mf = multiframe.fit_multi_frame_gpu(fits['pts3'], fits['m'], fits['cyl_raw'], angles, radius, frame_ok=frame_ok,
                                            group_start=[0, F], method='lm' if multi_frame == 'lm' else 'nm')
        back = torch.cat([mf['T'][0], mf['fvals'][0], mf['status'][0:1].to(torch.float64),
                          frame_ok.sum().to(torch.float64).reshape(1)]).cpu().tolist()
        n_good, status = int(back[19]), int(back[18])
        if n_good < 2:
            warnings.warn(f'{n_good} fitted frame(s): fitCylinderWPts3sAngs needs two')
        elif status != 0:
            warnings.warn(f'multi-frame fit ended with status {status} (include/cpe.h: cpe_multi_frame_fit_batch)')
        else:
            res['T_cam_agv'], res['fval'] = back[:16], back[17]
    elif multi_frame:
        bad = {s['index'] for s in skipped}
        good = [i for i in range(F) if i not in bad]
        if len(good) < 2:
            warnings.warn(f'{len(good)} fitted frame(s): fitCylinderWPts3sAngs needs two')
        else:
            g = torch.tensor(good, device=dev)
            mf = multiframe.fit_multi_frame(fits['pts3'][g], fits['m'][g], fits['cyl_raw'][g], angles[good], radius)
            res['T_cam_agv'], res['fval'] = mf['T'], mf['fvals'][1]
    if frame_angles:
        res.update(angles_est=None, angles_status=None, angles_delta_deg=None)
        if res['T_cam_agv'] is not None:
            bad = {s['index'] for s in skipped}
            good = [i for i in range(F) if i not in bad]
            g = torch.tensor(good, device=dev)
            fa = multiframe.estimate_frame_angles_gpu(fits['pts3'][g], fits['m'][g], fits['cyl_raw'][g], res['T_cam_agv'], radius)
            est, status = np.full((F, 2), np.nan), np.full(F, -1, dtype=np.int32)
            st = fa['status'].cpu().numpy()
            status[good] = st
            est[good] = np.where((st == 0)[:, None], fa['angles'].cpu().numpy(), np.nan)
            res.update(angles_est=est, angles_status=status, angles_delta_deg=np.rad2deg(est - angles))
    return res
