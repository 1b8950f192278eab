"""The MATLAB experiment, exp_gridDetection.m:22-94 without its figures, on a folder of raw stereo images:

    getUniqueName -> parseImgInfo -> per image pair: imread, preProcessing, makePyGridPts L/R, fitSingleCylinder
                  -> fitCylinderWPts3sAngs over the frames that were fitted

Image pairs are read in windows of `chunk`; a window is uploaded as it was decoded (uint8 / uint16, grey or RGB) and goes
through FramePipeline.run_raw: the fused pre-step (iotool.StereoPrestep), one detect call for both cameras and the batched
fitSingleCylinder, all resident on the GPU."""
import math
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


def _list_pairs(input_path):
    """the stems of the folder and their (left, right) paths; every `<stem>L.png` needs its `<stem>R.png`"""
    names = unique_names(input_path)
    if not names:
        raise FileNotFoundError(f'no <name>L.png in {input_path}')
    paths = [(os.path.join(input_path, s + 'L.png'), os.path.join(input_path, s + 'R.png')) for s in names]
    for pair in paths:
        for p in pair:
            if not os.path.isfile(p):
                raise FileNotFoundError(p)
    return names, paths


def _run_pairs(names, paths, camera_json, dev, chunk, make_fits, make_pipeline, source='stereo'):
    """the read / upload loop of run_experiment and run_plane_experiment: the pairs are read in windows of `chunk`, runs of one
    element type and channel count are uploaded together and go through FramePipeline.run_raw of make_pipeline(h, w, chunk)
    -> records f64 [F,16], the tensors of make_fits(F) filled.  source 'left' / 'right': the other camera's files are not read"""
    cam_l, cam_r = iotool.load_camera_data(camera_json)
    F, chunk = len(names), max(1, int(chunk))
    pipe = pre = None
    recs = torch.empty((F, pipeline.REC), dtype=torch.float64, device=dev)
    fits = make_fits(F)
    for w0 in range(0, F, chunk):
        imgs = [(read_raw_image(l) if source != 'right' else None, read_raw_image(r) if source != 'left' else None)
                for l, r in paths[w0:w0 + chunk]]
        if pipe is None:
            h, w = next(a for a in imgs[0] if a is not None).shape[:2]
            pre = iotool.StereoPrestep(cam_l, cam_r, h, w, dev)
            pipe = make_pipeline(h, w, chunk)
        kinds = [tuple((a.dtype, a.shape) for a in pair if a is not None) for pair in imgs]
        for kd, s in zip(kinds, names[w0:]):
            if any(shape[:2] != (pipe.h, pipe.w) for _, shape in kd):
                raise _lib.CpeError(f'{s}: image size differs from the first pair ({pipe.w}x{pipe.h})')
        i0 = 0
        while i0 < len(imgs):                           # frames of one element type and channel count go together
            i1 = i0 + 1
            while i1 < len(imgs) and kinds[i1] == kinds[i0]:
                i1 += 1
            left = _upload([p[0] for p in imgs[i0:i1]], dev) if source != 'right' else None
            right = _upload([p[1] for p in imgs[i0:i1]], dev) if source != 'left' else None
            recs[w0 + i0:w0 + i1] = pipe.run_raw(left, right, pre, {k: t[w0 + i0:w0 + i1] for k, t in fits.items()})
            i0 = i1
    return recs, fits


def _frame_status(names, recs, match_flags=None, also=None):
    """the records' status words -> frame_ok i32[F] on the device (1: both detect statuses and the fit status are zero, and with
    match_flags i32[F] the frame is not fit.MATCH_WEAK), `skipped`: the other frames as dict(index, name, det_left, det_right,
    fit[, match]), and the host values of also(frame_ok), a list of device scalars -- all brought back in one copy"""
    F = len(names)
    _, _, d_fit, d_l, d_r = pipeline.unpack_counters(recs[:, 15])
    frame_ok = (d_fit == 0) & (d_l == 0) & (d_r == 0)
    words = dict(det_left=d_l, det_right=d_r, fit=d_fit)
    if match_flags is not None:
        frame_ok = frame_ok & ((match_flags & fit.MATCH_WEAK) == 0)
        words['match'] = match_flags
    frame_ok = frame_ok.to(torch.int32)
    extra = [] if also is None else list(also(frame_ok))
    back = torch.cat([torch.stack(list(words.values()) + [frame_ok]).to(torch.int64).reshape(-1)] +
                     [t.to(torch.int64).reshape(1) for t in extra]).cpu().tolist()
    host = {k: back[j * F:(j + 1) * F] for j, k in enumerate(words)}
    skipped = [dict(index=i, name=names[i], **{k: v[i] for k, v in host.items()}) for i in range(F) if not back[len(words) * F + i]]
    return frame_ok, skipped, back[(len(words) + 1) * F:]


def _index_range(idx, used):
    """lo, hi (device scalars) of the indices idx i32[F,MAXP,2] in the slots used bool[F,MAXP]; lo > hi when no slot is"""
    big = torch.iinfo(torch.int32).max
    return torch.where(used[..., None], idx, big).amin(), torch.where(used[..., None], idx, -big).amax()


def _take_multi_frame(res, n_good, status, what, T, fval):
    """the end of the resident multi-frame modes (what: 'fit' or 'consensus'): a warning, or T_cam_agv and fval taken -> taken?"""
    if n_good < 2:
        warnings.warn(f'{n_good} fitted frame(s): fitCylinderWPts3sAngs needs two')
    elif status != 0:
        warnings.warn(f'multi-frame {what} ended with status {status} (include/cpe.h: cpe_multi_frame_{what}_batch)')
    else:
        res['T_cam_agv'], res['fval'] = T, fval
    return n_good >= 2 and status == 0


def _fit_projector(fits, frame_ok, projector, family0, use=None, table_path=None):
    """the projector model of an experiment's own stereo points: fit.fit_projector_model over the kept frames with lo, hi the
    range of the indices they hold, and its table for -N..N, N the largest |index| seen (or projector['lo'], ['hi']): also the
    lines no frame showed.  projector: a dict of fit.fit_projector_model keywords beside lo, hi and renumber.
    renumber: None, or a dict of win, tau, min_score ({} = the defaults of fit.fit_projector_model_renumbered, which runs in
    place of the single fit): the frames are re-numbered against the first model's table and fitted again over the range
    widened by max(win); fit, model, laser_table and the list of trimmed frames then describe the refit, N is taken from the
    widened range, and the dict gains first (the first fit's dict) and shift (fit.index_shift_batch's dict).
    -> dict(fit, model (fit.ProjectorModel), laser_table) or None (a warning says why), the list of the frames where at
    least half of one family's residuals were trimmed: frames numbered off by a line, and with renumber the list of (frame, d0,
    d1) of the kept frames that got a non-zero shift (None without renumber)"""
    kw = dict(projector)
    t_lo, t_hi = kw.pop('lo', None), kw.pop('hi', None)
    ren = kw.pop('renumber', None)
    none = (None, [], None if ren is None else [])
    used = (torch.arange(fit.MAXP, device=frame_ok.device)[None, :] < fits['m'][:, None]) & (frame_ok != 0)[:, None]
    if use is not None:
        used = used & (use != 0)
    lo, hi = torch.stack(_index_range(fits['idx'], used)).cpu().tolist()
    if lo > hi:
        warnings.warn('no fitted frame: no projector model')
        return none
    if hi - lo + 1 > _lib.MAXL:
        warnings.warn(f'grid indices {lo}..{hi} span more than {_lib.MAXL} values: no projector model')
        return none
    extra, renumbered = {}, None
    if ren is None:
        out = fit.fit_projector_model(fits['pts3'], fits['idx'], fits['m'], lo, hi, use=use, frame_ok=frame_ok, **kw)
    else:
        unknown = set(ren) - {'win', 'tau', 'min_score'}
        if unknown:
            raise TypeError(f"projector['renumber'] holds win, tau, min_score; got {sorted(unknown)}")
        rn = fit.fit_projector_model_renumbered(fits['pts3'], fits['idx'], fits['m'], lo, hi, use=use, frame_ok=frame_ok,
                                                win=ren.get('win', (4, 4)), shift_tau=ren.get('tau'),
                                                shift_min_score=ren.get('min_score', 8), family0=family0, **kw)
        out, lo, hi = rn['fit'], rn['lo'], rn['hi']
        extra = dict(first=rn['first'], shift=rn['shift'])
        sh = torch.cat([rn['shift']['shift'], frame_ok.to(torch.int32)[:, None]], 1).cpu().tolist()
        renumbered = [(i, d0, d1) for i, (d0, d1, ok) in enumerate(sh) if ok and (d0 or d1)]
    model = fit.ProjectorModel.from_fit(out, family0)
    if model.status != 0:
        warnings.warn('the projector model was not fitted (fewer than 2 usable lines in a family, or planes that give no centre)')
    half = min(max(abs(lo), abs(hi)), (_lib.MAXL - 1) // 2)
    table = model.table(-half if t_lo is None else t_lo, half if t_hi is None else t_hi)
    if table_path is not None:
        table.save(table_path)
    fc = out['frame_counts'].cpu().numpy()
    shifted = [i for i in range(len(fc)) if any(fc[i, 2 * k + 1] > 0 and 2 * fc[i, 2 * k + 1] >= fc[i, 2 * k] + fc[i, 2 * k + 1] for k in range(2))]
    return dict(fit=out, model=model, laser_table=table, **extra), shifted, renumbered


def refine_listing(names, round_taken, renumbered):
    """round_taken i32 [F], renumbered i32 [F,2] of fit.fit_single_cylinder_refined_batch -> a list of dict(index, name, round,
    left, right) for the frames where a point of either image was re-numbered"""
    rt, rn = torch.as_tensor(round_taken).cpu().tolist(), torch.as_tensor(renumbered).cpu().tolist()
    return [dict(index=i, name=names[i], round=rt[i], left=rn[i][0], right=rn[i][1]) for i in range(len(names)) if rn[i][0] or rn[i][1]]


def repair_listing(names, shift, flags, round_taken, renumbered):
    """shift i32 [F,2], flags, round_taken, renumbered i32 [F] of fit.fit_single_cylinder_mono_repaired_batch -> a list of
    dict(index, name, shift, flags, round, renumbered) for the frames where anything changed: a non-zero shift, a flag, or a
    re-numbered point"""
    sh, fl, rt, rn = (torch.as_tensor(t).cpu().tolist() for t in (shift, flags, round_taken, renumbered))
    return [dict(index=i, name=names[i], shift=tuple(sh[i]), flags=fl[i], round=rt[i], renumbered=rn[i]) for i in range(len(names))
            if any(sh[i]) or fl[i] or rn[i]]


def run_experiment(input_path, camera_json, K1, K2, T21, radius=45.0, device='cuda:0', chunk=32, multi_frame=True, mat_path=None,
                   frame_angles=False, match_offset=None, laser_table=None, source='stereo', projector=None, table_path=None,
                   curvature=None, consensus=None, refine=None, pixels=None, multi_frame_pixels=None, multi_frame_joint=None,
                   repair=None):
    """-> dict(names, angles (rad, F x 2), records f64 [F,16] (pipeline.REC layout), pts3 f64 [F,MAXP,3] / cnt i32 [F],
               cyl_raw f64 [F,2,6] ([cylParams0; cylParams] of every frame, the multi-frame fit's third input), skipped,
               T_cam_agv (4x4 row-major list) / fval -- None without multi_frame or with fewer than 2 fitted frames)

    multi_frame: True = multiframe.fit_multi_frame (simplex on the host, bit-identical to the oracle); 'gpu' =
    multiframe.fit_multi_frame_gpu (the whole fit resident, device sin / cos: fval agrees to ~1e-12 relative); 'lm' = the same
    call with method='lm' (build-defined: all-frame initial pose + Levenberg-Marquardt, not the reference's path); 'consensus' =
    multiframe.fit_multi_frame_consensus_gpu (build-defined, below); False = none.
    The 'gpu', 'lm' and 'consensus' modes fit at most CPE_MULTI_MAXF = 1024 good frames: with more they warn (status 6,
    CPE_ST_OVERFLOW) and return None results, where the host mode would fit them.

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

    source='left' / 'right' with laser_table= (build-defined): the frames' points come from that camera alone and the projector's
    laser-plane table -- a fit.LaserTable, or the path of one saved by LaserTable.save / run_plane_experiment(table_path=) --
    through FramePipeline(source=..., laser_table=...): the other camera's files are not read (they must still exist), its detect
    status is 0 in the records, and the dict gains tri_counts i32 [F,4] and tri_stats f64 [F,2] (fit.table_triangulate_batch's
    counts and stats).  The table's gates keep their defaults here; FramePipeline(table=...) sets them.

    source='fused' with laser_table= (build-defined): both cameras' files are read and detected as for 'stereo', and every grid
    point of either image becomes a 3-D point from its rays and the laser planes in one solve (FramePipeline(source='fused'),
    fit.fit_single_cylinder_fused_batch): no selector, and a point that one camera alone found is kept.  Word 14 of a record is
    the rms ray residual of the pairs in pixels; tri_counts is i32 [F,6] and tri_stats f64 [F,4] (fit.fused_triangulate_batch's).
    match_offset is refused: the numbering is repaired before, not inside, this call.

    refine= with source='fused' (build-defined, opt-in): None, or a dict of fit.fit_single_cylinder_refined_batch keywords ({} =
    its defaults).  Every frame is fitted from its stereo pairs first; then each grid point of either image takes the index of
    the nearest node of the grid which that fit and the laser-plane table predict, and the frame is fitted again on the fused
    points of the re-numbered tables (FramePipeline(source='fused', refine=...)).  The dict has no tri_counts / tri_stats then
    and gains refine = dict(round_taken i32 [F] (0: the first fit stands), renumbered i32 [F,2] (points of the left, right image
    whose index changed), frames: a list of dict(index, name, round, left, right) for the frames where any did).  Any other source
    raises ValueError.

    repair= with source='left' / 'right' (build-defined, opt-in): None, or a dict of fit.fit_single_cylinder_mono_repaired_batch
    keywords ({} = its defaults with the search on: shift={}, one round).  Every frame's grid indices are searched for a
    frame-wide shift against the laser-plane table, and every grid point is then re-numbered against the grid the frame's fit
    predicts (FramePipeline(source=..., table=dict(repair=...))).  The dict gains repair = dict(shift i32 [F,2], flags i32 [F]
    (fit.SHIFT_*), round_taken i32 [F], renumbered i32 [F], frames: a list of dict(index, name, shift, flags, round, renumbered)
    for the frames where anything changed).  Any other source raises ValueError.

    projector: None, or a dict of fit.fit_projector_model keywords ({} = its defaults; build-defined): the projector's model
    (two pencils of planes through one centre) is fitted to the experiment's own stereo points and indices -- after the index
    shift of match_offset where that is on -- over the frames the multi-frame fit would keep; no boards are needed.  The dict
    gains projector = dict(fit, model, laser_table) (the call's outputs, the fit.ProjectorModel, and its table for the lines
    -N..N, N the largest |index| seen, family0 'col'; None when there is nothing to fit) and projector_shifted: the frames where at
    least half of one family's residuals fell outside the band tau, i.e. frames numbered one line off.  table_path: the table is
    saved there (LaserTable.save).  source must be 'stereo'.
    projector['renumber']: None, or a dict of win, tau, min_score ({} = (4, 4), the fit's tau, 8; needs the fit's tau > 0): such
    frames are re-numbered against the first model's table and the model is fitted again with them
    (fit.fit_projector_model_renumbered).  projector then also holds first and shift, its fit, model, laser_table and
    projector_shifted describe the refit, and the dict gains projector_renumbered: the (frame, d0, d1) of the kept frames that
    got a non-zero shift.  The shift is relative to the majority of the frames.

    multi_frame='consensus' (build-defined): a frame can end with status 0 and a wrong cylinder, and the other modes add every
    good frame's term up.  This one takes T_cam_agv and fval from multiframe.fit_multi_frame_consensus_gpu over the same frames
    -- the pose that the largest set of frames agrees with to within tau (rms of dist - radius, the unit of the points), fitted
    to those frames -- and the dict gains consensus = dict(inliers: names of the frames the pose was fitted to, rejected: a list
    of dict(index, name, rms = sqrt of the frame's term at the pose) for the other good frames, n_inliers, rounds, flags, status).
    It warns when frames are rejected or the status is non-zero.  consensus=: None, or a dict of tau, max_hyp, max_rounds,
    min_inliers (defaults 0.5, 2048, 4, 3); with any other multi_frame it raises ValueError.  A majority of frames that are
    wrong in the same way wins; a frame is in or out whole.

    frame_angles=True (build-defined, nothing like it in the reference): with a multi-frame result, the good frames go through
    multiframe.estimate_frame_angles_gpu with T_cam_agv, a self-check of the calibration in degrees.  The dict gains
    angles_est (F x 2, rad; NaN for a skipped or failed frame), angles_status (F; the solver's status, -1 for a frame that was
    not given to it) and angles_delta_deg (estimated - nominal); all three are None without a multi-frame result.

    curvature: None, or a dict of k, mode, rho_max, band, r_min, r_max ({} = 20, fit.CURV_INTERCEPT, 0.25 and the band radius
    (1 -/+ 1/3); build-defined): fit.est_curvatures_batch and fit.curvature_consensus_batch run on the pts3 / cnt the run holds
    anyway, and the dict gains curvature = their two dicts merged (Kdir, L, normal, pt_status, axis, n_gated, gate, status = the
    consensus', curv_status = the per-frame status of the curvatures).  The fits of the run are untouched.

    pixels= with source 'fused', 'left' or 'right' (build-defined, opt-in): None, or a dict of fit.fit_cylinder_pixels_batch keywords
    ({} = its defaults): every frame's pose is polished on the pixels of the tables its fit was made from (FramePipeline(pixels=...),
    fit.polish_with_pixels; after refine= / repair= on the re-numbered tables).  records, cyl_raw and the multi-frame fit then read
    the polished poses, and the dict gains pixels = dict(cyl f64 [F,6] (the polished cyl[:, 1]), T f64 [F,4,4], fvals f64 [F,2]
    (px^2 at the start and the end), px_rms f64 [F] (of both cameras), counts i32 [F,4], status i32 [F] (the pixel fit's; a frame
    whose pixel fit is not ST_OK keeps its 3-D fit)).  source='stereo' raises ValueError.

    multi_frame_pixels= with source 'fused', 'left' or 'right' and multi_frame 'gpu', 'lm' or 'consensus' (build-defined, opt-in):
    None, or a dict of multiframe.fit_multi_frame_pixels_gpu keywords ({} = its defaults: sel_cos, min_cos, gate_px, tol_x, tol_f,
    max_iter).  T_Cam_AGV is fitted once more, to the pixels of all frames at once (include/cpe.h
    cpe_multi_frame_fit_pixels_batch): the start is that multi_frame mode's pose, the kept frames are its good frames (with
    'consensus' its inliers), the tables are the ones the frames' fits were made from (after refine= / repair=), and with 'left' /
    'right' the other camera is absent.  The laser table must be rigid with camera 1 across the frames.  The dict gains
    multi_frame_pixels = dict(T_cam_agv (16 row-major values, None unless status is 0), x f64 [6], fvals f64 [2] (px^2 at the start
    and the end), px_rms (of all used detections), counts i32 [4], status, cov f64 [6,6] (of the step (dw, dt); NaN unless status is
    0), frame_cyl f64 [F,6], frame_stats f64 [F,4] (NaN for the frames that were not used)) -- None when the point-based fit gave no
    pose.  T_cam_agv, fval and everything else keep their values.  Any other source or multi_frame raises ValueError.

    multi_frame_joint= (build-defined, opt-in; the preconditions of multi_frame_pixels=): None, or a dict of
    multiframe.fit_multi_frame_pixels_angles_gpu keywords ({} = its defaults: sigma_px, sigma_angle, w_pan, w_tilt, sel_cos, ...).
    T_Cam_AGV and every kept frame's pan and tilt are fitted jointly to the pixels (include/cpe.h
    cpe_multi_frame_fit_pixels_angles_batch), for heads whose angles are not exact.  The start is multi_frame_pixels=' pose when that
    is given and ended with status 0, else the multi_frame mode's pose; the nominal angles are the file names'.  The dict gains
    multi_frame_joint = dict(T_cam_agv, x, fvals, px_rms, counts, status, cov, frame_cyl, frame_stats as multi_frame_pixels has them,
    angles f64 [F,2] (the fitted ones) and angle_sigma f64 [F,2], NaN for the frames that were not used) -- None when there is no
    start.  Every other entry of the result keeps its bits."""
    for name, given in (('multi_frame_pixels', multi_frame_pixels), ('multi_frame_joint', multi_frame_joint)):
        if given is not None and (source not in ('fused', 'left', 'right') or multi_frame is True
                                  or multi_frame not in ('gpu', 'lm', 'consensus')):
            raise ValueError(f"{name}= predicts the pixels from the laser-plane table and starts at a resident multi-frame fit: "
                             "source must be 'fused', 'left' or 'right' and multi_frame 'gpu', 'lm' or 'consensus'")
    want_tables = multi_frame_pixels is not None or multi_frame_joint is not None
    if pixels is not None and source == 'stereo':
        raise ValueError("pixels= predicts the pixels from the laser-plane table: source must be 'fused', 'left' or 'right'")
    if curvature is not None:
        curv_opts = fit._curvature_options('run_experiment', curvature, float(radius))
    if repair is not None and source not in ('left', 'right'):
        raise ValueError("repair= searches the index shift of one camera's frames: source must be 'left' or 'right' "
                         "(stereo frames have match_offset= and projector['renumber'], fused ones refine=)")
    names, paths = _list_pairs(input_path)
    angles = np.deg2rad(parse_img_info(names))          # exp_gridDetection.m:26-27
    dev = torch.device(device)
    if isinstance(laser_table, (str, os.PathLike)):
        laser_table = fit.LaserTable.load(laser_table, dev)
    if projector is not None and source != 'stereo':
        raise ValueError("projector= fits the model to stereo points: source must be 'stereo'")
    if consensus is not None and multi_frame != 'consensus':
        raise ValueError("consensus= are the options of multi_frame='consensus'")
    mono_table = None if repair is None else dict(repair=dict(repair))

    def make_fits(F):
        f = pipeline.alloc_fits(F, dev, source=source, refine=refine is not None)
        if repair is not None:
            f.update({k: torch.zeros((F,) + shape, dtype=dt, device=dev) for k, (shape, dt) in pipeline.MONO_REPAIR_OUTPUTS.items()})
        if pixels is not None:
            f.update({k: torch.zeros((F,) + shape, dtype=dt, device=dev) for k, (shape, dt) in pipeline.PIXELS_OUTPUTS.items()})
        if projector is not None:        # the model needs the points' indices, which the selector returns beside the points
            f['idx'] = torch.zeros((F, fit.MAXP, 2), dtype=torch.int32, device=dev)
        if want_tables:
            cams = dict(fused=(1, 2), left=(1,), right=(2,))[source]
            f.update({k: torch.zeros((F,) + shape, dtype=dt, device=dev) for k, (shape, dt) in pipeline.tables_outputs(cams).items()})
        return f
    recs, fits = _run_pairs(names, paths, camera_json, dev, chunk, make_fits,
                            lambda h, w, c: pipeline.FramePipeline(h, w, K1, K2, T21, radius, chunk=c, device=dev, match=match_offset,
                                                                   source=source, laser_table=laser_table, refine=refine,
                                                                   table=mono_table, pixels=pixels,
                                                                   keep_tables=want_tables), source)
    F = len(names)
    tables = {k: fits.pop(k) for k in list(fits) if k.startswith('tables_')}     # (multi_frame_pixels=: not among the fits' outputs)
    # frame_ok: the device mask of the frames that are not in `skipped`; the resident multi-frame modes mask with it
    frame_ok, skipped, _ = _frame_status(names, recs, None if match_offset is None else fits['match_flags'])
    res = dict(names=names, angles=angles, records=recs, pts3=fits['pts3'], cnt=fits['m'], cyl_raw=fits['cyl_raw'], skipped=skipped,
               T_cam_agv=None, fval=None)
    if match_offset is not None:
        res.update(offset=fits['offset'], match_score=fits['match_score'], match_flags=fits['match_flags'])
    if curvature is not None:
        k, mode, rho_max, r_min, r_max = curv_opts
        curv = fit.est_curvatures_batch(fits['pts3'], fits['m'], k=k, mode=mode)
        con = fit.curvature_consensus_batch(fits['pts3'], fits['m'], curv, rho_max=rho_max, r_min=r_min, r_max=r_max)
        res['curvature'] = dict(curv, curv_status=curv['status'], **con)
    if refine is not None:
        res['refine'] = dict(round_taken=fits['round_taken'], renumbered=fits['renumbered'],
                             frames=refine_listing(names, fits['round_taken'], fits['renumbered']))
    elif source != 'stereo':
        res.update(tri_counts=fits['counts'], tri_stats=fits['stats'])
    if pixels is not None:
        res['pixels'] = dict(cyl=fits['cyl'][:, 1], T=fits['T'], fvals=fits['pixels_fvals'], px_rms=fits['pixels_stats'][:, 2],
                             counts=fits['pixels_counts'], status=fits['pixels_status'])
    if repair is not None:
        res['repair'] = dict(shift=fits['shift'], flags=fits['shift_flags'], round_taken=fits['round_taken'], renumbered=fits['renumbered'],
                             frames=repair_listing(names, fits['shift'], fits['shift_flags'], fits['round_taken'], fits['renumbered']))
    if projector is not None:
        res['projector'], res['projector_shifted'], renumbered = _fit_projector(fits, frame_ok, projector, 'col', table_path=table_path)
        if renumbered is not None:
            res['projector_renumbered'] = renumbered
        fits = {k: v for k, v in fits.items() if k != 'idx'}
    if mat_path is not None:
        api.save_mat(mat_path, fits=fits, names=names)
    if multi_frame in ('gpu', 'lm'):
        # resident: the kept frames are named by the device mask, the whole tables go in as one group, and T, fval, status and
        # the count of kept frames come back in one copy
        mf = multiframe.fit_multi_frame_gpu(fits['pts3'], fits['m'], fits['cyl_raw'], angles, radius, frame_ok=frame_ok,
                                            group_start=[0, F], method='lm' if multi_frame == 'lm' else 'nm')
        back = torch.cat([mf['T'][0], mf['fvals'][0], mf['status'][0:1].to(torch.float64),
                          frame_ok.sum().to(torch.float64).reshape(1)]).cpu().tolist()
        _take_multi_frame(res, int(back[19]), int(back[18]), 'fit', back[:16], back[17])
        mfp_kept = frame_ok
    elif multi_frame == 'consensus':
        mf = multiframe.fit_multi_frame_consensus_gpu(fits['pts3'], fits['m'], fits['cyl_raw'], angles, radius, frame_ok=frame_ok,
                                                      group_start=[0, F], **(consensus or {}))
        g = multiframe.group_result(mf)
        status, n_good = g['status'], int(frame_ok.sum())
        mfp_kept = mf['inlier'] == 1
        res['consensus'] = dict(inliers=[], rejected=[], n_inliers=g['n_inliers'], rounds=g['info'][3], flags=g['flags'], status=status)
        if _take_multi_frame(res, n_good, status, 'consensus', g['T'], g['fvals'][1]):
            res['consensus']['inliers'] = [names[i] for i in range(F) if g['inlier'][i] == 1]
            res['consensus']['rejected'] = [dict(index=i, name=names[i], rms=math.sqrt(g['frame_terms'][i]))
                                            for i in range(F) if g['inlier'][i] == 0]
            if res['consensus']['rejected']:
                warnings.warn('multi-frame consensus left out ' + ', '.join(f"{r['name']} (rms {r['rms']:.2f})"
                                                                            for r in res['consensus']['rejected']))
    elif multi_frame:
        bad = {s['index'] for s in skipped}
        good = [i for i in range(F) if i not in bad]
        if len(good) < 2:
            warnings.warn(f'{len(good)} fitted frame(s): fitCylinderWPts3sAngs needs two')
        else:
            g = torch.tensor(good, device=dev)
            mf = multiframe.fit_multi_frame(fits['pts3'][g], fits['m'][g], fits['cyl_raw'][g], angles[good], radius)
            res['T_cam_agv'], res['fval'] = mf['T'], mf['fvals'][1]
    if multi_frame_pixels is not None:
        res['multi_frame_pixels'] = None
        if res['T_cam_agv'] is not None:
            t = lambda k: tables.get(k)
            px = multiframe.fit_multi_frame_pixels_gpu(t('tables_xy1'), t('tables_id1'), t('tables_cnt1'), t('tables_xy2'), t('tables_id2'),
                                                       t('tables_cnt2'), mf['TAGV'], mf['x'][0:1], radius, K1, K2, T21, laser_table,
                                                       frame_ok=mfp_kept, group_start=[0, F], **multi_frame_pixels)
            st = int(px['status'][0])
            if st != 0:
                warnings.warn(f'the multi-frame pixel fit ended with status {st} (include/cpe.h: cpe_multi_frame_fit_pixels_batch)')
            res['multi_frame_pixels'] = dict(T_cam_agv=px['T'][0].cpu().tolist() if st == 0 else None, x=px['x'][0], fvals=px['fvals'][0],
                                             px_rms=px['stats'][0, 2], counts=px['counts'][0], status=st, cov=px['cov'][0],
                                             frame_cyl=px['frame_cyl'], frame_stats=px['frame_stats'])
    if multi_frame_joint is not None:
        res['multi_frame_joint'] = None
        if res['T_cam_agv'] is not None:
            t = lambda k: tables.get(k)
            start = mf['x'][0:1]
            if multi_frame_pixels is not None and res['multi_frame_pixels']['status'] == 0:
                start = res['multi_frame_pixels']['x'][None]
            jt = multiframe.fit_multi_frame_pixels_angles_gpu(t('tables_xy1'), t('tables_id1'), t('tables_cnt1'), t('tables_xy2'),
                                                              t('tables_id2'), t('tables_cnt2'), angles, start, radius, K1, K2, T21,
                                                              laser_table, frame_ok=mfp_kept, group_start=[0, F], **multi_frame_joint)
            st = int(jt['status'][0])
            if st != 0:
                warnings.warn(f'the joint multi-frame fit ended with status {st} (include/cpe.h: cpe_multi_frame_fit_pixels_angles_batch)')
            res['multi_frame_joint'] = dict(T_cam_agv=jt['T'][0].cpu().tolist() if st == 0 else None, x=jt['x'][0], fvals=jt['fvals'][0],
                                            px_rms=jt['stats'][0, 2], counts=jt['counts'][0], status=st, cov=jt['cov'][0],
                                            frame_cyl=jt['frame_cyl'], frame_stats=jt['frame_stats'], angles=jt['angles'],
                                            angle_sigma=jt['angle_sigma'])
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


# Laser planes of one projector meet in its centre: 0.02 mm rms on 12 analytic poses with 0.25 px noise (tests/plane_fit_cases.py).
# Fifty times that says the planes are not one projector's, i.e. the index pairing between the two images is off.
PLANE_CENTRE_RMS_WARN = 1.0     # mm


def run_plane_experiment(input_path, camera_json, K1, K2, T21, tau=0.0, max_rounds=4, min_spread=1e-4, device='cuda:0', chunk=32,
                         table_path=None, projector=None, relabel=None):
    """BUILD-DEFINED (the reference stops at the planar detector): a folder of `<name>L.png` / `<name>R.png` pairs of a flat board
    in several poses -> the board's plane and pose in every frame, and the projector's laser-plane table with its centre.

    Per pair: imread, preProcessing, the planar detector L/R, the selector, fit.fit_plane_batch (tau, max_rounds) --
    FramePipeline(target='plane').run_raw over the same read / upload loop as run_experiment.  Then one
    fit.index_planes_batch call over the good frames and their inlier masks, with lo, hi the range of the grid indices those
    frames hold (both components).

    LIMIT.  Everything behind the detector pairs the grid points of the two images by equal index.  The planar detector (a
    restatement of the reference's) is not pinned to number both images alike: on boards rendered by synth.Scene(target='plane')
    it numbers the columns of the left and the right image in opposite directions, the pairs are then not the same grid points,
    and planes, poses and table come out with status 0 and millimetres wrong.  Nothing per frame shows it (planarity cannot
    score a correspondence); the table does: laser planes of a consistent numbering meet in the
    projector's centre to hundredths of a millimetre (0.02 mm rms on 12 analytic poses with 0.25 px noise).  A table whose
    centre is refused, or whose planes miss it by more than PLANE_CENTRE_RMS_WARN = 1 mm rms, raises a UserWarning, and
    `consistent` is False: do not calibrate from such a result.  relabel= (below) lifts this on rendered boards.

    -> dict(names, records f64 [F,16] (the planar layout beside pipeline.REC), P f64 [F,4], T f64 [F,4,4], grid f64 [F,3,3],
            stats f64 [F,8], pts3 f64 [F,MAXP,3], idx i32 [F,MAXP,2], cnt i32 [F], n_inliers i32 [F], inlier_mask u8 [F,MAXP],
            plane_flags i32 [F], skipped (as run_experiment: frames whose left / right detect status or fit status is non-zero),
            table = the dict of fit.index_planes_batch (P, stats, count, frames, status [2,L,..], centre, centre_status, lo, hi)
            or None when no frame is good or the indices span more than CPE_MAXL values (a warning says which),
            laser_table = that table as a fit.LaserTable with family0='row' (the planar detector writes its ids as (row, col)), what
            FramePipeline(source='left', laser_table=...) and run_experiment(laser_table=...) read; None without a table.  It is
            saved to table_path (.npz) when that is given.  A table that is not `consistent` is returned and saved all the same,
            consistent = the table exists, has a centre, and its planes meet there within PLANE_CENTRE_RMS_WARN)

    projector: None, or a dict of fit.fit_projector_model keywords (as run_experiment's): the projector's model is fitted to the
    same points, masks and frames as well.  The dict gains projector and projector_shifted as in run_experiment (family0 'row'),
    and projector_renumbered with projector['renumber'];
    laser_table and the file at table_path are then the MODEL's table, and consistent says that the model was fitted and its
    rms is within PLANE_CENTRE_RMS_WARN.  `table` stays the free table of fit.index_planes_batch.

    relabel: None, or a dict of fit.grid_relabel_batch keywords ({} = its defaults): every image's grid lines are re-labelled
    from their geometry before the two images are paired by index (FramePipeline(relabel=...)), which is what lifts the LIMIT
    above on boards.  The dict gains relabel = dict(counts i32 [F,2,2,4] (frame, image, id component: labels seen, supported,
    phantoms, kept), flags i32 [F,2] (fit.RELABEL_*)).  It composes with projector= unchanged."""
    names, paths = _list_pairs(input_path)
    dev = torch.device(device)
    def make_fits(F):
        fits = pipeline.alloc_fits(F, dev, 'plane')
        if relabel is not None:
            fits.update({k: torch.zeros((F,) + shape, dtype=dt, device=dev) for k, (shape, dt) in pipeline.RELABEL_OUTPUTS.items()})
        return fits
    recs, fits = _run_pairs(names, paths, camera_json, dev, chunk, make_fits,
                            lambda h, w, c: pipeline.FramePipeline(h, w, K1, K2, T21, 0.0, chunk=c, device=dev, target='plane',
                                                                   plane=dict(tau=tau, max_rounds=max_rounds), relabel=relabel))
    # the index range of the points the table may use comes back with the statuses in one copy
    frame_ok, skipped, (lo, hi) = _frame_status(
        names, recs, also=lambda ok: _index_range(fits['idx'], (fits['inlier_mask'] != 0) & (ok != 0)[:, None]))
    table, consistent, laser_table = None, False, None
    if lo > hi:
        warnings.warn('no fitted frame: no laser-plane table')
    elif hi - lo + 1 > _lib.MAXL:
        warnings.warn(f'grid indices {lo}..{hi} span more than {_lib.MAXL} values: no laser-plane table')
    else:
        table = fit.index_planes_batch(fits['pts3'], fits['idx'], fits['m'], lo, hi, use=fits['inlier_mask'], frame_ok=frame_ok,
                                       min_spread=min_spread)
        c_rms, c_st = torch.cat([table['centre'][3:4], table['centre_status'].to(torch.float64)]).cpu().tolist()
        if c_st != 0:
            warnings.warn('the laser planes give no common point (fewer than 2 usable lines in a family, or planes that do not '
                          'determine a point): no projector centre')
        elif c_rms > PLANE_CENTRE_RMS_WARN:
            warnings.warn(f'the laser planes miss their common point by {c_rms:.2f} mm rms (more than {PLANE_CENTRE_RMS_WARN} mm): the '
                          'grid numbering of the two images probably disagrees, planes and table are not to be trusted')
        else:
            consistent = True
        laser_table = fit.LaserTable.from_index_planes(table, lo, hi, 'row')
        if table_path is not None and projector is None:
            laser_table.save(table_path)
    if projector is not None:
        pm, shifted, renumbered = _fit_projector(fits, frame_ok, projector, 'row', use=fits['inlier_mask'], table_path=table_path)
        consistent = pm is not None and pm['model'].status == 0 and pm['model'].rms <= PLANE_CENTRE_RMS_WARN
        if pm is not None:
            laser_table = pm['laser_table']
            if pm['model'].status == 0 and not consistent:
                warnings.warn(f'the projector model leaves {pm["model"].rms:.2f} mm rms (more than {PLANE_CENTRE_RMS_WARN} mm): the grid '
                              'numbering of the two images probably disagrees, the table is not to be trusted')
        extra = dict(projector=pm, projector_shifted=shifted)
        if renumbered is not None:
            extra['projector_renumbered'] = renumbered
    else:
        extra = {}
    if relabel is not None:
        extra['relabel'] = dict(counts=fits['relabel_counts'], flags=fits['relabel_flags'])
    return dict(**extra, **dict(names=names, records=recs, P=fits['P'], T=fits['T'], grid=fits['grid'], stats=fits['stats'], pts3=fits['pts3'],
                idx=fits['idx'], cnt=fits['m'], n_inliers=fits['n_inliers'], inlier_mask=fits['inlier_mask'],
                plane_flags=fits['plane_flags'], skipped=skipped, table=table, consistent=consistent,
                laser_table=laser_table))
