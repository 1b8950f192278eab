"""Whole hot path for a batch of stereo frames, resident on one GPU:
    left/right u8 [F,h,w]  ->  detect_grid (both images)  ->  fitSingleCylinder  ->  pose records [F,16] f64

This is the loop body of exp_gridDetection.m:55-81 (makePyGridPts L/R, then fitSingleCylinder per frame)
turned into batched kernel launches; frames are processed in chunks so that the detect workspace stays
bounded (about 170 MB per 1920x1200 image: DESIGN.md section 3)."""
from collections import namedtuple

import torch

from . import api, fit

REC = 16   # f64 per frame: cyl0[6] | cyl[6] (both after applyCylParamsPrior) | f0 f | meanError | packed counters
# target='plane' (build-defined), the same 16 doubles:
#   0:4 P = [n, P4] | 4:7 origin | 7:10 x-axis (both of the pose T) | 10 |U| | 11 |V| (grid pitch on the board along either index) |
#   12 plane rms | 13 max |r| | 14 meanError | 15 pack_counters(m, refits, status, st_l, st_r)


def pack_counters(n_pts, iters, fit_status, det_l, det_r):
    """n_pts (<4096), iterations (<2^20), statuses -> one exactly representable double"""
    code = n_pts.to(torch.int64) + 4096 * (iters.to(torch.int64) + (1 << 20) * (fit_status.to(torch.int64) * 64 +
                                                                                 det_l.to(torch.int64) * 8 + det_r.to(torch.int64)))
    return code.to(torch.float64)


def unpack_counters(code):
    code = code.to(torch.int64)
    n_pts = code % 4096
    rest = code // 4096
    iters = rest % (1 << 20)
    st = rest // (1 << 20)
    return n_pts, iters, st // 64, (st // 8) % 8, st % 8


# ---- the per-frame outputs run_raw can keep: name -> (shape, dtype), the common core plus what each fit adds ----
_F64, _I32 = torch.float64, torch.int32
_POINTS = dict(pts3=((fit.MAXP, 3), _F64), idx=((fit.MAXP, 2), _I32), m=((), _I32))
_CYL = dict(cyl_raw=((2, 6), _F64), cyl=((2, 6), _F64), T=((4, 4), _F64), fvals=((2,), _F64), mean_err=((), _F64), status=((), _I32))


def _tri(counts, res, src, stats):
    """what the two table triangulations add per frame, by their widths"""
    return dict(counts=((counts,), _I32), res=((fit.MAXP, res), _F64), src=((fit.MAXP, src), _I32), stats=((stats,), _F64))


# fit.fit_single_cylinder_batch (the selector's idx is not kept)
FIT_OUTPUTS = dict({k: v for k, v in _POINTS.items() if k != 'idx'}, **_CYL, offset=((2,), _I32), match_score=((4,), _I32),
                   match_flags=((), _I32))
PLANE_FIT_OUTPUTS = dict(_POINTS, P=((4,), _F64), T=((4, 4), _F64), grid=((3, 3), _F64), stats=((8,), _F64), n_inliers=((), _I32),
                         inlier_mask=((fit.MAXP,), torch.uint8), plane_flags=((), _I32), mean_err=((), _F64), status=((), _I32))
# what fit.fit_single_plane_batch adds with relabel= (per frame and image); FramePipeline(relabel=...).run_raw keeps them when the
# fits dict holds tensors of these names
RELABEL_OUTPUTS = dict(relabel_counts=((2, 2, 4), _I32), relabel_flags=((2,), _I32))
MONO_FIT_OUTPUTS = dict(_POINTS, **_CYL, **_tri(4, 2, 2, 2))
FUSED_FIT_OUTPUTS = dict(_POINTS, **_CYL, **_tri(6, 4, 3, 4), flags=((), _I32))
# what fit.fit_single_cylinder_refined_batch returns per frame (FramePipeline(source='fused', refine=...))
REFINED_FIT_OUTPUTS = dict(_POINTS, **_CYL, round_taken=((), _I32), renumbered=((2,), _I32))
# what fit.fit_single_cylinder_mono_repaired_batch adds per frame; FramePipeline(source='left' / 'right', table=dict(repair=...))
# .run_raw keeps them when the fits dict holds tensors of these names
MONO_REPAIR_OUTPUTS = dict(shift=((2,), _I32), shift_flags=((), _I32), shift_score=((4,), _I32), round_taken=((), _I32),
                           renumbered=((), _I32))
# what fit.polish_with_pixels adds per frame; FramePipeline(pixels=...).run_raw keeps them when the fits dict holds tensors of
# these names
# the grid tables of camera c = 1, 2 that FramePipeline(keep_tables=True) adds to the fit's dict (a one-camera source: that camera's)
def tables_outputs(cameras=(1, 2)):
    return {f'tables_{k}{c}': v for c in cameras for k, v in (('xy', ((fit.MAXP, 2), _F64)), ('id', ((fit.MAXP, 2), _I32)), ('cnt', ((), _I32)))}


PIXELS_OUTPUTS = dict(pixels_taken=((), torch.bool), pixels_fvals=((2,), _F64), pixels_stats=((4,), _F64), pixels_counts=((4,), _I32),
                      pixels_status=((), _I32))


# ---- the two record layouts (beside REC) ----
def _cylinder_record(out, st_l, st_r):
    """the REC layout; word 14 is out['mean_err'] in the fit's own unit (pixels; mm off the laser planes for one camera).
    Without a fit (stage 'detect': BASELINE configs[1]) the fit's words are zero"""
    m = out['m']
    if 'cyl' in out:
        rec = torch.empty((m.shape[0], REC), dtype=torch.float64, device=m.device)
        rec[:, 0:6] = out['cyl'][:, 0]
        rec[:, 6:12] = out['cyl'][:, 1]
        rec[:, 12:14] = out['fvals']
        iters, status = out['iters'][:, 0], out['status']
    else:
        rec = torch.zeros((m.shape[0], REC), dtype=torch.float64, device=m.device)
        iters = status = torch.zeros_like(m)
    rec[:, 14] = out['mean_err']
    rec[:, 15] = pack_counters(m, iters, status, st_l, st_r)
    return rec


def _plane_record(out, st_l, st_r):
    rec = torch.empty((out['m'].shape[0], REC), dtype=torch.float64, device=out['m'].device)
    rec[:, 0:4] = out['P']
    rec[:, 4:7] = out['T'][:, :3, 3]
    rec[:, 7:10] = out['T'][:, :3, 0]
    rec[:, 10:12] = out['grid'][:, 1:3].norm(dim=2)
    rec[:, 12:14] = out['stats'][:, 0:2]
    rec[:, 14] = out['mean_err']
    rec[:, 15] = pack_counters(out['m'], out['stats'][:, 6], out['status'], st_l, st_r)
    return rec


# ---- tables -> fit dict, one per mode: (pipeline, g1, g2, the two images' centres, the chunk's first frame) ----
def _ransac(p, frame0):
    return None if p.ransac is None else dict(p.ransac, frame0=int(p.ransac.get('frame0', 0)) + frame0)


def _fit_stereo(p, g1, g2, ctr, frame0):
    return fit.fit_single_cylinder_batch(g1, g2, p.K1, p.K2, p.T21, p.radius, p.selector, 3, p.th, ransac=_ransac(p, frame0),
                                         match=p.match, mode=p.fit_mode)


def _fit_detect(p, g1, g2, ctr, frame0):
    return fit.select_triangulate_batch(g1, g2, p.K1, p.K2, p.T21, p.selector, 3, p.th)


def _fit_plane(p, g1, g2, ctr, frame0):
    rl = {} if p.relabel is None else dict(relabel=p.relabel, center1=ctr[0], center2=ctr[1])
    return fit.fit_single_plane_batch(g1, g2, p.K1, p.K2, p.T21, p.selector, 3, p.th, **p.plane, **rl)


def _fit_mono(p, g1, g2, ctr, frame0):
    g, K, Tc = (g1, p.K1, None) if g2 is None else (g2, p.K2, p.T21)
    table = dict(p.table)
    repair = table.pop('repair', None)
    if repair is None:
        return fit.fit_single_cylinder_mono_batch(g, K, Tc, p.laser_table, p.radius, ransac=_ransac(p, frame0), mode=p.fit_mode, **table)
    # repair (build-defined, opt-in): keywords of fit.fit_single_cylinder_mono_repaired_batch ({} = its defaults with shift={}, the
    # search on; image_size: the frame's unless given).  The table's other keywords go with them: max_res is one of that call's
    if p.ransac is not None:
        raise ValueError("table=dict(repair=...): every candidate and round is fitted with fit_cylinder_batch, ransac does not apply")
    kw = dict(dict(shift={}, image_size=(p.h, p.w), mode=p.fit_mode), **table)
    kw.update(repair)
    return fit.fit_single_cylinder_mono_repaired_batch(g, 1 if g2 is None else 2, p.K1, p.K2, p.T21, p.laser_table, p.radius, **kw)


def _fit_fused(p, g1, g2, ctr, frame0):
    return fit.fit_single_cylinder_fused_batch(g1, g2, p.K1, p.K2, p.T21, p.laser_table, p.radius, ransac=_ransac(p, frame0),
                                               mode=p.fit_mode, **p.table)


def _fit_refined(p, g1, g2, ctr, frame0):
    return fit.fit_single_cylinder_refined_batch(g1, g2, p.K1, p.K2, p.T21, p.laser_table, p.radius,
                                                 **dict(dict(fused=p.table, mode=p.fit_mode), **p.refine))


# ---- every combination of options FramePipeline runs: which cameras' images are detected ('LR', 'L', 'R'), tables -> fit dict,
#      the record writer, the outputs run_raw can keep (None: none) ----
_Mode = namedtuple('_Mode', 'cameras fit record outputs')
_MODES = {
    'stereo cylinder': _Mode('LR', _fit_stereo, _cylinder_record, FIT_OUTPUTS),
    'stereo detect-only': _Mode('LR', _fit_detect, _cylinder_record, None),
    'stereo plane': _Mode('LR', _fit_plane, _plane_record, PLANE_FIT_OUTPUTS),
    'mono left': _Mode('L', _fit_mono, _cylinder_record, MONO_FIT_OUTPUTS),
    'mono right': _Mode('R', _fit_mono, _cylinder_record, MONO_FIT_OUTPUTS),
    'fused': _Mode('LR', _fit_fused, _cylinder_record, FUSED_FIT_OUTPUTS),
    'fused refined': _Mode('LR', _fit_refined, _cylinder_record, REFINED_FIT_OUTPUTS),
}


def _mode_name(target='cylinder', source='stereo', stage='full', refine=False):
    """the key of _MODES for options that FramePipeline's constructor has let through"""
    if source == 'fused':
        return 'fused refined' if refine else 'fused'
    if source != 'stereo':
        return 'mono right' if source == 'right' else 'mono left'
    return 'stereo detect-only' if stage == 'detect' else 'stereo ' + target


def _split_detect(det, cameras, interleaved=False):
    """the detect call's dict -> (g1, g2, st_l, st_r, (centre1, centre2)) of the left and the right images.  cameras 'LR': the
    images lie interleaved (L0 R0 L1 R1 ...; the tables are copied out) or concatenated (all left, then all right; views);
    'L' / 'R': they are that camera's alone, the other one's tables are None and its status words zero"""
    n = det['n'].shape[0]
    if cameras == 'LR':
        sl = (slice(0, None, 2), slice(1, None, 2)) if interleaved else (slice(None, n // 2), slice(n // 2, None))
    else:
        sl = (slice(None), None) if cameras == 'L' else (None, slice(None))

    def camera(s):
        if s is None:
            return None, torch.zeros_like(det['status']), None
        return fit.GridTables(*(det[k][s].contiguous() for k in ('xy', 'id', 'n'))), det['status'][s], det['center'][s].contiguous()
    (g1, st_l, c1), (g2, st_r, c2) = camera(sl[0]), camera(sl[1])
    return g1, g2, st_l, st_r, (c1, c2)


class FramePipeline:
    """reusable workspaces for chunks of `chunk` stereo frames of size h x w; the options resolve to one row of _MODES"""

    def __init__(self, h, w, K1, K2, T21, radius, chunk=64, device='cuda:0', selector=fit.SEL_CHOOSE_IDX, th=0.3,
                 fit_mode=fit.FIT_NELDER_MEAD, lanes=1, ransac=None, stage='full', match=None, target='cylinder', plane=None,
                 source='stereo', laser_table=None, table=None, relabel=None, refine=None, pixels=None, keep_tables=False):
        # ---- which combinations exist: the rows of _MODES; everything else is refused here ----
        if stage not in ('full', 'detect'):
            raise ValueError("stage is 'full' or 'detect'")
        if target not in ('cylinder', 'plane'):
            raise ValueError("target is 'cylinder' or 'plane'")
        if target == 'plane' and (match is not None or ransac is not None):
            raise ValueError("target='plane': match and ransac score with the cylinder's radius and do not apply (radius is not read)")
        if target != 'plane' and plane is not None:
            raise ValueError("plane= holds keywords of the planar fit: target='plane' only")
        if relabel is not None and target != 'plane':
            raise ValueError("relabel= re-labels straight grid lines: target='plane' only (the cylinder's lines are curved, and "
                             "the cylinder script numbers them differently)")
        if source not in ('stereo', 'left', 'right', 'fused'):
            raise ValueError("source is 'stereo', 'left', 'right' or 'fused'")
        if source == 'stereo' and (laser_table is not None or table is not None):
            raise ValueError("laser_table= and table= belong to one camera: source='left' or 'right'")
        if source != 'stereo':
            if laser_table is None:
                raise ValueError(f"source='{source}' needs laser_table= (a fit.LaserTable)" +
                                 ('' if source == 'fused' else ': one camera has no other way to a 3-D point'))
            if match is not None:
                raise ValueError(f"source='{source}': match searches the index shift between two tables, there is one" if source != 'fused'
                                 else "source='fused': match feeds the stereo selector; repair the numbering first (fit.match_offset_batch)")
            if target == 'plane':
                raise ValueError(f"source='{source}': target='plane' builds the table from stereo points and does not read one")
            if stage == 'detect':
                raise ValueError(f"source='{source}': stage='detect' ends at the stereo selector")
        if refine is not None:
            if source != 'fused':
                raise ValueError("refine= re-numbers against the laser-plane table and fits fused points: source='fused' only")
            if target == 'plane':
                raise ValueError("refine= predicts the grid on a cylinder: target='cylinder' only")
            if ransac is not None:
                raise ValueError('refine= fits every round with fit_cylinder_batch: ransac does not apply')
            nodes = (laser_table.hi - laser_table.lo + 1) ** 2
            if refine.get('window') is None and nodes > fit.PRED_MAXN:
                raise ValueError(f'refine=: the table holds {nodes} nodes, more than {fit.PRED_MAXN}: give window=')
            refine = dict(dict(image_size=(h, w), first=dict(selector=selector, th=th, mode=fit_mode)), **refine)
        if pixels is not None:
            if target == 'plane':
                raise ValueError("pixels= fits a cylinder's pose to the pixels: target='cylinder' only")
            if source == 'stereo':
                raise ValueError("pixels= predicts the pixels from the laser-plane table: source='fused', 'left' or 'right' with "
                                 "laser_table=")
            fit._pixels_options('FramePipeline', pixels)
        self.mode = _mode_name(target, source, stage, refine is not None)     # a key of _MODES
        self.h, self.w, self.chunk, self.device = h, w, chunk, torch.device(device)
        self.K1, self.K2, self.T21, self.radius = K1, K2, T21, radius
        self.selector, self.th, self.fit_mode = selector, th, fit_mode
        self.stage = stage              # 'detect': stop after chooseIdx + triangulate (fitSingleCylinder.m:12-17), no cylinder fit
        self.target = target            # 'plane' (build-defined): the planar detector and fit.fit_single_plane_batch; records as beside REC
        # source (build-defined beyond 'stereo'): 'left' / 'right': only that camera's images are detected, and the points come from
        # its rays and the laser-plane table (fit.fit_single_cylinder_mono_batch); camera 2 uses K2 and T21.  'fused': both are
        # detected as for 'stereo', and every grid point of either table becomes a 3-D point from its rays and the laser planes in
        # one solve (fit.fit_single_cylinder_fused_batch); no selector
        self.source, self.laser_table = source, None if laser_table is None else laser_table.to(self.device)
        self.ransac = ransac            # None, or keywords of fit.fit_cylinder_ransac_batch (build-defined config 5)
        self.match = match              # None, or keywords of fit.match_offset_batch (build-defined: the index-shift search, stage 'full')
        self.plane = dict(plane or {})  # keywords of fit.fit_plane_batch: tau, max_rounds
        # relabel (build-defined): None, or keywords of fit.grid_relabel_batch ({} = its defaults): both images' tables are
        # re-labelled from the lines' geometry and the detect call's centres before the selector pairs them by index
        self.relabel = None if relabel is None else dict(relabel)
        # keywords of fit.table_triangulate_batch: need_both, min_sin, max_res; source 'fused': of fit.fused_triangulate_batch.
        # source 'left' / 'right' also reads repair= here (build-defined, opt-in): None, or a dict of
        # fit.fit_single_cylinder_mono_repaired_batch keywords ({} = the index-shift search and one re-numbering round)
        self.table = dict(table or {})
        # refine (build-defined, opt-in): None, or keywords of fit.fit_single_cylinder_refined_batch ({} = its defaults: rounds,
        # first, tau_px, ratio, window, min_cos, image_size -- the frame's size unless given): the stereo fit first, then every
        # grid point re-numbered against the grid that fit predicts and the fit again on fused points
        self.refine = refine
        # pixels (build-defined, opt-in): None, or keywords of fit.fit_cylinder_pixels_batch ({} = its defaults): a step AFTER the
        # mode's fit, no mode of its own: the fit's pose is polished on the pixels of the tables it was made from
        # (fit.polish_with_pixels); the records then hold the polished cyl, every other word stays the 3-D fit's
        self.pixels = None if pixels is None else dict(pixels)
        # keep_tables (opt-in): the fit's dict also holds the grid tables the fit was made from (after refine= / repair=), flat as
        # tables_outputs() names them, so that run_raw can keep them beside the fits (experiment.run_experiment(multi_frame_pixels=))
        self.keep_tables = bool(keep_tables)
        self.ws = {}
        # chunks are independent: `lanes` of them are in flight on their own HIP streams (each with its own
        # workspace), so the serial tails of one chunk (blob grouping, line fitting: one workgroup per frame)
        # run beside the wide kernels of the next
        self.lanes = max(1, int(lanes))
        self._streams = None
        self._stage = {}                # lane -> u8 [chunk,2,h,w]: where run_raw's pre-step writes the pairs of a chunk

    def _ws(self, n_img, lane=0):
        """one workspace per lane, made for the first (largest) chunk it sees; smaller chunks are laid out inside it"""
        ws = self.ws.get(lane)
        if ws is None or not ws.fits(n_img, self.h, self.w):
            ws = self.ws[lane] = api.DetectWorkspace(n_img, self.h, self.w, self.device)
        return ws.use(n_img)

    @staticmethod
    def _interleaved(left, right):
        """left = S[:, 0], right = S[:, 1] of one contiguous stereo tensor S [F,2,h,w] (frame-major pairs)?"""
        h, w = left.shape[1:]
        return (left.dim() == 3 and left.shape == right.shape and left.stride() == (2 * h * w, w, 1) and right.stride() == left.stride()
                and right.data_ptr() == left.data_ptr() + h * w and left.untyped_storage().data_ptr() == right.untyped_storage().data_ptr())

    def run_chunk(self, left, right, lane=0, frame0=0):
        """-> records f64 [c,16], the detect call's dict, the fit's dict.  With source 'left' / 'right' only that argument is
        read (the other may be None) and the detect call sees c images, not 2c"""
        mode = _MODES[self.mode]
        interleaved = mode.cameras == 'LR' and left.shape[0] > 0 and self._interleaved(left, right)
        if mode.cameras != 'LR':
            frames = (left if mode.cameras == 'L' else right).contiguous()
        elif interleaved:
            # the pairs already lie one after the other in memory: the detect call reads them in place (L0 R0 L1 R1 ...)
            frames = torch.as_strided(left, (2 * left.shape[0], self.h, self.w), (self.h * self.w, self.w, 1))
        else:
            frames = torch.cat([left, right])             # [2c,h,w]: one detect call for both cameras (a copy)
        det = api.detect_grid_batch(frames, self._ws(frames.shape[0], lane), target=self.target, debug_planes=False)   # only the tables are read
        g1, g2, st_l, st_r, centres = _split_detect(det, mode.cameras, interleaved)
        out = mode.fit(self, g1, g2, centres, frame0)
        if self.pixels is not None:
            if mode.cameras == 'LR':
                out = fit.polish_with_pixels(out, out.get('tables1', g1), out.get('tables2', g2), self.K1, self.K2, self.T21, self.laser_table,
                                             self.radius, self.pixels)
            else:
                K, Tc = (self.K1, None) if g2 is None else (self.K2, self.T21)
                out = fit.polish_mono_with_pixels(out, out.get('tables', g1 if g2 is None else g2), K, Tc, self.laser_table, self.radius,
                                                  self.pixels)
        if self.keep_tables:
            if mode.cameras == 'LR':
                kept = (out.get('tables1', g1), out.get('tables2', g2))
            else:
                one = out.get('tables', g1 if g2 is None else g2)
                kept = (one, None) if g2 is None else (None, one)
            out = dict(out)
            for c, t in zip((1, 2), kept):
                if t is not None:
                    out.update({f'tables_xy{c}': t.xy, f'tables_id{c}': t.id, f'tables_cnt{c}': t.cnt})
        return mode.record(out, st_l, st_r), det, out

    def run(self, left, right):
        """left/right: u8 [F,h,w] on the device -> records f64 [F,16] (source 'left' / 'right': the other one may be None)"""
        one = right if _MODES[self.mode].cameras == 'R' else left
        part = lambda t, i0, i1: None if t is None else t[i0:i1]
        return self._for_chunks(one.shape[0], one.device,
                                lambda i0, i1, lane: self.run_chunk(part(left, i0, i1), part(right, i0, i1), lane, i0)[0])

    def _for_chunks(self, F, device, body):
        """the walk over the chunks that run and run_raw share: records f64 [F,16] of body(i0, i1, lane); with lanes > 1
        every chunk runs on its lane's stream"""
        recs = torch.empty((F, REC), dtype=torch.float64, device=device)
        n_chunks = (F + self.chunk - 1) // self.chunk
        if self.lanes == 1 or n_chunks == 1 or device.type != 'cuda':
            for i0 in range(0, F, self.chunk):
                i1 = min(F, i0 + self.chunk)
                recs[i0:i1] = body(i0, i1, 0)
            return recs
        if self._streams is None:
            self._streams = [torch.cuda.Stream(device=device) for _ in range(self.lanes)]
        main = torch.cuda.current_stream(device)
        for st in self._streams:
            st.wait_stream(main)                          # inputs and `recs` are ready on the caller's stream
        for k, i0 in enumerate(range(0, F, self.chunk)):
            i1 = min(F, i0 + self.chunk)
            lane = k % self.lanes
            with torch.cuda.stream(self._streams[lane]):
                recs[i0:i1] = body(i0, i1, lane)
        for st in self._streams:
            main.wait_stream(st)
        return recs

    def run_raw(self, left_raw, right_raw, prestep, fits=None):
        """raw camera frames [F,h,w] / [F,h,w,3] on the device (uint8, uint16, float32, float64: iotool.StereoPrestep) ->
        records f64 [F,16].  Per chunk the pre-step (preProcessing.m:3-9) writes the undistorted grey pairs into the lane's
        staging tensor [chunk,2,h,w] and the detect call reads them there in place.
        fits: None, or tensors from alloc_fits(F, device[, target, source]) that receive every frame's fit outputs.
        With source 'left' / 'right' only that camera's frames are read (the other argument may be None) and pre-processed, into
        a staging tensor [chunk,h,w]."""
        if (prestep.h, prestep.w) != (self.h, self.w):
            raise ValueError(f'run_raw: the pre-step is for {prestep.w}x{prestep.h} frames, the pipeline for {self.w}x{self.h}')
        if fits is not None and self.stage != 'full':
            raise ValueError("run_raw: fit outputs exist only with stage='full'")
        from . import iotool
        cameras = _MODES[self.mode].cameras
        one = right_raw if cameras == 'R' else left_raw

        def body(i0, i1, lane):
            st = self._stage.get(lane)
            if st is None:
                shape = (self.chunk, 2, self.h, self.w) if cameras == 'LR' else (self.chunk, self.h, self.w)
                st = self._stage[lane] = torch.empty(shape, dtype=torch.uint8, device=one.device)
            st = st[:i1 - i0]
            if cameras == 'LR':
                prestep(left_raw[i0:i1], right_raw[i0:i1], out=st)
                rec, _, out = self.run_chunk(st[:, 0], st[:, 1], lane, i0)
            else:
                prestep._check(one[i0:i1], self.source)
                iotool._prestep(prestep.maps[int(cameras == 'R')], one[i0:i1], st, self.h * self.w)
                rec, _, out = self.run_chunk(st, st, lane, i0)
            if fits is not None:
                for k, t in fits.items():
                    t[i0:i1] = out[k]
            return rec
        return self._for_chunks(one.shape[0], one.device, body)


def alloc_fits(F, device, target='cylinder', source='stereo', refine=False):
    """zeroed [F, ...] tensors for the per-frame outputs of fit.fit_single_cylinder_batch (target='plane': of
    fit.fit_single_plane_batch; source 'left' / 'right': of fit.fit_single_cylinder_mono_batch; source 'fused': of
    fit.fit_single_cylinder_fused_batch, with refine of fit.fit_single_cylinder_refined_batch) that FramePipeline.run_raw can keep"""
    outputs = _MODES[_mode_name(target, source, 'full', refine)].outputs
    return {k: torch.zeros((F,) + shape, dtype=dt, device=device) for k, (shape, dt) in outputs.items()}
