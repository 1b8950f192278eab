"""Whole hot path for a batch of stereo frames, resident on one GPU:
    left/right u8 [F,h,w]  ->  detect_grid (both images)  ->  fitSingleCylinder  ->  pose records [F,16] f64

This is the loop body of exp_gridDetection.m:55-81 (makePyGridPts L/R, then fitSingleCylinder per frame)
turned into batched kernel launches; frames are processed in chunks so that the detect workspace stays
bounded (about 170 MB per 1920x1200 image: DESIGN.md section 3)."""
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


class FramePipeline:
    """reusable workspaces for chunks of `chunk` stereo frames of size h x w"""

    def __init__(self, h, w, K1, K2, T21, radius, chunk=64, device='cuda:0', selector=fit.SEL_CHOOSE_IDX, th=0.3,
                 fit_mode=fit.FIT_NELDER_MEAD, lanes=1, ransac=None, stage='full', match=None, target='cylinder', plane=None,
                 source='stereo', laser_table=None, table=None, relabel=None, refine=None):
        self.h, self.w, self.chunk, self.device = h, w, chunk, torch.device(device)
        self.K1, self.K2, self.T21, self.radius = K1, K2, T21, radius
        self.selector, self.th, self.fit_mode = selector, th, fit_mode
        self.ransac = ransac            # None, or keywords of fit.fit_cylinder_ransac_batch (build-defined config 5)
        self.match = match              # None, or keywords of fit.match_offset_batch (build-defined: the index-shift search, stage 'full')
        if stage not in ('full', 'detect'):
            raise ValueError("stage is 'full' or 'detect'")
        if target not in ('cylinder', 'plane'):
            raise ValueError("target is 'cylinder' or 'plane'")
        if target == 'plane' and (match is not None or ransac is not None):
            raise ValueError("target='plane': match and ransac score with the cylinder's radius and do not apply (radius is not read)")
        if target != 'plane' and plane is not None:
            raise ValueError("plane= holds keywords of the planar fit: target='plane' only")
        self.target = target            # 'plane' (build-defined): the planar detector and fit.fit_single_plane_batch; records as beside REC
        self.plane = dict(plane or {})  # keywords of fit.fit_plane_batch: tau, max_rounds
        # relabel (build-defined): None, or keywords of fit.grid_relabel_batch ({} = its defaults): both images' tables are
        # re-labelled from the lines' geometry and the detect call's centres before the selector pairs them by index
        if relabel is not None and target != 'plane':
            raise ValueError("relabel= re-labels straight grid lines: target='plane' only (the cylinder's lines are curved, and "
                             "the cylinder script numbers them differently)")
        self.relabel = None if relabel is None else dict(relabel)
        self.stage = stage              # 'detect': stop after chooseIdx + triangulate (fitSingleCylinder.m:12-17), no cylinder fit
        # source 'left' / 'right' (build-defined): only that camera's images are detected, and the points come from its rays and the
        # laser-plane table (fit.fit_single_cylinder_mono_batch) instead of the stereo pair; camera 2 uses K2 and T21
        # source 'fused' (build-defined): both cameras' images are detected as for 'stereo', and every grid point of either table
        # becomes a 3-D point from its rays and the laser planes in one solve (fit.fit_single_cylinder_fused_batch); no selector
        if source not in ('stereo', 'left', 'right', 'fused'):
            raise ValueError("source is 'stereo', 'left', 'right' or 'fused'")
        if source == 'stereo':
            if laser_table is not None or table is not None:
                raise ValueError("laser_table= and table= belong to one camera: source='left' or 'right'")
        else:
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
            laser_table = laser_table.to(self.device)
        self.source, self.laser_table = source, laser_table
        # keywords of fit.table_triangulate_batch: need_both, min_sin, max_res; source 'fused': of fit.fused_triangulate_batch
        self.table = dict(table or {})
        # refine (build-defined, opt-in; source 'fused' only): None, or keywords of fit.fit_single_cylinder_refined_batch ({} = its
        # defaults: rounds, first, tau_px, ratio, window, min_cos, image_size -- the frame's size unless given): the stereo fit
        # first, then every grid point re-numbered against the grid that fit predicts and the fit again on fused points
        if refine is not None:
            if source != 'fused':
                raise ValueError("refine= re-numbers against the laser-plane table and fits fused points: source='fused' only")
            if target == 'plane':
                raise ValueError("refine= predicts the grid on a cylinder: target='cylinder' only")
            if ransac is not None:
                raise ValueError('refine= fits every round with fit_cylinder_batch: ransac does not apply')
            refine = dict(refine)
            refine.setdefault('image_size', (h, w))
            refine.setdefault('first', dict(selector=selector, th=th, mode=fit_mode))
            nodes = (laser_table.hi - laser_table.lo + 1) ** 2
            if refine.get('window') is None and nodes > fit.PRED_MAXN:
                raise ValueError(f'refine=: the table holds {nodes} nodes, more than {fit.PRED_MAXN}: give window=')
        self.refine = refine
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

    def _run_chunk_mono(self, frames, lane, frame0):
        """run_chunk with source 'left' / 'right': one detect call over the c images of that camera"""
        c = frames.shape[0]
        det = api.detect_grid_batch(frames.contiguous(), self._ws(c, lane), target=self.target, debug_planes=False)
        K, Tc = (self.K1, None) if self.source == 'left' else (self.K2, self.T21)
        rk = None if self.ransac is None else dict(self.ransac, frame0=int(self.ransac.get('frame0', 0)) + frame0)
        out = fit.fit_single_cylinder_mono_batch(fit.GridTables(det['xy'], det['id'], det['n']), K, Tc, self.laser_table, self.radius,
                                                 ransac=rk, mode=self.fit_mode, **self.table)
        zero = torch.zeros_like(det['status'])
        st_l, st_r = (det['status'], zero) if self.source == 'left' else (zero, det['status'])
        rec = torch.empty((c, REC), dtype=torch.float64, device=frames.device)
        rec[:, 0:6] = out['cyl'][:, 0]
        rec[:, 6:12] = out['cyl'][:, 1]
        rec[:, 12:14] = out['fvals']
        rec[:, 14] = out['mean_err']          # mm off the laser planes, not pixels (fit.fit_single_cylinder_mono_batch)
        rec[:, 15] = pack_counters(out['m'], out['iters'][:, 0], out['status'], st_l, st_r)
        return rec, det, out

    def run_chunk(self, left, right, lane=0, frame0=0):
        """-> records f64 [c,16], the detect call's dict, the fit's dict.  With source 'left' / 'right' only that argument is
        read (the other may be None) and the detect call sees c images, not 2c"""
        if self.source in ('left', 'right'):
            return self._run_chunk_mono(left if self.source == 'left' else right, lane, frame0)
        c = left.shape[0]
        if c > 0 and self._interleaved(left, right):
            # the pairs already lie one after the other in memory: the detect call reads them in place (L0 R0 L1 R1 ...)
            frames = torch.as_strided(left, (2 * c, self.h, self.w), (self.h * self.w, self.w, 1))
            det = api.detect_grid_batch(frames, self._ws(2 * c, lane), target=self.target, debug_planes=False)   # only the tables are read
            sl = lambda k, o: det[k][o::2].contiguous()
            g1 = fit.GridTables(sl('xy', 0), sl('id', 0), sl('n', 0))
            g2 = fit.GridTables(sl('xy', 1), sl('id', 1), sl('n', 1))
            st_l, st_r = det['status'][0::2], det['status'][1::2]
            ctr = (sl('center', 0), sl('center', 1))
        else:
            frames = torch.cat([left, right])             # [2c,h,w]: one detect call for both cameras (a copy)
            det = api.detect_grid_batch(frames, self._ws(2 * c, lane), target=self.target, debug_planes=False)   # only the tables are read
            g1 = fit.GridTables(det['xy'][:c], det['id'][:c], det['n'][:c])
            g2 = fit.GridTables(det['xy'][c:], det['id'][c:], det['n'][c:])
            st_l, st_r = det['status'][:c], det['status'][c:]
            ctr = (det['center'][:c], det['center'][c:])
        if self.source == 'fused':
            rk = None if self.ransac is None else dict(self.ransac, frame0=int(self.ransac.get('frame0', 0)) + frame0)
            if self.refine is not None:
                out = fit.fit_single_cylinder_refined_batch(g1, g2, self.K1, self.K2, self.T21, self.laser_table, self.radius,
                                                            **dict(dict(fused=self.table, mode=self.fit_mode), **self.refine))
            else:
                out = fit.fit_single_cylinder_fused_batch(g1, g2, self.K1, self.K2, self.T21, self.laser_table, self.radius, ransac=rk,
                                                          mode=self.fit_mode, **self.table)
            rec = torch.empty((c, REC), dtype=torch.float64, device=frames.device)
            rec[:, 0:6] = out['cyl'][:, 0]
            rec[:, 6:12] = out['cyl'][:, 1]
            rec[:, 12:14] = out['fvals']
            rec[:, 14] = out['mean_err']          # rms ray residual of the pairs in pixels (fit.fit_single_cylinder_fused_batch)
            rec[:, 15] = pack_counters(out['m'], out['iters'][:, 0], out['status'], st_l, st_r)
            return rec, det, out
        if self.stage == 'detect':      # BASELINE configs[1]: grid detection + triangulation only
            out = fit.select_triangulate_batch(g1, g2, self.K1, self.K2, self.T21, self.selector, 3, self.th)
            rec = torch.zeros((c, REC), dtype=torch.float64, device=frames.device)
            rec[:, 14] = out['mean_err']
            zero = torch.zeros_like(out['m'])
            rec[:, 15] = pack_counters(out['m'], zero, zero, st_l, st_r)
            return rec, det, out
        if self.target == 'plane':
            rl = {} if self.relabel is None else dict(relabel=self.relabel, center1=ctr[0], center2=ctr[1])
            out = fit.fit_single_plane_batch(g1, g2, self.K1, self.K2, self.T21, self.selector, 3, self.th, **self.plane, **rl)
            rec = torch.empty((c, REC), dtype=torch.float64, device=frames.device)
            rec[:, 0:4] = out['P']
            rec[:, 4:7] = out['T'][:, :3, 3]
            rec[:, 7:10] = out['T'][:, :3, 0]
            rec[:, 10:12] = out['grid'][:, 1:3].norm(dim=2)
            rec[:, 12:14] = out['stats'][:, 0:2]
            rec[:, 14] = out['mean_err']
            rec[:, 15] = pack_counters(out['m'], out['stats'][:, 6], out['status'], st_l, st_r)
            return rec, det, out
        rk = None if self.ransac is None else dict(self.ransac, frame0=int(self.ransac.get('frame0', 0)) + frame0)
        out = fit.fit_single_cylinder_batch(g1, g2, self.K1, self.K2, self.T21, self.radius, self.selector, 3, self.th,
                                            ransac=rk, match=self.match, mode=self.fit_mode)
        rec = torch.empty((c, REC), dtype=torch.float64, device=frames.device)
        rec[:, 0:6] = out['cyl'][:, 0]
        rec[:, 6:12] = out['cyl'][:, 1]
        rec[:, 12:14] = out['fvals']
        rec[:, 14] = out['mean_err']
        rec[:, 15] = pack_counters(out['m'], out['iters'][:, 0], out['status'], st_l, st_r)
        return rec, det, out

    def run(self, left, right):
        """left/right: u8 [F,h,w] on the device -> records f64 [F,16] (source 'left' / 'right': the other one may be None)"""
        if self.source in ('left', 'right'):
            one = left if self.source == 'left' else right
            return self._for_chunks(one.shape[0], one.device, lambda i0, i1, lane: self._run_chunk_mono(one[i0:i1], lane, i0)[0])
        return self._for_chunks(left.shape[0], left.device, lambda i0, i1, lane: self.run_chunk(left[i0:i1], right[i0:i1], lane, i0)[0])

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

        def body_mono(i0, i1, lane):
            from . import iotool
            cam = 0 if self.source == 'left' else 1
            raw = (left_raw, right_raw)[cam][i0:i1]
            prestep._check(raw, self.source)
            st = self._stage.get(lane)
            if st is None:
                st = self._stage[lane] = torch.empty((self.chunk, self.h, self.w), dtype=torch.uint8, device=raw.device)
            iotool._prestep(prestep.maps[cam], raw, st[:i1 - i0], self.h * self.w)
            rec, _, out = self._run_chunk_mono(st[:i1 - i0], lane, i0)
            if fits is not None:
                for k, t in fits.items():
                    t[i0:i1] = out[k]
            return rec
        if self.source in ('left', 'right'):
            one = left_raw if self.source == 'left' else right_raw
            return self._for_chunks(one.shape[0], one.device, body_mono)

        def body(i0, i1, lane):
            st = self._stage.get(lane)
            if st is None:
                st = self._stage[lane] = torch.empty((self.chunk, 2, self.h, self.w), dtype=torch.uint8, device=left_raw.device)
            pairs = prestep(left_raw[i0:i1], right_raw[i0:i1], out=st[:i1 - i0])
            rec, _, out = self.run_chunk(pairs[:, 0], pairs[:, 1], lane, i0)
            if fits is not None:
                for k, t in fits.items():
                    t[i0:i1] = out[k]
            return rec
        return self._for_chunks(left_raw.shape[0], left_raw.device, body)


FIT_OUTPUTS = dict(pts3=((fit.MAXP, 3), torch.float64), m=((), torch.int32), cyl_raw=((2, 6), torch.float64), cyl=((2, 6), torch.float64),
                   T=((4, 4), torch.float64), fvals=((2,), torch.float64), mean_err=((), torch.float64), status=((), torch.int32),
                   offset=((2,), torch.int32), match_score=((4,), torch.int32), match_flags=((), torch.int32))


PLANE_FIT_OUTPUTS = dict(pts3=((fit.MAXP, 3), torch.float64), idx=((fit.MAXP, 2), torch.int32), m=((), torch.int32), P=((4,), torch.float64),
                         T=((4, 4), torch.float64), grid=((3, 3), torch.float64), stats=((8,), torch.float64), n_inliers=((), torch.int32),
                         inlier_mask=((fit.MAXP,), torch.uint8), plane_flags=((), torch.int32), mean_err=((), torch.float64),
                         status=((), torch.int32))


# what fit.fit_single_plane_batch adds with relabel= (per frame and image); FramePipeline(relabel=...).run_raw keeps them when the
# fits dict holds tensors of these names
RELABEL_OUTPUTS = dict(relabel_counts=((2, 2, 4), torch.int32), relabel_flags=((2,), torch.int32))


MONO_FIT_OUTPUTS = dict(pts3=((fit.MAXP, 3), torch.float64), idx=((fit.MAXP, 2), torch.int32), m=((), torch.int32),
                        cyl_raw=((2, 6), torch.float64), cyl=((2, 6), torch.float64), T=((4, 4), torch.float64), fvals=((2,), torch.float64),
                        mean_err=((), torch.float64), status=((), torch.int32), counts=((4,), torch.int32),
                        res=((fit.MAXP, 2), torch.float64), src=((fit.MAXP, 2), torch.int32), stats=((2,), torch.float64))


FUSED_FIT_OUTPUTS = dict(pts3=((fit.MAXP, 3), torch.float64), idx=((fit.MAXP, 2), torch.int32), m=((), torch.int32),
                         cyl_raw=((2, 6), torch.float64), cyl=((2, 6), torch.float64), T=((4, 4), torch.float64), fvals=((2,), torch.float64),
                         mean_err=((), torch.float64), status=((), torch.int32), counts=((6,), torch.int32),
                         res=((fit.MAXP, 4), torch.float64), src=((fit.MAXP, 3), torch.int32), stats=((4,), torch.float64),
                         flags=((), torch.int32))


# what fit.fit_single_cylinder_refined_batch returns per frame (FramePipeline(source='fused', refine=...))
REFINED_FIT_OUTPUTS = dict(pts3=((fit.MAXP, 3), torch.float64), idx=((fit.MAXP, 2), torch.int32), m=((), torch.int32),
                           cyl_raw=((2, 6), torch.float64), cyl=((2, 6), torch.float64), T=((4, 4), torch.float64), fvals=((2,), torch.float64),
                           mean_err=((), torch.float64), status=((), torch.int32), round_taken=((), torch.int32),
                           renumbered=((2,), torch.int32))


def alloc_fits(F, device, target='cylinder', source='stereo', refine=False):
    """zeroed [F, ...] tensors for the per-frame outputs of fit.fit_single_cylinder_batch (target='plane': of
    fit.fit_single_plane_batch; source 'left' / 'right': of fit.fit_single_cylinder_mono_batch; source 'fused': of
    fit.fit_single_cylinder_fused_batch, with refine of fit.fit_single_cylinder_refined_batch) that FramePipeline.run_raw can keep"""
    if source == 'fused':
        outputs = REFINED_FIT_OUTPUTS if refine else FUSED_FIT_OUTPUTS
    else:
        outputs = dict(cylinder=FIT_OUTPUTS, plane=PLANE_FIT_OUTPUTS)[target] if source == 'stereo' else MONO_FIT_OUTPUTS
    return {k: torch.zeros((F,) + shape, dtype=dt, device=device) for k, (shape, dt) in outputs.items()}
