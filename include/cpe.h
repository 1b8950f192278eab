/*
 * cpe.h -- C ABI of libcpe_hip.so: the MI355X (gfx950) implementation of the hot path of
 * cv3vpl-lab/cylinder-pose-estimation.
 *
 * The reference has no FFI for this path: its boundary is the Python function
 *     detect_grid(input_img) -> (col_img, result_json, rows_updated, cols_updated)
 *         (python_grid_detection_cylinder.py:68-112, called from MATLAB makePyGridPts.m:29)
 * and the MATLAB function
 *     [pts3, cylT, fvals, meanError] = fitSingleCylinder(...)   (utils/fitSingleCylinder.m:1)
 * Each entry point below names the reference code it replaces.  INTEGRATION.md shows the ctypes
 * binding a maintainer adds to python_grid_detection_cylinder.py.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; every buffer is caller-owned DEVICE memory
 *     (e.g. torch tensors, pass tensor.data_ptr()); no allocation inside, scratch comes from
 *     the caller-supplied workspace.  Process state: the thread-local error string, the optional profiling timers,
 *     and sets of three helper streams with their events, one set per (device, caller stream) for up to four caller
 *     streams per device (further ones share the last set): cpe_detect_grid_batch* overlaps the independent chains of a
 *     call on them, so calls on different caller streams do not serialise each other; the enqueue of a call (host side,
 *     fork to join) holds its set's mutex, so the library is thread-safe; CPE_SERIAL=1 in the environment keeps
 *     everything on the caller's stream.
 *   - Workspaces.  Every `ws` argument below (cpe_detect_workspace_bytes, cpe_fit_workspace_bytes,
 *     cpe_match_offset_workspace_bytes, cpe_multi_frame_consensus_workspace_bytes) is scratch in the full sense: what the
 *     block holds on entry is irrelevant to every output the call defines, so it needs no initialisation and no clearing
 *     between calls -- fresh memory, the leftovers of any earlier call (another batch size, and with it another layout,
 *     another target, another entry point) and arbitrary bytes all give the same results.  Each call initialises what it
 *     reads, and nothing is read or written at or beyond `ws_bytes`, the size the call was given: a block larger than the
 *     call needs keeps its tail.  What a call leaves in the block is defined only where this header says so (the CPE_PLANE_*
 *     planes, the line tables behind cpe_detect_line_tables / cpe_detect_results_*); it stays valid until the next call that
 *     is given the block.
 *     (tests/test_workspace_poison_gpu.py; the first writer of every buffer is listed in DESIGN.md section 3.)
 *   - every call is asynchronous on `stream` (a hipStream_t, passed as void*; NULL = default
 *     stream) and graph-capturable; no host synchronisation inside.
 *   - return value: 0 ok, <0 argument / launch error (text via cpe_last_error_string()).
 *   - per-frame failures never abort a batch: they are reported in a status[n] array
 *     (CPE_ST_*), mirroring the places where the reference raises inside detect_grid.
 *   - images are row-major u8, frame stride h*w, no padding.
 */
#ifndef CPE_H
#define CPE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CPE_VERSION 131  /* 100 + round: exports are only ever added (103: cpe_detect_grid_bgr_batch_ex, cpe_detect_constants;
                             104: cpe_detect_grid_bgr_batch_ex also takes the planar target; 105: cpe_debug_blob_region;
                             106: cpe_debug_preprocess; 107: cpe_debug_masks; 108: cpe_detect_results_sizes,
                             cpe_detect_results_pack; 109: cpe_debug_workspace_buffer; 110: cpe_debug_lines;
                             111: cpe_debug_clahe_planes_bgr; 112: cpe_multi_frame_fit_batch, cpe_pose_vec2T_batch,
                             cpe_pose_T2vec_batch; 113: cpe_multi_frame_fit_lm_batch; 114: cpe_agv_chain_batch,
                             cpe_frame_angles_lm_batch; 115: cpe_debug_region_hull; 116: cpe_match_offset_batch,
                             cpe_match_offset_workspace_bytes; 117: cpe_fit_plane_batch, cpe_index_planes_batch;
                             118: cpe_table_triangulate_batch; 119: cpe_fit_projector_model, cpe_projector_model_table;
                             120: cpe_index_shift_batch; 121: cpe_multi_frame_consensus_batch,
                             cpe_multi_frame_consensus_workspace_bytes; 122: cpe_fused_triangulate_batch;
                             123: cpe_grid_relabel_batch; 124: cpe_grid_predict_batch, cpe_grid_assign_batch;
                             125: cpe_debug_ccl_tiles; 126: cpe_debug_state_field;
                             127: cpe_mono_shift_batch; 128: cpe_est_curvatures_batch, cpe_curvature_consensus_batch;
                             129: cpe_fit_cylinder_pixels_batch; 130: cpe_multi_frame_fit_pixels_batch;
                             131: cpe_multi_frame_fit_pixels_angles_batch) */

#if defined(__GNUC__)
#define CPE_API __attribute__((visibility("default")))
#else
#define CPE_API
#endif

#define CPE_OK 0
#define CPE_ERR_ARG (-1)
#define CPE_ERR_LAUNCH (-2)
#define CPE_ERR_WORKSPACE (-3)

/* per-frame status codes */
#define CPE_ST_OK 0
#define CPE_ST_NO_REGION 1   /* no blob contour: cv2.convexHull(None), util_cylinder.py:1894 */
#define CPE_ST_NO_SPOT 2     /* no pixel > 240 after blur19: circle_radius0 unbound, :1974-2007 */
#define CPE_ST_NO_LINES 3    /* no valid rows / cols: indexing_data early returns, :1430-1460 */
#define CPE_ST_EMPTY 4       /* make_json raises on empty point list, :1703-1704 */
#define CPE_ST_FEW_POINTS 5  /* too few 3-D points for the fit (fitCylinderWPts3.m:8, estCurvatures.m:5) */
#define CPE_ST_OVERFLOW 6    /* a fixed capacity of the workspace was exceeded (build-defined) */
#define CPE_ST_SUBPIXEL_RAISED 7 /* optional sub-pixel stage: a line sample leaves the image through the top / left edge;
                                   compute_center_of_gravity_x/y raise there (util_cylinder.py:722,741,769,786) */

CPE_API int32_t cpe_version(void);
CPE_API const char *cpe_last_error_string(void);

/* Per-kernel hipEvent timers (the build's stand-in for the reference's commented line_profiler hooks,
 * util_cylinder.py:2010-2011).  Off by default; while on, every internal launch is bracketed by events on
 * its stream.  cpe_profile_report synchronises them, writes "kernel,calls,total_ms" lines (descending)
 * into csv and clears the records; returns the number of distinct kernels. */
CPE_API void cpe_profile_enable(int32_t on);
CPE_API int32_t cpe_profile_report(char *csv, size_t cap);

/* ------------------------------------------------------------------------------------------
 * Stage a-1: load_and_preprocess_image (util_cylinder.py:1769-1802) for a batch of frames.
 *   gray  u8[n,h,w]  ->  mask u8[n,h,w]  (255 = ridge: Hessian(sigma 3) smaller eigenvalue <= Sauvola
 *   threshold of itself, window 15, k 0.5, R 128; the reference's `binary_img`).
 * One fused kernel: gray tile -> LDS -> 5x5 binomial (integer) -> separable 25-tap Gaussian (f64)
 * -> two central differences -> eigenvalue -> 15x15 box mean / mean-of-squares -> compare.
 * No workspace.  h, w >= 8.
 */
CPE_API int32_t cpe_preprocess_batch(const uint8_t *gray, int32_t n, int32_t h, int32_t w, uint8_t *mask,
                             void *stream);

/* cpe_preprocess_batch with the f64 planes of its last stage stored beside the mask: b f64[n,h,w], the smaller Hessian
 * eigenvalue, and T f64[n,h,w], its Sauvola threshold (mask = 0 where b > T, 255 elsewhere).  The same arguments and
 * rules as cpe_preprocess_batch; a separate instantiation of the same kernel, so the product kernel stays as it is.
 * Test / debugging aid. */
CPE_API int32_t cpe_debug_preprocess(const uint8_t *gray, int32_t n, int32_t h, int32_t w, uint8_t *mask, double *b,
                                     double *T, void *stream);

/* ------------------------------------------------------------------------------------------
 * detect_grid(input_img) for a batch of n grey frames (python_grid_detection_cylinder.py:68-112 ->
 * util_cylinder.py stages 1-6): gray u8[n,h,w] (the 2-D array makePyGridPts.m:26 passes; a BGR frame
 * with three identical channels is the same image) ->
 *   xy f64[n,CPE_MAXP,2], id i32[n,CPE_MAXP,2] = (col,row), n_pts i32[n], center f64[n,2]:
 *   exactly the content make_json serialises (util_cylinder.py:1674-1727): points with col >= 0 sorted
 *   by (col,row), and the centre point;
 *   status i32[n]: CPE_ST_* (the places where the reference raises inside detect_grid and returns None).
 * ws: cpe_detect_workspace_bytes(n,h,w) bytes of 256-byte aligned device scratch; its content on entry is irrelevant and
 * nothing at or beyond ws_bytes is touched (Conventions, "Workspaces").  64 <= h,w <= 4096.
 */
CPE_API size_t cpe_detect_workspace_bytes(int32_t n, int32_t h, int32_t w);
CPE_API int32_t cpe_detect_grid_batch(const uint8_t *gray, int32_t n, int32_t h, int32_t w, void *ws, size_t ws_bytes,
                                      double *xy, int32_t *id, int32_t *n_pts, double *center, int32_t *status,
                                      void *stream);

/* The same with options.  subpixel != 0 inserts the reference's (disabled) grey-level centre-of-gravity refinement
 * of the fitted lines -- modify_grayscale_Cline(img, rows, cols, degree=2, sample_step, window_size), whose call is
 * commented out at util_cylinder.py:2040 -- between remove_label and the intersection step.  params NULL = defaults
 * = the live reference path (subpixel 0). */
typedef struct CpeDetectParams {
    int32_t subpixel;        /* 0 = off (reference behaviour) */
    int32_t subpixel_window; /* window_size (the commented call uses 7) */
    double subpixel_step;    /* sample_step (1.0) */
    int32_t target;          /* CPE_TARGET_CYLINDER (python_grid_detection_cylinder.py) or CPE_TARGET_PLANE (row f-2:
                                python_grid_detection_plane.py over utils/util_plane.py; point ids are (row, col) there,
                                every column is kept, sub-pixel refinement is not available) */
    int32_t flags;           /* CPE_DETECT_* bits; 0 = none.  A bit this build does not know: CPE_ERR_ARG, nothing is launched */
} CpeDetectParams;
#define CPE_TARGET_CYLINDER 0
#define CPE_TARGET_PLANE 1
/* Four of the public planes are debug outputs that no later stage reads where rows are a multiple of 16 pixels (the stages
 * then hand the line masks on as one-bit planes): CPE_PLANE_HMASK, CPE_PLANE_VMASK, CPE_PLANE_ROI_H, CPE_PLANE_ROI_V.  With
 * this bit set they are not written at such widths and their contents are UNDEFINED after the call; every other plane and
 * every result is what it is without the bit.  Other widths need the bytes and ignore the bit.  A caller that only wants
 * the point tables (the frame pipeline) sets it and saves four full-frame stores per frame. */
#define CPE_DETECT_SKIP_DEBUG_PLANES 1
CPE_API int32_t cpe_detect_grid_batch_ex(const uint8_t *gray, int32_t n, int32_t h, int32_t w, const CpeDetectParams *params,
                                         void *ws, size_t ws_bytes, double *xy, int32_t *id, int32_t *n_pts,
                                         double *center, int32_t *status, void *stream);

/* The reference's inline constants, as this build was compiled with them ("Config": the reference has no
 * configuration object -- every value below is a literal in util_cylinder.py / util_plane.py or an OpenCV default).  They are
 * compile-time constants of the kernels (window sizes decide register windows and LDS rings), so this is a REPORT, not a
 * setter: a maintainer who changes a literal in the reference finds here what to change in the kernels, and the tests pin the
 * table to the reference's values.  target: CPE_TARGET_CYLINDER or CPE_TARGET_PLANE. */
typedef struct CpeDetectConstants {
    int32_t blur_ksize;            /* cv2.GaussianBlur(gray, (5,5), 0)                         util_cylinder.py:1790 */
    double hessian_sigma;          /* detect_ridges(blurred, sigma=3.0)                        :1793 */
    int32_t sauvola_window;        /* sauvola_threshold_fast(b, window_size=15, k=0.5, R=128)  :1797 */
    double sauvola_k, sauvola_R;
    int32_t open_len;              /* MORPH_RECT (20,1) / (1,20) openings                      :1810-1811 */
    double clahe_clip;             /* detect_largest_blob(..., clipLimit=4.5)                  python_grid_detection_cylinder.py:88 */
    int32_t clahe_tiles;           /* tileGridSize=(4,4) (the colour branch: the image is always 3-channel here) :1843 */
    int32_t blob_thr_min, blob_thr_step, blob_thr_count;   /* SimpleBlobDetector defaults 50 .. 220 step 10: 17 binarisations */
    double blob_min_area, blob_max_area;                   /* params.minArea = 10 (:1858), default maxArea 5000 */
    double blob_min_dist;          /* default minDistBetweenBlobs 10 */
    int32_t blob_min_repeat;       /* default minRepeatability 2 */
    int32_t disc_extra_radius;     /* int(size / 2 + 4)                                        :1876 */
    int32_t spot_blur_ksize;       /* cv2.GaussianBlur(gray, (19,19), 0)                       :1962 */
    int32_t spot_threshold;        /* cv2.threshold(blurred, 240, ...)                         :1965 */
    int32_t spot_small_radius, spot_small_add, spot_large_add;   /* radius < 30: + 20, else + 5   :1981-1984 */
    int32_t frag_patch, frag_min_pixels, frag_max_pixels;        /* expand_line_roi(patch 15, 5 .. 200 pixels) :137 (plane: 8 .. 700) */
    int32_t frag_kernel_base;      /* kernel_size = 91 + circle_radius0 (:2022); plane: the fixed 201 (util_plane.py:2806) */
    int32_t index_blur_ksize;      /* cv2.GaussianBlur(img, (7,7), 0) of indexing_data         :1433 */
    int32_t poly_degree;           /* fit_and_draw_polynomial: 2 (cylinder), 1 (plane) */
    int32_t plane_threshold, plane_dilate_ksize;   /* get_convex_hull: threshold 127, MORPH_ELLIPSE (11,11) (util_plane.py:2590-2689); 0 for the cylinder */
    int32_t max_points, max_lines, max_joints, max_groups_per_dir, max_joints_per_group;   /* build capacities (CPE_ST_OVERFLOW) */
} CpeDetectConstants;
CPE_API int32_t cpe_detect_constants(int32_t target, CpeDetectConstants *out);

/* rows_updated / cols_updated of ONE frame of the last cpe_detect_grid_batch call on this workspace: the third and fourth
 * return values of detect_grid (python_grid_detection_cylinder.py:110; built by find_and_assign_intersections_P and
 * clean_and_relabel, util_cylinder.py:1106-1206).  Side 0 = rows ("row1".."rowR", ordered by mean y), side 1 = columns
 * ("col1".."colC", ordered by mean x; negative columns included -- remove_minus_labels only prunes the JSON).
 *   eq      f64[2, CPE_MAXL, 6]            [a2, a1, a0, min-50, max+50, span] of the quadratic fit (util_cylinder.py:473-550)
 *   npts    i32[2, CPE_MAXL]               intersections on the line
 *   pts     f64[2, CPE_MAXL, CPE_MAXL, 2]  (x, y) in the reference's loop order
 *   n_lines i32[2]                         R, C  (0, 0 for a frame that failed before this stage)
 * All device buffers; asynchronous on `stream`. */
#define CPE_MAXL 256
/* Capacities of the line stage, part of the boundary: the reference's lists are unbounded (util_cylinder.py:376-389,
 * 1106-1151); a frame with more joints inside the region rectangle than CPE_MAXJ, more label groups per direction than
 * CPE_MAXL, more joints in one group than CPE_MAXLP or more grid points than CPE_MAXP ends with CPE_ST_OVERFLOW -- in this
 * library AND in the test oracle (oracle/src/orc_lines.c reads these constants), so the two agree on every frame.
 * Seen: 8 000 joints / 5 500 inside the rectangle / 250 groups / 255 joints in a group on 1920x1200 frames degraded with
 * +-9 DN of noise and an intensity ramp (tools/stress_parity.py seeds 4011, 9508); clean frames: < 1 500 / < 64 / < 64. */
#define CPE_MAXJ 16384
#define CPE_MAXLP 1024
CPE_API int32_t cpe_detect_line_tables(const void *ws, size_t ws_bytes, int32_t n, int32_t h, int32_t w, int32_t frame,
                                       double *eq, int32_t *npts, double *pts, int32_t *n_lines, void *stream);

/* Packed results: everything detect_grid returns beside the picture, for ALL n frames of the last cpe_detect_grid_batch* call
 * on this workspace, as one variable-length record per frame in one device buffer -- one size read-back and one payload copy
 * per batch instead of cpe_detect_line_tables' dense 2 MB per frame.  Sequence:
 *   1. cpe_detect_results_sizes(ws, ws_bytes, n, h, w, n_pts, status, offsets, stream)
 *        offsets i64[n+1] (device): offsets[k] = byte offset of frame k's record in the payload, offsets[0] = 0, offsets[n] =
 *        bytes of all records.  Every offset is a multiple of 8 and offsets[k+1] > offsets[k].  The size of a record depends
 *        on n_pts and the workspace only; status is taken so that both calls are given the same tables.
 *   2. the caller copies offsets to the host (the one synchronisation of the sequence) and provides payload_bytes >=
 *      offsets[n] bytes of 8-byte aligned device memory;
 *   3. cpe_detect_results_pack(ws, ws_bytes, n, h, w, xy, id, n_pts, center, status, offsets, payload, payload_bytes, stream)
 *        with the tables the detect call wrote and the offsets of step 1 writes every byte of [0, offsets[n]), padding
 *        included, and nothing else.
 * Neither call allocates or synchronises; both are asynchronous on `stream` and must be ordered after the detect call and
 * before the next call that uses the workspace.  A payload_bytes smaller than offsets[n] cannot be seen by the host without
 * a synchronisation, so it is not an error: the kernel never writes at or beyond payload_bytes, a record that does not end
 * inside it (or whose offsets do not leave exactly its size) is skipped WHOLE, and its bytes keep what they held.  A
 * caller learns of it the way it sized the payload: it has read offsets[n]; a reader must refuse a payload shorter than that.
 *
 * Record of frame k at payload + offsets[k], little-endian, every array 8-byte aligned, padding bytes zero:
 *   offset 0   i32 status                  CPE_ST_* of the frame, as in status[k]
 *          4   i32 n_pts                   points of the xy / id tables, as in n_pts[k] (0 unless status is CPE_ST_OK)
 *          8   i32 n_rows                  R lines of side 0 ("row1".."rowR")
 *         12   i32 n_cols                  C lines of side 1 ("col1".."colC")
 *         16   i32 n_row_pts               intersections on all rows together
 *         20   i32 n_col_pts               intersections on all columns together
 *         24   i32 0, 0
 *         32   f64 center[2]               as in center[k]
 *         48   f64 xy[n_pts][2]            make_json order, as in the xy table
 *              i32 id[n_pts][2]            (col, row); (row, col) for the planar target
 *              f64 eq[R + C][6]            rows first, final order; the six numbers of cpe_detect_line_tables' eq
 *              i32 start[R + C + 1]        start[i] = intersections on the lines before line i (start[0] = 0, start[R] =
 *                                          n_row_pts, start[R + C] = n_row_pts + n_col_pts); one zero i32 of padding
 *                                          follows when R + C + 1 is odd
 *              f64 pts[n_row_pts + n_col_pts][2]   line i owns pts[start[i] .. start[i+1]): (x, y) in the reference's loop order
 *   bytes = 48 + 24 n_pts + 48 (R + C) + 8 ((R + C + 2) / 2) + 16 (n_row_pts + n_col_pts)      (integer division)
 * The line content is what cpe_detect_line_tables reports for the frame -- also for a frame whose status is not CPE_ST_OK
 * (0 / 0 lines if it failed before the line stage): the two interfaces agree on every frame, and equal frames give equal
 * records byte for byte. */
CPE_API int32_t cpe_detect_results_sizes(const void *ws, size_t ws_bytes, int32_t n, int32_t h, int32_t w, const int32_t *n_pts,
                                         const int32_t *status, int64_t *offsets, void *stream);
CPE_API int32_t cpe_detect_results_pack(const void *ws, size_t ws_bytes, int32_t n, int32_t h, int32_t w, const double *xy,
                                        const int32_t *id, const int32_t *n_pts, const double *center, const int32_t *status,
                                        const int64_t *offsets, void *payload, size_t payload_bytes, void *stream);

/* Colour input.  The reference's CLI hands detect_grid the H x W x 3 BGR array of cv2.imread (python_grid_detection_cylinder.py:34-44);
 * load_and_preprocess_image (util_cylinder.py:1781-1789) and mask_roi_around_center (:1957) work on cv2.cvtColor(BGR2GRAY) of it:
 * 8-bit fixed point, gray = (B*3735 + G*19235 + R*9798 + 2^14) >> 15 ([ext] OpenCV 4.5.5; identity on grey-replicated frames);
 * detect_largest_blob takes the L channel of cv2.cvtColor(BGR2LAB) of the COLOUR image (:1840) and indexing_data blurs the colour
 * image 7x7 channel by channel before converting it (:1433-1435).
 * The planar script (python_grid_detection_plane.py, CPE_TARGET_PLANE) reads the colour planes in two places as well; every other
 * step of it works on the grey image:
 *   get_convex_hull(original_img, 5) (python_grid_detection_plane.py:96, utils/util_plane.py:2590-2689) thresholds each channel
 *     at 127 (cv2.threshold, THRESH_BINARY) and converts that 0/255 image with BGR2GRAY: the first hull round starts from the
 *     pixels where ANY channel is above 127 (grey frames: gray > 127);
 *   indexing_data (util_plane.py:1334-1336) blurs the colour image 7x7 channel by channel before converting it, as above.
 *   cpe_bgr2gray_batch             bgr u8[n,h,w,3] interleaved -> gray u8[n,h,w]; both 4-byte aligned device buffers.
 *   cpe_detect_grid_bgr_batch_ex   the whole of detect_grid on true-colour frames: same outputs, workspace and status codes as
 *                                  cpe_detect_grid_batch_ex (cylinder or planar target, no sub-pixel refinement); on
 *                                  grey-replicated frames it returns what cpe_detect_grid_batch returns for the grey plane.
 *                                  Planar target: CPE_PLANE_CLAHE (unused by that target) holds the 0/255 any-channel
 *                                  mask after the call. */
CPE_API int32_t cpe_detect_grid_bgr_batch_ex(const uint8_t *bgr, int32_t n, int32_t h, int32_t w, const CpeDetectParams *params,
                                             void *ws, size_t ws_bytes, double *xy, int32_t *id, int32_t *n_pts,
                                             double *center, int32_t *status, void *stream);
CPE_API int32_t cpe_bgr2gray_batch(const uint8_t *bgr, int32_t n, int32_t h, int32_t w, uint8_t *gray, void *stream);

/* Where an intermediate of the last cpe_detect_grid_batch call lives inside the workspace (for
 * stage-by-stage parity tests and debugging): plane-major, frame f at offset + f * bytes_per_frame.
 * After a call with CPE_DETECT_SKIP_DEBUG_PLANES the planes HMASK, VMASK, ROI_H and ROI_V are undefined (see the flag).
 *
 * Planes of a frame that ends early.  The three chains in front of the join run for every frame of a batch, whatever becomes
 * of it later, and no plane of one frame depends on another frame or on what the workspace held before the call:
 *   every status       BINARY, HMASK, VMASK, BLUR19 (as `> 240`) and, cylinder target, CLAHE and SWEEP are what they are for a
 *                      good frame; STATE: status and overflow; the line tables report 0 rows and 0 columns unless the lines
 *                      stage ran (CPE_ST_OK, CPE_ST_NO_LINES and later), and the packed record has n_pts 0 unless CPE_ST_OK.
 *   CPE_ST_NO_REGION   MASK_CONTOUR, ROI_H, ROI_V, EXP_H and EXP_V are ZERO on every pixel; JOINTS and the other words of
 *                      STATE are undefined.
 *   CPE_ST_NO_SPOT     MASK_CONTOUR and STATE's rect, n_kp are the region's; ROI_H, ROI_V, EXP_H, EXP_V (the reference stops in
 *                      front of them) and JOINTS are UNDEFINED.
 *   CPE_ST_NO_LINES and every later ending (CPE_ST_EMPTY, CPE_ST_OVERFLOW of the lines stage, CPE_ST_SUBPIXEL_RAISED)
 *                      every plane above, JOINTS up to STATE's n_joints, r0 and spot as for a good frame.
 *   BLUR7              defined for frames with CPE_ST_OK only, in the 64 x 32 tiles within the largest indexing window of the
 *                      region rectangle; UNDEFINED elsewhere and for every other frame.
 *   planar target      CPE_PLANE_CLAHE (grey entry) and CPE_PLANE_SWEEP are not written: UNDEFINED.
 * Rows of xy / id at or past n_pts[k] are not written.  UNDEFINED content may depend on earlier calls; everything else above is
 * held to the oracle and to a run on a zeroed workspace by tests/test_workspace_poison_gpu.py. */
#define CPE_PLANE_BINARY 0        /* u8[h,w]  load_and_preprocess_image -> binary_img */
#define CPE_PLANE_HMASK 1         /* u8[h,w]  extract_joints -> horizontal_mask */
#define CPE_PLANE_VMASK 2         /* u8[h,w]  extract_joints -> vertical_mask */
#define CPE_PLANE_MASK_CONTOUR 3  /* u8[h,w]  detect_largest_blob -> mask_contour */
#define CPE_PLANE_ROI_H 4         /* u8[h,w]  mask_roi_around_center -> mask_roi_h */
#define CPE_PLANE_ROI_V 5
#define CPE_PLANE_EXP_H 6         /* u8[h,w]  expands_line_roi -> horizontal_expanded */
#define CPE_PLANE_EXP_V 7
#define CPE_PLANE_JOINTS 8        /* i32[CPE_MAXJ,2] cylinder_centroids in contour order */
#define CPE_PLANE_STATE 9         /* per-frame state record (see csrc/cpe_dev.h FrameState) */
#define CPE_PLANE_CLAHE 10        /* u8[h,w]  CLAHE'd L channel (planar target: the any-channel mask of colour frames) */
#define CPE_PLANE_BLUR19 11       /* u8[h,w]  cv2.GaussianBlur(gray, (19,19), 0) in the 64x32 tiles where it can exceed 240,
                                     0 elsewhere: the spot chain only asks blurred > 240 (util_cylinder.py:1958), so the
                                     contract is (plane > 240) == (blurred > 240) on every pixel, not the values below */
#define CPE_PLANE_BLUR7 12        /* u8[h,w] */
#define CPE_PLANE_SWEEP 14        /* i32[192] blob-sweep counters: [8+k] dark components, [25+k] bright components,
                                     [42+k] blobs of threshold 50+10k (k < 17); see csrc/region.hip SW_* */
CPE_API int32_t cpe_detect_workspace_plane(int32_t n, int32_t h, int32_t w, int32_t plane, size_t *offset,
                                           size_t *bytes_per_frame);

/* Row `index` (0, 1, ...; CPE_ERR_ARG past the last) of the workspace's table of buffers (csrc/workspace.h) for an (n,h,w)
 * call: its name (at most name_cap - 1 characters), where it lies, the overlay it belongs to (0: it shares memory with nothing;
 * buffers of the same overlay on different sides do) and its side, and its CPE_PLANE_* number or -1.  Host code only: no GPU
 * call.  Offsets are not a contract.  Test / debugging aid. */
CPE_API int32_t cpe_debug_workspace_buffer(int32_t n, int32_t h, int32_t w, int32_t index, char *name_out, size_t name_cap,
                                           size_t *offset, size_t *bytes_per_frame, int32_t *overlay, int32_t *side,
                                           int32_t *public_plane);

/* Row `index` (0, 1, ...; CPE_ERR_ARG past the last) of the per-frame state record behind CPE_PLANE_STATE (csrc/cpe_dev.h,
 * CPE_STATE_FIELDS), in the order of its 32-bit words: the field's name (at most name_cap - 1 characters), the words it takes
 * (an array of 4 takes 4) and whether they hold floats (else int32).  Host code only: no GPU call.  Test / debugging aid. */
CPE_API int32_t cpe_debug_state_field(int32_t index, char *name_out, size_t name_cap, int32_t *words, int32_t *is_float);

/* One stand-alone connected-component pass (cv2.connectedComponents / the front end of cv2.findContours,
 * util_cylinder.py:28,161,1817,1883,1968) over img u8[n,h,w]: set = (img > thr) != invert, 8- or 4-connected;
 * labels (raster index of the component's first pixel, -1 outside the set) land in workspace plane
 * CPE_PLANE_LABELS.  count_mode / want_bbox / want_roots switch the optional by-products (profiling aid). */
#define CPE_PLANE_LABELS 13       /* i32[h,w] */
CPE_API int32_t cpe_debug_ccl(const uint8_t *img, int32_t n, int32_t h, int32_t w, int32_t thr, int32_t invert,
                              int32_t conn8, int32_t count_mode, int32_t want_bbox, int32_t want_roots, void *ws,
                              size_t ws_bytes, void *stream);

/* The first labelling of the blob sweep's dark forest (csrc/region.hip) on img u8[n,h,w]: the 4-connected components of
 * img <= thr inside rect i32[n,4] (x0, y0, x1, y1 inclusive, device memory), flattened, with per-root pixel counts, the
 * root list and, outside the set, the sweep's pre-linked runs of one grey-level bucket (0 <= thr <= 95).  path 0: the
 * byte-level passes, 1: the passes the detector runs (w % 16 == 0: the set read from the first of 17 one-bit planes per
 * frame, thresholds thr, thr + 10, ..., word-level finish).  Outputs (device
 * memory): lab, cnt i32[n,h,w] (-1 where a pass writes nothing), roots i32[n,CPE_MAXROOTS_DEBUG] (any order), n_roots i32[n].
 * Test / debugging aid. */
#define CPE_MAXROOTS_DEBUG 262144
CPE_API int32_t cpe_debug_dark_labels(const uint8_t *img, int32_t n, int32_t h, int32_t w, int32_t thr, const int32_t *rect,
                                      int32_t path, void *ws, size_t ws_bytes, int32_t *lab, int32_t *cnt, int32_t *roots,
                                      int32_t *n_roots, void *stream);

/* The component list the detector's stages start from (csrc/ccl.hip, ccl_components) on img u8[n,h,w] (h >= 1, w >= 16): the
 * components of img > thr, 8-connected if conn8, else 4-connected, inside rect i32[n,4] (x0, y0, x1, y1 inclusive, inside the
 * frame, device memory; NULL: the whole frame).  bits != 0: the passes read the set from its one-bit plane, which is built
 * first (w % 16 == 0; other widths read the bytes).  Outputs (device memory): lab i32[n,h,w], the label plane as the passes
 * leave it -- every pixel of the set inside rect holds the index of a smaller pixel of its component or, the component's
 * first pixel, its own; -1 everywhere else --, roots i32[n,CPE_MAXROOTS_DEBUG] (the first pixels, any order), n_roots i32[n].
 * Test / debugging aid. */
CPE_API int32_t cpe_debug_ccl_tiles(const uint8_t *img, int32_t n, int32_t h, int32_t w, int32_t thr, int32_t conn8,
                                    int32_t bits, const int32_t *rect, void *ws, size_t ws_bytes, int32_t *lab, int32_t *roots,
                                    int32_t *n_roots, void *stream);

/* The RETR_EXTERNAL rule of cv2.findContours as the detector applies it (util_cylinder.py:161, 1817; the other two call
 * sites, :1883 and :1968, keep only the largest contour, which is never a nested one): of the 8-connected components of
 * mask != 0, the raster-first pixels (y * w + x, any order) of those that do not lie inside a hole of another component.
 * first_px i32[n,cap], count i32[n] (may exceed cap: then only cap entries were stored).  Test / debugging aid. */
CPE_API int32_t cpe_debug_external_components(const uint8_t *mask, int32_t n, int32_t h, int32_t w, void *ws, size_t ws_bytes,
                                              int32_t *first_px, int32_t cap, int32_t *count, void *stream);

/* LAB-L + CLAHE(4.5, 4x4) of grey frames u8[n,h,w] and the blob detector's 17 threshold planes (img > 50 + 10 t, 64 x 8
 * tiles), as the region stage makes them.  fused 1: the passes the detector runs (w % 16 == 0 and wide tiles: the apply pass
 * writes the planes), 0: the byte-level apply and the planes from a pass of their own.  Outputs (device memory): cl u8[n,h,w],
 * planes (n * 17 planes of ceil(h / 8) * (ceil(w / 64) + 2) * 8 u64 words), buckets i32[n,18] (pixels per grey-level
 * bucket, 0 unused), box i32[n,4] (x0, y0, x1, y1 of the pixels > 50).  Test / debugging aid. */
CPE_API int32_t cpe_debug_clahe_planes(const uint8_t *gray, int32_t n, int32_t h, int32_t w, int32_t fused, void *ws, size_t ws_bytes,
                                       uint8_t *cl, uint32_t *planes, int32_t *buckets, int32_t *box, void *stream);

/* The same front end for true-colour frames bgr u8[n,h,w,3]: the L channel of BGR2LAB as cpe_detect_grid_bgr_batch_ex makes it
 * (copied out: L u8[n,h,w]), then CLAHE of that plane (no grey LAB-L table) and the planes, bucket sizes and box as above.
 * Test / debugging aid. */
CPE_API int32_t cpe_debug_clahe_planes_bgr(const uint8_t *bgr, int32_t n, int32_t h, int32_t w, int32_t fused, void *ws,
                                           size_t ws_bytes, uint8_t *L, uint8_t *cl, uint32_t *planes, int32_t *buckets,
                                           int32_t *box, void *stream);

/* The blob stage of detect_largest_blob (util_cylinder.py:1830-1899) on a given image: the library's region stage, with
 * img u8[n,h,w] (64 <= h,w <= 4096) as the image its SimpleBlobDetector sweeps -- LAB-L and CLAHE are replaced by an identity
 * table, so CPE_PLANE_CLAHE holds img afterwards -- run serially on `stream`.  Outputs:
 *   kp      f32[n,kp_cap,3]      key points (x, y, size) in the detector's group order; n_kp i32[n] their number (may exceed
 *                                kp_cap: then only kp_cap were stored)
 *   blobs   f64[n,17,blob_cap,3] accepted blobs (x, y, radius) of threshold 50 + 10 k, hole borders first, otherwise in no
 *                                defined order; n_blobs i32[n,17] their number (may exceed blob_cap)
 * and in the workspace, as after cpe_detect_grid_batch: CPE_PLANE_STATE (rect, n_kp, n_groups, overflow, status 0 or
 * CPE_ST_NO_REGION), CPE_PLANE_MASK_CONTOUR and CPE_PLANE_SWEEP.  Test / debugging aid. */
CPE_API int32_t cpe_debug_blob_region(const uint8_t *img, int32_t n, int32_t h, int32_t w, void *ws, size_t ws_bytes,
                                      float *kp, int32_t kp_cap, int32_t *n_kp, double *blobs, int32_t blob_cap,
                                      int32_t *n_blobs, void *stream);

/* The masks stage of detect_grid on given inputs: extract_joints, the joint filter of find_cylinder_centroids_and_center,
 * mask_roi_around_center and expands_line_roi (util_cylinder.py:35-237, 1805-2007; util_plane.py for CPE_TARGET_PLANE) --
 * what cpe_detect_grid_batch_ex runs between the pre-process and the lines stage, in the same order, serially on `stream`
 * (no helper streams), followed by the 7x7 blur of the indexing step.  Inputs (device memory):
 *   binary        u8[n,h,w]  the pre-process's ridge mask (CPE_PLANE_BINARY)
 *   gray          u8[n,h,w]  the grey frame (saturated spot, 7x7 blur)
 *   mask_contour  u8[n,h,w]  the region stage's mask (CPE_PLANE_MASK_CONTOUR); must be zero outside rect, as the region stage
 *                            guarantees: the roi kernel reads only the rectangle's pixels
 *   rect          i32[n,4]   boundingRect (x, y, w, h) of the region, inside the frame (w, h >= 1)
 *   region_status i32[n]     CPE_ST_OK or CPE_ST_NO_REGION
 * target: CPE_TARGET_CYLINDER or CPE_TARGET_PLANE.  64 <= h, w <= 4096; ws: cpe_detect_workspace_bytes(n, h, w).  Afterwards
 * the workspace holds what a cpe_detect_grid_batch_ex call holds there before its lines stage: the planes HMASK, VMASK,
 * ROI_H / ROI_V, EXP_H / EXP_V, JOINTS, BLUR19, BLUR7 and the state record (status, r0, spot, n_joints, n_joints_all,
 * n_seg, gang, glen, overflow).  Test / debugging aid. */
CPE_API int32_t cpe_debug_masks(const uint8_t *binary, const uint8_t *gray, const uint8_t *mask_contour, const int32_t *rect,
                                const int32_t *region_status, int32_t n, int32_t h, int32_t w, int32_t target, void *ws,
                                size_t ws_bytes, void *stream);

/* The lines stage of detect_grid on given inputs: the label lookup of the joints, the per-line fits, remove_label, the optional
 * sub-pixel refinement, the intersections, clean_and_relabel, indexing_data and make_json's ordering (util_cylinder.py:376-1727;
 * util_plane.py for CPE_TARGET_PLANE) -- what cpe_detect_grid_batch_ex runs after the masks stage: the unions of the two
 * expanded masks inside the region rectangle + 2 px, then the lines kernel with the same sample capacity (max(h, w) + 128 per
 * line), serially on `stream`.  Inputs (device memory):
 *   exp_h, exp_v  u8[n,h,w]          the expanded masks (CPE_PLANE_EXP_H / _V); their non-zero pixels lie inside rect, as the
 *                                    masks stage guarantees (a pixel farther than 2 px outside rect is its own component here)
 *   joints        i32[n,CPE_MAXJ,2]  (x, y) of the joints inside rect, in the order the masks stage leaves them; any values
 *                                    (a joint outside the frame or on background belongs to no line)
 *   n_joints      i32[n]             0 .. CPE_MAXJ
 *   rect          i32[n,4]           boundingRect (x, y, w, h) of the region, x, y >= 0 (it may reach past the right / bottom
 *                                    edge: the label window is clipped to the frame, the rectangle test of the intersections
 *                                    is not)
 *   r0            i32[n]             circle_radius0 (>= 0)
 *   stage_status  i32[n]             CPE_ST_OK, or the status an earlier stage ended the frame with (the frame is then skipped)
 *   g7            u8[n,h,w]          the 7x7-blurred image indexing_data takes its window means from
 *   gray          u8[n,h,w]          the grey frame (read by the sub-pixel refinement only)
 * params: as for cpe_detect_grid_batch_ex (subpixel, subpixel_window 1 .. 13, subpixel_step, target; flags 0); NULL = defaults.
 * xy, id, n_pts, center, status: the five tables of cpe_detect_grid_batch.  64 <= h, w <= 4096; ws:
 * cpe_detect_workspace_bytes(n, h, w).  Afterwards the workspace is what it is after a detect call as far as this stage goes:
 * the state record (status, n_rows, n_cols, overflow), the planes EXP_H / EXP_V, JOINTS, BLUR7, and the line tables that
 * cpe_detect_line_tables and cpe_detect_results_sizes / _pack read.  Test / debugging aid. */
CPE_API int32_t cpe_debug_lines(const uint8_t *exp_h, const uint8_t *exp_v, const int32_t *joints, const int32_t *n_joints,
                                const int32_t *rect, const int32_t *r0, const int32_t *stage_status, const uint8_t *g7,
                                const uint8_t *gray, int32_t n, int32_t h, int32_t w, const CpeDetectParams *params, void *ws,
                                size_t ws_bytes, double *xy, int32_t *id, int32_t *n_pts, double *center, int32_t *status,
                                void *stream);

/* The hull stage of detect_grid on a given image: cv2.findContours(RETR_EXTERNAL) -> the contour of largest contourArea ->
 * cv2.convexHull -> the filled polygon -> cv2.boundingRect, through the one host function both region stages end in.
 *   mode 0  the cylinder target's tail (detect_largest_blob, util_cylinder.py:1805-1870, after its cv2.circle calls): img
 *           u8[n,h,w] is a disc-union image, non-zero = set.  A frame whose set is ONE component must give that component
 *           a contour of positive area (the product's precondition: a union of discs of radius >= 4).
 *   mode 1  the planar target's region stage (get_convex_hull, util_plane.py:2590-2689) on grey frames img u8[n,h,w]: the set
 *           img > 127, its hull, the 11 x 11 elliptic dilation, the hull of that.
 * 64 <= h, w <= 4096; ws: cpe_detect_workspace_bytes(n, h, w).  Afterwards the workspace holds what a detect call holds there
 * after its region stage: CPE_PLANE_MASK_CONTOUR, the state record (status CPE_ST_OK / CPE_ST_NO_REGION, rect, hull_n,
 * n_roots, overflow) and, in the workspace row `hull` (cpe_debug_workspace_buffer), the hull_n vertices (x, y) as i32 pairs.
 * Test / debugging aid. */
CPE_API int32_t cpe_debug_region_hull(const uint8_t *img, int32_t n, int32_t h, int32_t w, int32_t mode, void *ws, size_t ws_bytes,
                                      void *stream);

/* ------------------------------------------------------------------------------------------
 * Grid-point tables.  One table per image: xy f64[n,CPE_MAXP,2] pixel coordinates, id i32[n,CPE_MAXP,2]
 * (col,row) grid indices, cnt i32[n] -- the padded form of the reference's N x 4 matrix
 * [x y colIdx rowIdx] (makePyGridPts.m:39-41, pointsStruct2mat.m:16).
 */
#define CPE_MAXP 2048          /* capacity of one grid-point table (a 3840x2160 frame holds ~1000-1400 points) */
#define CPE_FIT_TABLE_DIM 128  /* (col,row) indices of one frame must span < 128 in each direction */

#define CPE_FIT_FLAG_FALLBACK 1 /* selector found nothing -> plain index join (chooseIdx.m:101-104) */
#define CPE_FIT_FLAG_OVERFLOW 2 /* index span exceeds CPE_FIT_TABLE_DIM or |index| > 9999: frame skipped */
#define CPE_FIT_MIN_POINTS 5    /* fewest 3-D points a cylinder is fitted to (the local quadric has 5 unknowns) */

#define CPE_SEL_CHOOSE_IDX 0     /* chooseIdx(gp1,gp2,.,.,patch,th)          fitSingleCylinder.m:12 (live) */
#define CPE_SEL_THRESHOLD 1      /* triangulateWithThreshold(gp1,gp2,.,.,th) fitSingleCylinder.m:11 */
#define CPE_SEL_JOIN 2           /* findGridCorrespondences(gp1,gp2)         fitSingleCylinder.m:10 */

CPE_API size_t cpe_fit_workspace_bytes(int32_t n);

/* Index matching + triangulation for n stereo frames (one wavefront per frame).
 * Replaces chooseIdx.m / triangulateWithThreshold.m / findGridCorrespondences.m followed by
 * triangulate(cgp1, cgp2, stereoParams) at fitSingleCylinder.m:12-17.
 *   K1, K2   f64[9]  row-major intrinsics (getCamParams.m:6-7), T21 f64[16] row-major T_C2_C1 (:9)
 *   outputs  p1,p2 f64[n,CPE_MAXP,2] selected pixel pairs; idx i32[n,CPE_MAXP,2]; X f64[n,CPE_MAXP,3]
 *            points in the camera-1 frame; err f64[n,CPE_MAXP] per-point reprojection error;
 *            m i32[n] number of selected points; mean_err f64[n]; flags i32[n] (CPE_FIT_FLAG_*)
 *   ws       cpe_fit_workspace_bytes(n) bytes of device scratch (content on entry irrelevant: Conventions, "Workspaces")
 * cnt1 / cnt2 are clamped to [0, CPE_MAXP]; slots past them are never read.  The (col,row) indices of a frame (both
 * tables) go through a dense CPE_FIT_TABLE_DIM x CPE_FIT_TABLE_DIM table: a frame whose indices span CPE_FIT_TABLE_DIM
 * or more in either direction, or has an index outside [-9999, 9999], is skipped with CPE_FIT_FLAG_OVERFLOW, m = 0,
 * mean_err = 0 and nothing written to the per-point outputs (the reference has no such limit).  A (col,row) that occurs
 * more than once in a table is looked up through its first occurrence, as find() does in the reference.  An empty table on
 * either side gives m = 0 with no flag.
 */
CPE_API int32_t cpe_select_triangulate_batch(const double *xy1, const int32_t *id1, const int32_t *cnt1,
                                             const double *xy2, const int32_t *id2, const int32_t *cnt2, int32_t n,
                                             const double *K1, const double *K2, const double *T21, int32_t selector,
                                             int32_t patch, double th, void *ws, size_t ws_bytes, double *p1,
                                             double *p2, int32_t *idx, double *X, double *err, int32_t *m,
                                             double *mean_err, int32_t *flags, void *stream);

/* The two halves of the above on their own (SURVEY 8b lists them as separate entry points).
 * cpe_choose_idx_batch: [cgp1, cgp2] = chooseIdx(gp1, gp2, imgInfo, stereoParams, patch, th) (chooseIdx.m:1-105; call at
 *   fitSingleCylinder.m:12 with patch 3, th 0.3), fallback to findGridCorrespondences included (flags).  Outputs p1, p2, idx,
 *   m, flags as above; ws as above.
 * cpe_triangulate_batch: [worldPoints, reprojectionErrors] = triangulate(cgp1, cgp2, stereoParams) for pairs that are already
 *   matched, and meanError = mean(reprojectionErrors) (fitSingleCylinder.m:15-17).  p1, p2 f64[n,CPE_MAXP,2], cnt i32[n] ->
 *   X f64[n,CPE_MAXP,3] (camera-1 frame), err f64[n,CPE_MAXP], mean_err f64[n].  cnt is clamped to [0, CPE_MAXP]; mean_err of
 *   an empty frame is 0. */
CPE_API int32_t cpe_choose_idx_batch(const double *xy1, const int32_t *id1, const int32_t *cnt1, const double *xy2,
                                     const int32_t *id2, const int32_t *cnt2, int32_t n, const double *K1, const double *K2,
                                     const double *T21, int32_t patch, double th, void *ws, size_t ws_bytes, double *p1,
                                     double *p2, int32_t *idx, int32_t *m, int32_t *flags, void *stream);
CPE_API int32_t cpe_triangulate_batch(const double *p1, const double *p2, const int32_t *cnt, int32_t n, const double *K1,
                                      const double *K2, const double *T21, double *X, double *err, double *mean_err,
                                      void *stream);

typedef struct CpeFitParams {
    double tol_x;          /* fminsearch TolX  (fitCylinderWPts3.m:33: 1e-5) */
    double tol_f;          /* fminsearch TolFun (1e-5) */
    int32_t max_iter;      /* MaxIter (1e5) */
    int32_t max_fun_evals; /* MaxFunEvals (1e5) */
    int32_t mode;          /* CPE_FIT_NELDER_MEAD (reference behaviour, default) or CPE_FIT_LM */
    int32_t reserved;      /* 0 */
} CpeFitParams;
#define CPE_FIT_NELDER_MEAD 0 /* fminsearch clone: what fitCylinderWPts3.m:38 runs */
#define CPE_FIT_LM 1          /* Levenberg-Marquardt on the same objective (fast mode; not in the reference) */

/* fitCylinderWPts3(pts3, radius) + applyCylParamsPrior + cylParams2T for n frames, one wavefront per
 * frame (fitSingleCylinder.m:20-25).  X f64[n,CPE_MAXP,3], cnt i32[n].  params NULL = reference values.
 *   cyl_raw f64[n,2,6]  [cylParams0; cylParams] as returned by fitCylinderWPts3
 *   cyl     f64[n,2,6]  the same after applyCylParamsPrior
 *   T       f64[n,16]   row-major cylT = cylParams2T(cyl(2,:))
 *   fvals   f64[n,2]    [f0, f]        iters i32[n,2] = [iterations, function evaluations]
 *   status  i32[n]      CPE_ST_OK or CPE_ST_FEW_POINTS
 * cnt is clamped to [0, CPE_MAXP] (a count above CPE_MAXP fits the first CPE_MAXP points); slots past it are never read.
 * A frame ends in CPE_ST_FEW_POINTS, with every output of the frame zero, when it has fewer than CPE_FIT_MIN_POINTS points
 * -- the 5-coefficient quadric of estCurvatures is underdetermined there, and MATLAB's `A \ b` would return a rank-deficient
 * basic solution -- or when the initial or the final cylinder is not finite.  So CPE_ST_OK implies finite cyl_raw, cyl,
 * fvals and T.  The reference fits from 3 points on; this is a documented deviation.
 */
CPE_API int32_t cpe_fit_cylinder_batch(const double *X, const int32_t *cnt, int32_t n, double radius,
                                       const CpeFitParams *params, double *cyl_raw, double *cyl, double *T,
                                       double *fvals, int32_t *iters, int32_t *status, void *stream);

/* BUILD-DEFINED extension (BASELINE.json configs[4] "RANSAC-wrapped fitSingleCylinder"; the reference has no RANSAC):
 * per frame, `hypotheses` LM fits (`hyp_iters` iterations each) on random subsets -- hypothesis 0 = all points, the others
 * keep a point with probability sample / count, decided by a counter-based hash of (seed, frame0 + frame, hypothesis, point)
 * -- scored by the number of points with |dist(point, axis) - radius| < tau; the final fit (`params->mode`) runs on the
 * inliers of the best hypothesis.  Outputs as cpe_fit_cylinder_batch (cyl_raw row 0 = the all-points initial cylinder,
 * fvals[0] = objective there, fvals[1] = objective of the final fit over the inliers) plus
 *   n_inliers i32[n], inlier_mask u8[n,CPE_MAXP] (1 = used by the final fit; 0 for every slot >= the point count).
 * Counts and CPE_ST_FEW_POINTS as cpe_fit_cylinder_batch; such a frame also has n_inliers = 0 and an all-zero mask. */
typedef struct {
    int32_t hypotheses;   /* default 64 */
    int32_t sample;       /* expected subset size, default 12 (>= 6) */
    double tau;           /* inlier band around the radius, same unit as the points, default 0.5 */
    uint64_t seed;
    uint64_t frame0;      /* global index of frame 0 of this call (shards of one batch get different streams) */
    int32_t hyp_iters;    /* LM iterations per hypothesis, default 8 */
    int32_t reserved;
} CpeRansacParams;
CPE_API int32_t cpe_fit_cylinder_ransac_batch(const double *X, const int32_t *cnt, int32_t n, double radius,
                                              const CpeFitParams *params, const CpeRansacParams *ransac, double *cyl_raw,
                                              double *cyl, double *T, double *fvals, int32_t *iters, int32_t *status,
                                              int32_t *n_inliers, uint8_t *inlier_mask, void *stream);

/* BUILD-DEFINED extension (nothing like it in the reference): stereo matching that survives a grid-index shift between the
 * two images of a frame.  The selectors above pair points of equal (col,row); a detector that numbers one image a column or a
 * row off (a spot ellipse that cuts the centre column) leaves pairs that still pass the reprojection
 * test -- a column shift moves the partner along the epipolar line -- at a wrong depth.  This call searches the shift of
 * table 1 under which the triangulated points lie on a cylinder of the known radius, one wavefront per (frame, candidate).
 *
 * Score of the candidate (dc, dr), dc in [-win_c, win_c], dr in [-win_r, win_r] (the order is part of the contract):
 *   1. (dc, dr) is added to every index of table 1;
 *   2. plain index join with table 2 as findGridCorrespondences does: image-1 order, a duplicate index of table 2 is looked
 *      up through its first occurrence, every row of table 1 that finds a partner is a pair, no fallback;
 *   3. every pair is triangulated (the DLT of cpe_triangulate_batch);
 *   4. the pairs with err < th are kept, in join order;
 *   5. fewer than CPE_FIT_MIN_POINTS kept pairs: score 0;
 *   6. otherwise the initial cylinder of cpe_fit_cylinder_batch on the kept points and hyp_iters iterations of its
 *      CPE_FIT_LM mode (tolerances 1e-5); a non-finite initial or final cylinder: score 0;
 *   7. score = number of kept points with |dist(point, axis) - radius| < tau (the inlier test of
 *      cpe_fit_cylinder_ransac_batch).
 * Winner: the candidate with the smallest key (-score, |dc|+|dr|, |dc|, dc, dr), so (0,0) wins every tie it is part of.
 *
 *   inputs   the tables, K1, K2, T21 as cpe_select_triangulate_batch; radius as cpe_fit_cylinder_batch; params NULL = defaults
 *   ws       cpe_match_offset_workspace_bytes(n, win_c, win_r) bytes of device scratch, content on entry irrelevant (0 for a window outside
 *            0..CPE_MATCH_MAX_WIN)
 *   offset   i32[n,2]  the shift (dc, dr) applied to table 1
 *   score    i32[n,4]  best score | runner-up (the second-largest value among all candidates; 0 with a single candidate) |
 *                      score at (0,0) | pairs kept at the winner
 *   scores   i32[n,ncand] or NULL: every candidate, ncand = (2 win_c + 1)(2 win_r + 1), dc the outer index, dr the inner,
 *            both ascending
 *   flags    i32[n]    CPE_MATCH_FLAG_* (independent bits)
 *   id1_out  i32[n,CPE_MAXP,2]  id1 + offset in the slots below cnt1 (slots past it are not written); may not be id1.
 *            cpe_select_triangulate_batch and the fit read it in place of id1: the absolute numbering then follows image
 *            2, which is harmless because only the correspondence reaches the fit.
 * cnt1 / cnt2 are clamped to [0, CPE_MAXP]; slots past them are never read.  An empty table on either side scores 0
 * everywhere (offset (0,0), CPE_MATCH_FLAG_WEAK unless min_score is 0).  Table 2 goes through a dense CPE_FIT_TABLE_DIM x
 * CPE_FIT_TABLE_DIM table, built once per frame: a frame with two non-empty tables whose table 2 spans CPE_FIT_TABLE_DIM or
 * more in either direction, or that has an index outside [-9999, 9999] in either table -- a frame
 * cpe_select_triangulate_batch refuses too -- gets CPE_MATCH_FLAG_OVERFLOW, offset (0,0) and scores 0.
 * Limits: one shift per frame (a piecewise shift, such as a centre column split in two, recovers only its larger part);
 * cylinder target only (the planar target has no radius to score with).
 * Kernel launches on `stream` only (table, one scoring launch per size class of table 1, winner), no host synchronisation. */
#define CPE_MATCH_MAX_WIN 8
#define CPE_MATCH_FLAG_SHIFTED 1   /* a non-zero offset was chosen and applied */
#define CPE_MATCH_FLAG_WEAK 2      /* the best score is below min_score: the winner is not trusted, offset forced to (0,0) */
#define CPE_MATCH_FLAG_EDGE 4      /* the winner lies on the border of a non-zero window: the true shift may lie outside
                                      (the offset is still applied unless the frame is also WEAK) */
#define CPE_MATCH_FLAG_OVERFLOW 8  /* an index the dense table cannot hold (see above): offset (0,0), scores 0 */
typedef struct CpeMatchParams {
    int32_t win_c, win_r;   /* candidates dc in [-win_c, win_c], dr in [-win_r, win_r]; 0..CPE_MATCH_MAX_WIN; default 4, 4 */
    double th;              /* reprojection error a pair must stay under, px; default 0.3 (fitSingleCylinder.m:12) */
    double tau;             /* inlier band |dist - radius| < tau, the unit of the points; default 0.5 (CpeRansacParams) */
    int32_t hyp_iters;      /* LM iterations per candidate, 1..200; default 8 (CpeRansacParams) */
    int32_t min_score;      /* a winner below this is not trusted (>= 0); default 8 */
} CpeMatchParams;
CPE_API size_t cpe_match_offset_workspace_bytes(int32_t n, int32_t win_c, int32_t win_r);
CPE_API int32_t cpe_match_offset_batch(const double *xy1, const int32_t *id1, const int32_t *cnt1, const double *xy2,
                                       const int32_t *id2, const int32_t *cnt2, int32_t n, const double *K1, const double *K2,
                                       const double *T21, double radius, const CpeMatchParams *params, void *ws, size_t ws_bytes,
                                       int32_t *offset, int32_t *score, int32_t *scores, int32_t *flags, int32_t *id1_out,
                                       void *stream);

/* BUILD-DEFINED, the geometric half of the planar target (CPE_TARGET_PLANE): the plane of a flat board per frame, the grid
 * the projector draws on it, and the board's pose.  One wavefront per frame.  The plane is fitplane.m:1-16 -- cov(pts'), eig,
 * normal V(:,1), P = [n, -mean(n*pts)] -- everything else is build-defined.
 *   X f64[n,CPE_MAXP,3], idx i32[n,CPE_MAXP,2], cnt i32[n] as cpe_select_triangulate_batch writes them (the two components
 *   of idx are called a and b here: which of them is "col" is never interpreted); params NULL = {tau 0, max_rounds 4}.
 * Rule (the order is the contract):
 *   1. a point with a non-finite coordinate is never used;
 *   2. round 0 fits all usable points: centroid, then the centred covariance / (N - 1) in a second pass, eigenvalues
 *      ascending; n = first eigenvector with n_z > 0 (n_z == 0: the first non-zero component positive, DESIGN.md section 2,
 *      deviation 2); P = [n, -n.centroid];
 *   3. tau > 0: the inliers of the last plane are the usable points with |n.X + P4| < tau; when they are the set the last plane
 *      was fitted to, or after max_rounds refits, the loop ends, otherwise the plane is refitted to them.  tau <= 0: fitplane;
 *   4. a fit to fewer than 3 points, or with lambda_mid <= 1e-12 lambda_max (collinear, coincident), ends the frame:
 *      CPE_ST_FEW_POINTS and every output of the frame zero.  So CPE_ST_OK implies finite outputs;
 *   5. grid map over the points of the last fit: least squares X ~ O + a U + b V, indices and points centred first, the 2 x 2
 *      normal equations solved by elimination; Saa Sbb - Sab^2 <= 1e-12 Saa Sbb (all indices on one line): CPE_PLANEFIT_NO_GRID,
 *      grid and its rms zero;
 *   6. pose T (board frame -> camera 1, as cylT): z = n; x = normalise(U - (U.n) n), U = [1,0,0] under NO_GRID (cylParams2T.m),
 *      [0,1,0] should that leave nothing; y = z x x; origin = the first point of the last fit, in table order, with index
 *      (0,0), projected onto the plane (CPE_PLANEFIT_ORIGIN_POINT), else O projected onto the plane, else (NO_GRID) the centroid.
 * Outputs: P f64[n,4]; T f64[n,16] row-major; grid f64[n,9] = O U V; stats f64[n,8] = plane rms (sqrt of the mean squared
 *   distance), max |distance|, the three eigenvalues ascending, grid-map rms (sqrt of the mean squared 3-D misfit), refits done, 0
 *   -- all over the points of the last fit; n_inliers i32[n] their number; inlier_mask u8[n,CPE_MAXP] 1 on them, 0 elsewhere and
 *   past the count; flags i32[n] CPE_PLANEFIT_*; status i32[n].
 * cnt is clamped to [0, CPE_MAXP]; slots past it are never read.  One launch on `stream`, no host synchronisation. */
#define CPE_PLANEFIT_NO_GRID 1        /* bits of `flags` */
#define CPE_PLANEFIT_ORIGIN_POINT 2
#define CPE_PLANEFIT_MAX_ROUNDS 64
typedef struct CpePlaneFitParams {
    double tau;           /* inlier band |n.X + P4| < tau, the unit of the points; <= 0: no trimming (default) */
    int32_t max_rounds;   /* refits at the most, 0..CPE_PLANEFIT_MAX_ROUNDS; default 4 */
    int32_t reserved;     /* 0 */
} CpePlaneFitParams;
CPE_API int32_t cpe_fit_plane_batch(const double *X, const int32_t *idx, const int32_t *cnt, int32_t n,
                                    const CpePlaneFitParams *params, double *P, double *T, double *grid, double *stats,
                                    int32_t *n_inliers, uint8_t *inlier_mask, int32_t *flags, int32_t *status, void *stream);

/* BUILD-DEFINED: the laser planes of the projector from several board poses.  A grid line of fixed index is a plane of light
 * through the projector; the points that carry the index in several frames determine it, and all planes together the
 * projector's centre.  One wavefront per (family k, index v): family k in {0,1} is component k of idx, v in [lo, hi],
 * L = hi - lo + 1 in 1..CPE_MAXL (otherwise CPE_ERR_ARG).
 *   X, idx, cnt as above; use u8[n,CPE_MAXP] or NULL (all points; the inlier_mask above); frame_ok i32[n] or NULL (non-zero =
 *   the frame is kept); min_spread >= 0 (1e-4 is a good value).
 * The wavefront walks the kept frames and takes the usable (finite, `use`) points with idx[k] == v: centroid, centred
 * covariance / (N - 1) in a second pass, n = first eigenvector with its largest-magnitude component (the first of them)
 * positive (MATLAB pca's sign rule), P = [n, -n.centroid].
 *   P f64[2,L,4]; stats f64[2,L,4] = rms, max |distance|, lambda_mid / lambda_max, 0; count i32[2,L] points; frames i32[2,L]
 *   kept frames that contributed; status i32[2,L]: CPE_ST_FEW_POINTS, with the line's P and stats zero (count and frames
 *   stay), for fewer than 3 points, fewer than 2 frames (one pose gives a straight line), lambda_max <= 0 or
 *   lambda_mid / lambda_max < min_spread.
 * A last wavefront (second launch) solves the 3 x 3 normal equations of the point C minimising sum (n_k.C + P4_k)^2 over the
 * OK lines of both families: centre f64[4] = C, rms; centre_status i32[1] = CPE_ST_FEW_POINTS (centre zero) when either family
 * has fewer than 2 OK lines or the elimination meets a zero pivot.
 * cnt is clamped to [0, CPE_MAXP]; slots past it are never read; n = 0 is allowed (every line CPE_ST_FEW_POINTS). */
CPE_API int32_t cpe_index_planes_batch(const double *X, const int32_t *idx, const int32_t *cnt, int32_t n, const uint8_t *use,
                                       const int32_t *frame_ok, int32_t lo, int32_t hi, double min_spread, double *P,
                                       double *stats, int32_t *count, int32_t *frames, int32_t *status, double *centre,
                                       int32_t *centre_status, void *stream);

/* BUILD-DEFINED: the projector as a model, fitted to the points of many frames -- board poses, or the stereo points of the
 * cylinder experiment itself.  A diffractive grid projector sends out two pencils of planes through one centre C: the plane of
 * index v of family k has the normal n = a_k + v b_k and holds C.  The model is x = C[3], a_0[3], b_0[3], a_1[3], b_1[3] (15
 * doubles, |a_k| = 1: 13 degrees of freedom in place of the 2 L 3 of cpe_index_planes_batch), so it also gives planes for
 * indices that no frame showed, and a frame whose lines are numbered one off cannot pull a line's plane away.
 *   X, idx, cnt, use, frame_ok, lo, hi: as cpe_index_planes_batch (L = hi - lo + 1 in 1..CPE_MAXL, otherwise CPE_ERR_ARG);
 *   params NULL = the defaults of CpeProjectorModelParams; x0 f64[15] DEVICE memory or NULL: the start of round 0 (|a_k| = 1).
 * Rule (the order is the contract):
 *   1. a point is usable when its frame is kept, its slot is below the clamped count, `use` is non-zero and its coordinates are
 *      finite.  It gives one residual per family k whose index v = idx[k] lies in [lo, hi]:  r = n.(X - C) / |n|;
 *   2. moments pass, one wavefront per (family, index): over the kept residuals of the line the count N, the centroid m, then in
 *      a second pass the centred scatter S = sum (X - m)(X - m)'.  Round 0 keeps every residual of step 1; from round 1 on a
 *      residual is kept when |r| < tau under the model of the round before.  sum r^2 = nh'(S + N (m - C)(m - C)') nh, and J'J,
 *      J'r follow from N, m, S as well: the solve never sees a point;
 *   3. a line is usable for the start when N >= 3, >= 2 frames contributed, lambda_max > 0 and lambda_mid / lambda_max >=
 *      min_spread of S; its free plane has the normal n_l = the first eigenvector of S.  Fewer than 2 usable lines in either
 *      family: CPE_ST_FEW_POINTS (every round checks this);
 *   4. start of round 0 (x0 NULL): C solves (sum n_l n_l') C = sum n_l (n_l.m_l) over the usable lines of both families by
 *      elimination (a zero pivot or a non-finite C: CPE_ST_FEW_POINTS).  Per family: u = the first eigenvector of sum n_l n_l';
 *      e1 = the normal of the usable line nearest to v = 0 (the lower index on a tie), its largest-magnitude component positive,
 *      with its part along u removed, normalised; e2 = u x e1; least squares (n_l.e2) / (n_l.e1) ~ alpha + beta v over the usable
 *      lines, v centred; a = (e1 + alpha e2) / |e1 + alpha e2|, b = beta e2 / |e1 + alpha e2|.  A later round starts from the
 *      model of the round before;
 *   5. Levenberg-Marquardt on sum r^2 over all kept residuals (the loop of the cylinder fit: lambda 1e-3, x 10 / 10, at most 12
 *      trials per iteration and min(maxiter, 200) iterations, stop on a step <= tolx that gains <= tolf 1e-3 (1 + f)); a step is
 *      dC, then per family two coordinates in the tangent plane of a_k (basis: the coordinate axis of the smallest |a_i|, the
 *      first of them, made perpendicular to a_k and normalised, and a_k x that) and db_k; a_k is brought back to length 1;
 *   6. tau > 0 and max_rounds > 0: round r = 1, 2, ... builds the mask of step 2 under the last model; when no byte of it
 *      differs from the mask the last model was fitted to, or after max_rounds refits, the loop ends; otherwise the model is
 *      refitted to the new moments.  All rounds are enqueued at once; the kernels of a round return at once when the loop has
 *      ended.  No host synchronisation, no floating-point atomics; two calls on the same inputs give the same bits;
 *   7. a non-finite start, objective or result: CPE_ST_FEW_POINTS.  With that status model is zero (moments, count, frames,
 *      inlier_mask and frame_counts describe the last moments pass all the same).  So CPE_ST_OK implies finite outputs.
 * Outputs:
 *   model f64[16]            x, then the objective sum r^2 over the kept residuals
 *   info i32[8]              status, refits done, LM iterations and objective evaluations over all rounds, kept residuals of
 *                            family 0 and of family 1, 0, 0 (the last two carry the loop's flags while the call runs)
 *   moments f64[2,L,12]      N, m[3], S = xx xy xz yy yz zz, the line's rms sqrt(sum r^2 / N) under the final model (0 for an empty
 *                            line or a failed fit), 0
 *   count, frames i32[2,L]   kept residuals of the line, kept frames that contributed one
 *   inlier_mask u8[2,n,CPE_MAXP]   plane k: 1 where the point's residual of family k is kept, 0 elsewhere and past the count
 *   frame_counts i32[n,4]    per frame: kept and trimmed residuals of family 0, kept and trimmed residuals of family 1
 * cnt is clamped to [0, CPE_MAXP]; slots past it are never read; n = 0 is allowed (CPE_ST_FEW_POINTS).
 * Limits: the spacing of a pencil is linear in tan(theta) -- no distortion term for real gratings; one tau for both families;
 * a frame that is mis-numbered in both images alike is trimmed, not re-numbered (cpe_index_shift_batch re-numbers it against
 * this model's table, and a second call fits the frames so repaired). */
typedef struct CpeProjectorModelParams {
    double tau;           /* band |r| < tau of the trimming rounds, the unit of the points; <= 0: no trimming (default) */
    int32_t max_rounds;   /* refits at the most, 0..CPE_PLANEFIT_MAX_ROUNDS; default 4 */
    int32_t maxiter;      /* LM iterations per round at the most (200 at the most); default 100 */
    double min_spread;    /* a line's lambda_mid / lambda_max for the start; default 1e-4 */
    double tolx, tolf;    /* LM's stop; default 1e-9 each */
} CpeProjectorModelParams;
CPE_API int32_t cpe_fit_projector_model(const double *X, const int32_t *idx, const int32_t *cnt, int32_t n, const uint8_t *use,
                                        const int32_t *frame_ok, int32_t lo, int32_t hi, const CpeProjectorModelParams *params,
                                        const double *x0, double *model, int32_t *info, double *moments, int32_t *count,
                                        int32_t *frames, uint8_t *inlier_mask, int32_t *frame_counts, void *stream);

/* The laser-plane table of a model for ANY index range lo..hi (L in 1..CPE_MAXL, otherwise CPE_ERR_ARG), in the layout
 * cpe_table_triangulate_batch reads.  model, info: what cpe_fit_projector_model wrote (device memory).
 *   P f64[2,L,4] = [nh, -nh.C], nh = (a_k + v b_k) / |a_k + v b_k| with its largest-magnitude component (the first of them)
 *   positive, the sign rule of cpe_index_planes_batch; status i32[2,L] CPE_ST_OK; centre f64[4] = C, sqrt(objective / kept
 *   residuals); centre_status i32[1].  A model whose status is not CPE_ST_OK, or a line with a zero or non-finite normal, gives
 *   CPE_ST_FEW_POINTS and zeros. */
CPE_API int32_t cpe_projector_model_table(const double *model, const int32_t *info, int32_t lo, int32_t hi, double *P, int32_t *status,
                                          double *centre, int32_t *centre_status, void *stream);

/* BUILD-DEFINED: 3-D points from ONE camera and the laser-plane table.  A grid point with the indices (id[0], id[1]) lies on the
 * plane of light of either index, so it is the cut of its pixel ray with those planes: no stereo partner and no index matching.
 * One wavefront per frame, rounds of 64 points, one launch, no atomics, no workspace, no host synchronisation.
 *   xy f64[n,CPE_MAXP,2], id i32[n,CPE_MAXP,2], cnt i32[n]: the grid-point tables of one camera (cpe_detect_grid_batch)
 *   K f64[9] row-major, Tc f64[16] row-major or NULL: DEVICE memory; Tc maps camera-1 coordinates (the table's) to this
 *     camera's: NULL = identity (camera 1), T_C2_C1 for camera 2.  R, t below are its rotation and translation
 *   P f64[2,L,4], line_status i32[2,L], lo, hi: exactly what cpe_index_planes_batch wrote; L = hi - lo + 1 in 1..CPE_MAXL
 *     (otherwise CPE_ERR_ARG)
 *   params NULL = the defaults of CpeTableTriParams
 * The order is the contract; per point of the table, in table order:
 *   1. cnt is clamped to [0, CPE_MAXP]; slots past it are never read.  A point with a non-finite pixel coordinate is refused;
 *   2. ray in camera-1 coordinates: o = -R't; vy = (y - K[5]) / K[4]; vx = (x - K[2] - K[1] vy) / K[0]; d = R'(vx, vy, 1),
 *      normalised;
 *   3. component c in {0,1} of id addresses family k = c ^ swap with v = id[c]; the plane [n_k, P4_k] = P[k, v - lo] is usable
 *      when lo <= v <= hi and line_status[k, v - lo] == CPE_ST_OK; then a_k = n_k.d and b_k = n_k.o + P4_k;
 *   4. no usable plane, or only one with need_both: refused (counts[2]);
 *   5. den = sum a_k^2 over the usable planes; den < min_sin^2, or den not finite: refused (counts[2]).  An error of a plane's
 *      offset reaches the depth multiplied by 1 / sin of the angle between ray and plane: at the default 0.01 the table's
 *      0.02 - 0.2 mm plane rms becomes 2 - 20 mm;
 *   6. s = -sum a_k b_k / den; s <= 0 or not finite: refused (counts[3]); X = o + s d.  The point lies on the ray exactly; with
 *      two planes it is the point of the ray with the least sum of squared distances to both;
 *   7. res[c] = n_k.X + P4_k for a used plane, 0 for an unused one (c is the component, not the family); max_res > 0 and a used
 *      |res[c]| > max_res: refused (counts[3]);
 *   8. accepted points go, in table order, to slots 0..m-1 of X f64[n,CPE_MAXP,3], idx i32[n,CPE_MAXP,2] (a copy of id), res
 *      f64[n,CPE_MAXP,2] and src i32[n,CPE_MAXP,2]: src[0] bit 0 = the plane of component 0 was used, bit 1 = component 1's;
 *      src[1] = the point's slot in the input table.  Slots from m on are NOT written;
 *   9. m i32[n]; counts i32[n,4] = m, points with both planes, refused in steps 1/4/5, refused in steps 6/7; stats f64[n,2] =
 *      sqrt of the mean squared res over the used planes of the accepted points, max |res|; both 0 when m = 0.
 * The outputs may not overlap the inputs.  n == 0 is a no-op. */
typedef struct CpeTableTriParams {
    int32_t swap;       /* 0: id component c addresses table family c; 1: component c addresses family 1 - c */
    int32_t need_both;  /* 1: a point needs both of its planes; 0 (default): one usable plane is enough */
    double  min_sin;    /* a point whose usable planes give sum a_k^2 < min_sin^2 is refused; >= 0, default 0.01 */
    double  max_res;    /* > 0: refuse a point with |res| > max_res on any used plane; <= 0 (default): no gate */
} CpeTableTriParams;
CPE_API int32_t cpe_table_triangulate_batch(const double *xy, const int32_t *id, const int32_t *cnt, int32_t n, const double *K,
                                            const double *Tc, const double *P, const int32_t *line_status, int32_t lo, int32_t hi,
                                            const CpeTableTriParams *params, double *X, int32_t *idx, double *res, int32_t *src,
                                            int32_t *m, int32_t *counts, double *stats, void *stream);

/* BUILD-DEFINED, opt-in: FUSED 3-D points.  The projector is a third view: a grid point seen by both cameras on two known
 * planes of light has 2 + 2 + 2 constraints on its 3 unknowns, a point seen by one camera still 4.  This call uses all of them:
 * every grid point of either table becomes a candidate, not only the pairs a selector kept, and every point carries a
 * three-view residual.  One wavefront per frame, one launch, no atomics, no workspace, no host synchronisation; two calls on the
 * same inputs give the same bits.
 *   xy1, id1, cnt1, xy2, id2, cnt2, K1, K2, T21: as cpe_select_triangulate_batch (K1, K2, T21 in DEVICE memory)
 *   P f64[2,L,4], line_status i32[2,L], lo, hi: exactly what cpe_table_triangulate_batch reads; L = hi - lo + 1 in 1..CPE_MAXL
 *     (otherwise CPE_ERR_ARG)
 *   params NULL = the defaults of CpeFusedTriParams
 * Rule (the order is the contract):
 *   1. cnt1, cnt2 are clamped to [0, CPE_MAXP]; slots past them are never read.  With both tables non-empty the indices of both
 *      go through a dense CPE_FIT_TABLE_DIM x CPE_FIT_TABLE_DIM table, and a frame that fails the limits of
 *      cpe_select_triangulate_batch (a span >= CPE_FIT_TABLE_DIM in either direction, or an |index| > 9999) is skipped with
 *      CPE_FIT_FLAG_OVERFLOW, m = 0, counts and stats 0 and nothing written to the per-point outputs.  A frame with an empty
 *      table needs no join and has no such limit: an index may be any int, as in cpe_table_triangulate_batch;
 *   2. join by equal (id[0], id[1]), as CPE_SEL_JOIN does: an entry of table 1 pairs with the FIRST entry of table 2 that has its
 *      index; later duplicates of table 1 pair with the same partner (findGridCorrespondences).  An entry of table 2 is "taken"
 *      when any entry of table 1 paired with it; a later duplicate in table 2 is never taken;
 *   3. candidates, in this order: every entry of table 1 in table order, paired or left-only; then every untaken entry of table 2
 *      in table order, right-only.  A candidate with a non-finite pixel coordinate in a ray it would use is refused;
 *   4. rays (o_j, d_j): step 2 of cpe_table_triangulate_batch with Tc = NULL for camera 1 and Tc = T21 for camera 2.  Planes:
 *      step 3 of that rule, from the candidate's own index (a pair has one index);
 *   5. start point X0.  Paired: the unweighted least-squares point of the two rays, sum_j (I - d_j d_j')(X0 - o_j) = 0, by
 *      Gaussian elimination with partial pivoting; a zero pivot is refused.  One ray: steps 4 - 7 of
 *      cpe_table_triangulate_batch (need_both, min_sin, s > 0 and the max_res gate included), by the same device function, so
 *      the same bits; that point is also the final point, and steps 6 and 7 below do not apply to it;
 *   6. paired only: s_j = (X0 - o_j).d_j; s_j <= 0 or not finite: refused.  w_j = K_j[0] / (s_j sigma_px): a pixel of sigma_px at
 *      the depth s_j, as a distance from the ray; w_p = 1 / sigma_mm for each usable plane.  A pair needs no plane (need_both and
 *      min_sin are for one-ray candidates).  One solve, no iteration:
 *        [sum_j w_j^2 (I - d_j d_j') + sum_k w_p^2 n_k n_k'] X = sum_j w_j^2 (I - d_j d_j') o_j - sum_k w_p^2 P4_k n_k;
 *      a zero pivot or a non-finite X is refused;
 *   7. residuals of a pair: res[0], res[1] = the distance of X from ray 1, ray 2 times K_j[0] / s_j, s_j = (X - o_j).d_j
 *      (pixels); res[2], res[3] = n_k.X + P4_k of the plane of component 0, 1 (mm), 0 for an unused plane.  A residual that is
 *      not finite, or a ray residual below 0 (X behind that camera), refuses the pair, so no NaN is written.  max_px > 0 and a ray
 *      residual > max_px, or max_res > 0 and a used |plane residual| > max_res: refused.  A one-ray point lies on its ray: its
 *      res[0], res[1] are 0 and max_px does not apply; res[2], res[3] are the res of cpe_table_triangulate_batch;
 *   8. accepted candidates go, in candidate order, to slots 0..m-1 of X f64[n,CPE_MAXP,3], idx i32[n,CPE_MAXP,2] (the
 *      candidate's index), res f64[n,CPE_MAXP,4] and src i32[n,CPE_MAXP,3]: src[0] bit 0 = ray 1 used, bit 1 = ray 2, bit 2 = the
 *      plane of component 0, bit 3 = the plane of component 1; src[1] = the slot in table 1 or -1; src[2] = the slot in table 2
 *      or -1.  Slots from m on are NOT written.  Accepted candidates past CPE_MAXP are dropped, counted in counts[5], and the
 *      frame gets CPE_FUSED_FLAG_TRUNCATED;
 *   9. m i32[n]; counts i32[n,6] = m | written pairs | written left-only | written right-only | refused candidates | truncated;
 *      stats f64[n,4] = rms | max of the ray residuals of the written pairs (pixels; two per pair), rms | max |.| of the plane
 *      residuals over the used planes of the written points (mm); each pair of them is 0 without such a constraint;
 *      flags i32[n] = CPE_FIT_FLAG_OVERFLOW | CPE_FUSED_FLAG_TRUNCATED.
 * The outputs may not overlap the inputs.  n == 0 is a no-op.
 * Limits: the weights come from the one start point, there is no reweighting; one sigma_mm for the whole table; the points
 * inherit the table's errors; the call does not re-number: a mis-numbered frame is repaired first (cpe_match_offset_batch between
 * the images, cpe_index_shift_batch against the table). */
#define CPE_FUSED_FLAG_TRUNCATED 4 /* more than CPE_MAXP candidates were accepted: the last ones are dropped (counts[5]) */
typedef struct CpeFusedTriParams {
    int32_t swap;       /* as in CpeTableTriParams */
    int32_t need_both;  /* as in CpeTableTriParams: one-ray candidates only */
    double  min_sin;    /* as in CpeTableTriParams, default 0.01: one-ray candidates only */
    double  sigma_px;   /* standard deviation of a pixel coordinate, > 0, default 0.25 */
    double  sigma_mm;   /* standard deviation of a point's distance from a plane of the table, > 0, default 0.02 */
    double  max_res;    /* mm; > 0: refuse a candidate with a used |plane residual| above it; <= 0 (default): no gate */
    double  max_px;     /* px; > 0: refuse a pair with a ray residual above it; <= 0 (default): no gate */
} CpeFusedTriParams;
CPE_API int32_t cpe_fused_triangulate_batch(const double *xy1, const int32_t *id1, const int32_t *cnt1, const double *xy2,
                                            const int32_t *id2, const int32_t *cnt2, int32_t n, const double *K1, const double *K2,
                                            const double *T21, const double *P, const int32_t *line_status, int32_t lo, int32_t hi,
                                            const CpeFusedTriParams *params, double *X, int32_t *idx, double *res, int32_t *src,
                                            int32_t *m, int32_t *counts, double *stats, int32_t *flags, void *stream);

/* BUILD-DEFINED: re-number STEREO frames against a laser-plane table.  cpe_match_offset_batch makes the two images of a frame
 * agree with each other; a frame that is then numbered a line off in both images alike carries indices that mean other planes
 * than in the rest of the experiment.  A stereo point's position does not depend on its index, so the frame's points and any
 * table that is right for the majority of the frames -- cpe_projector_model_table of a model fitted with tau > 0, or a table from
 * boards -- determine the frame's shift: per index component, the d for which the most points lie on the plane of index + d.
 * One wavefront per (frame, component), one launch on `stream`, no workspace, no atomics, no host synchronisation; two calls on
 * the same inputs give the same bits.
 *   X f64[n,CPE_MAXP,3], idx i32[n,CPE_MAXP,2], cnt i32[n]: as cpe_select_triangulate_batch writes them; use u8[n,CPE_MAXP] or
 *   NULL (all points); P f64[2,L,4], line_status i32[2,L], lo, hi: a table as cpe_index_planes_batch or
 *   cpe_projector_model_table writes it, L = hi - lo + 1 in 1..CPE_MAXL (otherwise CPE_ERR_ARG); params NULL = the defaults of
 *   CpeIndexShiftParams.
 * Rule (the order is the contract):
 *   1. cnt is clamped to [0, CPE_MAXP]; slots past it are never read.  A point is usable when its slot is below the count, `use`
 *      is non-zero and its three coordinates are finite;
 *   2. component c in {0,1} of idx addresses family k = c ^ swap.  For the candidate d in [-win[c], win[c]] a usable point with
 *      v = idx[c] + d counts when lo <= v <= hi, line_status[k, v - lo] == CPE_ST_OK and |n.X + P4| < tau for the plane
 *      P[k, v - lo].  A point whose idx[c] lies outside [lo - win[c], hi + win[c]] counts for no candidate: that test is made
 *      before any addition, so an index may be any int;
 *   3. score(c, d) = the number of such points.  Winner: the candidate with the smallest key (-score, |d|, d), so 0 wins every
 *      tie it is part of;
 *   4. the component is trusted when best >= min_score and best >= 2 runner_up (integers), runner_up = the second-largest value
 *      among the component's candidates (0 with a single candidate).  Otherwise CPE_SHIFT_FLAG_WEAK and the shift is 0;
 *   5. CPE_SHIFT_FLAG_EDGE when |winner| == win[c] > 0; CPE_SHIFT_FLAG_SHIFTED when a non-zero shift was applied;
 *   6. score i32[n,2,4] = best | runner-up | score at d = 0 | usable points;
 *   7. rms f64[n,2,2] = sqrt of the mean squared n.X + P4 over the points that count, at the applied shift | at d = 0; 0 when
 *      none counts;
 *   8. scores i32[n, 2 win[0] + 1 + 2 win[1] + 1] or NULL: every candidate, component 0 first, d ascending;
 *   9. idx_out i32[n,CPE_MAXP,2] = idx + the applied shift in the slots below the count (a sum past int32 wraps); slots past it
 *      are not written; may not be idx.
 * shift i32[n,2] the applied shift per component; flags i32[n,2] CPE_SHIFT_FLAG_* (independent bits).  n == 0 is a no-op.  A
 * frame without a usable point scores 0 everywhere: shift 0, and CPE_SHIFT_FLAG_WEAK unless min_score is 0.
 * Limits: the shift is relative to the majority of the frames -- a shift common to all frames is absorbed by the model the
 * table comes from; one shift per frame and family; stereo points only: a point of cpe_table_triangulate_batch cut with ONE
 * plane moves with its index, so it lies on the plane of whatever index it carries.  Cut with both planes it is one ray against
 * two planes, over-determined by one, and its res says whether the pair of indices is right: that is what
 * cpe_mono_shift_batch searches. */
#define CPE_SHIFT_MAX_WIN 8
#define CPE_SHIFT_FLAG_SHIFTED 1   /* a non-zero shift was chosen and applied */
#define CPE_SHIFT_FLAG_WEAK 2      /* best < min_score or best < 2 runner-up: the winner is not trusted, shift forced to 0 */
#define CPE_SHIFT_FLAG_EDGE 4      /* the winner lies on the border of a non-zero window: the true shift may lie outside (the
                                      shift is still applied unless the component is also WEAK) */
typedef struct CpeIndexShiftParams {
    int32_t win[2];     /* candidates d in [-win[c], win[c]] for id component c; 0..CPE_SHIFT_MAX_WIN; default 4, 4 */
    double  tau;        /* a point counts when |n.X + P4| < tau, the unit of the points; > 0; default 1.0 */
    int32_t min_score;  /* a winner below this is not trusted (>= 0); default 8 */
    int32_t swap;       /* as CpeTableTriParams.swap: component c addresses family c ^ swap */
} CpeIndexShiftParams;
CPE_API int32_t cpe_index_shift_batch(const double *X, const int32_t *idx, const int32_t *cnt, int32_t n, const uint8_t *use,
                                      const double *P, const int32_t *line_status, int32_t lo, int32_t hi,
                                      const CpeIndexShiftParams *params, int32_t *shift, int32_t *score, int32_t *scores, double *rms,
                                      int32_t *flags, int32_t *idx_out, void *stream);

/* BUILD-DEFINED, opt-in: the grid-index shift of ONE-CAMERA frames against a laser-plane table.  A grid point of one camera is one
 * ray cut with the two planes of light its indices name: three unknowns, four constraints.  The two residuals res of
 * cpe_table_triangulate_batch therefore measure the inconsistency of the index PAIR, and a frame numbered (d0, d1) off as a
 * whole shows it: per candidate shift, the points whose two residuals both stay below tau vote.  The call searches, ranks and
 * reports; it applies nothing.  Two launches on `stream` (one wavefront per (frame, d0), then one per frame), no atomics, no
 * workspace, no host synchronisation; two calls on the same inputs give the same bits.
 *   xy f64[n,CPE_MAXP,2], id i32[n,CPE_MAXP,2], cnt i32[n]; K, Tc (NULL = camera 1), P f64[2,L,4], line_status i32[2,L], lo, hi:
 *     exactly as cpe_table_triangulate_batch reads them; L = hi - lo + 1 in 1..CPE_MAXL (otherwise CPE_ERR_ARG)
 *   win0, win1: candidates d_c in [-win_c, win_c] for id component c, 0..CPE_SHIFT_MAX_WIN (the Python layer's default 4, 4);
 *   tau: a point counts when both |res| < tau (mm), > 0 (0.1); min_sin: as CpeTableTriParams.min_sin, >= 0 (0.01); min_score: a
 *   best count below this is CPE_SHIFT_FLAG_WEAK, >= 0 (8); swap: as CpeTableTriParams.swap, component c addresses family
 *   c ^ swap; top_k: candidates reported in cand / cand_score, 1..8 (4).  They travel as plain arguments: there are no defaults
 *   on this side of the boundary
 * Rule (the order is the contract):
 *   1. cnt is clamped to [0, CPE_MAXP]; slots past it are never read.  A point is usable when its slot is below the count and both
 *      pixel coordinates are finite.  Its ray is step 2 of cpe_table_triangulate_batch;
 *   2. candidates d = (d0, d1) with |d_c| <= win_c.  Component c in {0,1} of id addresses family k = c ^ swap with
 *      v = id[c] + d_c; the plane is usable when lo <= v <= hi and line_status[k, v - lo] == CPE_ST_OK.  A point with an id[c]
 *      outside [lo - win_c, hi + win_c] counts for no candidate: that test is made before any addition, so an index may be any
 *      int.  Both planes must be usable: with one plane there is no redundancy;
 *   3. a_k, b_k, den = a_0^2 + a_1^2 >= min_sin^2 and finite, s = -sum a_k b_k / den > 0 and finite, X = o + s d and
 *      res[c] = n_k.X + P4_k are steps 3 - 7 of cpe_table_triangulate_batch with need_both and no max_res gate, by the same device
 *      function, so the same bits.  The point counts for d when |res[0]| < tau and |res[1]| < tau;
 *   4. scores i32[n, (2 win0 + 1)(2 win1 + 1)] (required): the count of every candidate, d0-major, both ascending;
 *   5. the candidates are ranked by the key (-score, |d0| + |d1|, |d0|, d0, d1), the smallest first, so (0, 0) wins every tie it is
 *      part of.  cand i32[n,top_k,2] and cand_score i32[n,top_k]: the first top_k of that order; slots past the number of
 *      candidates hold (0, 0) and -1.
 *      score i32[n,4] = best | runner-up (the second of that order; 0 with a single candidate) | at (0, 0) | usable points;
 *      rms f64[n,2] = sqrt((sum of res[0]^2 + res[1]^2 over the counting points) / their number) at the best candidate | at
 *      (0, 0); 0 when none counts;
 *      flags i32[n]: CPE_SHIFT_FLAG_EDGE when the best candidate has |d_c| == win_c > 0 for either c; CPE_SHIFT_FLAG_WEAK when
 *      best < min_score or best < 2 runner-up (integers).  CPE_SHIFT_FLAG_SHIFTED is never set:
 *   6. nothing is applied.  The caller adds a candidate to id and calls cpe_table_triangulate_batch.
 * No output may overlap an input or another output (CPE_ERR_ARG).  n == 0 is a no-op.  A window outside 0..CPE_SHIFT_MAX_WIN,
 * tau <= 0 or NaN, min_sin < 0, min_score < 0, swap other than 0 / 1 and top_k outside 1..8 are refused with CPE_ERR_ARG before
 * anything is written.
 * Limits: one shift per frame; tau must lie above the residuals that the table's errors and the pixel noise leave at the true
 * indices and below those of a wrong pair (at most 0.089 mm; at least 0.43 mm rms on the frames of tests/mono_shift_cases.py):
 * a table worse than that gives CPE_SHIFT_FLAG_WEAK, not a wrong shift.  One alias remains: a shift along the epipolar direction of projector and camera keeps
 * both residuals small for most points while it moves them far in depth; votes do not always tell it from the true shift, the
 * fixed-radius cylinder fit does (fit.fit_single_cylinder_mono_repaired_batch), and a board has no such second criterion. */
CPE_API int32_t cpe_mono_shift_batch(const double *xy, const int32_t *id, const int32_t *cnt, int32_t n, const double *K,
                                     const double *Tc, const double *P, const int32_t *line_status, int32_t lo, int32_t hi,
                                     int32_t win0, int32_t win1, double tau, double min_sin, int32_t min_score, int32_t swap,
                                     int32_t top_k, int32_t *scores, int32_t *cand, int32_t *cand_score,
                                     int32_t *score, double *rms, int32_t *flags, void *stream);

/* BUILD-DEFINED: re-label the grid lines of PLANAR-target tables from their geometry, per image.  The planar detector's labels
 * group the grid points into true lines, but their VALUES are not the lines' indices: on rendered boards one image comes out
 * reflected, the other permuted, with phantom lines along the rim of the centre spot.  Everything behind
 * the detector pairs the two images by equal index.  This call keeps the grouping and drops the values: per image and id
 * component it orders the lines by where they cross the centre, drops phantoms, and steps the index by the measured pitch.
 * One workgroup of two wavefronts per image (wavefront c = id component c), one launch on `stream`, no workspace, no atomics on
 * floating point, no host synchronisation; two calls on the same inputs give the same bits.
 *   xy f64[n,CPE_MAXP,2], id i32[n,CPE_MAXP,2], cnt i32[n]: tables as cpe_detect_grid_batch writes them; center f64[n,2] (x, y)
 *   as it writes it; params NULL = the defaults of CpeRelabelParams.
 * Rule (the order is the contract), per image and component c:
 *   1. cnt is clamped to [0, CPE_MAXP]; slots past it are never read.  A point is usable when its slot is below the count and both
 *      pixel coordinates are finite.  A non-finite center: CPE_RELABEL_FLAG_NO_CENTRE, cnt_out 0;
 *   2. a line is the usable points of one label value id[c].  A label span max - min (in 64 bits) >= CPE_MAXL in either
 *      component (so also more than CPE_MAXL labels): CPE_RELABEL_FLAG_OVERFLOW, cnt_out 0.  An image flagged by 1 or 2 reports
 *      counts and pitch 0 for both components and writes no line slot;
 *   3. per line, u the positional coordinate and t the other one (c ^ swap == 0: u = y, t = x; otherwise u = x, t = y): the
 *      point count N, the sums of t and of u in slot order, the means tm = sum / N and um, then in a second pass in slot order
 *      Stt = sum (t - tm)^2 and Stu = sum (t - tm)(u - um); a = Stu / Stt; p = um + a (t_centre - tm).  The line is unsupported
 *      when N < min_pts, Stt is not > 0, or p is not finite;
 *   4. the supported lines are sorted by (p, label); pitch0 = the median of the consecutive gaps (the mean of the two middle
 *      ones, (g[(m-1)/2] + g[m/2]) / 2 of the m sorted gaps), 0 without a gap;
 *   5. line i of that order is a phantom when a neighbour j = i - 1 or i + 1 lies closer than merge_frac * pitch0 and has more
 *      points, or as many and j < i.  All lines are judged at once, on the list of 4;
 *   6. the remaining lines give the gaps g_i.  pitch_i = the median of the g_k, k in {i-2, i-1, i+1, i+2}, that exist, with
 *      fewer than two of them the median of all remaining gaps; inc_i = max(1, floor(g_i / pitch_i + 0.5)), 1 when pitch_i is not
 *      > 0, at most CPE_RELABEL_MAX_INC.  No remaining line: CPE_RELABEL_FLAG_FEW_LINES << c (every point of the image is then
 *      dropped);
 *   7. the remaining line whose p is nearest to the centre's positional coordinate is the anchor (the first in order on a tie);
 *      new index = dir[c] * (the sum of the inc before the line - the sum before the anchor);
 *   8. a point is written when it is usable and the lines of both its components are kept: xy_out, id_out (the new indices, the
 *      component order unchanged) and src (its slot in the input) in slot order, cnt_out their number.  Slots from cnt_out on
 *      are not written.
 * lines i32[n,2,CPE_MAXL,4]: per image, component and line slot (the labels seen, ascending) label | new index | points |
 *   CPE_RELABEL_LINE_*; line_p f64[n,2,CPE_MAXL] the position p (0 where Stt is not > 0 or p is not finite); index 0 for a line
 *   that is not kept.  Slots from counts[.,.,0] on are not written.
 * pitch f64[n,2] = pitch0; counts i32[n,2,4] = labels seen | supported | dropped as phantom | kept; flags i32[n].
 * No output may overlap an input or another output (CPE_ERR_ARG); n == 0 is a no-op.  min_pts < 2, merge_frac outside (0, 1),
 * dir other than +-1 and swap other than 0 / 1 are refused with CPE_ERR_ARG before anything is written.
 * Limits: boards only (a line is straight in the image); one centre per image; a line with fewer than min_pts points is lost
 * with its points; an image whose anchor line is missing ends a line off, which is what cpe_index_shift_batch repairs. */
#define CPE_RELABEL_FLAG_NO_CENTRE 1
#define CPE_RELABEL_FLAG_OVERFLOW 2
#define CPE_RELABEL_FLAG_FEW_LINES 4     /* component 0; component 1 is CPE_RELABEL_FLAG_FEW_LINES << 1 */
#define CPE_RELABEL_LINE_KEPT 0
#define CPE_RELABEL_LINE_UNSUPPORTED 1
#define CPE_RELABEL_LINE_PHANTOM 2
#define CPE_RELABEL_MAX_INC 1048576
typedef struct CpeRelabelParams {
    int32_t swap;        /* 0: id component 0 is positioned in y (the planar detector's (row, col)); 1: in x.  Default 0 */
    int32_t min_pts;     /* a line with fewer usable points is unsupported; >= 2; default 3 */
    double  merge_frac;  /* a neighbour closer than merge_frac * pitch0 makes the weaker line a phantom; in (0, 1); default 0.65 */
    int32_t dir[2];      /* +1 or -1: the new index of component c grows (falls) with the position; default +1, +1 */
} CpeRelabelParams;
CPE_API int32_t cpe_grid_relabel_batch(const double *xy, const int32_t *id, const int32_t *cnt, const double *center, int32_t n,
                                       const CpeRelabelParams *params, double *xy_out, int32_t *id_out, int32_t *cnt_out,
                                       int32_t *src, int32_t *lines, double *line_p, double *pitch, int32_t *counts, int32_t *flags,
                                       void *stream);

/* BUILD-DEFINED, opt-in: the grid a fitted cylinder PREDICTS.  Once a frame has a cylinder pose, the pose and the laser-plane
 * table say where every grid node (u, v) falls in each image: the node is the line of two planes of light, cut with the cylinder
 * and projected.  cpe_grid_assign_batch names each detection by its nearest predicted node, point by point and per image, which no
 * frame-wide shift can do.  One lane per (frame, node), one launch for the nodes and one for the counts on `stream`, no atomics,
 * no workspace, no host synchronisation; two calls on the same inputs give the same bits.
 *   cyl f64[n,6]: a point o_c on the axis and the axis direction a (any length), camera-1 coordinates: what
 *     cpe_fit_cylinder_batch writes to cyl[:,1,:] (row stride 6); use u8[n] or NULL (all frames); radius R > 0, finite
 *   K1, K2 f64[9], T21 f64[16]: DEVICE memory, as cpe_fused_triangulate_batch
 *   P f64[2,L,4], line_status i32[2,L], lo, hi: exactly what cpe_table_triangulate_batch reads; L = hi - lo + 1 in 1..CPE_MAXL
 *   centre f64[3] (device): the projector's centre (the first three numbers of the table's centre)
 *   params NULL = the defaults of CpeGridPredictParams: the window [lo, hi] in both families, min_cos 0.1, no image bound
 * The nodes are the window win_lo[k]..win_hi[k] of table family k, inside [lo, hi]: Nu x Nv = N of them, 1 <= N <= CPE_PRED_MAXN
 * (otherwise CPE_ERR_ARG); node j = (u - win_lo[0]) Nv + (v - win_lo[1]).  Dot products are (a0 b0 + a1 b1) + a2 b2.
 * Rule per (frame, node) (the order is the contract):
 *   1. the frame is unusable when use is 0, any of its six numbers is not finite, or |a| is 0 or not finite: every node of the
 *      frame gets CPE_PRED_NO_FRAME.  ah = a / |a|;
 *   2. both planes [n0, p0] = P[0, u - lo], [n1, p1] = P[1, v - lo] must have line_status CPE_ST_OK, else CPE_PRED_NO_PLANE;
 *   3. w = n0 x n1; |w|^2 < CPE_PRED_MIN_W2 or not finite: CPE_PRED_PARALLEL;
 *   4. q = (-p0 (n1 x w) - p1 (w x n0)) / |w|^2, the point of the planes' line nearest to the origin; wh = w / |w|;
 *   5. e = q - o_c, ep = e - (e.ah) ah, wp = wh - (wh.ah) ah, A = |wp|^2, B = ep.wp, C = |ep|^2 - R^2, disc = B B - A C;
 *   6. A, B, C or disc not finite, A == 0 or disc <= 0: CPE_PRED_MISS;
 *   7. s = sqrt(disc), t- = (-B - s) / A, t+ = (-B + s) / A, tC = (centre - q).wh.  The lit root t is the one nearer to tC:
 *      t- when |t- - tC| <= |t+ - tC| (a tie goes to t-), otherwise t+;
 *   8. X = q + t wh (not finite: CPE_PRED_MISS); g = X - o_c; outward normal nu = (g - (g.ah) ah) / R;
 *   9. |nu.wh| < min_cos: CPE_PRED_GRAZING.  nu.wh = +-sqrt(disc) / R, so this keeps the square root away from zero: the error
 *      of t grows with 1 / sqrt(disc) <= 1 / (min_cos R);
 *  10. per camera j (R_j, t_j the rotation and translation of Tc, the identity and 0 for camera 1, T21 for camera 2; o_j as in
 *      step 2 of cpe_table_triangulate_batch): Xc = R_j X + t_j (camera 1: X itself), Z = Xc[2], v = o_j - X.  The node is
 *      visible when Z > 0, nu.v > min_cos |v|, and with x = (K[0] (Xc[0] / Z) + K[1] (Xc[1] / Z)) + K[2],
 *      y = K[4] (Xc[1] / Z) + K[5], x and y are finite and, with an image bound, 0 <= x < img_w and 0 <= y < img_h (img_w <= 0 or
 *      img_h <= 0: no bound).
 * Outputs, every slot of every node written: X f64[n,N,3] (0 unless the state is CPE_PRED_OK); px f64[n,2,N,2] = (x, y) per
 * camera (0 where the node is not visible in that camera); state i32[n,N]; vis i32[n,N]: bit 0 camera 1, bit 1 camera 2;
 * counts i32[n,4] = OK nodes | visible in camera 1 | in camera 2 | in both.  n == 0 is a no-op.
 * Limits: a rigid, ideal cylinder of the given radius; the table's errors and the pose's move the predictions alike. */
#define CPE_PRED_MAXN 4096
#define CPE_PRED_MIN_W2 1e-6   /* planes of light closer than 0.057 degrees to parallel: q carries the roundings of w times
                                  1 / |w|^2, so at this gate a rounding of 1e-16 has grown to 1e-10 of the offsets, still an
                                  order below the 1e-8 mm the points are held to; real families meet near 90 degrees */
#define CPE_PRED_OK 0
#define CPE_PRED_NO_FRAME 1
#define CPE_PRED_NO_PLANE 2
#define CPE_PRED_PARALLEL 3
#define CPE_PRED_MISS 4
#define CPE_PRED_GRAZING 5
typedef struct CpeGridPredictParams {
    int32_t win_lo[2];  /* first node index of table family 0, 1; >= lo */
    int32_t win_hi[2];  /* last node index of table family 0, 1; <= hi and >= win_lo */
    double  min_cos;    /* the grazing and facing gate, in (0, 1); default 0.1 */
    int32_t img_w;      /* image bound in pixels; <= 0 (default): none */
    int32_t img_h;
} CpeGridPredictParams;
CPE_API int32_t cpe_grid_predict_batch(const double *cyl, const uint8_t *use, int32_t n, double radius, const double *K1,
                                       const double *K2, const double *T21, const double *P, const int32_t *line_status, int32_t lo,
                                       int32_t hi, const double *centre, const CpeGridPredictParams *params, double *X, double *px,
                                       int32_t *state, int32_t *vis, int32_t *counts, void *stream);

/* BUILD-DEFINED, opt-in: re-number ONE image's detections against one camera's predicted pixels: every detection takes the index
 * of its nearest predicted node, when that node is near, unambiguous and not claimed by a nearer detection.  One workgroup per
 * image, the camera's predicted pixels staged in LDS, one lane per detection scanning them; the winner per node by integer LDS
 * atomics only; one launch on `stream`, no workspace, no host synchronisation; two calls on the same inputs give the same bits.
 *   xy f64[n,CPE_MAXP,2], id i32[n,CPE_MAXP,2], cnt i32[n]: as cpe_detect_grid_batch writes them
 *   px: image f's predicted pixels are the N (x, y) pairs at px + f px_stride (px_stride in doubles, >= 2 N): px_stride = 4 N
 *     and px + 2 N cam_bit address camera cam_bit of cpe_grid_predict_batch's px; vis i32[n,N] with cam_bit in {0, 1}: node j
 *     is visible when bit cam_bit of vis[j] is set and both its pixel coordinates are finite
 *   win_lo0, win_lo1, Nu, Nv: the window of the prediction, N = Nu Nv in 1..CPE_PRED_MAXN (otherwise CPE_ERR_ARG); node j
 *     stands for u = win_lo0 + j / Nv of table family 0 and v = win_lo1 + j % Nv of family 1
 *   params NULL = the defaults of CpeGridAssignParams
 * Rule (the order is the contract), per image:
 *   1. cnt is clamped to [0, CPE_MAXP]; slots past it are never read.  A point with a non-finite pixel is refused (counts[3]);
 *   2. over the visible nodes in node order: d^2 = (x - px) (x - px) + (y - py) (y - py).  The nearest node is the first with
 *      the smallest d^2 below +inf, the second nearest is taken likewise among the others; d1, d2 the square roots, d2 = +inf
 *      with a single such node.  No such node: refused (counts[3]);
 *   3. d1 >= tau_px: refused (far, counts[4]);
 *   4. d1 > ratio d2: refused (ambiguous, counts[5]);
 *   5. among the remaining points that name the same node the smallest (d1, slot) keeps it, the others are refused (conflict,
 *      counts[6]);
 *   6. kept points go in slot order to slots 0..m-1 of xy_out f64[n,CPE_MAXP,2] (a copy), id_out i32[n,CPE_MAXP,2] (component c
 *      holds the node's index in family c ^ swap), src i32[n,CPE_MAXP] (the input slot) and dist f64[n,CPE_MAXP] (d1).  Slots
 *      from m on are NOT written;
 *   7. m i32[n]; counts i32[n,8] = m | kept with id_out equal to id | kept and re-numbered | refused in steps 1 / 2 | far |
 *      ambiguous | conflict | 0; stats f64[n,2] = sqrt of the mean squared d1 and the largest d1 of the kept points, both 0
 *      when m = 0; node_slot i32[n,N] or NULL: per node the input slot of the point that kept it, or -1.
 * tau_px <= 0 or not finite, ratio outside (0, 1] and swap other than 0 / 1 are refused with CPE_ERR_ARG.  No output may overlap
 * an input or another output (CPE_ERR_ARG).  n == 0 is a no-op.
 * Limits: the brute-force scan costs cnt x N distances per image; a detection with no predicted node (one the window or the
 * visibility tests left out) is dropped, not kept under its old index. */
typedef struct CpeGridAssignParams {
    double  tau_px;     /* a detection farther than this from its nearest node is refused; > 0; default 4.0 */
    double  ratio;      /* d1 > ratio d2 is ambiguous; in (0, 1]; default 0.5 */
    int32_t swap;       /* as CpeTableTriParams.swap */
    int32_t reserved;
} CpeGridAssignParams;
CPE_API int32_t cpe_grid_assign_batch(const double *xy, const int32_t *id, const int32_t *cnt, int32_t n, const double *px,
                                      int64_t px_stride, const int32_t *vis, int32_t cam_bit, int32_t win_lo0, int32_t win_lo1,
                                      int32_t Nu, int32_t Nv, const CpeGridAssignParams *params, double *xy_out, int32_t *id_out,
                                      int32_t *src, double *dist, int32_t *m, int32_t *counts, double *stats, int32_t *node_slot,
                                      void *stream);

/* Row f-3: the undistortion pre-step of the CLI entry point, utils/iotool.py:22-39
 *   undistort_image(image, camera_params) = cv2.undistort(image, IntrinsicMatrix, hstack(Radial, Tangential))
 * cv2.undistort rebuilds its fixed-point map per image; here the map is built once per camera and applied per frame.
 *   cpe_undistort_map: K f64[9] row-major and dist f64[n_dist] are HOST pointers (n_dist in {0,4,5,8,12}, OpenCV order
 *     k1 k2 p1 p2 [k3 [k4 k5 k6 [s1 s2 s3 s4]]]); map_xy i16[h,w,2] and map_f u16[h,w] are device buffers in OpenCV's
 *     CV_16SC2 / CV_16UC1 convention (integer source pixel; 5-bit fractions fy*32 + fx).
 *   cpe_remap_bilinear_batch: dst[n,h,w] = remap(src[n,h,w], map, INTER_LINEAR, BORDER_CONSTANT 0); src != dst. */
CPE_API int32_t cpe_undistort_map(const double *K, const double *dist, int32_t n_dist, int32_t h, int32_t w,
                                  int16_t *map_xy, uint16_t *map_f, void *stream);
CPE_API int32_t cpe_remap_bilinear_batch(const uint8_t *src, int32_t n, int32_t h, int32_t w, const int16_t *map_xy,
                                         const uint16_t *map_f, uint8_t *dst, void *stream);

/* Row f-3, second mode: the MATLAB entry point undistorts with undistortImage(I, cameraParams, 'cubic')
 * (utils/preProcessing.m:3-4, :15).  Output view 'same', fill value `fill`.
 *   cpe_undistort_map_matlab: K f64[9] row-major as the camera JSON holds it (createCameraDataJSON.m:7: [fx s cx; 0 fy cy;
 *     0 0 1] with MATLAB's 1-based principal point), radial f64[n_radial] (n_radial 0..3: k1 k2 [k3]), tangential f64[2] or
 *     NULL -- HOST pointers; map f32[h,w,2] device buffer: 0-based source (x, y) of every output pixel (distortPoints in f64).
 *   cpe_remap_cubic_batch: dst[n,h,w] = interp2d(src[n,h,w], map, 'cubic', fill): cubic convolution (a = -1/2) in single
 *     precision, result rounded half away from zero and saturated; src != dst; h, w >= 3. */
CPE_API int32_t cpe_undistort_map_matlab(const double *K, const double *radial, int32_t n_radial, const double *tangential,
                                         int32_t h, int32_t w, float *map, void *stream);
CPE_API int32_t cpe_remap_cubic_batch(const uint8_t *src, int32_t n, int32_t h, int32_t w, const float *map, int32_t fill,
                                      uint8_t *dst, void *stream);

/* Row f-3, the whole of utils/preProcessing.m:3-9 for a batch of frames of ONE camera, in one pass:
 *   im2uint8 -> undistortImage(..., 'cubic') per channel -> rgb2gray (channels == 3) -> u8 grey
 * src: [n,h,w] (channels 1) or [n,h,w,3] RGB channel-last (channels 3), contiguous, element type `dtype` (what MATLAB's
 *   imread / a camera driver hands over: uint8, uint16 of a 16-bit PNG, single, double).
 * map: f32[h,w,2] from cpe_undistort_map_matlab; dst frame f starts at dst + f * dst_frame_stride (bytes, >= h*w), so the
 *   left camera of a stereo chunk goes to dst and the right one to dst + h*w, both with stride 2*h*w (frame-major pairs).
 * The result is byte for byte what the separate steps give:
 *   im2uint8  [ext, parity unpinned vs MATLAB]  uint8: identity; uint16: round(x / 257) = (x + 128) / 257 in integers;
 *             single / double: x * 255 in the input's precision, NaN -> 0, saturated to [0, 255], rounded half away from zero
 *   cubic     cpe_remap_cubic_batch on every channel (each rounded to u8), `fill` outside
 *   rgb2gray  floor(R * 0.298936021293775 + G * 0.587043074451121 + B * 0.114020904255103 + 0.5) in f64, left to right
 * h, w >= 3; src != dst; n == 0 is a no-op. */
#define CPE_PIX_U8 0
#define CPE_PIX_U16 1
#define CPE_PIX_F32 2
#define CPE_PIX_F64 3
CPE_API int32_t cpe_matlab_prestep_batch(const void *src, int32_t n, int32_t h, int32_t w, int32_t dtype, int32_t channels,
                                         const float *map, int32_t fill, uint8_t *dst, int64_t dst_frame_stride, void *stream);

/* Row f-1: the per-frame terms of the multi-frame objective of fitCylinderWPts3sAngs.m:82-94 (`dist`):
 * terms[i] = mean((getDistPts3ToLine(Pts3s{i}, line(T * TAGVcyls{i})) - radius)^2), one wavefront per frame.
 * X f64[n,CPE_MAXP,3], cnt i32[n], TAGVcyl f64[n,16] (row-major getTAGVcyl(pan,tilt)), T f64[16] (device, row-major
 * vec2T(agvPose)).  For a 6-parameter Nelder-Mead driven from the host (cpe_amd/multiframe.py: fit_multi_frame); the
 * resident form of the whole fit is cpe_multi_frame_fit_batch. */
CPE_API int32_t cpe_multi_frame_terms(const double *X, const int32_t *cnt, int32_t n, const double *TAGVcyl,
                                      const double *T, double radius, double *terms, void *stream);

/* Row f-1, resident: [T, fval] = fitCylinderWPts3sAngs(Pts3s, angs, cylRadius) (exp_gridDetection.m:87) for G groups of
 * frames in one call, one workgroup per group: initial pose (fitCylinderWPts3sAngs.m:40-69), fminsearch (:75, the loop of
 * cpe_fit_cylinder_batch) over `dist` (:82-94) and vec2T of the result, all on the device.
 *   X f64[n,CPE_MAXP,3], cnt i32[n], cyl_raw f64[n,2,6]: the frames' points and [cylParams0; cylParams] as
 *     cpe_fit_cylinder_batch returns them; TAGVcyl f64[n,16]: row-major getTAGVcyl(pan, tilt) of every frame
 *   frame_ok i32[n] or NULL: a frame with 0 is left out of its group (a frame whose detection or fit failed: the cell the
 *     script's try / warning leaves empty)
 *   group_start i32[G+1], DEVICE memory: group g is made of the frames [group_start[g], group_start[g+1]) that are kept, in
 *     order; groups may overlap, be empty, and come in any order
 *   x0_in f64[G,6] or NULL: the initial agvPose [rotation vector, translation] of every group; NULL = :40-69 from the
 *     first two kept frames of the group (cyl_raw may be NULL when x0_in is given)
 *   params NULL = the reference's optimset (:75): TolX = TolFun = 1e-5, MaxIter = MaxFunEvals = 1e5.  mode must be
 *     CPE_FIT_NELDER_MEAD (CPE_ERR_ARG otherwise: the LM form is cpe_multi_frame_fit_lm_batch)
 * Outputs per group: x0, x f64[G,6] (initial and fitted agvPose), T f64[G,16] row-major vec2T(x), fvals f64[G,2] = [f0, f],
 * iters i32[G,2] = [iterations, function evaluations], n_used i32[G] kept frames, status i32[G]:
 *   CPE_ST_OVERFLOW    group_start[g] .. group_start[g+1] is not 0 <= a <= b <= n, or more than CPE_MULTI_MAXF frames are kept
 *   CPE_ST_FEW_POINTS  fewer than two kept frames (assert(nAngles >= 2), :29); one of the first two kept frames has no point
 *                      (applyCylParamsPrior takes min() of its points; checked with x0_in as well); x0, f0, x or f not finite
 * With either, every other output of the group is zero (n_used included), so CPE_ST_OK implies finite outputs.  The status is
 * decided in the kernel (group_start lives on the device); no argument of the call makes it fail after the launch.
 * cnt is clamped to [0, CPE_MAXP] as in cpe_fit_cylinder_batch.  Deviation: a kept frame without points beyond the first two
 * contributes the term 0, as in cpe_multi_frame_terms (the reference divides 0 by 0 there and returns NaN).
 * Arithmetic: a frame's term has the bits of cpe_multi_frame_terms and the terms are added in kept-frame order (:92), the
 * simplex is the fixed-order fminsearch of the per-frame fit.  sin / cos (vec2T) and acos / sin (T2vec, initial pose only) are
 * the device math library's, not the host libm's, so against a host-driven fit the objective may differ in its last bits:
 * x and the iteration path agree where no comparison of the simplex is that close, f to about 1e-12 relative.
 * Asynchronous on `stream`, no allocation, no workspace, no host synchronisation; G == 0 is a no-op. */
#define CPE_MULTI_MAXF 1024   /* kept frames of one group */
CPE_API int32_t cpe_multi_frame_fit_batch(
    const double *X, const int32_t *cnt, const double *TAGVcyl, const double *cyl_raw, /* [n,MAXP,3] [n] [n,16] [n,2,6] */
    const int32_t *frame_ok,      /* i32[n] or NULL: a frame with 0 is left out of its group */
    const int32_t *group_start,   /* i32[G+1], device */
    int32_t G, int32_t n, double radius, const CpeFitParams *params,
    const double *x0_in,          /* f64[G,6] or NULL = fitCylinderWPts3sAngs.m:40-69 */
    double *x0, double *x, double *T, double *fvals, int32_t *iters, int32_t *n_used, int32_t *status, void *stream);

/* Row f-1, BUILD-DEFINED fast mode (nothing like it in the reference, as CPE_FIT_LM and RANSAC are for the per-frame fit): the
 * multi-frame fit by Levenberg-Marquardt from an initial pose made of all kept frames.  Same objective, same 6-vector x and
 * same groups / frame_ok / statuses as cpe_multi_frame_fit_batch, about ten passes over the points instead of thousands.  The
 * reference-faithful forms stay cpe_multi_frame_fit_batch and the host-driven simplex.
 *   x0_in NULL: the initial pose is a closed form over all *usable* kept frames -- cnt >= 1 and the fitted row
 *     cyl_raw[i,1,:] finite with a non-zero direction -- in place of fitCylinderWPts3sAngs.m:40-69 (first two frames, the
 *     linear-indexing quirk of applyCylParamsPrior).  o_i = cyl_raw[i,1,0:3]; d_i = cyl_raw[i,1,3:6] normalised and turned so
 *     that d_i . d_first >= 0 (d_first: the first usable frame's); a_i, p_i = columns 2, 4 of TAGVcyl_i.  For sigma = +1, -1:
 *     Rot = the proper rotation maximising sum (Rot a_i).(sigma d_i) (Horn's quaternion), t = argmin sum |(I - d_i d_i')(Rot p_i
 *     + t - o_i)|^2; the sigma with the lower objective is kept (a tie: +1) and x0 = T2vec([Rot t]).  A kept frame that is not
 *     usable still counts in the objective.
 *   LM: residuals r_ik = (d_ik - radius) / sqrt(n_i) (their squares sum to the objective), analytic Jacobian for the step
 *     Rot <- exp([dw]x) Rot, t <- t + dt, the candidate x = T2vec of that pose evaluated by the objective itself.  Damping,
 *     acceptance, up to 12 trials per iteration, the 6x6 solve and the stop rule are those of the per-frame CPE_FIT_LM:
 *     (f_prev - f) <= tol_f * 1e-3 * (1 + f) and max |delta| <= tol_x; at most min(max_iter, 200) iterations.
 *   params NULL = tol_x = tol_f = 1e-5, max_iter 100000; a given mode must be CPE_FIT_LM (CPE_ERR_ARG otherwise);
 *     max_fun_evals is not used.
 * Outputs as cpe_multi_frame_fit_batch: fvals = [f(x0), f(x)], iters = [iterations, objective evaluations] (the two candidate
 * poses of a NULL x0_in are two of them), T = vec2T(x), and
 *   frame_terms f64[n] or NULL: frame_terms[f] = the term of kept frame f at the returned pose (the bits of
 *     cpe_multi_frame_terms at T), by one more evaluation that iters does not count.  Written only for the kept frames of
 *     groups that end CPE_ST_OK: initialise it.  A frame kept by several groups receives the term of one of them.
 * Statuses: CPE_ST_OVERFLOW as cpe_multi_frame_fit_batch; CPE_ST_FEW_POINTS: fewer than two kept frames, fewer than two
 * usable frames (x0_in NULL), or x0, f0, x or f not finite.  With either every other per-group output is zero.  With x0_in
 * no frame needs a point: a frame without points has the term 0.
 * Arithmetic: f(x0), f(x) and frame_terms have the bits of cpe_pose_vec2T_batch + cpe_multi_frame_terms with the terms added
 * in kept-frame order; the sums of the initial pose and of the Jacobian are made in a fixed order, so a call repeats its bits.
 * Asynchronous on `stream`, no allocation, no workspace, no host synchronisation; G == 0 is a no-op. */
CPE_API int32_t cpe_multi_frame_fit_lm_batch(
    const double *X, const int32_t *cnt, const double *TAGVcyl, const double *cyl_raw, /* [n,MAXP,3] [n] [n,16] [n,2,6] */
    const int32_t *frame_ok, const int32_t *group_start, int32_t G, int32_t n, double radius, const CpeFitParams *params,
    const double *x0_in,          /* f64[G,6] or NULL = the all-frame initial pose */
    double *x0, double *x, double *T, double *fvals, int32_t *iters, int32_t *n_used, int32_t *status,
    double *frame_terms,          /* f64[n] or NULL */
    void *stream);

/* Row f-1, BUILD-DEFINED: the LM form with a consensus over FRAMES in front of it.  cpe_multi_frame_fit_lm_batch minimises a plain
 * sum over every kept frame, and a frame can end with status 0 and a wrong cylinder; a few of them pull T_Cam_AGV away and nothing
 * reports it.  Here poses made of two frames each are scored by the frames that agree with them, the best one's frames are
 * fitted, and the frames that do not agree are reported.
 *   X, cnt, TAGVcyl, cyl_raw (not NULL), frame_ok, group_start, G, n, radius, the kept frames, the clamping of
 *   cnt, CPE_ST_OVERFLOW and the "usable" frame: exactly as cpe_multi_frame_fit_lm_batch; params as there (NULL, or mode
 *   CPE_FIT_LM); cons NULL = the defaults of CpeConsensusParams, a value outside its ranges: CPE_ERR_ARG, nothing is written;
 *   ws: cpe_multi_frame_consensus_workspace_bytes(G, max_hyp) bytes of 8-byte aligned device scratch (0 for G <= 0 or a max_hyp
 *   outside its range), content on entry irrelevant (Conventions, "Workspaces"); missing or too small: CPE_ERR_WORKSPACE.
 * term_f(x) below is frame f's term at the pose x with the bits of cpe_pose_vec2T_batch + cpe_multi_frame_terms, and the
 * objective over a list of frames is their terms added in list order.  A kept frame is an INLIER of x when cnt >= 1 and
 * term_f(x) < tau^2, i.e. the rms of its dist - radius is below tau.  Rule (the order is the contract), per group:
 *   1. K = the kept frames (m of them), U = the usable ones among them in kept order, u = |U|; u < 2: CPE_ST_FEW_POINTS;
 *   2. hypotheses: R = max(1, max_hyp div u); if R >= u div 2 then R = u div 2 and off_k = 1 + k (every unordered pair of U
 *      occurs), otherwise off_k = 1 + ((2k + 1)(u div 2 - 1)) div (2R): R different offsets spread over 1..u div 2 - 1 (the
 *      offsets off and u - off name the same pairs); H = min(R u, max_hyp); hypothesis h in 0..H-1 takes a = h mod
 *      u, b = (a + off_(h div u)) mod u, and x_h = the closed-form initial pose of cpe_multi_frame_fit_lm_batch over the list
 *      (U[a], U[b]): both sigma, the lower objective over that list kept, a tie to +1.  x_h or that objective not finite: void.
 *      With the offset u/2 of an even u (R = u div 2 only) every pair occurs twice, as (a, b) and (b, a): the second, a >= u/2,
 *      is void as well (two poses that differ by rounding alone would leave the winner to the last bits);
 *   3. key_h = (-number of inliers of x_h, sum of their terms added in kept order, h); the smallest key of a hypothesis that is
 *      not void wins: x0 = its pose, S_0 = its inliers.  No such hypothesis, or |S_0| < min_inliers: CPE_ST_FEW_POINTS;
 *   4. for r = 1..max_rounds: x_r = cpe_multi_frame_fit_lm_batch's LM loop over the list S_(r-1) from x_(r-1) (its bits, with
 *      frame_ok = the list and x0_in = x_(r-1)); S_r = the inliers of x_r among ALL kept frames; stop after round r when S_r =
 *      S_(r-1) (CPE_CONSENSUS_CONVERGED) or when |S_r| < min_inliers (CPE_CONSENSUS_SHRUNK; x_r stays the result).  x = the
 *      last x_r, or x0 with max_rounds = 0.  A start, result or objective that is not finite: CPE_ST_FEW_POINTS;
 *   5. per group: x0, x f64[G,6]; T f64[G,16] = vec2T(x); fvals f64[G,2] = the objective of x0 over S_0 | of x over the list x was
 *      fitted to; iters i32[G,2] = LM iterations | objective evaluations, each round counted as its cpe_multi_frame_fit_lm_batch
 *      call would (the scoring of hypotheses and of inliers is not counted); n_used i32[G] = m; n_inliers i32[G] = the length
 *      of the list x was fitted to; info i32[G,4] = winning h | frame U[a] | frame U[b] | rounds done; flags i32[G]
 *      CPE_CONSENSUS_* (independent bits; neither: max_rounds ran out); status i32[G];
 *   6. per frame, written only for the kept frames of groups that end CPE_ST_OK (initialise them; a frame kept by several groups
 *      receives the values of one of them): inlier i32[n] = 1 when the frame is in the list x was fitted to, else 0;
 *      frame_terms f64[n] or NULL = term_f(x) of every kept frame, outliers included;
 *   7. a group that is not CPE_ST_OK has every other per-group output zero, so CPE_ST_OK implies finite outputs.
 * Limits: the consensus is the largest set of frames that agree with ONE pose, so a majority of frames that are wrong in the
 * same way wins; one tau per call; a frame is in or out whole (no per-point trimming here: that is cpe_fit_cylinder_ransac_batch's
 * part); neighbouring frames with nearly equal pan and tilt make poor hypotheses -- they simply score low.
 * Two launches on `stream` (one wavefront per (hypothesis, group), then one workgroup per group), vector stores only, no
 * atomics, no allocation, no host synchronisation; two calls on the same inputs give the same bits; G == 0 is a no-op. */
#define CPE_CONSENSUS_MAX_HYP 4096
#define CPE_CONSENSUS_CONVERGED 1   /* a round returned the list of frames it was given */
#define CPE_CONSENSUS_SHRUNK 2      /* a round left fewer than min_inliers inliers: its pose is returned, fitted to the list before */
typedef struct CpeConsensusParams {
    double  tau;          /* a frame agrees with a pose when its term < tau^2; the unit of the points; > 0; default 0.5 */
    int32_t max_hyp;      /* hypotheses per group, 1..CPE_CONSENSUS_MAX_HYP; default 2048 */
    int32_t max_rounds;   /* refinement rounds, 0..16; default 4 */
    int32_t min_inliers;  /* a consensus of fewer frames is refused; >= 2; default 3 */
} CpeConsensusParams;
CPE_API size_t cpe_multi_frame_consensus_workspace_bytes(int32_t G, int32_t max_hyp);
CPE_API int32_t cpe_multi_frame_consensus_batch(
    const double *X, const int32_t *cnt, const double *TAGVcyl, const double *cyl_raw, /* [n,MAXP,3] [n] [n,16] [n,2,6] */
    const int32_t *frame_ok, const int32_t *group_start, int32_t G, int32_t n, double radius, const CpeFitParams *params,
    const CpeConsensusParams *cons, void *ws, size_t ws_bytes,
    double *x0, double *x, double *T, double *fvals, int32_t *iters, int32_t *n_used, int32_t *n_inliers, int32_t *info,
    int32_t *flags, int32_t *status,
    int32_t *inlier,              /* i32[n] */
    double *frame_terms,          /* f64[n] or NULL */
    void *stream);

/* vec2T.m / T2vec.m for n poses, one lane per pose: x f64[n,6] = [rotation vector, translation], T f64[n,16] row-major 4x4
 * (exp_gridDetection.m:92 calls T2vec(T_Cam_cyl) for every frame).  [ext] rotvec2mat3d / rotmat2vec3d restated as in
 * oracle/src/orc_fit.c (parity unpinned): vec2T gives the identity rotation for |rotation vector| < 1e-6; T2vec has three
 * branches -- sin(theta) >= 1e-4: theta * r / (2 sin theta); theta near 0: (1/2 - (trace - 3) / 12) * r; theta near pi: from
 * the largest diagonal entry -- and does not re-orthogonalise its input (rotmat2vec3d's SVD).  These are the device functions
 * cpe_multi_frame_fit_batch itself uses, with the device math library's sin / cos / acos (a few ulp from the host libm's).
 * The bottom row of T is written as 0 0 0 1 / not read.  n == 0 is a no-op. */
CPE_API int32_t cpe_pose_vec2T_batch(const double *x, int32_t n, double *T, void *stream);   /* vec2T.m */
CPE_API int32_t cpe_pose_T2vec_batch(const double *T, int32_t n, double *x, void *stream);   /* T2vec.m */

/* getTAGVcyl.m (default config) for n pairs of angles, one lane per pair: angles f64[n,2] = (pan, tilt) in rad, TAGVcyl
 * f64[n,16] row-major 4x4 -- the table cpe_multi_frame_terms and the multi-frame fits take, which until now only the host
 * could make.  The full product TAP * TPT0 * T01 * T12 * T2C of the five matrices in the operation order of
 * cpe_amd/multiframe.py::get_TAGVcyl: cos(pan), sin(pan), cos(-tilt), sin(-tilt), -tan(tilt) * L, every entry of a product as
 * ((a*b + c*d) + e*f) + g*h.  It differs from the host only through the device math library's sin / cos / tan (rotation
 * entries within 16 * 2^-53, column 4 within 1e-12 mm: DESIGN.md §3.7).  This is the device function
 * cpe_frame_angles_lm_batch itself uses.  n == 0 is a no-op. */
CPE_API int32_t cpe_agv_chain_batch(const double *angles /*[n,2] pan,tilt rad*/, int32_t n, double *TAGVcyl /*[n,16]*/, void *stream);

/* BUILD-DEFINED (nothing like it in the reference, as CPE_FIT_LM, RANSAC and cpe_multi_frame_fit_lm_batch are): pan and tilt of
 * every frame from a calibrated camera-AGV pose.  exp_gridDetection.m:90-93 goes the other way: it forms T_Cam_AGV *
 * getTAGVcyl(pan, tilt) from the nominal angles in the file names.  One wavefront per frame, any n:
 *     minimise over q = (pan, tilt):  f(q) = mean((d - radius)^2)  of the frame's points against the axis of T * A(q),
 * A(q) = the chain of cpe_agv_chain_batch; f(q) has the bits of cpe_agv_chain_batch + cpe_multi_frame_terms.
 *   X f64[n,CPE_MAXP,3], cnt i32[n]: as cpe_fit_cylinder_batch leaves them; cyl_raw f64[n,2,6] its [cylParams0; cylParams]
 *   T f64[G,16], DEVICE memory: row-major T_Cam_AGV (vec2T of a fitted agvPose); pose_index i32[n] (device) names the pose of
 *     every frame, NULL = every frame uses T[0]
 *   a0_in f64[n,2] or NULL: the start.  NULL never means zero (from (0, 0) one frame fit in twelve ends in a second minimum
 *     0.35-0.46 rad away: DESIGN.md §3.7) but a closed form from the frame's own fitted axis d = cyl_raw[f,1,3:6] (the frame
 *     must be usable by the rule of cpe_multi_frame_fit_lm_batch: that row finite, its direction not zero): a = Rot' d / |d|,
 *     negated when a_x > 0, pan = atan2(-a_y, -a_x), tilt = asin(clamp(-a_z, -1, 1)) -- the chain's second column is
 *     Rz(pan) (-cos tilt, 0, -sin tilt).  This ASSUMES |pan| < pi/2 (the sign of a fitted direction is arbitrary), and it is
 *     as good as the per-frame fit: five points do not pin a cylinder of known radius down (about a quarter of 5-point frames
 *     are fitted more than 0.1 rad off their axis), so give a0_in -- the nominal angles -- for frames with few points.
 *     cyl_raw may be NULL when a0_in is given.
 *   LM: residuals r_k = (d_k - radius) / sqrt(cnt); Jacobian = the per-frame CPE_FIT_LM's dr/do, dr/dv chained with the
 *     closed-form derivatives of the chain's columns 2 and 4 (values always come from the full product); five sums per pass
 *     (J'J, J'r) in the fixed lane-strided order and 64-lane tree; the damped 2 x 2 system with CPE_FIT_LM's (1 + lambda)
 *     diagonal and 1e-12 * trace ridge solved in closed form; lambda from 1e-3, / 10 on acceptance (floor 1e-12), x 10 on
 *     rejection, up to 12 trials per iteration; stop when (f_prev - f) <= tol_f * 1e-3 * (1 + f) and max |delta| <= tol_x; at
 *     most min(max_iter, 200) iterations.  A candidate that is not finite or has |tilt| >= pi/2 - 1e-3 (the chain's tan), or
 *     whose objective is not finite, is a rejected trial, so every loop is bounded whatever the data.
 *   params NULL = tol_x = tol_f = 1e-5, max_iter 100000; a given mode must be CPE_FIT_LM (CPE_ERR_ARG otherwise);
 *     max_fun_evals is not used.
 * Outputs per frame: angles0, angles f64[n,2] (start and result); fvals f64[n,2] = [f(a0), f(a)]; iters i32[n,2] = [iterations,
 * objective evaluations]; TAGVcyl f64[n,16] or NULL: the chain at the result (the bits of cpe_agv_chain_batch(angles)); Tcyl
 * f64[n,16] or NULL: T * TAGVcyl (exp_gridDetection.m:91), every entry as ((a*b + c*d) + e*f) + g*h; status i32[n]:
 *   CPE_ST_OVERFLOW    pose_index[f] is outside [0, G)
 *   CPE_ST_FEW_POINTS  cnt < CPE_FIT_MIN_POINTS; no a0_in and the frame is not usable; a start, result or objective not finite
 * With either, every other output of the frame is zero, so CPE_ST_OK implies finite outputs.  The status is decided in the
 * kernel.  cnt is clamped to [0, CPE_MAXP].  A call repeats its bits, and a frame's outputs do not depend on its place in the
 * batch.  Asynchronous on `stream`, no allocation, no workspace, no host synchronisation; n == 0 is a no-op. */
CPE_API int32_t cpe_frame_angles_lm_batch(
    const double *X, const int32_t *cnt,      /* [n,CPE_MAXP,3], [n] */
    const double *cyl_raw,                    /* [n,2,6] or NULL when a0_in is given */
    const double *T,                          /* f64[G,16] device, row-major T_Cam_AGV */
    const int32_t *pose_index,                /* i32[n] device or NULL = every frame uses T[0] */
    int32_t G, int32_t n, double radius, const CpeFitParams *params,
    const double *a0_in,                      /* f64[n,2] or NULL = closed form from cyl_raw[f,1,3:6] */
    double *angles0, double *angles,          /* [n,2] start and result (pan, tilt) */
    double *fvals, int32_t *iters,            /* [n,2] = [f(a0), f(a)], [iterations, objective evaluations] */
    double *TAGVcyl, double *Tcyl,            /* [n,16] each or NULL */
    int32_t *status, void *stream);

/* ---- local surface curvature of every 3-D point --------------------------------------------------------------------------
 * [K, L] = estCurvatures(Pts3) for n frames (estCurvatures.m with knnsearch, fitplane.m, createLocCoordSys, fitquadsurf, eig:
 * HOT LOOP E of SURVEY.md), one lane per point.  cpe_fit_cylinder_batch computes this for the one point its start needs; this
 * call returns it for all of them.
 *   X f64[n,CPE_MAXP,3], cnt i32[n] as cpe_fit_cylinder_batch takes them: cnt is clamped to [0, CPE_MAXP], slots past it are
 *   never read.  k: neighbours per point, the point itself included (the reference's value: CPE_CURV_K = 20); mode:
 *   CPE_CURV_REFERENCE or CPE_CURV_INTERCEPT.  k must lie in [unknowns, CPE_CURV_MAXK] (unknowns = 5 in mode 0, 6 in mode 1);
 *   an unknown mode or such a k is CPE_ERR_ARG.  A frame with fewer than k points uses all of them (K = min(k, cnt)).  (k and
 *   mode are plain arguments, as the parameters of cpe_mono_shift_batch are, not a structure.)
 * The rule, in this order:
 *   1. Neighbours of point p: d2(j) = (a*a + b*b) + c*c of the coordinate differences X[j] - X[p]; the K smallest by
 *      (d2, index), p itself included -- knnsearch's ties by index; a duplicate of p is a legitimate neighbour.
 *   2. CPE_CURV_REFERENCE: mu = (sum over the neighbours in rank order) / K, per coordinate; C = sum e e' / (K - 1), e = X - mu,
 *      in rank order; z = the first eigenvector of C (cyclic Jacobi, eigenvalues ascending by a stable exchange), negated when
 *      z[2] < 0; x0 = (1,0,0), or (0,1,0) when |z[0]| > 0.9; y = z x x0; x = y x z -- NOT normalised, as createLocCoordSys
 *      leaves them; per neighbour lx = (e.x), ly = (e.y), lz = (e.z), each ((.)+(.))+(.); row = [lx^2, lx ly, ly^2, lx, ly];
 *      M += row row', rhs += row lz in rank order; co = M \ rhs by Gaussian elimination with partial pivoting (first largest
 *      pivot); a = 2 co[0], b = co[1], c = 2 co[2]; hd = (a - c) / 2, mid = (a + c) / 2, rad = sqrt(hd*hd + b*b);
 *      L = [mid - rad, mid + rad]; the eigenvector of lambda is (b, lambda - a) when |lambda - a| >= |lambda - c|, else
 *      (lambda - c, b), divided by its length (a zero length gives (1,0) for the first and (0,1) for the second: eig of a
 *      multiple of the identity); K(:,j) = x v0 + y v1.
 *   3. Bit contract: this is the arithmetic and the summation order of the start of cpe_fit_cylinder_batch, so for the point
 *      that start picks, Kdir[f,p,0,:] has the bits of cyl_raw[f,0,3:6].
 *   4. CPE_CURV_INTERCEPT (build-defined): y is divided by its length before x = y x z (a unit frame), the row is
 *      [lx^2, lx ly, ly^2, lx, ly, 1] and the solve has 6 unknowns; everything else as in mode 0.  L then holds the principal
 *      curvatures in 1/mm up to the small-neighbourhood bias; mode 0's L are the reference's numbers, which are not.
 * Outputs per point: Kdir f64[n,CPE_MAXP,2,3] (Kdir[.,p,j,:] = K(:,j,p), eigenvalues ascending), L f64[n,CPE_MAXP,2],
 *   normal f64[n,CPE_MAXP,3] (the z that was used), nbr i32[n,CPE_MAXP,k] or NULL (the neighbours in rank order; ranks from K
 *   on hold -1), pt_status u8[n,CPE_MAXP]: 0 good, 1 where the elimination meets a zero pivot or a result is not finite --
 *   Kdir, L and normal of that point are then zero.  Every output of a slot past the count is zero.
 * Output per frame: status i32[n] = CPE_ST_OK, or CPE_ST_FEW_POINTS when the count is below the number of unknowns; every
 *   output of that frame is then zero.
 * Asynchronous on `stream`, no allocation, no workspace, no host synchronisation, no atomics; a call repeats its bits and a
 * frame's outputs do not depend on its place in the batch; n == 0 is a no-op. */
#define CPE_CURV_REFERENCE 0 /* estCurvatures.m as it stands */
#define CPE_CURV_INTERCEPT 1 /* build-defined: unit local frame, quadric with a constant term (6 unknowns) */
#define CPE_CURV_MAXK 32
#define CPE_CURV_K 20         /* knnsearch(..., 'K', 20) of estCurvatures.m */
CPE_API int32_t cpe_est_curvatures_batch(const double *X, const int32_t *cnt, int32_t n, int32_t k, int32_t mode, double *Kdir,
                                         double *L, double *normal, int32_t *nbr, uint8_t *pt_status, int32_t *status,
                                         void *stream);

/* BUILD-DEFINED (the reference has nothing like it): what a frame's curvatures say together, one wavefront per frame.
 *   X, cnt and Kdir, L, normal, pt_status as cpe_est_curvatures_batch takes and leaves them; the gate: rho_max (the largest
 *   |lambda|min / |lambda|max of a cylinder-like point; the Python layer's default is 0.25) and the open interval (r_min, r_max)
 *   for 1 / |lambda|max (0 and +inf: no band); rho_max >= 0 and 0 <= r_min < r_max, otherwise CPE_ERR_ARG.
 * A point below the count is gated in when pt_status is 0, |lambda|max > 0, |lambda|min / |lambda|max <= rho_max,
 * r_min < 1 / |lambda|max < r_max, and the column of the smaller |lambda| has a finite length > 0 (|lambda|max is |L[1]| when
 * |L[1]| > |L[0]|, else |L[0]|).  Over the gated points: t = that column / its length; dir = the eigenvector of sum t t' for
 * its largest eigenvalue (Jacobi, as above) with its largest-magnitude component (the first of them) made positive, the sign
 * rule of cpe_index_planes_batch; c = X + normal / lambda_big (signed), the centre of curvature; origin = mean of c; radius =
 * the lower median of 1 / |lambda|max, the element of rank (g - 1) / 2, by exact selection on the bit patterns; spread = the
 * rms distance of the c from the line (origin, dir).  All sums in the fixed lane-strided order and 64-lane tree.
 *   axis f64[n,8] = origin[3], dir[3], radius, spread; n_gated i32[n]; gate u8[n,CPE_MAXP] (zero past the count);
 *   status i32[n] = CPE_ST_OK, or CPE_ST_FEW_POINTS with axis zero when fewer than 3 points are gated in or a result is not
 *   finite (gate and n_gated say what was gated all the same).
 * Asynchronous on `stream`, no allocation, no workspace, no host synchronisation; n == 0 is a no-op. */
CPE_API int32_t cpe_curvature_consensus_batch(const double *X, const int32_t *cnt, int32_t n, const double *Kdir, const double *L,
                                              const double *normal, const uint8_t *pt_status, double rho_max, double r_min,
                                              double r_max, double *axis, int32_t *n_gated, uint8_t *gate, int32_t *status,
                                              void *stream);

/* BUILD-DEFINED, opt-in: the cylinder pose fitted to the PIXELS of both images.  Every other fit here minimises sum (d - R)^2
 * over triangulated points, whose noise is pixel noise stretched along depth.  This call minimises the pixel distance between
 * every detection and the predicted pixel of its own grid node (steps 2 - 10 of cpe_grid_predict_batch): the maximum-likelihood
 * pose for isotropic pixel noise.  It needs no join of the two tables and no triangulation, and uses detections only one camera
 * found.  One wavefront per frame, one launch on `stream`, no atomics, no workspace, no host synchronisation; two calls on
 * equal inputs give equal bits, and a frame's outputs do not depend on its place in the batch.
 *   xy1 f64[n,CPE_MAXP,2], id1 i32[n,CPE_MAXP,2], cnt1 i32[n]: camera 1's tables as cpe_detect_grid_batch writes them; xy2, id2,
 *     cnt2: camera 2's.  Either camera's three pointers may ALL be NULL: that camera is absent.  Both absent, or a camera given
 *     in part: CPE_ERR_ARG.
 *   cyl0 f64[n,6]: the start pose, a point on the axis and a direction of any length, camera-1 coordinates: what
 *     cpe_fit_cylinder_batch writes to cyl[:,1,:]; use u8[n] or NULL (all frames); radius R > 0, finite (it stays fixed)
 *   K1, K2, T21, P f64[2,L,4], line_status i32[2,L], lo, hi, centre f64[3]: exactly as cpe_grid_predict_batch reads them
 *   swap: as CpeTableTriParams.swap (component c of id addresses table family c ^ swap); min_cos in (0, 1): step 9's gate;
 *   gate_px: <= 0 (or NaN) = off; tol_x, tol_f > 0, max_iter >= 1: the Levenberg-Marquardt loop's (at most 200 iterations)
 * Rule per frame (the order is the contract; x = (o, a) are the six unknowns):
 *   1. the frame is unusable when use is 0, any number of cyl0 is not finite, or |a| is 0 or not finite: status
 *      CPE_ST_FEW_POINTS, every numeric output 0 (counts included), pt_state 1 below the counts and -1 past them;
 *   2. cnt1, cnt2 are clamped to [0, CPE_MAXP]; slots past them are never read.  A detection is USABLE when its pixel is finite;
 *      both its indices lie in [lo, hi] and both planes (component c reads family c ^ swap) have line_status CPE_ST_OK; steps 3 - 9
 *      of cpe_grid_predict_batch give CPE_PRED_OK for its node at cyl0; Z > 0 in its own camera; and its predicted pixel
 *      (step 10's formula) is finite.  There is no facing test and no image bound: the detection exists;
 *   3. with gate_px > 0 a usable detection whose residual norm at cyl0 is >= gate_px is gated out.  The used set S is decided
 *      here, once, and never changes, so the objective is smooth;
 *   4. fewer than CPE_PIXFIT_MIN_PTS detections in S: CPE_ST_FEW_POINTS;
 *   5. F(x) = sum over S of (rx rx + ry ry), r = pi_j(X(u, v; x)) - p: X by steps 4 - 8 of the prediction at the pose x, pi_j by
 *      step 10's formula for the detection's camera j.  When any member of S fails steps 6 - 9 or has Z <= 0 at x, or x itself
 *      fails rule 1's test, F(x) is NaN, which the loop treats as a rejected trial;
 *   6. Levenberg-Marquardt from (cyl0, F(cyl0)) on the six unknowns -- lambda from 1e-3, x 10 on a rejected trial, / 10 on an
 *      accepted one, 12 trials per iteration, stop at an improvement <= tol_f 1e-3 (1 + F) with a step <= tol_x: the loop of
 *      cpe_fit_cylinder_batch's CPE_FIT_LM.  The two gauge directions (o along a, |a|) are left to the damping, as there;
 *   7. the Jacobian of a detection's two residuals: g = X - o, ah = a / |a|, gp = g - (g.ah) ah; dt/d(o, a) = (gp,
 *      (g.ah) gp / |a|) / (gp.wh); dX = wh dt; s = (d pi / d Xc) R_j wh with d x / d Xc = (K0 / Z, K1 / Z, -(K0 Xc0 + K1 Xc1) /
 *      Z^2) and d y / d Xc = (0, K4 / Z, -K4 Xc1 / Z^2); the rows are s_x dt and s_y dt (rank one);
 *   8. the outputs are written at the final x.  A final pose or F that is not finite: CPE_ST_FEW_POINTS.
 * Outputs, every slot of every frame written:
 *   cyl f64[n,6] the final pose as the loop left it (no prior applied); fvals f64[n,2] = F(cyl0), F(cyl); iters i32[n,2] =
 *   iterations, objective evaluations (F(cyl0) included); counts i32[n,4] = |S| of camera 1 | of camera 2 | detections below
 *   the counts refused by rule 2 | gated by rule 3; stats f64[n,4] = rms residual norm of camera 1 | of camera 2 |
 *   sqrt(F / |S|) | the largest residual norm, pixels at cyl; status i32[n].
 *   Optional (NULL: not written): res f64[n,2,CPE_MAXP,2] the residual (predicted - detected) per camera and slot at cyl;
 *   pt_state i32[n,2,CPE_MAXP]: 0 in S, 1 refused by rule 2, 2 gated, -1 past the count (every slot of an absent camera);
 *   X f64[n,2,CPE_MAXP,3] the node's 3-D point at cyl.  res and X are 0 outside S and past the counts.
 *   With CPE_ST_FEW_POINTS by rule 4 or 8, cyl, fvals, iters, stats, res and X are zero; counts and pt_state say what rules 2
 *   and 3 decided all the same.  So CPE_ST_OK implies finite outputs.
 * CPE_ERR_ARG, nothing launched or written: radius not finite or <= 0; L outside 1..CPE_MAXL; min_cos outside (0, 1); swap other
 * than 0 or 1; tol_x or tol_f not > 0; max_iter < 1; a NULL required pointer; an output that overlaps an input or another
 * output.  n == 0 is a no-op.
 * Limits: the radius is fixed and the cylinder ideal and rigid; the table's errors enter as for every table-based call; the
 * indices are trusted (re-number first: cpe_grid_assign_batch); S is fixed at the start pose; no covariance is returned;
 * planar targets are not covered. */
#define CPE_PIXFIT_MIN_PTS 6
CPE_API int32_t cpe_fit_cylinder_pixels_batch(const double *xy1, const int32_t *id1, const int32_t *cnt1, const double *xy2,
                                              const int32_t *id2, const int32_t *cnt2, const double *cyl0, const uint8_t *use,
                                              int32_t n, double radius, const double *K1, const double *K2, const double *T21,
                                              const double *P, const int32_t *line_status, int32_t lo, int32_t hi,
                                              const double *centre, int32_t swap, double min_cos, double gate_px, double tol_x,
                                              double tol_f, int32_t max_iter, double *cyl, double *fvals, int32_t *iters,
                                              int32_t *counts, double *stats, int32_t *status, double *res, int32_t *pt_state,
                                              double *X, void *stream);

/* Row f-1, BUILD-DEFINED, opt-in: T_Cam_AGV fitted to the PIXELS of every frame of a group at once.  The three point-based forms
 * (cpe_multi_frame_fit_batch, _lm_batch, _consensus_batch) minimise dist - R over triangulated points; cpe_fit_cylinder_pixels_batch
 * fits one frame's four observable unknowns alone.  Here every kept frame's cylinder is T_Cam_AGV * getTAGVcyl(pan, tilt) and the
 * six unknowns of T_Cam_AGV are fitted to every detection of every kept frame: the maximum-likelihood calibration for isotropic
 * pixel noise, with the laser table rigid in camera-1 coordinates across the frames.  One workgroup per group, one launch on
 * `stream`, no atomics, no workspace, no allocation, no host synchronisation; two calls on equal inputs give equal bits, and a
 * group's outputs do not depend on its place in the batch.
 *   xy1, id1, cnt1, xy2, id2, cnt2: the two cameras' tables for n frames, exactly as cpe_fit_cylinder_pixels_batch takes them
 *     (either camera may be absent: all three pointers NULL; both absent, or one given in part: CPE_ERR_ARG)
 *   TAGVcyl f64[n,16], frame_ok i32[n] or NULL, group_start i32[G+1] (device), G, n: exactly as cpe_multi_frame_fit_lm_batch takes
 *     them (kept frames, CPE_MULTI_MAXF, CPE_ST_OVERFLOW).  Unlike there, the ranges of two groups may not share a frame: pt_state
 *     holds the membership of S while the call runs (not checked)
 *   x0_in f64[G,6], REQUIRED: the start [rotation vector, translation] of T_Cam_AGV, as the point-based calls return in x.  There
 *     is no closed-form start in pixel space: NULL is CPE_ERR_ARG
 *   radius, K1, K2, T21, P, line_status, lo, hi, centre, swap, min_cos, gate_px, tol_x, tol_f, max_iter: as
 *     cpe_fit_cylinder_pixels_batch, with the same CPE_ERR_ARG cases
 *   sel_cos in [min_cos, 1): the grazing gate for MEMBERSHIP only (rule 3); outside that range: CPE_ERR_ARG.  A silhouette node
 *     that just exists at the start pose ceases to exist a step later and its NaN refuses every such trial; members chosen with
 *     a stricter gate than the one they are evaluated with keep their nodes on the way (the Python layer's default is 0.35)
 * Rule per group (the order is the contract):
 *   1. the kept frames are those of cpe_multi_frame_fit_lm_batch; fewer than two: CPE_ST_FEW_POINTS.  Any number of x0_in[g] not
 *      finite: CPE_ST_FEW_POINTS;
 *   2. the pose of kept frame i at x: o_i = Rot p_i + t, a_i = Rot a_col_i with [Rot t] = vec2T(x) and a_col_i, p_i columns 2 and 4
 *      of TAGVcyl_i (the axis and origin cpe_multi_frame_terms uses);
 *   3. the used set S, decided ONCE at x0: a detection of a kept frame belongs to S when it passes rule 2 of
 *      cpe_fit_cylinder_pixels_batch at the pose (o_i, a_i) with sel_cos in place of min_cos, and, with gate_px > 0, its residual
 *      norm is below gate_px.  A kept frame contributes what it has, down to nothing.  |S| over the group below
 *      CPE_PIXFIT_MIN_PTS, or fewer than two kept frames with a member: CPE_ST_FEW_POINTS;
 *   4. F(x) = sum over S of (rx rx + ry ry), evaluated with min_cos.  When any member fails at x, or x or any kept frame's pose is
 *      not finite, F(x) is NaN and the trial is rejected;
 *   5. Levenberg-Marquardt from (x0, F(x0)) on six unknowns: the loop of cpe_multi_frame_fit_lm_batch (damping, 12 trials per
 *      iteration, stop rule, at most min(max_iter, 200) iterations) with its step Rot <- exp([dw]x) Rot, t <- t + dt, the candidate
 *      x = T2vec of that pose;
 *   6. the Jacobian of a member's two residuals: with u = gp / den, w = (g.ah) gp / (|a| den), s_x, s_y of rule 7 of
 *      cpe_fit_cylinder_pixels_batch at (o_i, a_i) and m_i = Rot p_i:  j_w = m_i x u + a_i x w,  j_t = u;  the rows are s_x (j_w, j_t)
 *      and s_y (j_w, j_t)  (do = dw x m_i + dt, da = dw x a_i);
 *   7. the outputs are written at the final x.  A final x or F that is not finite: CPE_ST_FEW_POINTS.
 * Outputs per group, every slot written: x f64[G,6]; T f64[G,16] = vec2T(x); fvals f64[G,2] = F(x0), F(x); iters i32[G,2] =
 *   iterations, objective evaluations (F(x0) included); n_used i32[G] kept frames; counts i32[G,4] = |S| of camera 1 | of camera 2
 *   | refused | gated, over the kept frames; stats f64[G,4] = rms residual norm of camera 1 | of camera 2 | sqrt(F / |S|) | the
 *   largest residual norm; status i32[G]; N f64[G,21] or NULL: the upper triangle (packed by rows) of J'J at x in the step's
 *   coordinates (dw, dt), from one more Jacobian pass that iters does not count -- the covariance of (dw, dt) is
 *   F / (2 |S| - 6) * inverse(N).  A group that is not CPE_ST_OK has every other per-group output zero.
 * Outputs per frame: pt_state i32[n,2,CPE_MAXP], REQUIRED: 0 in S, 1 refused, 2 gated, -1 past the count (every slot of an absent
 *   camera); written for every frame of every group's range, kept or not, whatever the group's status (a range outside [0, n]
 *   excepted); a frame that is not kept, and every frame of a group that rule 1 refuses, has 1 below the counts.
 *   frame_cyl f64[n,6] = (o_i, a_i) at x; frame_stats f64[n,4] = the frame's rms of camera 1 | of camera 2 | of both | largest
 *   residual norm (0 where it has no member); res f64[n,2,CPE_MAXP,2] or NULL: predicted - detected at x, 0 outside S and past the
 *   counts.  These three are written only for the kept frames of groups that end CPE_ST_OK, as frame_terms of
 *   cpe_multi_frame_fit_lm_batch is: initialise them.
 * CPE_ERR_ARG, nothing launched or written: the cases of cpe_fit_cylinder_pixels_batch; sel_cos outside [min_cos, 1); G < 0 or
 * n < 0; a NULL required pointer (x0_in and pt_state among them); an output that overlaps an input or another output.  G == 0 is
 * a no-op.
 * Limits: the radius is fixed and the cylinder ideal and rigid; the table must be rigid with camera 1 across the frames; the
 * indices are trusted (re-number first); S is fixed at the start pose, so the start must come from a point-based multi-frame fit;
 * the nominal pan and tilt are taken as exact. */
CPE_API int32_t cpe_multi_frame_fit_pixels_batch(const double *xy1, const int32_t *id1, const int32_t *cnt1, const double *xy2,
                                                 const int32_t *id2, const int32_t *cnt2, const double *TAGVcyl,
                                                 const int32_t *frame_ok, const int32_t *group_start, int32_t G, int32_t n,
                                                 const double *x0_in, double radius, const double *K1, const double *K2,
                                                 const double *T21, const double *P, const int32_t *line_status, int32_t lo,
                                                 int32_t hi, const double *centre, int32_t swap, double min_cos, double sel_cos,
                                                 double gate_px, double tol_x, double tol_f, int32_t max_iter, double *x, double *T,
                                                 double *fvals, int32_t *iters, int32_t *n_used, int32_t *counts, double *stats,
                                                 int32_t *status, double *N, int32_t *pt_state, double *frame_cyl,
                                                 double *frame_stats, double *res, void *stream);

/* Row f-1, BUILD-DEFINED, opt-in: T_Cam_AGV AND every kept frame's pan and tilt fitted jointly to the PIXELS of a group.
 * cpe_multi_frame_fit_pixels_batch takes the nominal angles as exact; the head has a finite repeatability, and an angle error of
 * 0.17 degrees keeps that fit a factor 3 - 5 above the noise floor.  Here the unknowns are the six of
 * T_Cam_AGV and (pan_i, tilt_i) of every kept frame, 6 + 2 F in all, with a Gaussian prior that holds each angle at its nominal
 * value with the weight w = sigma_pixel / sigma_angle.  The system is an arrowhead: the angles of a frame meet only that frame's
 * detections, so every trial eliminates the 2 x 2 blocks in closed form and solves a 6 x 6 system.  One workgroup per group, one
 * launch on `stream`, no atomics, no workspace, no allocation, no host synchronisation; two calls on equal inputs give equal
 * bits, and a group's outputs do not depend on its place in the batch.
 *   xy1 .. cnt2, frame_ok, group_start, G, n, x0_in, radius, K1, K2, T21, P, line_status, lo, hi, centre, swap, min_cos, sel_cos,
 *     gate_px, tol_x, tol_f, max_iter: exactly as cpe_multi_frame_fit_pixels_batch takes them, with the same CPE_ERR_ARG cases
 *   angles0 f64[n,2]: the nominal (pan, tilt) of every frame in rad, in place of TAGVcyl; the chain getTAGVcyl(pan, tilt) is
 *     evaluated in the kernel with the bits of cpe_agv_chain_batch
 *   w_pan, w_tilt: the prior weights in pixels per radian; both finite and > 0, otherwise CPE_ERR_ARG
 *   CPE_MFJOINT_MAXF: the most kept frames of one group (the per-frame blocks live in LDS); more: CPE_ST_OVERFLOW.  The
 *     fixed-angle call remains for larger groups
 * Rule per group (the order is the contract):
 *   1. the kept frames and the refusals of x0_in are those of cpe_multi_frame_fit_pixels_batch's rule 1;
 *   2. the pose of kept frame i at (x, q_i), q_i = (pan_i, tilt_i): (o_i, a_i) of that call's rule 2 with getTAGVcyl(q_i) for
 *      TAGVcyl_i.  It is usable when o_i, a_i and q_i are finite, |a_i| != 0 and |tilt_i| < pi/2 - 1e-3 (the pole of the chain's
 *      tan, the rule of cpe_frame_angles_lm_batch);
 *   3. the used set S, decided ONCE at (x0, angles0) by that call's rule 3: sel_cos, then gate_px; a frame whose pose is not
 *      usable has no member.  |S| below CPE_PIXFIT_MIN_PTS, or fewer than two kept frames with a member: CPE_ST_FEW_POINTS;
 *   4. F(x, q) = sum over S of (rx rx + ry ry) + sum over the kept frames of (w_pan^2 (pan_i - pan_i0)^2 + w_tilt^2 (tilt_i -
 *      tilt_i0)^2), the pixel part evaluated with min_cos.  F is NaN when a member fails, when x or a kept frame's pose is not
 *      usable (rule 2), and the trial is rejected;
 *   5. the Jacobian of a member's two residuals: with u, w, s_x, s_y and the pose columns j_w, j_t of that call's rule 6, and
 *      dp / dq_k, da / dq_k the derivatives of columns 4 and 2 of the chain by pan (k = 0) and tilt (k = 1):
 *      j_q,k = u . (Rot dp / dq_k) + w . (Rot da / dq_k); the rows are s_x (j_w, j_t, j_q) and s_y (j_w, j_t, j_q).  The prior
 *      adds w_k^2 to the diagonal of the frame's 2 x 2 block and w_k^2 (q_k - q_k0) to its gradient;
 *   6. the normal equations in blocks: U (upper triangle, 21 sums) and g_x (6) of the pose columns; per kept frame V_i (3: 00 01
 *      11), W_i (6 x 2, pose column by angle) and g_i (2);
 *   7. one damped trial: every diagonal entry a of U and of every V_i becomes a + lambda a + 1e-12 (that block's own trace); V_i
 *      is inverted in closed form; Y_i = W_i inverse(V_i); S = U - sum Y_i W_i'; b = -g_x + sum Y_i g_i; S dx = b by Gaussian
 *      elimination with partial pivoting; dq_i = -inverse(V_i) (g_i + W_i' dx).  A zero determinant of any block is a rejected
 *      trial that is not evaluated;
 *   8. the loop of cpe_multi_frame_fit_lm_batch: lambda from 1e-3, x 10 on a rejected trial, / 10 (floor 1e-12) on an accepted
 *      one, 12 trials per iteration, at most min(max_iter, 200) iterations, stop at an improvement <= tol_f 1e-3 (1 + F) with a
 *      step <= tol_x, the step taken as the largest |.| over dx and every dq_i.  The candidate is Rot <- exp([dw]x) Rot, t <- t +
 *      dt, q_i <- q_i + dq_i;
 *   9. a kept frame without a member has W_i = 0 and g_i = 0 and keeps its nominal angles bit for bit (an angle whose step is
 *      zero is copied, not added to: -0.0 stays -0.0);
 *  10. the outputs are written at the final (x, q).  A final x or F that is not finite: CPE_ST_FEW_POINTS.
 * Outputs: x, T, fvals, iters, n_used, counts, stats, status, pt_state, frame_cyl, frame_stats, res as
 *   cpe_multi_frame_fit_pixels_batch writes them, with fvals = F(x0, angles0), F(x, q) (the prior included) and stats[2] = the rms
 *   residual norm over S (the prior excluded), and
 *   N f64[G,21] or NULL: the upper triangle of the undamped reduced matrix U - sum W_i inverse(V_i) W_i' at the result, from one
 *     more Jacobian pass that iters does not count.  The covariance of (dw, dt) with the angles marginalised is
 *     F / (2 |S| - 6) * inverse(N): the 2 F prior rows and the 2 F angles cancel in the degrees of freedom;
 *   angles f64[n,2], REQUIRED: the fitted (pan, tilt);
 *   frame_N f64[n,17] or NULL: V_i (3) | W_i (12, row-major 6 x 2) | g_i (2) at the result, the prior included.
 *   angles and frame_N are written only for the kept frames of groups that end CPE_ST_OK, as frame_cyl is: initialise them.
 * CPE_ERR_ARG, nothing launched or written: the cases of cpe_multi_frame_fit_pixels_batch (angles0 and angles among the required
 * pointers); w_pan or w_tilt not finite or <= 0.  G == 0 is a no-op.
 * Limits: those of cpe_multi_frame_fit_pixels_batch except its last (the radius is fixed and the cylinder ideal and rigid; the
 * table must be rigid with camera 1 across the frames; the indices are trusted; S is fixed at the start); a pan offset common to
 * all frames is the same thing as a rotation of T_Cam_AGV (the chain's leftmost factor is Rz(pan)), so that direction is held by
 * the prior alone and T_Cam_AGV gains less than the frames' cylinders do; with exact angles the frames' cylinders end 2 - 15 x
 * farther off than the fixed-angle call's (still below 0.03 degrees and 0.09 mm on the test scenes); there is one weight pair per call; a group holds at most CPE_MFJOINT_MAXF kept frames. */
#define CPE_MFJOINT_MAXF 256
CPE_API int32_t cpe_multi_frame_fit_pixels_angles_batch(const double *xy1, const int32_t *id1, const int32_t *cnt1, const double *xy2,
                                                        const int32_t *id2, const int32_t *cnt2, const double *angles0,
                                                        const int32_t *frame_ok, const int32_t *group_start, int32_t G, int32_t n,
                                                        const double *x0_in, double w_pan, double w_tilt, double radius,
                                                        const double *K1, const double *K2, const double *T21, const double *P,
                                                        const int32_t *line_status, int32_t lo, int32_t hi, const double *centre,
                                                        int32_t swap, double min_cos, double sel_cos, double gate_px, double tol_x,
                                                        double tol_f, int32_t max_iter, double *x, double *T, double *fvals,
                                                        int32_t *iters, int32_t *n_used, int32_t *counts, double *stats,
                                                        int32_t *status, double *N, int32_t *pt_state, double *frame_cyl,
                                                        double *frame_stats, double *res, double *angles, double *frame_N,
                                                        void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CPE_H */
