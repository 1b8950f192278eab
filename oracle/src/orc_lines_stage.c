/*
 * ORACLE (test infrastructure) -- the lines stage as one call: from the label lookup of the joints to the sorted point
 * table, i.e. what detect_grid does after expand_line_roi
 *   cylinder script: util_cylinder.color_and_expand_lines (:2014-2060) from cv2.connectedComponents on, then indexing_data
 *   planar script:   util_plane.color_and_expand_lines (:2799-2845), degree 1, no remove_label / remove_minus_labels
 * orc_detect_grid_ex, orc_detect_grid_bgr and orc_detect_grid_plane run their frames through orc_lines_core, so the stage a
 * test drives on its own (orc_lines_stage) is the code the golden vectors pin.
 */
#include "orc_common.h"

#include "orc_lines.h"

int orc_connected_components(const uint8_t *mask, int h, int w, int32_t *labels);
void orc_group_points(const int *cent, int n, const int32_t *labels, int lh, int lw, int x_off, int y_off, orc_lineset *out);
void orc_fit_lines(orc_lineset *ls, int is_row);
void orc_remove_label(orc_lineset *rows, orc_lineset *cols);
void orc_intersections(orc_lineset *rows, orc_lineset *cols, const int *rect);
void orc_clean_and_relabel(orc_lineset *rows, orc_lineset *cols);
int orc_subpixel_refine(const uint8_t *gray, int h, int w, orc_lineset *rows, orc_lineset *cols, int window, double step);
int orc_index_points(const orc_lineset *rows, const orc_lineset *cols, const uint8_t *gauss7, int h, int w, int r0,
                     double *center, double *xy, int *id, int cap);
void orc_fit_lines_plane(orc_lineset *rows, orc_lineset *cols);
void orc_intersections_plane(orc_lineset *rows, orc_lineset *cols, const int *rect);
void orc_clean_plane(orc_lineset *ls);
int orc_index_points_plane(const orc_lineset *rows, const orc_lineset *cols, const uint8_t *gauss7, int h, int w, int radius,
                           double *center, double *xy, int *id, int cap);

/* more samples on one line than the library's sample buffer holds (sp_cap per line; <= 0: no limit): build-defined overflow */
static void sample_capacity(const orc_lineset *ls, double step, int sp_cap)
{
    for (int g = 0; g < ls->nlines; g++) {
        const double lo = ls->eq[g][3], hi = ls->eq[g][4];
        if (hi < lo) continue;
        if (ceil(((hi + 0.0001) - lo) / step) > (double)sp_cap) orc_capacity_overflow = 1;
    }
}

/* exp_h / exp_v: the expanded masks (h x w); cyl: the ncyl joints inside rect, in contour order; gauss7: the 7x7-blurred
 * image indexing_data reads; gray: read by the sub-pixel refinement only.  rows / cols: caller's storage, on return the
 * line sets as the stage leaves them (after clean_and_relabel when the status is 0, 3 or 4); n_groups (may be NULL): the
 * label groups per direction before any line is removed.
 * Returns the status 0, 3, 4 or 7 and *n_out; sets orc_capacity_overflow where a capacity of include/cpe.h is exceeded
 * (the callers turn that into ORC_ST_OVERFLOW). */
int orc_lines_core(const uint8_t *exp_h, const uint8_t *exp_v, int h, int w, const int *cyl, int ncyl, const int *rect, int r0,
                   const uint8_t *gauss7, const uint8_t *gray, int subpixel, int sp_window, double sp_step, int sp_cap,
                   int planar, double *center, double *xy, int *id, int cap, int *n_out, orc_lineset *rows, orc_lineset *cols,
                   int *n_groups)
{
    int st = 0;
    int x0 = rect[0], y0 = rect[1], cw = rect[2], ch = rect[3];
    *n_out = 0;
    /* numpy slicing clips the crop at the image border */
    if (x0 + cw > w) cw = w - x0;
    if (y0 + ch > h) ch = h - y0;
    if (cw < 0) cw = 0;
    if (ch < 0) ch = 0;
    uint8_t *crop = (uint8_t *)calloc((size_t)cw * ch + 1, 1);
    int32_t *lab_h = (int32_t *)malloc((size_t)cw * ch * sizeof(int32_t));
    int32_t *lab_v = (int32_t *)malloc((size_t)cw * ch * sizeof(int32_t));
    for (int y = 0; y < ch; y++) memcpy(crop + (size_t)y * cw, exp_h + (size_t)(y0 + y) * w + x0, (size_t)cw);
    orc_connected_components(crop, ch, cw, lab_h);
    for (int y = 0; y < ch; y++) memcpy(crop + (size_t)y * cw, exp_v + (size_t)(y0 + y) * w + x0, (size_t)cw);
    orc_connected_components(crop, ch, cw, lab_v);
    orc_group_points(cyl, ncyl, lab_h, ch, cw, x0, y0, rows);
    orc_group_points(cyl, ncyl, lab_v, ch, cw, x0, y0, cols);
    if (n_groups) { n_groups[0] = rows->nlines; n_groups[1] = cols->nlines; }
    int n = 0;
    if (planar) {
        orc_fit_lines_plane(rows, cols);
        orc_intersections_plane(rows, cols, rect);
        orc_clean_plane(rows);
        orc_clean_plane(cols);
        n = orc_index_points_plane(rows, cols, gauss7, h, w, r0, center, xy, id, cap);
    } else {
        orc_fit_lines(cols, 0);
        orc_fit_lines(rows, 1);
        orc_remove_label(rows, cols);
        if (subpixel) {
            if (sp_cap > 0) { sample_capacity(rows, sp_step, sp_cap); sample_capacity(cols, sp_step, sp_cap); }
            st = orc_subpixel_refine(gray, h, w, rows, cols, sp_window, sp_step);
        }
        if (st == 0) {
            orc_intersections(rows, cols, rect);
            orc_clean_and_relabel(rows, cols);
            n = orc_index_points(rows, cols, gauss7, h, w, r0, center, xy, id, cap);
        }
    }
    if (st == 0) {
        if (n < 0) st = -n;
        else if (n > CPE_MAXP) orc_capacity_overflow = 1;   /* more grid points than a table of the boundary holds */
        else *n_out = n;
    }
    free(crop); free(lab_h); free(lab_v);
    return st;
}

/* The stage on its own.  joints: nj x 2 (x, y), already filtered to rect; more than CPE_MAXJ is an overflow, as in
 * orc_detect_grid_ex.  sp_cap: samples per line the sub-pixel refinement may take (the library's: max(h, w) + 128).
 * Returns the status with the overflow rule applied (ORC_ST_OVERFLOW, *n_out = 0); *overflow: the flag itself. */
ORC_API int orc_lines_stage(const uint8_t *exp_h, const uint8_t *exp_v, int h, int w, const int *joints, int nj, const int *rect,
                            int r0, const uint8_t *gauss7, const uint8_t *gray, int subpixel, int sp_window, double sp_step,
                            int sp_cap, int planar, double *center, double *xy, int *id, int cap, int *n_out,
                            orc_lineset *rows, orc_lineset *cols, int *n_groups, int *overflow)
{
    orc_capacity_overflow = 0;
    if (nj > CPE_MAXJ) { orc_capacity_overflow = 1; nj = CPE_MAXJ; }
    int st = orc_lines_core(exp_h, exp_v, h, w, joints, nj, rect, r0, gauss7, gray, subpixel, sp_window, sp_step, sp_cap, planar,
                            center, xy, id, cap, n_out, rows, cols, n_groups);
    if (overflow) *overflow = orc_capacity_overflow;
    if (orc_capacity_overflow) { st = ORC_ST_OVERFLOW; *n_out = 0; }
    return st;
}
