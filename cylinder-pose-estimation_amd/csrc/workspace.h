// The detect workspace: one table of named buffers (included by detect.hip only; all of it is host code).
// Every stage of detect_grid works inside one caller-supplied block (cpe_detect_workspace_bytes), plane-major: buffer b holds
// [n][bytes_per_frame(b)] bytes, so every kernel streams [n, h, w] planes with fully coalesced accesses.
#pragma once
#include "cpe_dev.h"
#include <algorithm>
#include <string.h>

namespace cpe {
namespace {

// Buffers whose lifetimes never overlap share memory.  The call is three chains -- ridge mask / joints, saturated spot,
// region -- that run side by side and meet in the masks stage, then the lines stage; only buffers of ONE chain, or of stages
// separated by the join, may be paired.  An overlay is a set of sides that start at the same offset; the buffers of one side
// lie one after the other, and the overlay is as large as its largest side.
enum WsOverlay {
    OV_NONE = 0,
    // borders | groups: the border points and the distance scratch of the blob tracers are read last by k_blob_median; the
    // blob groups are first written by k_blob_merge (.. k_discs), which follows the medians on the caller's stream.
    OV_BORDERS,
    // bright forest | masks: the forest and its accumulator are read last by k_enclosed_all.  The other side is first written
    // by the region stage's clearing of the disc-union image and mask_contour after k_blob_merge, on the same stream; the
    // masks stage's planes and the 7x7 blur follow behind the join.
    // (Colour frames: the L plane borrows the disc-union plane before the sweep; CLAHE has read it when the forest is seeded.)
    // mask_contour and blur7 are readable after the call: nothing is written over this overlay after the forest is dead.
    OV_BRIGHT,
    // chain labels | lines | tracer tables: the label planes of the joints and spot chains are only needed inside those
    // chains' own labelling (roots-only passes: last reader ccl_components of each chain).  The border-chunk ids and distance
    // offsets of the blob tracers live there between the hole traces (first writer k_blob_trace<1>, whose stream waits for
    // RegionSide::joints_done / spot_done) and the medians (last reader k_blob_median); the masks stage then labels the
    // vertical fragment mask in the spot plane again, and the lines stage's tables (first writer lines_stage, last of all)
    // come after that.
    OV_CHAINS,
    // dark forest | blob records: the forest and its per-root counts are read last by the last dark step of the sweep
    // (k_sw_snap); the blob records are first written by the hole traces that follow it and read last by k_blob_merge.  After
    // k_discs the forest plane serves again for the region's own labelling, then the two as the expanded masks' label planes.
    OV_DARK,
    OV_COUNT
};

// capacities of the blob sweep that grow with the frame (border points per threshold ~ cells x perimeter)
static int region_maxch(int h, int w) { long long v = (long long)h * w / 256; return (int)std::min(65535LL, std::max(8192LL, v)); }
static int region_maxdf(int h, int w) { long long v = (long long)h * w / 16; return (int)std::max(65536LL, v); }   // x 17, pooled

// X(identifier, bytes per frame in terms of N = h * w, h, w; public CPE_PLANE_* number or -1; overlay, side)
// The printable name is the identifier in lower case.  Buffers are placed overlay by overlay, then the rest in table order.
// A buffer that serves several roles in sequence has one row; its roles are listed in the row's comment.
#define CPE_WS_TABLE(X) \
    X(DISTS,  (size_t)17 * region_maxdf(h, w) * sizeof(double), -1, OV_BORDERS, 0)   /* distance scratch of the tracers */ \
    X(POOL,   (size_t)17 * region_maxch(h, w) * 128,            -1, OV_BORDERS, 0)   /* border points of the traces (chunked) */ \
    X(GROUPS, (size_t)MAXG * sizeof(Group),                     -1, OV_BORDERS, 1)   /* blob groups */ \
    X(BRIGHT_NODES,  N * 8, -1, OV_BRIGHT, 0)   /* bright forest of the blob sweep: {parent, merge-history word} per pixel */ \
    X(BRIGHT_COUNTS, N * 4, -1, OV_BRIGHT, 0)   /* ... its per-root accumulator */ \
    X(ROI_H,  N, CPE_PLANE_ROI_H, OV_BRIGHT, 1) \
    X(ROI_V,  N, CPE_PLANE_ROI_V, OV_BRIGHT, 1) \
    X(BASE_H, N, -1, OV_BRIGHT, 1)              /* bytes of the fragment masks' base: written only where the labelling reads bytes */ \
    X(BASE_V, N, -1, OV_BRIGHT, 1) \
    X(EXP_H,  N, CPE_PLANE_EXP_H, OV_BRIGHT, 1) \
    X(EXP_V,  N, CPE_PLANE_EXP_V, OV_BRIGHT, 1) \
    X(TMPA,   N, -1, OV_BRIGHT, 1)              /* unused since the expansion stores into EXP_* directly (the overlay costs no memory) */ \
    X(TMPB,   N, -1, OV_BRIGHT, 1)              /* unused, as TMPA */ \
    X(DISCS,  N, -1, OV_BRIGHT, 1)              /* disc-union image (widths whose union is not drawn straight into its one-bit plane); before the sweep, the L plane of colour frames */ \
    X(MASK_CONTOUR, N, CPE_PLANE_MASK_CONTOUR, OV_BRIGHT, 1) \
    X(BLUR7,  N, CPE_PLANE_BLUR7, OV_BRIGHT, 1) \
    X(LABELS_JOINTS, N * 4, -1, OV_CHAINS, 0)   /* label plane of the joints chain */ \
    X(LABELS_SPOT,   N * 4, -1, OV_CHAINS, 0)   /* label plane of the spot chain, then of the vertical fragment mask */ \
    X(LINES,  lines_ws_bytes(), -1, OV_CHAINS, 1)   /* the lines stage's tables (cpe_detect_line_tables, results_*) */ \
    X(SUBPIX, (size_t)2 * MAXL * 2 * (size_t)(std::max(h, w) + 128) * sizeof(float), -1, OV_CHAINS, 1) \
    X(BLOB_CH, (size_t)17 * MAXB * 16 * sizeof(unsigned short), -1, OV_CHAINS, 2)   /* first 16 chunk ids of every blob's border */ \
    X(BLOB_D,  (size_t)17 * MAXB * 2 * sizeof(int),             -1, OV_CHAINS, 2)   /* (chunk | distance offset, points) per blob */ \
    X(LABELS,     N * 4, CPE_PLANE_LABELS, OV_DARK, 0)   /* dark forest -> the region's labelling -> lab_h; cpe_debug_ccl's labels */ \
    X(LABELS_AUX, N * 4, -1, OV_DARK, 0)        /* per-root pixel counts beside LABELS (dark sweep, cpe_debug_ccl) -> lab_v */ \
    X(BLOBS,  (size_t)17 * MAXB * sizeof(BlobRec), -1, OV_DARK, 1)   /* blob records */ \
    X(BINARY, N, CPE_PLANE_BINARY, OV_NONE, 0) \
    X(HMASK,  N, CPE_PLANE_HMASK, OV_NONE, 0) \
    X(VMASK,  N, CPE_PLANE_VMASK, OV_NONE, 0) \
    X(JOINTS, (size_t)MAXJ * 2 * sizeof(int), CPE_PLANE_JOINTS, OV_NONE, 0) \
    X(STATE,  sizeof(FrameState), CPE_PLANE_STATE, OV_NONE, 0) \
    X(CLAHE,  N, CPE_PLANE_CLAHE, OV_NONE, 0)   /* CLAHE'd L channel; planar target, colour frames: the any-channel mask */ \
    X(BLUR19, N, CPE_PLANE_BLUR19, OV_NONE, 0) \
    X(JOINTS_MASK, N, -1, OV_NONE, 0)           /* joints mask as bytes; where its readers take JOINT_BITS (rows of 16 k pixels): hmask, vmask as one-bit planes, n frames each */ \
    X(CM,     N, -1, OV_NONE, 0) \
    X(TOUCH,  N, -1, OV_NONE, 0) \
    X(ROOTS,  (size_t)MAXROOTS * sizeof(int), -1, OV_NONE, 0) \
    X(JTMP,   (size_t)MAXJ * 3 * sizeof(int), -1, OV_NONE, 0) \
    X(VERTS,  (size_t)MAXV * 2 * sizeof(int), -1, OV_NONE, 0) \
    X(BEST,   sizeof(unsigned long long), -1, OV_NONE, 0)   /* largest-contour key of the region */ \
    X(SEGS,   (size_t)2 * MAXSEG * sizeof(SegRec), -1, OV_NONE, 0) \
    X(HIST,   16 * 256 * sizeof(unsigned int), -1, OV_NONE, 0) \
    X(LUT,    16 * 256, -1, OV_NONE, 0) \
    X(ORDER,  (size_t)2 * MAXB * sizeof(int), -1, OV_NONE, 0)   /* + scratch of k_blob_merge's bucketed ranking; then the key-point records of the disc union */ \
    X(LOHI,   (size_t)2 * w * sizeof(int), -1, OV_NONE, 0) \
    X(HULL,   (size_t)4 * w * sizeof(int), -1, OV_NONE, 0) \
    X(NRECT,  16 * sizeof(int), -1, OV_NONE, 0)             /* CLAHE's bounding box */ \
    X(SWEEP,  192 * sizeof(int), CPE_PLANE_SWEEP, OV_NONE, 0) \
    X(LIST_DARK,   (size_t)sweep_pool(h, w, SWL_DARK) * sizeof(int2),   -1, OV_NONE, 0)   /* component lists of the blob sweep */ \
    X(LIST_BRIGHT, (size_t)sweep_pool(h, w, SWL_BRIGHT) * sizeof(int2), -1, OV_NONE, 0) \
    X(LIST_TRACE,  (size_t)sweep_pool(h, w, SWL_TRACE) * sizeof(int2),  -1, OV_NONE, 0) \
    X(BUCKET_PIXELS, N * 4, -1, OV_NONE, 0)     /* the sweep's pixels sorted by grey-level bucket */ \
    X(BITS,   (size_t)17 * bit_plane_words(h, w) * 8, -1, OV_NONE, 0)   /* 17 one-bit planes (cpe_dev.h tiled layout) */ \
    X(ROOTS_JOINTS, (size_t)MAXROOTS * sizeof(int), -1, OV_NONE, 0) \
    X(ROOTS_SPOT,   (size_t)MAXROOTS * sizeof(int), -1, OV_NONE, 0) \
    X(BEST_SPOT,    sizeof(unsigned long long), -1, OV_NONE, 0) \
    X(JOINT_BITS,   bit_plane_words(h, w) * 8, -1, OV_NONE, 0)   /* one-bit plane of the joints mask, written by k_open20_joints */ \
    X(GMID,   (size_t)(MAXG - MAXG_LDS) * 4 * sizeof(double), -1, OV_NONE, 0)   /* x, y, r, next group in the grid cell */ \
    X(FLJ,    (size_t)2 * h * ((w + 63) / 64) * sizeof(unsigned long long), -1, OV_NONE, 0)   /* joints chain: background / outer-background bit masks */ \
    X(GRAYIN, N, -1, OV_NONE, 0)                /* grey plane of colour frames */

enum WsId {
#define X(id, bytes, pub, ov, side) WS_##id,
    CPE_WS_TABLE(X)
#undef X
    WS_COUNT
};

struct WsRow { const char *name; int public_plane; WsOverlay overlay; int side; };
constexpr WsRow WS_ROWS[WS_COUNT] = {
#define X(id, bytes, pub, ov, side) {#id, pub, ov, side},
    CPE_WS_TABLE(X)
#undef X
};
constexpr int WS_SIDES = 3;
constexpr bool ws_sides_ok()   // make_layout places sides 0 .. WS_SIDES - 1 of an overlay
{
    for (int i = 0; i < WS_COUNT; i++)
        if (WS_ROWS[i].side < 0 || WS_ROWS[i].side >= WS_SIDES) return false;
    return true;
}
static_assert(ws_sides_ok(), "CPE_WS_TABLE: a row names a side that make_layout does not place");

size_t ws_bytes_per_frame(WsId id, int h, int w)
{
    const size_t N = (size_t)h * w;
    switch (id) {
#define X(id, bytes, pub, ov, side) case WS_##id: return (bytes);
    CPE_WS_TABLE(X)
#undef X
    default: return 0;
    }
}

// the buffer behind a public plane number (WS_COUNT: none)
constexpr WsId ws_public(int plane)
{
    for (int i = 0; i < WS_COUNT; i++)
        if (WS_ROWS[i].public_plane == plane) return (WsId)i;
    return WS_COUNT;
}
constexpr int CPE_PLANE_COUNT = 15;
static_assert(ws_public(CPE_PLANE_BINARY) == WS_BINARY && ws_public(CPE_PLANE_HMASK) == WS_HMASK && ws_public(CPE_PLANE_VMASK) == WS_VMASK &&
              ws_public(CPE_PLANE_MASK_CONTOUR) == WS_MASK_CONTOUR && ws_public(CPE_PLANE_ROI_H) == WS_ROI_H &&
              ws_public(CPE_PLANE_ROI_V) == WS_ROI_V && ws_public(CPE_PLANE_EXP_H) == WS_EXP_H && ws_public(CPE_PLANE_EXP_V) == WS_EXP_V &&
              ws_public(CPE_PLANE_JOINTS) == WS_JOINTS && ws_public(CPE_PLANE_STATE) == WS_STATE && ws_public(CPE_PLANE_CLAHE) == WS_CLAHE &&
              ws_public(CPE_PLANE_BLUR19) == WS_BLUR19 && ws_public(CPE_PLANE_BLUR7) == WS_BLUR7 && ws_public(CPE_PLANE_LABELS) == WS_LABELS &&
              ws_public(CPE_PLANE_SWEEP) == WS_SWEEP && ws_public(CPE_PLANE_COUNT) == WS_COUNT,
              "include/cpe.h: CPE_PLANE_* 0..14 and the public column of CPE_WS_TABLE disagree");

struct Layout {
    size_t off[WS_COUNT];
    size_t bytes_per_frame[WS_COUNT];
    size_t total;
};

Layout make_layout(int n, int h, int w)
{
    Layout L;
    for (int i = 0; i < WS_COUNT; i++) L.bytes_per_frame[i] = ws_bytes_per_frame((WsId)i, h, w);
    size_t o = 0;
    auto place = [&](int i, size_t at) { L.off[i] = at; return at + align_up(L.bytes_per_frame[i] * (size_t)n, 256); };
    for (int ov = OV_NONE + 1; ov < OV_COUNT; ov++) {   // every side of an overlay starts where the overlay starts
        size_t end = o;
        for (int side = 0; side < WS_SIDES; side++) {
            size_t cur = o;
            for (int i = 0; i < WS_COUNT; i++)
                if (WS_ROWS[i].overlay == ov && WS_ROWS[i].side == side) cur = place(i, cur);
            end = std::max(end, cur);
        }
        o = end;
    }
    for (int i = 0; i < WS_COUNT; i++)
        if (WS_ROWS[i].overlay == OV_NONE) o = place(i, o);
    L.total = o;
    return L;
}

// An opened workspace: the layout of an (n, h, w) call over the caller's block.
struct Workspace {
    uint8_t *base = nullptr;
    Layout L;
    // builds the layout and checks the block against it; `entry` names the caller in the error text.  too_small: the code
    // for a missing or short block (cpe_detect_grid_batch* report CPE_ERR_WORKSPACE, every other entry CPE_ERR_ARG)
    int32_t open(const void *ws, size_t ws_bytes, int n, int h, int w, const char *entry, int32_t too_small = CPE_ERR_ARG)
    {
        L = make_layout(n, h, w);
        if (!ws || ws_bytes < L.total) {
            cpe::set_error("%s: workspace too small for an (n,h,w) = (%d,%d,%d) call (%zu < %zu)", entry, n, h, w, ws_bytes, L.total);
            return too_small;
        }
        CPE_CHECK_ARG(((uintptr_t)ws & 255) == 0, "%s: workspace must be 256-byte aligned", entry);
        base = (uint8_t *)ws;
        return CPE_OK;
    }
    template <class T> T *at(WsId id) const { return (T *)(base + L.off[id]); }
    FrameState *state() const { return at<FrameState>(WS_STATE); }
};

}  // namespace
}  // namespace cpe
