// Device-side building blocks shared by the image-stage kernels (gfx950).
#pragma once
#include <cstddef>
#include <type_traits>
#include "cpe_internal.h"

namespace cpe {

// ---------------------------------------------------------------- per-image state kept in the workspace
constexpr int MAX_DIM = 4096;    // tallest and widest frame the entry points take (detect.hip checks h, w <= MAX_DIM): coordinates fit 12 bits
constexpr int MAXROOTS = 262144;  // components per labelling pass and image (4K frames: ~48k noise specks in the joints mask)
// component lists of the blob sweep: one pool of (first pixel, count) entries per frame and list, the 17 thresholds one
// after the other in the order they are filled (the first entry of a threshold = the sum of the counters of the ones before
// it, region.hip sw_slot).  CLAHE turns sensor noise into specks: 1920x1200 frames with +-7..11 DN of noise (and an intensity
// ramp, tools/stress_parity.py) were seen with 770 000 dark components away from the border, 560 000 bright ones and 115 000
// followed hole borders over all thresholds; clean frames stay below 30 000.
enum { SWL_DARK = 0, SWL_BRIGHT = 1, SWL_TRACE = 2 };
__host__ __device__ inline int sweep_pool(int h, int w, int which)
{
    const long long N = (long long)h * w;
    long long v = which == SWL_TRACE ? N / 8 : N / 2;   // largest totals seen: 770 000 dark (noise + intensity ramp), 560 000 bright, 115 000
    const long long lo = which == SWL_TRACE ? (1 << 18) : (1 << 19);   // small frames: what 17 lists of 32768 entries held
    v = v < lo ? lo : (v > (1 << 23) ? (1 << 23) : v);
    return (int)((v + 255) / 256 * 256);
}
constexpr int MAXJ = CPE_MAXJ;   // joints kept inside the region rectangle (include/cpe.h)
constexpr int MAXB = 32768;      // blobs per threshold
constexpr int MAXG = 32768;      // blob groups (one per unmatched blob: a noisy intensity ramp makes thousands)
constexpr int MAXG_LDS = 1024;   // ... whose middle centres sit in k_blob_merge's LDS (24 KB; a clean frame has ~500); the rest are read from HBM
constexpr int GCAP = 48;         // centres per group (17 thresholds + same-threshold neighbours that fall into the same group)
constexpr int MAXV = 131072;     // contour-vertex scratch (int2) per image
constexpr int MAXL = CPE_MAXL;   // grid lines per direction (label groups of the joints: noise joints make extra ones)
constexpr int MAXLP = CPE_MAXLP; // joints per label group: a limit, not a slot size (the groups share one pool of MAXJ points)
constexpr int MAXSEG = 2048;     // line fragments per mask in the expansion stage

struct BlobRec { double x, y, r; int key; int pad; };
struct Group { int n; int pad; double c[GCAP][3]; };

// The per-frame state record, declared once: X(type, name, count), type int or float, count 1 (a scalar), 2 or 4 (an array).
// struct FrameState and the name table behind cpe_debug_state_field (the names DetectWorkspace.state() reports) both come
// from these rows, in this order; a row added here needs the word count of the size assert below and nothing else.
#define CPE_STATE_FIELDS(X) \
    X(int, status, 1) \
    X(int, rect, 4)          /* boundingRect(max_contour) */ \
    X(int, r0, 1)            /* circle_radius0 */ \
    X(int, spot, 4)          /* ellipse cx, cy, a, b */ \
    X(int, n_roots, 1)       /* scratch counters (reset by the stage that uses them) */ \
    X(int, n_comps, 1) \
    X(int, n_joints_all, 1)  /* all joints */ \
    X(int, n_joints, 1)      /* joints inside rect (sorted in OpenCV contour order) */ \
    X(int, n_blobs, 1) \
    X(int, n_groups, 1) \
    X(int, n_groups_prev, 1) \
    X(int, n_kp, 1) \
    X(int, n_verts, 1)       /* bump pointer of the vertex scratch */ \
    X(int, n_dists, 1)       /* bump pointer of the distance scratch */ \
    X(int, best_comp, 1)     /* index of the selected contour */ \
    X(int, n_seg, 2)         /* valid fragments per mask (h, v) */ \
    X(float, gang, 2) \
    X(float, glen, 2) \
    X(int, n_rows, 1) \
    X(int, n_cols, 1) \
    X(int, overflow, 1) \
    X(int, hull_n, 1) \
    X(int, crect, 4)         /* working rectangle of a restricted labelling pass (x0, y0, x1, y1) */ \
    X(int, nrect, 4)         /* bounding-box accumulator */ \
    X(int, n_roots_p, 1)     /* component count of the joints labelling (runs on its own stream, beside the region stage) */ \
    X(int, n_roots_s, 1)     /* component count of the spot labelling (third stream) */ \
    X(int, spot_fail, 1)     /* the spot chain found no saturated spot: folded into `status` when the chains join */ \
    X(int, srect, 4)         /* window of the spot labelling (x0, y0, x1, y1): the tiles that hold a pixel > 240, + 16 px */
#define CPE_STATE_DIM_1
#define CPE_STATE_DIM_2 [2]
#define CPE_STATE_DIM_4 [4]
struct FrameState {
#define X(type, name, count) type name CPE_STATE_DIM_##count;
    CPE_STATE_FIELDS(X)
#undef X
};
struct StateField { const char *name; int words; bool is_float; };
constexpr StateField STATE_FIELDS[] = {
#define X(type, name, count) {#name, count, std::is_same<type, float>::value},
    CPE_STATE_FIELDS(X)
#undef X
};
static_assert(sizeof(FrameState) == 46 * sizeof(int), "FrameState: the record is 46 words (tests and tools read them by name)");
static_assert(offsetof(FrameState, status) == 0 && offsetof(FrameState, r0) == 5 * 4 && offsetof(FrameState, n_seg) == 21 * 4 &&
              offsetof(FrameState, gang) == 23 * 4 && offsetof(FrameState, crect) == 31 * 4 && offsetof(FrameState, srect) == 42 * 4,
              "FrameState: a row of CPE_STATE_FIELDS moved");

struct SegRec { float p1x, p1y, p2x, p2y, angle, len; int valid; int pad; };

// stage buffer bundles (all device pointers into the caller's workspace, plane-major [n][...])
struct RegionBuffers {
    uint8_t *cl, *ext, *mc, *touch;
    int *lab, *cnt, *lab2, *cnt2, *roots, *sw, *nrect, *bk;
    double *gmid;              // middle centres (x, y, r) of the blob groups beyond MAXG_LDS
    uint32_t *pool;   // border points of the hole traces (chunked)
    unsigned short *blob_ch;   // first 16 chunk ids of every blob's border
    int maxch, maxdf;          // capacities per frame and threshold: border-point chunks, distance scratch (doubles)
    uint32_t *bits;   // 17 one-bit planes per frame (threshold images), reused for single mask planes later
    int2 *hl, *bl, *tl;   // per-threshold component lists of the blob sweep (dark / bright)
    unsigned int *hist;
    uint8_t *lut;
    BlobRec *blobs;
    int *blob_d, *order;
    double *dists;
    Group *groups;
    unsigned long long *best;
    int *lohi, *hull;
};
// test entry of the region stage (cpe_debug_blob_region): null on the product path.  identity: the sweep sees the input
// image itself (an identity CLAHE table instead of LAB-L + CLAHE); blobs / n_blobs: the blob records of every threshold are
// copied out after the group merge (their memory is reused by the disc-union labelling); kp / n_kp: the key points of the
// groups, in group order, as k_discs computes them
struct RegionProbe {
    int identity;
    double *blobs; int blob_cap; int *n_blobs;   // f64 [n, 17, blob_cap, 3] (x, y, r), i32 [n, 17]
    float *kp; int kp_cap; int *n_kp;            // f32 [n, kp_cap, 3] (x, y, size), i32 [n]
};
// grid.x of the kernels that walk a per-frame list (components, blobs, fragments) in turns: enough workgroups per frame
// to fill the chip when the batch is small, few when it is large (a grid sized for the list capacity would be mostly
// empty workgroups: hundreds of thousands of them cost more than the work)
inline unsigned frame_waves(int lists, int lo, int hi)
{
    const int v = 16384 / (lists > 0 ? lists : 1);
    return (unsigned)(v < lo ? lo : (v > hi ? hi : v));
}
// optional helper stream of the region stage: the hole borders are followed while the bright sweep runs
struct RegionSide { hipStream_t s; hipEvent_t clahe_done, dark_done, traced, medians;
                    hipEvent_t joints_done = nullptr, spot_done = nullptr; };   // ends of the joints / spot chains (their label planes hold the tracers' tables afterwards)
struct MaskBuffers {
    uint8_t *binary, *hmask, *vmask, *joints_mask, *g19, *cm, *mc, *roi_h, *roi_v, *base_h, *base_v, *exp_h,
        *exp_v, *touch;
    int *lab, *roots, *jtmp, *joints, *verts;
    int *lab_p, *roots_p, *lab_s, *roots_s;
    int *lab_h, *lab_v;                       // union-find planes of the two expanded masks (read by k_lines)   // label planes / component lists of the joints and spot chains
    uint32_t *bits;
    unsigned long long *best, *best_s;
    unsigned long long *fl_j;                 // joints chain: [n][h * ceil(w/64)] background masks, then the same of outer background
    uint32_t *jbits;                          // one-bit plane of the joints mask (build_bitplanes layout, one plane per frame)
    SegRec *segs;
    // CPE_DETECT_SKIP_DEBUG_PLANES: where the line masks travel as one-bit planes (line_masks_as_bits, masks.hip) the bytes of
    // hmask / vmask / roi_h / roi_v are not written
    bool skip_debug = false;
};

// FrameState::overflow is a bit mask of the fixed capacity that was exceeded (any bit => CPE_ST_OVERFLOW)
enum { OVF_ROOTS = 1, OVF_LINES = 2, OVF_TRACE = 4, OVF_JOINTS = 8, OVF_VERTS = 16, OVF_SEGS = 32, OVF_KERNEL = 64,
       OVF_EXPAND = 128, OVF_BLOBS = 256, OVF_DISTS = 512, OVF_GROUPS = 1024, OVF_SWEEP = 2048 };
__device__ __forceinline__ void set_overflow(FrameState &S, int bit) { atomicOr(&S.overflow, bit); }

// the per-frame component list a labelling pass fills; its counter is FrameState::n_roots, n_roots_p (joints chain) or n_roots_s
// (spot chain, whose planes the vertical fragment mask reuses)
enum RootList : int { ROOTS_MAIN = 0, ROOTS_JOINTS = 1, ROOTS_SPOT = 2 };
__device__ __forceinline__ int *root_counter(FrameState &S, RootList list)
{
    return list == ROOTS_MAIN ? &S.n_roots : (list == ROOTS_JOINTS ? &S.n_roots_p : &S.n_roots_s);
}

// the part of a frame that a labelling pass or a RETR_EXTERNAL flood works in: the frame; FrameState::crect, the blob sweep's
// working rectangle (ccl_set_sweep_rect); the region rectangle (boundingRect of the hull) + 2 px, which holds every mask
// derived from mask_contour; FrameState::srect, the window of the spot labelling (may be empty)
enum Window : int { WIN_FRAME = 0, WIN_SWEEP = 1, WIN_REGION = 2, WIN_SPOT = 3 };
struct Rect { int x0, y0, x1, y1; };   // inclusive; empty when x1 < x0
__device__ __forceinline__ Rect window_rect(const FrameState *st, size_t f, Window win, int h, int w)   // frame f's window
{
    Rect r;
    if (win == WIN_SWEEP) { r.x0 = st[f].crect[0]; r.y0 = st[f].crect[1]; r.x1 = st[f].crect[2]; r.y1 = st[f].crect[3]; }
    else if (win == WIN_REGION) {
        const int *q = st[f].rect;
        r.x0 = max(q[0] - 2, 0); r.y0 = max(q[1] - 2, 0); r.x1 = min(q[0] + q[2] + 1, w - 1); r.y1 = min(q[1] + q[3] + 1, h - 1);
    } else if (win == WIN_SPOT) { r.x0 = st[f].srect[0]; r.y0 = st[f].srect[1]; r.x1 = st[f].srect[2]; r.y1 = st[f].srect[3]; }
    else { r.x0 = 0; r.y0 = 0; r.x1 = w - 1; r.y1 = h - 1; }
    return r;
}

// ---------------------------------------------------------------- RETR_EXTERNAL (ccl.hip: k_outside_flood)
// A flood that has not converged after FLOOD_MAX_PASSES sweeps sets OVF_TRACE (a sweep walks one band of rows, a sixteenth of
// the window: 65536 of them are the 4096 whole-window sweeps of round 2).
constexpr int FLOOD_MAX_PASSES = 65536;
// a component (raster-first pixel `root`) is external iff the pixel west of that pixel is outer background
// (cv2.findContours(RETR_EXTERNAL) drops the components that lie in a hole of another one)
__device__ __forceinline__ bool comp_is_external(const unsigned long long *out_f, int w, int root, int win_x0)
{
    const int y = root / w, x = root - y * w;
    if (x - 1 < win_x0) return true;          // the window border / the image border is outer background
    return (out_f[(size_t)y * ((w + 63) >> 6) + ((x - 1) >> 6)] >> ((x - 1) & 63)) & 1ull;
}

// grey-level bucket of a CLAHE value for the blob sweep: 0: v <= 50 (dark at every threshold), b: 50 + 10 (b - 1) < v <= 50 + 10 b,
// 17: v > 210.  Bucket b joins the dark forest at threshold slot b and the bright forest at slot b - 1.
__host__ __device__ inline int sweep_level(int v) { return v <= 50 ? 0 : (((v - 41) / 10) < 17 ? ((v - 41) / 10) : 17); }

// ---------------------------------------------------------------- union-find on an int label plane
// S: ints per node (1: a plain label plane; 2: the bright forest of the blob sweep, whose node is {parent, merge-history word})
template <int S = 1> __device__ __forceinline__ int uf_load(const int *L, int i)
{
    return __hip_atomic_load(L + (size_t)i * S, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <int S = 1> __device__ __forceinline__ int uf_find(const int *L, int x)
{
    int p;
    while ((p = uf_load<S>(L, x)) != x) x = p;
    return x;
}
// find with intermediate pointer jumping (ECL-CC): every node on the walked path is re-pointed at its
// grandparent.  Parents always have smaller indices and roots are never written, so concurrent use with
// uf_unite is safe; stale writes can only re-point a node at another of its ancestors.
template <int S = 1> __device__ __forceinline__ int uf_find_c(int *L, int x)
{
    int curr = uf_load<S>(L, x);
    if (curr != x) {
        int prev = x, next;
        while (curr > (next = uf_load<S>(L, curr))) {
            __hip_atomic_store(L + (size_t)prev * S, next, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            prev = curr;
            curr = next;
        }
    }
    return curr;
}
template <int S = 1> __device__ __forceinline__ void uf_unite(int *L, int a, int b)
{
    for (;;) {
        a = uf_find_c<S>(L, a);
        b = uf_find_c<S>(L, b);
        if (a == b) return;
        if (a < b) { int t = a; a = b; b = t; }
        int old = atomicMin(&L[(size_t)a * S], b);
        if (old == a) return;
        a = old;
    }
}
// The dark forest of the blob sweep has one terminal parent more: a parent below 0 says "this tree is outside" (it reaches
// the border of the working rectangle, so it is no hole).  -1 is smaller than every pixel index, so a union with outside makes
// outside the root through the same atomic minimum that links the larger root under the smaller, and every later union with
// such a tree inherits it.  The walks test the sign of a loaded parent before they use it as an index: -1 is returned, never
// indexed with.
__device__ __forceinline__ int uf_find_out(const int *L, int x)
{
    for (;;) {
        const int p = uf_load(L, x);
        if (p < 0) return -1;
        if (p == x) return x;
        x = p;
    }
}
// uf_find_c for that forest.  The pointer jumping may store -1 into a non-root: a correct shortening.
__device__ __forceinline__ int uf_find_c_out(int *L, int x)
{
    int curr = uf_load(L, x);
    if (curr < 0) return -1;
    if (curr != x) {
        int prev = x;
        for (;;) {
            const int next = uf_load(L, curr);
            if (next >= curr) break;                 // curr is a root
            __hip_atomic_store(L + prev, next < 0 ? -1 : next, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (next < 0) return -1;
            prev = curr;
            curr = next;
        }
    }
    return curr;
}
// uf_unite for that forest; a or b may be -1 (outside itself).  A minimum that returns the root it was sent to made the link.
// Any other answer is the parent somebody else gave that root first -- a smaller index, or -1 -- and the union goes on from
// it: every retry strictly lowers the index it works on and -1 ends it, so the loop ends.
__device__ __forceinline__ void uf_unite_out(int *L, int a, int b)
{
    for (;;) {
        a = a < 0 ? -1 : uf_find_c_out(L, a);
        b = b < 0 ? -1 : uf_find_c_out(L, b);
        if (a == b) return;                          // one tree, or both outside
        if (a < b) { int t = a; a = b; b = t; }      // a >= 0; b may be -1
        const int old = atomicMin(&L[a], b);
        if (old == a) return;
        a = old;
    }
}

// uf_unite on the bright forest of the blob sweep (node = {parent, merge-history word}, history 0xFFFFFFFF while the node is a
// root): the thread whose link wins also writes "absorbed by b at step `step`", b | step << 24, in the same 64-bit
// compare-and-swap of the whole node {a, never} -> {b, history}.  Only roots are ever swapped and the pointer-jumping stores of
// uf_find_c only touch the parent word of non-roots, so the two never meet in a node.  A failed swap writes nothing: a is no
// longer a root, and the union goes on from the parent the swap returned.
__device__ __forceinline__ void uf_unite_hist(int *L, int a, int b, int step)
{
    for (;;) {
        a = uf_find_c<2>(L, a);
        b = uf_find_c<2>(L, b);
        if (a == b) return;
        if (a < b) { int t = a; a = b; b = t; }
        const unsigned long long never = (unsigned long long)(unsigned)a | (0xFFFFFFFFull << 32);
        const unsigned long long link = (unsigned long long)(unsigned)b | ((unsigned long long)((unsigned)b | ((unsigned)step << 24)) << 32);
        const unsigned long long old = atomicCAS(reinterpret_cast<unsigned long long *>(L + 2 * (size_t)a), never, link);
        if (old == never) return;
        a = (int)(unsigned)old;
    }
}

// ---------------------------------------------------------------- Suzuki border following (OpenCV icvFetchContour)
// Pred(x, y) -> bool : pixel is non-zero (false outside the image).
// Visitor.point(x, y, is_vertex): every border pixel in order (CHAIN_APPROX_NONE); is_vertex marks the
// subset CHAIN_APPROX_SIMPLE keeps.  Returns false if the step bound was hit.
// The 8 neighbours of the current pixel are fetched together (independent loads, one memory latency per
// border step instead of one per examined neighbour); the direction search then runs on the bit mask.
template <class Pred>
__device__ __forceinline__ unsigned nbr_mask(Pred &nz, int x, int y)
{
    const bool b0 = nz(x + 1, y), b1 = nz(x + 1, y - 1), b2 = nz(x, y - 1), b3 = nz(x - 1, y - 1);
    const bool b4 = nz(x - 1, y), b5 = nz(x - 1, y + 1), b6 = nz(x, y + 1), b7 = nz(x + 1, y + 1);
    return (b0 ? 1u : 0u) | (b1 ? 2u : 0u) | (b2 ? 4u : 0u) | (b3 ? 8u : 0u) | (b4 ? 16u : 0u) | (b5 ? 32u : 0u) |
           (b6 ? 64u : 0u) | (b7 ? 128u : 0u);
}

// 1-bit planes (threshold images, single masks) in 64 x 8 tiles.  A tile is 8 consecutive u64 words = one 64-byte line:
// word r of tile (ty, tx) holds row 8 ty + r, its bit i pixel 64 (tx - 1) + i.  Tile columns 0 and bit_tile_cols(w) - 1 and
// the rows >= h of the last tile row are zero, so a 64-column window that starts on a 32-column boundary is one or two
// words of one row and never needs a horizontal bounds test.  Rows y .. y + 7 of 64 columns are one line: the word-level
// walks read 8 rows with one request, a 16-row tracer window is 2-4 lines (16 in the row-major layout this replaced).
// Planes are multiples of 64 bytes; the workspace keeps their bases 256-byte aligned, so every tile is one line.
__host__ __device__ inline int bit_tile_cols(int w) { return ((w + 63) >> 6) + 2; }
__host__ __device__ inline size_t bit_plane_words(int h, int w) { return (size_t)((h + 7) >> 3) * bit_tile_cols(w) * 8; }   // u64 words
// index of the word with pixels 64 j .. 64 j + 63 of row y (0 <= y < 8 ceil(h / 8); j = -1 and j = ceil(w / 64) are the
// zero columns), tc = bit_tile_cols(w)
__host__ __device__ inline size_t bit_word(int tc, int y, int j) { return ((size_t)(y >> 3) * tc + (j + 1)) * 8 + (y & 7); }
// plane i of a run of planes that starts at `base`
__host__ __device__ inline const unsigned long long *bit_plane(const uint32_t *base, size_t i, int h, int w)
{
    return reinterpret_cast<const unsigned long long *>(base) + i * bit_plane_words(h, w);
}
__host__ __device__ inline unsigned long long *bit_plane(uint32_t *base, size_t i, int h, int w)
{
    return reinterpret_cast<unsigned long long *>(base) + i * bit_plane_words(h, w);
}

// rows y0 .. y0 + R - 1 (y0, R: multiples of 8) of a tiled one-bit plane, word(tr, j) = row y0 + tr, pixels
// 64 j .. 64 j + 63: whole tiles, 8 consecutive threads of the workgroup (256 threads) per 64-byte tile.  The zero tile
// columns and the rows >= h of the last tile row are written as zeros.
template <class Word>
__device__ __forceinline__ void store_plane_band(unsigned long long *plane, int h, int w, int y0, int R, int t, Word word)
{
    const int tc = bit_tile_cols(w);
    const int rows = min(R, ((h + 7) & ~7) - y0);
    unsigned long long *o = plane + (size_t)(y0 >> 3) * tc * 8;
    for (int i = t; i < rows * tc; i += 256) {
        const int tile = i >> 3, tyl = tile / tc, tx = tile - tyl * tc, tr = tyl * 8 + (i & 7);
        o[i] = (tx == 0 || tx == tc - 1 || y0 + tr >= h) ? 0ull : word(tr, tx - 1);
    }
}

// BitWin keeps a 16-row x 64-column window of a plane around the current border pixel in LDS (one column of `win` per
// lane): a border step costs three LDS reads, and global memory is touched only when the border leaves the window (every
// ~10 steps) instead of eight dependent loads per step.  The window starts on a tile row and on a 32-column boundary: a
// refill reads the 2 tiles of one tile column, or 4 when it straddles two.  LS is the number of windows `win` holds side by
// side (the lanes of a wavefront that follow borders): a kernel declares BW_ROWS * LS words and passes win + lane.
constexpr int BW_ROWS = 16;
template <int LS = 64, bool WIDE_LOADS = false>
struct BitWin {
    const unsigned long long *plane;   // this frame's plane
    int w, h;
    unsigned long long *win;     // LDS, row r of this lane at win[r * LS]
    int wx0 = 0, wy0 = INT_MIN / 2;   // pixel column of window column 0 (a multiple of 32), image row of window row 0 (a multiple of 8)
    // (re)fill the window around (x, y): the pixel lands in rows row_lo .. row_lo + 7 and columns col_lo .. col_lo + 31.  The
    // window is put ahead of the border's direction of travel: leaving through the top / bottom row puts the pixel on the
    // bottom / top side of the new window, leaving through the left / right columns puts it on the right / left side --
    // borders keep their heading for a while, so a refill lasts longer than one of a centred window.
    // Two forms of the loads, chosen by WIDE_LOADS; which is faster for a kernel is measured (r36).  The default: the window
    // is read as the 32 half-words (dwords) it consists of, all loads issued before the first is waited for and
    // none under a branch.  Half-word k of a row is the lower half of window row r: dword (k & 1) of word k >> 1, 8 r bytes
    // into that tile; the upper half is the dword after it, 4 bytes on in the same word (k even) or 60 bytes on, at the
    // start of the same row of the next tile (k odd; j + 2 <= tc - 1).  A tile row outside the image reads tile (0, 0), which
    // is zero like all of tile column 0, with the 4-byte step.
    __device__ __forceinline__ void load(int x, int y, int row_lo, int col_lo)
    {
        const int k = (x - col_lo) >> 5;   // >= -2: window column 0 is at pixel -64 at the least (tile column 0)
        wx0 = 32 * k;
        wy0 = (y - row_lo) & ~7;
        const int tc = bit_tile_cols(w), th = (h + 7) >> 3, j = k >> 1, odd = k & 1;
        // the largest plane has MAX_DIM / 8 tile rows of MAX_DIM / 64 + 2 tiles of 16 dwords: ty * tc is a 24-bit product and
        // the dword index fits 32 bits
        static_assert((long long)(MAX_DIM / 8) * (MAX_DIM / 64 + 2) * 16 < (1 << 24), "BitWin::load: 32-bit tile index");
        if constexpr (WIDE_LOADS) {
            // whole tile rows in 16-byte loads, 8 of them, or 16 when the window straddles two tile columns (the halves are
            // funnelled together); the first 8 are all issued before any is waited for.  For a kernel whose lanes all fill
            // their first window at once (k_joint_centroids: 64 short borders a wavefront), where 32 scattered dword
            // requests per lane cost more than the instructions they save (profiles/README.md, r36).
            typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
            const u64x2 *a[2];
            bool in[2];
#pragma unroll
            for (int t = 0; t < 2; t++) {
                const int ty = (wy0 >> 3) + t;
                in[t] = (unsigned)ty < (unsigned)th;
                a[t] = reinterpret_cast<const u64x2 *>(plane + (in[t] ? (__mul24(ty, tc) + j + 1) * 8 : 0));
            }
            u64x2 v[8];
#pragma unroll
            for (int q = 0; q < 8; q++) v[q] = a[q >> 2][q & 3];
            if (odd) {   // columns 32 .. 63 of word j, 0 .. 31 of word j + 1 (the next tile; j + 2 <= tc - 1)
                u64x2 u[8];
#pragma unroll
                for (int q = 0; q < 8; q++) u[q] = a[q >> 2][4 + (q & 3)];
#pragma unroll
                for (int q = 0; q < 8; q++) { v[q] = (v[q] >> 32) | (u[q] << 32); if (!in[q >> 2]) v[q] = 0ull; }
            }
#pragma unroll
            for (int q = 0; q < 8; q++) { win[(2 * q) * LS] = v[q].x; win[(2 * q + 1) * LS] = v[q].y; }
        } else {
            const uint32_t *lo[2];
            int up[2];   // dwords from the lower to the upper half
#pragma unroll
            for (int t = 0; t < 2; t++) {
                const int ty = (wy0 >> 3) + t;
                const bool in = (unsigned)ty < (unsigned)th;
                lo[t] = reinterpret_cast<const uint32_t *>(plane) + (in ? (__mul24(ty, tc) + j + 1) * 16 + odd : 0);
                up[t] = (in && odd) ? 15 : 1;
            }
            uint32_t a[BW_ROWS], b[BW_ROWS];
#pragma unroll
            for (int r = 0; r < BW_ROWS; r++) { a[r] = lo[r >> 3][2 * (r & 7)]; b[r] = lo[r >> 3][2 * (r & 7) + up[r >> 3]]; }
#pragma unroll
            for (int r = 0; r < BW_ROWS; r++) win[r * LS] = (unsigned long long)a[r] | ((unsigned long long)b[r] << 32);
        }
    }
    __device__ __forceinline__ unsigned nbrs(int x, int y)
    {
        int p = x - wx0, r = y - wy0;
        if (p < 1 || p > 62 || r < 1 || r > BW_ROWS - 2) {
            const bool fresh = wy0 == INT_MIN / 2;
            int row = 4, col = 16;
            if (!fresh) {
                if (r < 1) row = 7;            // heading up: rows 7 .. 14
                else if (r > BW_ROWS - 2) row = 1;   // heading down: rows 1 .. 8
                if (p < 1) col = 29;           // heading left: columns 29..60
                else if (p > 62) col = 3;      // heading right: columns 3..34
            }
            load(x, y, row, col);
            p = x - wx0; r = y - wy0;
        }
        const unsigned ta = (unsigned)(win[(r - 1) * LS] >> (p - 1)) & 7u;   // bit 0: x - 1, bit 1: x, bit 2: x + 1
        const unsigned tb = (unsigned)(win[r * LS] >> (p - 1)) & 7u;
        const unsigned tc = (unsigned)(win[(r + 1) * LS] >> (p - 1)) & 7u;
        return ((tb >> 2) & 1u) | (((ta >> 2) & 1u) << 1) | (((ta >> 1) & 1u) << 2) | ((ta & 1u) << 3) | ((tb & 1u) << 4) |
               ((tc & 1u) << 5) | (((tc >> 1) & 1u) << 6) | (((tc >> 2) & 1u) << 7);
    }
    __device__ __forceinline__ bool operator()(int x, int y) const   // single pixel, straight from the plane
    {
        if ((unsigned)x >= (unsigned)w || (unsigned)y >= (unsigned)h) return false;
        return (plane[bit_word(bit_tile_cols(w), y, x >> 6)] >> (x & 63)) & 1ull;
    }
};
template <int LS, bool WIDE_LOADS>
__device__ __forceinline__ unsigned nbr_mask(BitWin<LS, WIDE_LOADS> &bw, int x, int y) { return bw.nbrs(x, y); }

// direction s = 0..7 counter-clockwise from east (x right, y down): DX = {1,1,0,-1,-1,-1,0,1}, DY = {0,-1,-1,-1,0,1,1,1},
// stored as 2-bit fields (value + 1) so a step needs no table in memory
__device__ __forceinline__ int trace_dx(int s) { return (int)((0x901Au >> (2 * s)) & 3u) - 1; }
__device__ __forceinline__ int trace_dy(int s) { return (int)((0xA901u >> (2 * s)) & 3u) - 1; }

template <class Pred, class Visitor>
__device__ bool trace_border(Pred &nz, int x0, int y0, bool is_hole, Visitor &vis, int max_steps)
{
    int s, s_end;
    s_end = s = is_hole ? 0 : 4;
    unsigned bits = nbr_mask(nz, x0, y0);
    do {
        s = (s - 1) & 7;
    } while (!((bits >> s) & 1u) && s != s_end);
    if (s == s_end) {
        vis.point(x0, y0, true);
        return true;
    }
    const int x1 = x0 + trace_dx(s), y1 = y0 + trace_dy(s);
    int x3 = x0, y3 = y0, prev_s = s ^ 4;
    for (int step = 0; step < max_steps; step++) {
        // first set neighbour counter-clockwise after s (the pixel we came from is always set, so one exists)
        const unsigned rot = ((bits | (bits << 8)) >> ((s + 1) & 7)) & 0xFFu;
        if (rot) s = (s + __ffs(rot)) & 7;
        const int x4 = x3 + trace_dx(s), y4 = y3 + trace_dy(s);
        bool vertex = (s != prev_s);
        // exactly one point per iteration in every lane that is still following its border: StoreVisitor (region.hip) takes
        // the phase of its chunk stores from the first active lane.  A visitor or a change here that skips or repeats a
        // point in some lanes only (an uneven stop() before point(), say) breaks that.
        vis.point(x3, y3, vertex);
        if (vertex) prev_s = s;
        if (x4 == x0 && y4 == y0 && x3 == x1 && y3 == y1) return true;
        if (vis.stop()) return true;   // the visitor has seen enough (e.g. more vertices than its consumer accepts)
        x3 = x4;
        y3 = y4;
        s = (s + 4) & 7;
        bits = nbr_mask(nz, x3, y3);
    }
    return false;
}

struct ThreshPred {  // binarised = img > t
    const uint8_t *m;
    int w, h, t;
    __device__ __forceinline__ bool operator()(int x, int y) const
    {
        const bool inb = (unsigned)x < (unsigned)w && (unsigned)y < (unsigned)h;
        const int cx = min(max(x, 0), w - 1), cy = min(max(y, 0), h - 1);
        const int v = m[(size_t)cy * w + cx];
        return inb & (v > t);
    }
};

// Green sums + counts + bbox; optional vertex store
struct StatVisitor {
    long long a00 = 0, a10 = 0, a01 = 0;
    int npts = 0, nverts = 0;
    int minx = INT_MAX, maxx = INT_MIN, miny = INT_MAX, maxy = INT_MIN;
    bool have_prev = false;
    int fx = 0, fy = 0, px = 0, py = 0;  // first and previous written point
    // One edge of the Green sums, for the edges of a border: every one goes to an 8-neighbour (the closing edge too; a
    // single pixel closes on itself).  Coordinates lie in 0 .. MAX_DIM - 1 = 4095 (the entry points refuse taller or wider frames), so
    // x0 y1 and x1 y0 are 24-bit products below 2^24, and with (x1, y1) = (x0 + dx, y0 + dy) dxy = x0 dy - y0 dx, |dxy| <=
    // 8190 < 2^13.  x0 + x1 and y0 + y1 are <= 8190 < 2^13 as well: the products of the moment sums are 24-bit products
    // too, below 2^26 in magnitude.  Only the running sums are 64 bits wide.
    static_assert((long long)(MAX_DIM - 1) * (MAX_DIM - 1) < (1 << 24) && 2 * (MAX_DIM - 1) < (1 << 13),
                  "StatVisitor::edge: 24-bit products");
    __device__ __forceinline__ void edge(int x0, int y0, int x1, int y1)
    {
        const int dxy = __mul24(x0, y1) - __mul24(x1, y0);
        a00 += dxy;
        a10 += __mul24(dxy, x0 + x1);
        a01 += __mul24(dxy, y0 + y1);
    }
    __device__ __forceinline__ void point(int x, int y, bool vertex)
    {
        npts++;
        if (vertex) nverts++;
        minx = min(minx, x); maxx = max(maxx, x); miny = min(miny, y); maxy = max(maxy, y);
        if (have_prev) edge(px, py, x, y);
        else { fx = x; fy = y; have_prev = true; }
        px = x; py = y;
    }
    __device__ __forceinline__ void finish() { if (have_prev) edge(px, py, fx, fy); }
    __device__ __forceinline__ bool stop() const { return false; }
};

// cv2.moments(contour): m00, m10, m01 from the Green sums (contourMoments)
__device__ __forceinline__ void moments_from_sums(long long a00, long long a10, long long a01, double &m00,
                                                  double &m10, double &m01)
{
    m00 = m10 = m01 = 0;
    double d00 = (double)a00;
    if (fabs(d00) > 1.1920928955078125e-07) {
        double db1_2, db1_6;
        if (d00 > 0) { db1_2 = 0.5; db1_6 = 0.16666666666666666666666666666667; }
        else { db1_2 = -0.5; db1_6 = -0.16666666666666666666666666666667; }
        m00 = d00 * db1_2;
        m10 = (double)a10 * db1_6;
        m01 = (double)a01 * db1_6;
    }
}

// ================================================================ host entry points shared between the translation units
// ---- ccl.hip: one-bit planes, connected components, RETR_EXTERNAL
// planes[t] = (img > thr0 + t * step), t < nplanes, in the tiled layout above; plane t of frame f is
// bit_plane(planes, f * nplanes + t, h, w)
int build_bitplanes(const uint8_t *img, int n, int h, int w, int thr0, int step, int nplanes, uint32_t *planes, hipStream_t s);

// Component list: the 8-connected components of img > thr inside window `win` of every frame, listed by their first pixel
// (raster index) in roots[f * MAXROOTS ...], their number in the counter of `list`.  bits (may be null): the one-bit plane of
// the same set (build_bitplanes, one plane per frame), which the walks then read instead of img.  The labels of the set are
// left as union-find links (a root is a pixel whose label is its own index); labels outside the set are not written.
int ccl_components(const uint8_t *img, const uint32_t *bits, int n, int h, int w, int thr, Window win, int *L, int *roots,
                   RootList list, FrameState *st, hipStream_t s);
// the same with the connectivity as an argument (conn8 0: 4-connected components).  The detector lists 8-connected sets only;
// cpe_debug_ccl_tiles takes the word-level passes through both connectivities.
int ccl_components_conn(const uint8_t *img, const uint32_t *bits, int n, int h, int w, int thr, int conn8, Window win, int *L,
                        int *roots, RootList list, FrameState *st, hipStream_t s);
// true: a ccl_components call with these arguments reads the set from `bits` alone and never touches img (a caller that has
// the plane need not produce the bytes)
bool ccl_components_reads_bits(const uint32_t *bits, int w, const int *L);
// Unions only: the links of a component list of mask != 0 (thr 0), for a consumer that resolves the few labels it needs with
// uf_find (k_lines).
int ccl_unions(const uint8_t *mask, int n, int h, int w, Window win, int *L, FrameState *st, hipStream_t s);
// The first labelling of the blob sweep's dark forest: the 4-connected components of img <= thr inside WIN_SWEEP, flattened,
// with pixel counts in cnt and the list in roots (ROOTS_MAIN); pixels outside the set get the sweep's pre-linked runs
// (OUTSIDE_SWEEP_RUNS).  planes: img > thr as the first of nplanes one-bit planes per frame, written on `s` before this.
int ccl_dark_first(const uint8_t *img, const uint32_t *planes, int nplanes, int n, int h, int w, int thr, int *L, int *roots,
                   int *cnt, FrameState *st, hipStream_t s);
// labels of the pixels outside the set: -1; not written (never read: component lists, unions); the sweep's pre-linked runs, a
// singleton or, in a run of one grey-level bucket (sweep_level) inside a 64-pixel chunk, a link to the run's first pixel
enum CclOutside : int { OUTSIDE_NONE = 0, OUTSIDE_UNTOUCHED = 1, OUTSIDE_SWEEP_RUNS = 3 };
// pixel counts per root in cnt (zeroed inside the window unless COUNT_NONE): none, every pixel of the component, its interior
// pixels (8 neighbours in the set, inside the image), none (cnt only zeroed)
enum CclCount : int { COUNT_NONE = 0, COUNT_ALL = 1, COUNT_INTERIOR = 2, COUNT_ZERO = 3 };
// options of the general pass; the set is {(img > thr) != invert}, 8-connected if conn8, else 4-connected
struct CclPass {
    int thr = 0, invert = 0, conn8 = 1;
    Window win = WIN_FRAME;
    CclOutside outside = OUTSIDE_NONE;
    CclCount count = COUNT_NONE; int *cnt = nullptr;
    uint8_t *touch = nullptr;   // holes only: components that reach the window's border are dropped (touch: scratch plane)
    int *roots = nullptr;       // component list (ROOTS_MAIN)
    int *nrect = nullptr;       // int[n][16]: accumulate the set's bounding box (x0, y0, x1, y1) there
};
// The general pass: the label of every pixel of the set flattened to its root (the component's first pixel), and what `p` asks for.
int ccl_label(const uint8_t *img, int n, int h, int w, int *L, const CclPass &p, FrameState *st, hipStream_t s);
// The blob sweep's working rectangle (WIN_SWEEP) = the bounding box accumulated in nrect (k_clahe_apply); nrect is emptied.
int ccl_set_sweep_rect(FrameState *st, int *nrect, int n, hipStream_t s);

// Outer-background mask of every frame's window (WIN_FRAME or WIN_REGION): out[f][y][j] bit b = pixel (64 j + b, y) is
// background and 4-connected to the window border.  bgw / out: n * plane_words u64 of scratch each, plane_words >=
// h * ceil(w / 64).  bits (may be null): the mask's one-bit plane (build_bitplanes with one plane per frame); the first sweep
// reads it instead of the bytes.  Frames up to 4096 columns wide (one wavefront holds a row as 64 words of 64 pixels; wider
// frames are refused with CPE_ERR_ARG by the callers' argument check).
int outside_flood(const uint8_t *mask, int n, int h, int w, FrameState *st, Window win, unsigned long long *bgw,
                  unsigned long long *out, size_t plane_words, hipStream_t s, const uint32_t *bits);

// ---- region.hip
int region_stage(const uint8_t *gray, int n, int h, int w, double clip, const RegionBuffers &B, FrameState *st, hipStream_t s,
                 const RegionSide *side, const uint8_t *lplane, const RegionProbe *probe);
int region_stage_plane(const uint8_t *gray, int n, int h, int w, const RegionBuffers &B, FrameState *st, hipStream_t s);
// largest external contour of img > thr -> convex hull -> filled polygon in dst, st[].rect: the tail of both region stages
int region_hull(const uint8_t *img, int n, int h, int w, int thr, bool bits_ready, int single_is_positive, uint8_t *dst,
                const RegionBuffers &B, FrameState *st, hipStream_t s);
int clahe_front_probe(const uint8_t *gray, int n, int h, int w, int fused, int lab_lut, const RegionBuffers &B, hipStream_t s,
                      uint8_t *cl, uint32_t *planes, int *buckets, int *box);

// ---- masks.hip
int joints_mask_stage(int n, int h, int w, const MaskBuffers &B, FrameState *st, hipStream_t s);
int spot_stage(const uint8_t *gray, int n, int h, int w, const MaskBuffers &B, FrameState *st, hipStream_t s, int planar);
int masks_stage(const uint8_t *gray, int n, int h, int w, const MaskBuffers &B, FrameState *st, hipStream_t s,
                const RegionSide *side, int planar, hipStream_t sj);
int blur7_u8(const uint8_t *src, int n, int h, int w, const FrameState *st, uint8_t *dst, hipStream_t s);
int blur7_bgr(const uint8_t *bgr, int n, int h, int w, const FrameState *st, uint8_t *dst, hipStream_t s);

// ---- lines.hip
size_t lines_ws_bytes();
int lines_stage(const int *lab_h, const int *lab_v, const uint8_t *exp_h, const uint8_t *exp_v, const uint8_t *g7, int n, int h, int w, const int *joints,
                FrameState *st, void *lines_ws, double *o_xy, int *o_id, int *o_n, double *o_center, const uint8_t *gray,
                int subpixel, int sp_window, double sp_step, float *sp_scratch, int sp_cap, hipStream_t s, int planar);
int lines_export(const void *lines_ws, int f, double *eq, int *npts, double *pts, int *n_lines, hipStream_t s);
// packed per-frame records of a whole call (include/cpe.h): byte offsets, then the records
int results_sizes(const void *lines_ws, int n, const int *n_pts, long long *offsets, hipStream_t s);
int results_pack(const void *lines_ws, int n, const double *xy, const int *id, const int *n_pts, const double *center,
                 const int *status, const long long *offsets, void *payload, size_t payload_bytes, hipStream_t s);

}  // namespace cpe
