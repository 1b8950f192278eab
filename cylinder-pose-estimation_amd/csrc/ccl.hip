// Connected-component labelling on the GPU (replaces cv2.connectedComponents, util_cylinder.py:28, and
// is the front end of every cv2.findContours call site: components -> one border trace each).
//
// Set membership: in(p) = (img[p] > thr) != invert.  Foreground sets use 8-connectivity, background
// sets 4-connectivity (the pairing under which Suzuki-Abe outer / hole borders are defined).
// Passes over an int32 label plane (label = raster index of the component's first pixel):
//   init   : one wavefront per image row; every pixel points at the first pixel of its horizontal run
//            (ballot + bit scan, carried across 64-pixel chunks)
//   merge  : runs are united with the row above through atomicMin union-find (only where a run
//            starts on either side, so a long run costs O(1) unions per neighbour run)
//   touch  : (hole search only) components that reach the border of the working rectangle are flagged
//   finish : flatten + per-component pixel counts (aggregated per wavefront before the atomic) + root list
//            + bounding box of the set, all in one read of the label plane
// When rows start on 16-byte boundaries, the init of a pass that leaves the labels outside the set untouched, the merge and the
// component list have word-level forms (k_ccl_init64 / k_ccl_merge64 / k_ccl_roots64): 64 pixels per thread and row as one bit
// mask, the label plane is touched only where a run starts or two runs start to overlap.  A thread's 64 x 8 tile is in its
// registers, so k_ccl_init64 labels the components of the tile itself and k_ccl_merge64 unites only across tile edges.
// Entry points (cpe_dev.h): ccl_components (component list), ccl_unions (links only), ccl_dark_first and the general pass
// ccl_label; each chooses its kernels.  A pass works inside a window of the frame (Window, cpe_dev.h).  WIN_SWEEP
// (FrameState::crect) serves the blob detector:
// every hole of the binarisation at threshold t lies inside the bounding box of the bright pixels at t,
// which lies inside the box at t-10; a dark pixel on the box border is 4-connected to the outside, so
// "touches the box" == "is not a hole".  HBM bytes per pixel inside the rectangle: 1 (image) + 4 written,
// 1 + sparse label traffic, 4 read + 4 written.
#include "cpe_dev.h"

namespace cpe {

namespace {

__device__ __forceinline__ bool pred(const uint8_t *img, size_t i, int thr, int invert)
{
    return (((int)img[i] > thr) ? 1 : 0) != invert;
}

constexpr int CCL_INIT_ROWS = 16;
constexpr int CCL_INIT_AHEAD = 4;     // 64-pixel chunks of a row whose bytes are loaded before the first of them is processed
__global__ __launch_bounds__(256) void k_ccl_init(const uint8_t *__restrict__ img, int rows_total, int h, int w,
                                                  int thr, int invert, const FrameState *__restrict__ st, Window win,
                                                  int *__restrict__ L, int *__restrict__ cnt, CclOutside outside)
{
    const int lane = threadIdx.x & 63;
    for (int rr = 0; rr < CCL_INIT_ROWS / 4; rr++) {   // CCL_INIT_ROWS rows per workgroup, one wavefront per row and turn
    const int row = (blockIdx.x * (CCL_INIT_ROWS / 4) + rr) * 4 + (threadIdx.x >> 6);
    if (row >= rows_total) return;
    const int f = row / h, y = row - f * h;
    const Rect r = window_rect(st, f, win, h, w);
    if (y < r.y0 || y > r.y1 || r.x1 < r.x0) continue;
    const size_t base = (size_t)row * w;  // == frame * h*w + y*w
    int carry_in = 0, carry_start = 0;
    // CCL_INIT_AHEAD chunks of 64 pixels at a time: their byte loads are all issued before the first ballot, so a row waits for
    // memory once per group and not once per chunk; only the carry (carry_in, carry_start) passes from chunk to chunk.  A
    // pixel is read once, for the set and for its grey-level bucket.
    for (int xg = r.x0; xg <= r.x1; xg += 64 * CCL_INIT_AHEAD) {
    int px[CCL_INIT_AHEAD];
#pragma unroll
    for (int c = 0; c < CCL_INIT_AHEAD; c++) {
        const int x = xg + 64 * c + lane;
        px[c] = x <= r.x1 ? (int)img[base + x] : 0;
    }
#pragma unroll
    for (int c = 0; c < CCL_INIT_AHEAD; c++) {
        const int x0 = xg + 64 * c;
        if (x0 > r.x1) break;                      // (wave-uniform: the ballots below need every lane)
        int x = x0 + lane;
        bool valid = x <= r.x1;
        bool in = valid && ((px[c] > thr) ? 1 : 0) != invert;
        unsigned long long b = __ballot(in);
        unsigned long long prev = (b << 1) | (unsigned long long)carry_in;
        unsigned long long starts = b & ~prev;
        if (cnt && valid) cnt[base + x] = 0;
        // OUTSIDE_SWEEP_RUNS: first node of a pixel outside the set = the first pixel of its run of one grey-level bucket inside
        // this 64-pixel chunk (the run joins the dark forest of the blob sweep as one component; depth 1, like the run labels above)
        int pre = -1;
        if (outside == OUTSIDE_SWEEP_RUNS) {
            const int lv = (valid && !in) ? sweep_level(px[c]) : 0;
            const int lvl_left = __shfl_up(lv, 1, 64);
            const bool same = lv > 0 && lane > 0 && lvl_left == lv;
            const unsigned long long st3 = __ballot(lv > 0 && !same);
            if (lv > 0) pre = y * w + x - (lane - (63 - __clzll((long long)(st3 & ((lane == 63) ? ~0ull : ((2ull << lane) - 1ull))))));
        }
        if (in) {
            unsigned long long m = starts & ((lane == 63) ? ~0ull : ((2ull << lane) - 1ull));
            int sx = m ? (x0 + 63 - __clzll(m)) : carry_start;
            L[base + x] = y * w + sx;
        } else if (valid && outside != OUTSIDE_UNTOUCHED) {
            // OUTSIDE_SWEEP_RUNS (the dark forest of the blob sweep): singletons, except that the pixels of a run that joins the
            // set at one threshold (same grey-level bucket) start as children of the run's first pixel -- the run is one
            // component the moment it joins, and these stores are coalesced, which the per-bucket lists' are not
            L[base + x] = pre >= 0 ? pre : (outside != OUTSIDE_NONE ? y * w + x : -1);
        }
        bool last_in = (b >> 63) & 1ull;
        if (last_in) {
            carry_start = starts ? (x0 + 63 - __clzll(starts)) : carry_start;
            carry_in = 1;
        } else {
            carry_in = 0;
        }
    }
    }
    }
}

// grid = (ceil(N / CCL_BLK_PX), n): a workgroup walks CCL_BLK_PX pixels, a thread 4 consecutive ones per step (one dword
// of the image when rows allow), so the common case -- none of them in the set -- costs one load and no 64-bit index
// arithmetic, and the grid stays small enough that workgroup dispatch is not what the pass waits for
constexpr int CCL_BLK_PX = 8192;
__global__ __launch_bounds__(256) void k_ccl_merge(const uint8_t *__restrict__ img, int h, int w, int thr,
                                                   int invert, int conn8, const FrameState *__restrict__ st, Window win,
                                                   int *__restrict__ L)
{
    const int N = h * w;
    const size_t f = blockIdx.y;
    const Rect r = window_rect(st, f, win, h, w);
    const uint8_t *im = img + f * (size_t)N;
    int *Lf = L + f * (size_t)N;
    const bool aligned = ((((size_t)im) | (size_t)N) & 3) == 0;
    for (int it = 0; it < CCL_BLK_PX / 1024; it++) {
        const int i0 = blockIdx.x * CCL_BLK_PX + it * 1024 + threadIdx.x * 4;
        if (i0 >= N) break;
        int y = i0 / w, x = i0 - y * w;
        if (y > r.y1 || y + 1 < r.y0) continue;
        if (aligned) {
            const uint32_t v4 = *reinterpret_cast<const uint32_t *>(im + i0);
            bool any = false;
#pragma unroll
            for (int k = 0; k < 4; k++) any |= ((((int)((v4 >> (8 * k)) & 255u) > thr) ? 1 : 0) != invert);
            if (!any) continue;
        }
        for (int k = 0; k < 4; k++, x++) {
            const int i = i0 + k;
            if (i >= N) break;
            if (x == w) { x = 0; y++; }
            if (y <= r.y0 || y > r.y1 || x < r.x0 || x > r.x1) continue;
            if (!pred(im, i, thr, invert)) continue;
            const bool up = pred(im, i - w, thr, invert);
            const bool left = x > r.x0 && pred(im, i - 1, thr, invert);
            if (up) {
                bool upleft = x > r.x0 && pred(im, i - w - 1, thr, invert);
                if (!(left && upleft)) uf_unite(Lf, i, i - w);
            } else if (conn8) {
                if (x < r.x1 && pred(im, i - w + 1, thr, invert)) {
                    bool right = pred(im, i + 1, thr, invert);
                    if (!right) uf_unite(Lf, i, i - w + 1);
                }
                if (x > r.x0 && !left && pred(im, i - w - 1, thr, invert)) uf_unite(Lf, i, i - w - 1);
            }
        }
    }
}

// ---- word-level walks (rows 16-byte aligned): a thread owns one 64-pixel word column over CCL_STRIP rows, packs each
// row's membership into a 64-bit mask (SWAR byte compare + multiply gather) and finds the pixels that have work to do --
// run starts, run-overlap starts -- with shifts and ANDs; only those few touch the label plane.
constexpr int CCL_STRIP = 8;
__device__ __forceinline__ unsigned pack8_gt(unsigned long long v, int thr, int invert)   // bit k = ((byte k > thr) != invert)
{
    const unsigned long long H = 0x8080808080808080ull, O = 0x0101010101010101ull;
    const unsigned long long g = ((v & ~H) + (unsigned long long)(0x7f - (thr & 0x7f)) * O) & H;   // low 7 bits > low 7 bits of thr
    unsigned long long res = (thr < 128) ? ((v & H) | g) : ((v & H) & g);
    if (invert) res ^= H;
    return (unsigned)(((res >> 7) * 0x0102040810204080ull) >> 56);
}
__device__ __forceinline__ unsigned long long pack_row64(const uint8_t *row, int x0, int w, int thr, int invert)
{
    unsigned long long bits = 0;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const int x = x0 + 16 * c;
        if (x < w) {   // w % 16 == 0: the 16 pixels are all inside
            const uint4 v = *reinterpret_cast<const uint4 *>(row + x);
            const unsigned long long lo = v.x | ((unsigned long long)v.y << 32), hi = v.z | ((unsigned long long)v.w << 32);
            bits |= (unsigned long long)(pack8_gt(lo, thr, invert) | (pack8_gt(hi, thr, invert) << 8)) << (16 * c);
        }
    }
    return bits;
}
__device__ __forceinline__ unsigned long long col_mask64(int x0, int lo, int hi)   // pixels x0 + b with lo <= x0 + b <= hi
{
    const int a = max(lo - x0, 0), b = min(hi - x0, 63);
    if (b < a) return 0ull;
    const unsigned long long m = (b == 63) ? ~0ull : ((1ull << (b + 1)) - 1ull);
    return m & ~((1ull << a) - 1ull);
}

// where the word-level walks read the set from: the u8 image (compare with a threshold) or a one-bit plane of it that
// already exists (cpe_dev.h tiled layout: the 8 rows of a walk's strip are one 64-byte line; zero beyond the image) -- an
// eighth of the bytes
struct ByteSrc {
    const uint8_t *img; int w, thr, invert;
    __device__ __forceinline__ ByteSrc frame(size_t f, int h) const { return ByteSrc{img + f * (size_t)h * w, w, thr, invert}; }
    __device__ __forceinline__ unsigned long long pack(int y, int x0) const { return pack_row64(img + (size_t)y * w, x0, w, thr, invert); }
    __device__ __forceinline__ bool px(int y, int x) const { return pred(img + (size_t)y * w, x, thr, invert); }
    // rows y8 .. y8 + 7 (y8 = 8 * strip) of word column x0, the rows outside ya .. yb as zero
    __device__ __forceinline__ void strip(int y8, int ya, int yb, int x0, unsigned long long (&m)[CCL_STRIP]) const
    {
#pragma unroll
        for (int k = 0; k < CCL_STRIP; k++) m[k] = (y8 + k >= ya && y8 + k <= yb) ? pack(y8 + k, x0) : 0ull;
    }
    // bit k: pixel x of row y8 + k (rows outside ya .. yb: 0)
    __device__ __forceinline__ unsigned colbits(int y8, int ya, int yb, int x) const
    {
        unsigned b = 0;
#pragma unroll
        for (int k = 0; k < CCL_STRIP; k++)
            if (y8 + k >= ya && y8 + k <= yb && px(y8 + k, x)) b |= 1u << k;
        return b;
    }
};
struct BitSrc {
    const unsigned long long *plane; int tc; size_t plane_words;
    __device__ __forceinline__ BitSrc frame(size_t f, int) const { return BitSrc{plane + f * plane_words, tc, plane_words}; }
    // x0: a multiple of 64
    __device__ __forceinline__ unsigned long long pack(int y, int x0) const { return plane[bit_word(tc, y, x0 >> 6)]; }
    __device__ __forceinline__ bool px(int y, int x) const { return (plane[bit_word(tc, y, x >> 6)] >> (x & 63)) & 1ull; }
    // a strip is one tile: its 8 rows in four 16-byte loads (rows outside ya .. yb are left in, the walks skip them)
    __device__ __forceinline__ void strip(int y8, int, int, int x0, unsigned long long (&m)[CCL_STRIP]) const
    {
        typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
        const u64x2 *t = reinterpret_cast<const u64x2 *>(plane + bit_word(tc, y8, x0 >> 6));
#pragma unroll
        for (int q = 0; q < 4; q++) { const u64x2 v = t[q]; m[2 * q] = v.x; m[2 * q + 1] = v.y; }
    }
    __device__ __forceinline__ unsigned colbits(int y8, int ya, int yb, int x) const
    {
        unsigned long long m[CCL_STRIP];
        strip(y8, ya, yb, x & ~63, m);
        unsigned b = 0;
#pragma unroll
        for (int k = 0; k < CCL_STRIP; k++) b |= (unsigned)((m[k] >> (x & 63)) & 1ull) << k;
        return b;
    }
};

// the complement of a one-bit plane (the dark set of the blob sweep's first labelling is the complement of plane 0) in a stack
// of planes per frame (frame f's plane at plane + f * frame_words).  Bits past the image read as set here: every walk masks its
// columns with the rectangle and skips the rows outside it.
struct NotBitSrc {
    BitSrc b;
    size_t frame_words;
    __device__ __forceinline__ NotBitSrc frame(size_t f, int) const
    {
        return NotBitSrc{BitSrc{b.plane + f * frame_words, b.tc, b.plane_words}, frame_words};
    }
    __device__ __forceinline__ unsigned long long pack(int y, int x0) const { return ~b.pack(y, x0); }
    __device__ __forceinline__ bool px(int y, int x) const { return !b.px(y, x); }
    __device__ __forceinline__ void strip(int y8, int ya, int yb, int x0, unsigned long long (&m)[CCL_STRIP]) const
    {
        b.strip(y8, ya, yb, x0, m);
#pragma unroll
        for (int k = 0; k < CCL_STRIP; k++) m[k] = ~m[k];
    }
    __device__ __forceinline__ unsigned colbits(int y8, int ya, int yb, int x) const { return ~b.colbits(y8, ya, yb, x) & 0xffu; }
};

// ---- a tile's own components.  The thread of a word-level walk holds its 64 x 8 tile as eight row masks, so the components of
// the set inside the tile (inside the window) need no memory: k_ccl_init64 works them out with shifts and ANDs and stores
// them as first labels, and k_ccl_merge64 only unites across the tile's edges.  Both kernels decide from the same masks
// whether a tile is handled that way (tile_is_local), so nothing has to pass from one to the other.

// every run of bg that holds a bit of f (f inside bg), whole: adding the seeds ripples a carry to the end of their runs (fill
// towards the high bits), the same on the bit-reversed word fills towards the low bits (as flood_row below does)
__device__ __forceinline__ unsigned long long fill_runs(unsigned long long bg, unsigned long long f)
{
    f = (((bg + f) ^ bg) & bg) | f;
    const unsigned long long rb = __brevll(bg), rf = __brevll(f);
    return __brevll((((rb + rf) ^ rb) & rb) | rf);
}
// one step of a component's growth: the runs of row `bg` that touch `from`, the component's pixels in the row above or below,
// join its pixels `c` of that row (4-connected: the same column; 8-connected: the columns next to it as well)
__device__ __forceinline__ bool tile_spread(unsigned long long from, unsigned long long bg, unsigned long long &c, int conn8)
{
    unsigned long long s = conn8 ? (from | (from << 1) | (from >> 1)) : from;
    s &= bg & ~c;
    if (!s) return false;
    c |= fill_runs(bg, s);
    return true;
}
// The in-tile work is bounded by the number of runs of the tile (its rows inside the window): a tile has at most as many
// components as runs, and one with more than CCL_TILE_RUNS of them -- a checkerboard, dense noise -- keeps the per-run first
// labels and the in-tile unions of the merge.  Either way the merge ends with the same components.
constexpr int CCL_TILE_RUNS = 24;
__device__ __forceinline__ bool tile_is_local(const unsigned long long (&rows)[CCL_STRIP])
{
    int runs = 0;
#pragma unroll
    for (int k = 0; k < CCL_STRIP; k++) runs += __popcll(rows[k] & ~(rows[k] << 1));
    return runs <= CCL_TILE_RUNS;
}
// bit k: row y8 + k lies in ya .. yb
__device__ __forceinline__ unsigned row_mask8(int y8, int ya, int yb)
{
    return ya > yb ? 0u : (((2u << (yb - y8)) - 1u) & ~((1u << (ya - y8)) - 1u));
}
__device__ __forceinline__ void store_labels(int *Lrow, int a, int e, int label)   // Lrow[a .. e - 1] = label; Lrow 16-byte aligned
{
    int b = a;
    while (b < e) {
        if ((b & 3) == 0 && b + 4 <= e) { *reinterpret_cast<int4 *>(Lrow + b) = make_int4(label, label, label, label); b += 4; }
        else { Lrow[b] = label; b++; }
    }
}
__device__ __forceinline__ void store_row_labels(int *Lrow, unsigned long long m, int label)   // Lrow[b] = label for the bits b of m
{
    while (m) {
        const unsigned long long low = m & (0ull - m), run = m & ~(m + low);
        const int a = __ffsll((long long)low) - 1;
        store_labels(Lrow, a, a + __popcll(run), label);
        m &= ~run;
    }
}

// First labels of a sparse pass.  A tile that tile_is_local: every pixel of a component of the tile (conn8: 8-connected, else
// 4-connected; inside the window) points at the component's first pixel in raster order, its seed.  If the seed is the
// word's first pixel and the set goes on in the word to the left, the whole component points at that word's last pixel of
// the row instead (base - 1: smaller than every index of the component, so parents stay smaller, and no atomic is needed
// because nothing else writes these labels before the merge); every other contact with a neighbouring tile is left to the
// merge.  The components are found one at a time: the lowest pixel not yet labelled is the seed, its run the start, and
// downward and upward sweeps over the eight rows add the runs that touch the component until a round adds nothing.
// Other tiles: every pixel points at the first pixel of its run inside the word, a run that continues from the word to the
// left at that word's last pixel (a chain of at most one link per word: the forest the row-wise k_ccl_init builds, a few
// links deeper).
template <class SRC>
__global__ __launch_bounds__(256) void k_ccl_init64(SRC src0, int h, int w, int conn8,
                                                    const FrameState *__restrict__ st, Window win, int *__restrict__ L)
{
    const int WW = (w + 63) >> 6, strips = (h + CCL_STRIP - 1) / CCL_STRIP;
    const size_t f = blockIdx.y;
    const int gi = blockIdx.x * 256 + threadIdx.x;
    if (gi >= WW * strips) return;
    const int sy = gi / WW, j = gi - sy * WW;
    const Rect r = window_rect(st, f, win, h, w);
    const int x0 = j * 64;
    if (r.x1 < r.x0 || x0 > r.x1 || x0 + 63 < r.x0) return;
    const int ya = max(sy * CCL_STRIP, r.y0), yb = min(sy * CCL_STRIP + CCL_STRIP - 1, r.y1);
    const size_t N = (size_t)h * w;
    const SRC src = src0.frame(f, h);
    int *Lf = L + f * N;
    const unsigned long long cmask = col_mask64(x0, r.x0, r.x1);
    const bool hasL = x0 - 1 >= r.x0;
    const int y8 = sy * CCL_STRIP;
    unsigned long long rows[CCL_STRIP], any = 0;
    src.strip(y8, ya, yb, x0, rows);
#pragma unroll
    for (int k = 0; k < CCL_STRIP; k++) { rows[k] = (y8 + k >= ya && y8 + k <= yb) ? rows[k] & cmask : 0ull; any |= rows[k]; }
    if (!any) return;
    // the left neighbours only matter for a run that starts in column 0 of the word
    const unsigned lb = (hasL && (any & 1ull)) ? src.colbits(y8, ya, yb, x0 - 1) : 0u;
    if (!tile_is_local(rows)) {
#pragma unroll
        for (int k = 0; k < CCL_STRIP; k++) {
            unsigned long long m = rows[k];
            const int base = (y8 + k) * w + x0;
            const bool cL = (m & 1ull) && ((lb >> k) & 1u);
            while (m) {
                const unsigned long long low = m & (0ull - m), run = m & ~(m + low);
                const int a = __ffsll((long long)low) - 1;
                store_labels(Lf + base, a, a + __popcll(run), (a == 0 && cL) ? base - 1 : base + a);
                m &= ~run;
            }
        }
        return;
    }
    for (;;) {     // one component per turn; rows[] keeps the pixels not yet labelled
        unsigned long long comp[CCL_STRIP];
        int label = -1;
#pragma unroll
        for (int k = 0; k < CCL_STRIP; k++) {
            comp[k] = 0ull;
            if (label < 0 && rows[k]) {
                const unsigned long long m = rows[k], low = m & (0ull - m);
                const int base = (y8 + k) * w + x0;
                comp[k] = m & ~(m + low);
                label = ((low & 1ull) && ((lb >> k) & 1u)) ? base - 1 : base + __ffsll((long long)low) - 1;
            }
        }
        if (label < 0) break;
        // Sweeps alternate until one adds nothing: the component is then closed in that direction, and still closed in the
        // other one, because nothing changed since the sweep before.  Nothing unlabelled lies above the seed, so a first
        // downward sweep that adds nothing ends it as well.
        for (bool down = true;; down = !down) {
            bool grew = false;
            if (down) {
#pragma unroll
                for (int k = 1; k < CCL_STRIP; k++) grew |= tile_spread(comp[k - 1], rows[k], comp[k], conn8);
            } else {
#pragma unroll
                for (int k = CCL_STRIP - 2; k >= 0; k--) grew |= tile_spread(comp[k + 1], rows[k], comp[k], conn8);
            }
            if (!grew) break;
        }
#pragma unroll
        for (int k = 0; k < CCL_STRIP; k++) rows[k] &= ~comp[k];
        // (written out: the compiler does not unroll a loop of these inside the component loop, and comp[] must stay in registers)
        static_assert(CCL_STRIP == 8, "k_ccl_init64 stores the eight rows of a component one by one");
        int *Lt = Lf + y8 * w + x0;
        store_row_labels(Lt, comp[0], label);         store_row_labels(Lt + w, comp[1], label);
        store_row_labels(Lt + 2 * w, comp[2], label); store_row_labels(Lt + 3 * w, comp[3], label);
        store_row_labels(Lt + 4 * w, comp[4], label); store_row_labels(Lt + 5 * w, comp[5], label);
        store_row_labels(Lt + 6 * w, comp[6], label); store_row_labels(Lt + 7 * w, comp[7], label);
    }
}

// The unions of a word-level pass, in terms of pixel pairs (the same pairs as k_ccl_merge).  A pixel p of the set is united
//   (v) with the pixel above it, unless the pair one column to the left is a member pair too: p and its left neighbour are
//       one run, so are the two pixels above them, and that pair is united by its own (v);
//   (r) conn8, nothing above p: with the pixel up-right, unless p's right neighbour is in the set -- that one has the
//       up-right pixel above it, (v), and is in p's run;
//   (l) conn8, nothing above p: with the pixel up-left, unless p's left neighbour is in the set (likewise).
// Two pixels next to each other in a row are one run and were linked by the first labels -- inside a word always, across a
// word's left edge when the first labels are the row-wise ones (k_ccl_init) or the per-run ones of k_ccl_init64.
// TILES false (first labels from k_ccl_init): all of (v), (r), (l) for every row of the tile.
// TILES true (first labels from k_ccl_init64), a tile that tile_is_local: its rows are already united among themselves by
// the first labels, which leaves
//   - the tile's first row against the row above it: (v), (r), (l) as they stand;
//   - rows 1 .. 7: (r) at the word's last pixel and (l) at its first one, the only pairs that cross the tile's edge there.
//     The skips hold as above: where they point at a pixel above p or beside the pixel up-right / up-left, that pixel is in
//     p's or the neighbour's tile together with the one it is joined to, and joined to it by that tile's first labels (or,
//     in a tile that is not local, by that tile's own (v));
//   - (h) the first pixel of a row with its left neighbour, the last pixel of the word to the left, unless the row above, in
//       the same tile, has the same contact: the two pixels of this word lie above each other in one tile and so do the two
//       of the left word, so both pairs are joined already, and the row above makes its own (h).  The tile's first row always
//       makes its (h): its (v) at the first pixel counts on it.  A (h) that the first labels made (the label of the row's
//       first pixel is its left neighbour) is seen with one load and skipped.
//   What a skipped union counts on is always a union or a first label of a pair further up or further left, never the other
//   way round, so no two skips count on each other.
// TILES true, any other tile: as TILES false; its first labels are the per-run ones.
// A vertical line costs one union per tile it crosses instead of one per row, a solid region one (v) and one (h) per tile.
template <class SRC, bool TILES>
__global__ __launch_bounds__(256) void k_ccl_merge64(SRC src0, int h, int w,
                                                     int conn8, const FrameState *__restrict__ st, Window win,
                                                     int *__restrict__ L)
{
    const int WW = (w + 63) >> 6, strips = (h + CCL_STRIP - 1) / CCL_STRIP;
    const size_t f = blockIdx.y;
    const int gi = blockIdx.x * 256 + threadIdx.x;
    if (gi >= WW * strips) return;
    const int sy = gi / WW, j = gi - sy * WW;
    const Rect r = window_rect(st, f, win, h, w);
    const int x0 = j * 64;
    if (r.x1 < r.x0 || x0 > r.x1 || x0 + 63 < r.x0) return;
    const int y8 = sy * CCL_STRIP;
    const int ya = max(y8, r.y0), yb = min(y8 + CCL_STRIP - 1, r.y1);
    if (ya > yb) return;
    const size_t N = (size_t)h * w;
    const SRC src = src0.frame(f, h);
    int *Lf = L + f * N;
    const unsigned long long cmask = col_mask64(x0, r.x0, r.x1);
    const bool hasL = x0 - 1 >= r.x0, hasR = x0 + 64 <= r.x1;
    // the tile's rows inside the window, the others as zero
    unsigned long long rows[CCL_STRIP], any = 0;
    src.strip(y8, ya, yb, x0, rows);
#pragma unroll
    for (int k = 0; k < CCL_STRIP; k++) { rows[k] = (y8 + k >= ya && y8 + k <= yb) ? rows[k] & cmask : 0ull; any |= rows[k]; }
    if (!any) return;
    // the neighbour columns only enter at bit 0 (left) / bit 63 (right) of a row of the strip
    const unsigned rm = row_mask8(y8, ya, yb);
    const unsigned lb = (hasL && (any & 1ull)) ? src.colbits(y8, ya, yb, x0 - 1) & rm : 0u;
    const unsigned rb = (hasR && (any >> 63)) ? src.colbits(y8, ya, yb, x0 + 64) & rm : 0u;
    // the row above the tile, when the window has it, for the pixels that can ask for it
    unsigned long long A = 0, aL = 0, aR = 0;
    if (y8 - 1 >= r.y0 && rows[0]) {
        A = src.pack(y8 - 1, x0) & cmask;
        aL = (hasL && (rows[0] & 1ull) && src.px(y8 - 1, x0 - 1)) ? 1ull : 0ull;
        aR = (hasR && (rows[0] >> 63) && src.px(y8 - 1, x0 + 64)) ? 1ull : 0ull;
    }
    const bool local = TILES && tile_is_local(rows);
#pragma unroll
    for (int k = 0; k < CCL_STRIP; k++) {
        const unsigned long long C = rows[k];
        const unsigned long long cL = (lb >> k) & 1u, cR = (rb >> k) & 1u;
        if (C) {
            const bool edges = local && k > 0;     // only the pairs across the tile's left / right edge are left
            const unsigned long long Cs = (C << 1) | cL, As = (A << 1) | aL;            // left, up-left
            const int base = (y8 + k) * w + x0;
            unsigned long long m = edges ? 0ull : C & A & ~(Cs & As);
            while (m) { const int b = __ffsll((long long)m) - 1; m &= m - 1; uf_unite(Lf, base + b, base + b - w); }
            if (local && (C & 1ull) && cL && !(k > 0 && (A & 1ull) && aL) && uf_load(Lf, base) != base - 1) uf_unite(Lf, base, base - 1);
            if (conn8) {
                const unsigned long long Cr = (C >> 1) | (cR << 63), Ar = (A >> 1) | (aR << 63);   // right, up-right
                const unsigned long long nu = C & ~A;
                m = nu & Ar & ~Cr & (edges ? 1ull << 63 : ~0ull);
                while (m) { const int b = __ffsll((long long)m) - 1; m &= m - 1; uf_unite(Lf, base + b, base + b - w + 1); }
                m = nu & As & ~Cs & (edges ? 1ull : ~0ull);
                while (m) { const int b = __ffsll((long long)m) - 1; m &= m - 1; uf_unite(Lf, base + b, base + b - w - 1); }
            }
        }
        A = C; aL = cL; aR = cR;
    }
}

// component list of a roots-only pass: only the first pixel of a horizontal run can carry its own index
template <class SRC>
__global__ __launch_bounds__(256) void k_ccl_roots64(SRC src0, int h, int w,
                                                     FrameState *__restrict__ st, Window win, const int *__restrict__ L,
                                                     int *__restrict__ roots, RootList list)
{
    const int WW = (w + 63) >> 6, strips = (h + CCL_STRIP - 1) / CCL_STRIP;
    const size_t f = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int gi = blockIdx.x * 256 + threadIdx.x;
    const Rect r = window_rect(st, f, win, h, w);
    const size_t N = (size_t)h * w;
    const SRC src = src0.frame(f, h);
    const int *Lf = L + f * N;
    const int sy = gi / WW, j = gi - sy * WW, x0 = j * 64;
    const bool live = gi < WW * strips && !(r.x1 < r.x0 || x0 > r.x1 || x0 + 63 < r.x0);
    // (an empty rectangle may be INT_MAX .. -1: nothing of it enters the row arithmetic unless `live`)
    const int ya = live ? max(sy * CCL_STRIP, r.y0) : 0, yb = live ? min(sy * CCL_STRIP + CCL_STRIP - 1, r.y1) : -1;
    const unsigned long long cmask = live ? col_mask64(x0, r.x0, r.x1) : 0ull;
    const bool hasL = live && x0 - 1 >= r.x0;
    const int y8 = sy * CCL_STRIP;
    unsigned long long rows[CCL_STRIP], any = 0;
    unsigned lb = 0;
    if (live) {
        src.strip(y8, ya, yb, x0, rows);
#pragma unroll
        for (int k = 0; k < CCL_STRIP; k++) any |= (y8 + k >= ya && y8 + k <= yb) ? rows[k] & cmask : 0ull;
        if (hasL && (any & 1ull)) lb = src.colbits(y8, ya, yb, x0 - 1);
    }
#pragma unroll
    for (int k = 0; k < CCL_STRIP; k++) {     // wave-uniform trip count: the appends below are wavefront collectives
        const int y = y8 + k;
        unsigned long long starts = 0;
        if (live && y >= ya && y <= yb) {
            const unsigned long long C = rows[k] & cmask;
            const unsigned long long cL = (C & 1ull) && ((lb >> k) & 1u) ? 1ull : 0ull;
            starts = C & ~((C << 1) | cL);
        }
        while (__ballot(starts != 0)) {
            int i = -1;
            if (starts) { const int b = __ffsll((long long)starts) - 1; starts &= starts - 1; i = y * w + x0 + b; }
            const bool cand = i >= 0 && Lf[i] == i;
            const unsigned long long rb = __ballot(cand);
            if (!rb) continue;
            int base = 0;
            const int leader = __ffsll((long long)rb) - 1;
            if (lane == leader) base = atomicAdd(root_counter(st[f], list), __popcll(rb));
            base = __shfl(base, leader, 64);
            if (cand) {
                const int q = base + __popcll(rb & ((1ull << lane) - 1ull));
                if (q < MAXROOTS) roots[f * MAXROOTS + q] = i;
                else set_overflow(st[f], OVF_ROOTS);
            }
        }
    }
}

// k_ccl_finish of a pass with pixel counts (COUNT_ALL; labels outside the set not read, no touch, no bounding box), word-level: the pixels of a run
// inside a word are one component, so a run costs one uf_find, its labels are stored as the root in 16-byte stores, and its
// length goes to the root's count once (a thread sums consecutive runs of one root, a wavefront the threads' last sums).
// Only the first pixel of a run can be a root (roots are the smallest index of their component).
template <class SRC>
__global__ __launch_bounds__(256) void k_ccl_finish64(SRC src0, int h, int w, FrameState *__restrict__ st, Window win,
                                                      int *__restrict__ L, int *__restrict__ cnt, int *__restrict__ roots, RootList list)
{
    const int WW = (w + 63) >> 6, strips = (h + CCL_STRIP - 1) / CCL_STRIP;
    const size_t f = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int gi = blockIdx.x * 256 + threadIdx.x;
    const Rect r = window_rect(st, f, win, h, w);
    const size_t N = (size_t)h * w;
    const SRC src = src0.frame(f, h);
    int *Lf = L + f * N, *cf = cnt + f * N;
    const int sy = gi / WW, j = gi - sy * WW, x0 = j * 64;
    const bool live = gi < WW * strips && !(r.x1 < r.x0 || x0 > r.x1 || x0 + 63 < r.x0);
    if (!__ballot(live)) return;   // (wave-uniform: the appends and sums below are wavefront collectives)
    const int ya = live ? max(sy * CCL_STRIP, r.y0) : 0, yb = live ? min(sy * CCL_STRIP + CCL_STRIP - 1, r.y1) : -1;
    const unsigned long long cmask = live ? col_mask64(x0, r.x0, r.x1) : 0ull;
    const bool hasL = live && x0 - 1 >= r.x0;
    const int y8 = sy * CCL_STRIP;
    unsigned long long rows[CCL_STRIP], any = 0;
    unsigned lb = 0;
    if (live) {
        src.strip(y8, ya, yb, x0, rows);
#pragma unroll
        for (int k = 0; k < CCL_STRIP; k++) any |= (y8 + k >= ya && y8 + k <= yb) ? rows[k] & cmask : 0ull;
        if (hasL && (any & 1ull)) lb = src.colbits(y8, ya, yb, x0 - 1);
    }
    int key = -1, kc = 0;   // root and pixel count not yet added to cnt
#pragma unroll
    for (int k = 0; k < CCL_STRIP; k++) {
        const int y = y8 + k;
        unsigned long long m = (live && y >= ya && y <= yb) ? rows[k] & cmask : 0ull;
        const bool cL = (m & 1ull) && ((lb >> k) & 1u);
        const int base = y * w + x0;
        while (__ballot(m != 0)) {
            int i = -1;
            if (m) {
                const unsigned long long low = m & (0ull - m), run = m & ~(m + low);
                const int a = __ffsll((long long)low) - 1, e = a + __popcll(run);
                m &= ~run;
                // read-only walk, as in k_ccl_finish
                const int root = uf_find(Lf, base + a);
                if (root == base + a && !(a == 0 && cL)) {
                    i = root;   // a run whose first pixel is the root: its labels already point there
                } else {
                    int b = a;
                    while (b < e) {
                        if ((b & 3) == 0 && b + 4 <= e) { *reinterpret_cast<int4 *>(Lf + base + b) = make_int4(root, root, root, root); b += 4; }
                        else { Lf[base + b] = root; b++; }
                    }
                }
                if (root != key) {
                    if (key >= 0) atomicAdd(&cf[key], kc);
                    key = root; kc = 0;
                }
                kc += e - a;
            }
            const unsigned long long rb = __ballot(i >= 0);
            if (!rb) continue;
            int q0 = 0;
            const int leader = __ffsll((long long)rb) - 1;
            if (lane == leader) q0 = atomicAdd(root_counter(st[f], list), __popcll(rb));
            q0 = __shfl(q0, leader, 64);
            if (i >= 0) {
                const int q = q0 + __popcll(rb & ((1ull << lane) - 1ull));
                if (q < MAXROOTS) roots[f * MAXROOTS + q] = i;
                else set_overflow(st[f], OVF_ROOTS);
            }
        }
    }
    // the threads' last sums: one atomic per root of the wavefront
    unsigned long long active = __ballot(key >= 0);
    while (active) {
        const int leader = __ffsll((long long)active) - 1;
        const int lk = __shfl(key, leader, 64);
        const unsigned long long same = __ballot(key == lk) & active;
        int c = (key == lk) ? kc : 0;
        for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off, 64);
        if (lane == leader) atomicAdd(&cf[lk], c);
        active &= ~same;
    }
}

// components of the set that reach the border of the working rectangle: touch[root] = 1
__global__ __launch_bounds__(256) void k_ccl_touch(const int *__restrict__ L, int n, int h, int w,
                                                   const FrameState *__restrict__ st, Window win,
                                                   uint8_t *__restrict__ touch)
{
    const int per = 2 * w + 2 * h;
    int gi = blockIdx.x * blockDim.x + threadIdx.x;
    if (gi >= n * per) return;
    int f = gi / per, k = gi - f * per;
    const Rect r = window_rect(st, f, win, h, w);
    if (r.x1 < r.x0) return;
    const int rw = r.x1 - r.x0 + 1, rh = r.y1 - r.y0 + 1;
    int x, y;
    if (k < w) { if (k >= rw) return; x = r.x0 + k; y = r.y0; }
    else if (k < 2 * w) { if (k - w >= rw) return; x = r.x0 + k - w; y = r.y1; }
    else if (k < 2 * w + h) { if (k - 2 * w >= rh) return; x = r.x0; y = r.y0 + k - 2 * w; }
    else { if (k - 2 * w - h >= rh) return; x = r.x1; y = r.y0 + k - 2 * w - h; }
    size_t N = (size_t)h * w;
    const int *Lf = L + f * N;
    int v = Lf[(size_t)y * w + x];
    if (v >= 0) touch[f * N + uf_find(Lf, v)] = 1;
}

// component list (ccl_components): a root is a pixel of the set whose label is its own index.  Same walk as
// k_ccl_merge (CCL_BLK_PX pixels per workgroup, 4 per thread and step, dword reject).
__global__ __launch_bounds__(256) void k_ccl_roots4(const uint8_t *__restrict__ img, int h, int w, int thr, int invert,
                                                    FrameState *__restrict__ st, Window win, const int *__restrict__ L,
                                                    int *__restrict__ roots, RootList list)
{
    const int N = h * w;
    const size_t f = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const uint8_t *im = img + f * (size_t)N;
    const int *Lf = L + f * (size_t)N;
    const Rect r = window_rect(st, f, win, h, w);
    const bool aligned = ((((size_t)im) | (size_t)N) & 3) == 0;
    for (int it = 0; it < CCL_BLK_PX / 1024; it++) {
        const int i0 = blockIdx.x * CCL_BLK_PX + it * 1024 + threadIdx.x * 4;
        bool cand[4] = {false, false, false, false};
        if (i0 < N) {
            int y = i0 / w, x = i0 - y * w;
            if (!(y > r.y1 || y + 1 < r.y0)) {
                bool any = true;
                if (aligned) {
                    const uint32_t v4 = *reinterpret_cast<const uint32_t *>(im + i0);
                    any = false;
#pragma unroll
                    for (int k = 0; k < 4; k++) any |= ((((int)((v4 >> (8 * k)) & 255u) > thr) ? 1 : 0) != invert);
                }
                if (any) {
                    for (int k = 0; k < 4; k++, x++) {
                        const int i = i0 + k;
                        if (i >= N) break;
                        if (x == w) { x = 0; y++; }
                        if (y < r.y0 || y > r.y1 || x < r.x0 || x > r.x1) continue;
                        cand[k] = pred(im, i, thr, invert) && Lf[i] == i;
                    }
                }
            }
        }
        if (!__ballot(cand[0] || cand[1] || cand[2] || cand[3])) continue;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const unsigned long long rb = __ballot(cand[k]);
            if (!rb) continue;
            int base = 0;
            const int leader = __ffsll((long long)rb) - 1;
            if (lane == leader) base = atomicAdd(root_counter(st[f], list), __popcll(rb));
            base = __shfl(base, leader, 64);
            if (cand[k]) {
                const int q = base + __popcll(rb & ((1ull << lane) - 1ull));
                if (q < MAXROOTS) roots[f * MAXROOTS + q] = i0 + k;
                else set_overflow(st[f], OVF_ROOTS);
            }
        }
    }
}

// flatten + count (CclCount) + collect roots + bounding box, one read of the label plane.  COUNT_INTERIOR gives exact prune
// bounds to the blob detector: a hole of >= 5000 pixels, or a bright component with >= 5000 interior pixels, has
// border-polygon area >= 5000 (polygon edges only cross the unit squares of their own end-point pixels).
constexpr int CCL_FIN_PX = 8192;
__global__ __launch_bounds__(256) void k_ccl_finish(const uint8_t *__restrict__ img, int h, int w, int thr,
                                                    int invert, FrameState *__restrict__ st, Window win,
                                                    int *__restrict__ L, const uint8_t *__restrict__ touch, CclCount count,
                                                    int *__restrict__ cnt, int *__restrict__ roots, int *__restrict__ nrect,
                                                    CclOutside outside, RootList list)
{
    // grid = (ceil(N / CCL_FIN_PX), n): a workgroup never straddles two frames, so every wave-level aggregate below is
    // per frame; many steps of 256 pixels per workgroup keep the grid (and its dispatch time) small
    const size_t N = (size_t)h * w;
    const size_t f = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const Rect r = window_rect(st, f, win, h, w);
    {   // the workgroup's pixels lie in rows ya .. yb: outside the working rectangle there is nothing to flatten, count or list
        const size_t p0 = (size_t)blockIdx.x * CCL_FIN_PX;
        const int ya = (int)(p0 / w), yb = (int)((min(p0 + CCL_FIN_PX, N) - 1) / w);
        if (r.x1 < r.x0 || yb < r.y0 || ya > r.y1) return;
    }
    for (int it = 0; it < CCL_FIN_PX / 256; it++) {
    const int i = blockIdx.x * CCL_FIN_PX + it * 256 + threadIdx.x;
    if ((size_t)(blockIdx.x * CCL_FIN_PX + it * 256) >= N) break;
    const size_t gi = f * N + (size_t)i;
    int root = -1, x = 0, y = 0;
    if ((size_t)i < N) {
        y = i / w; x = i - y * w;
        if (!(y < r.y0 || y > r.y1 || x < r.x0 || x > r.x1) && (outside == OUTSIDE_NONE || pred(img + f * N, i, thr, invert))) {
            int v = L[gi];
            if (v >= 0) {
                // read-only walk: the pointer jumping of uf_find_c re-points nodes at *an* ancestor, and such a store from
                // another thread's walk through this pixel may land after the store below and leave it one hop short
                root = uf_find(L + f * N, v);
                L[gi] = root;
            }
        }
    }
    const bool in = root >= 0;
    if (nrect && __ballot(in)) {
        int mnx = in ? x : INT_MAX, mxx = in ? x : INT_MIN, mny = in ? y : INT_MAX, mxy = in ? y : INT_MIN;
        for (int off = 32; off >= 1; off >>= 1) {
            mnx = min(mnx, __shfl_xor(mnx, off, 64)); mxx = max(mxx, __shfl_xor(mxx, off, 64));
            mny = min(mny, __shfl_xor(mny, off, 64)); mxy = max(mxy, __shfl_xor(mxy, off, 64));
        }
        if (lane == 0) {
            // most wavefronts already lie inside the accumulated box: test first, keep the atomics rare
            int *nr = nrect + 16 * f;   // 64 B per frame: its own cache line
            if (mnx < __hip_atomic_load(nr + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(nr + 0, mnx);
            if (mny < __hip_atomic_load(nr + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(nr + 1, mny);
            if (mxx > __hip_atomic_load(nr + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(nr + 2, mxx);
            if (mxy > __hip_atomic_load(nr + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(nr + 3, mxy);
        }
    }
    const bool touched = in && touch && touch[f * N + root];
    if (roots) {
        // root list: one atomic per wavefront
        const bool is_root = in && !touched && root == i;
        unsigned long long rb = __ballot(is_root);
        if (rb) {
            int base = 0;
            const int leader = __ffsll((long long)rb) - 1;
            if (lane == leader) base = atomicAdd(root_counter(st[f], list), __popcll(rb));
            base = __shfl(base, leader, 64);
            if (is_root) {
                int k = base + __popcll(rb & ((1ull << lane) - 1ull));
                if (k < MAXROOTS) roots[f * MAXROOTS + k] = i;
                else set_overflow(st[f], OVF_ROOTS);
            }
        }
    }
    if (count == COUNT_ALL || count == COUNT_INTERIOR) {
        bool c = in && !touched;
        if (c && count == COUNT_INTERIOR) {
            const uint8_t *im = img + f * N;
            bool inter = x > 0 && x < w - 1 && y > 0 && y < h - 1;
            if (inter) {
                inter = pred(im, i - w - 1, thr, invert) && pred(im, i - w, thr, invert) && pred(im, i - w + 1, thr, invert) &&
                        pred(im, i - 1, thr, invert) && pred(im, i + 1, thr, invert) && pred(im, i + w - 1, thr, invert) &&
                        pred(im, i + w, thr, invert) && pred(im, i + w + 1, thr, invert);
            }
            c = inter;
        }
        int key = c ? root : -1;
        unsigned long long active = __ballot(key >= 0);
        while (active) {
            int leader = __ffsll((long long)active) - 1;
            int lk = __shfl(key, leader, 64);
            unsigned long long same = __ballot(key == lk) & active;
            if (lane == leader) atomicAdd(&cnt[f * N + lk], __popcll(same));
            active &= ~same;
        }
    }
    }
}

enum CtlOp : int { CTL_RESET_ROOTS, CTL_SWEEP_RECT };
__global__ void k_ccl_ctl(FrameState *st, int *nrect, int n, CtlOp op, RootList list)
{
    int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n) return;
    FrameState &S = st[f];
    if (op == CTL_RESET_ROOTS) {
        *root_counter(S, list) = 0;
    } else {   // CTL_SWEEP_RECT: working rectangle = accumulated bounding box; accumulator emptied
        int *nr = nrect + 16 * f;
        for (int k = 0; k < 4; k++) { S.crect[k] = nr[k]; S.nrect[k] = nr[k]; }
        nr[0] = INT_MAX; nr[1] = INT_MAX; nr[2] = -1; nr[3] = -1;
    }
}

// Writers of the tiled one-bit planes (cpe_dev.h).  Every row of a plane's last tile row is written, the rows >= h as zeros,
// and so are the two zero tile columns.

// one wavefront per 512 pixels of a row (8 groups of 64): a ballot per threshold is the 64-bit group of that plane; lane t
// collects plane t's eight groups.  rows_total = n * 8 ceil(h / 8) (the padding rows included)
__global__ __launch_bounds__(256) void k_bitplanes(const uint8_t *__restrict__ img, int rows_total, int h, int w, int thr0, int step,
                                                   int nplanes, unsigned long long *__restrict__ planes)
{
    const int lane = threadIdx.x & 63;
    const int chunks = (w + 63) >> 6, groups = (chunks + 7) >> 3, tc = bit_tile_cols(w), hp = (h + 7) & ~7;
    const long long gw = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gw >= (long long)rows_total * groups) return;
    const int row = (int)(gw / groups), g = (int)(gw - (long long)row * groups);
    const int f = row / hp, y = row - f * hp;
    const size_t plane_words = bit_plane_words(h, w);
    unsigned long long *out = planes + (size_t)f * nplanes * plane_words;
    unsigned long long mine[8];
    const int c0 = g * 8, nc = min(8, chunks - c0);
#pragma unroll
    for (int q = 0; q < 8; q++) {
        mine[q] = 0;
        if (q < nc) {
            const int x = (c0 + q) * 64 + lane;
            const int v = (x < w && y < h) ? (int)img[((size_t)f * h + y) * w + x] : -1;
            for (int t = 0; t < nplanes; t++) {
                unsigned long long b = __ballot(v > thr0 + t * step);
                if (lane == t) mine[q] = b;
            }
        }
    }
    if (lane < nplanes) {
        unsigned long long *o = out + (size_t)lane * plane_words;
#pragma unroll
        for (int q = 0; q < 8; q++)
            if (q < nc) o[bit_word(tc, y, c0 + q)] = mine[q];
        if (g == 0) o[bit_word(tc, y, -1)] = 0ull;
        if (g == groups - 1) o[bit_word(tc, y, chunks)] = 0ull;
    }
}

// the same planes when rows start on 16-byte boundaries: a thread loads 64 pixels once (4 x 16 bytes) and makes their word of
// every plane with SWAR compares -- no ballots, 16 times fewer load instructions.  Thread order (frame, tile row, word
// column, row in the tile): 8 consecutive lanes write one whole tile of every plane.  A word column's threads of tile
// column 0 / the last one also write those (zero) tiles.
__global__ __launch_bounds__(256) void k_bitplanes64(const uint8_t *__restrict__ img, int n, int h, int w, int thr0, int step,
                                                     int nplanes, unsigned long long *__restrict__ planes)
{
    const int chunks = (w + 63) >> 6, tc = bit_tile_cols(w), th = (h + 7) >> 3;
    const long long gi = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gi >= (long long)n * th * chunks * 8) return;
    const int r = (int)(gi & 7);
    const long long tile = gi >> 3;
    const int j = (int)(tile % chunks);
    const long long ft = tile / chunks;
    const int f = (int)(ft / th), y = (int)(ft - (long long)f * th) * 8 + r;
    const size_t plane_words = bit_plane_words(h, w);
    unsigned long long *out = planes + (size_t)f * nplanes * plane_words;
    unsigned long long v[8];
    const uint8_t *p = img + ((size_t)f * h + y) * w + j * 64;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        uint4 q = make_uint4(0, 0, 0, 0);
        if (y < h && j * 64 + 16 * c < w) q = *reinterpret_cast<const uint4 *>(p + 16 * c);   // w % 16 == 0: all 16 inside
        v[2 * c] = q.x | ((unsigned long long)q.y << 32);
        v[2 * c + 1] = q.z | ((unsigned long long)q.w << 32);
    }
    // pixels past the end of the row (and rows past the image) were loaded as 0 and every threshold is >= 0: their bits stay clear
    const size_t wi = bit_word(tc, y, j);
    for (int t = 0; t < nplanes; t++) {
        const int thr = thr0 + t * step;
        unsigned long long bits = 0;
#pragma unroll
        for (int c = 0; c < 8; c++) bits |= (unsigned long long)pack8_gt(v[c], thr, 0) << (8 * c);
        unsigned long long *o = out + (size_t)t * plane_words;
        o[wi] = bits;
        if (j == 0) o[wi - 8] = 0ull;
        if (j == chunks - 1) o[wi + 8] = 0ull;
    }
}

// single plane (mask != 0 / image > thr): one thread per byte of the plane = 8 pixels of one row, 64 consecutive bytes (one
// tile) per 64 threads
__global__ __launch_bounds__(256) void k_bitplane1(const uint8_t *__restrict__ img, int n, int h, int w, int thr,
                                                   unsigned long long *__restrict__ plane)
{
    const int tc = bit_tile_cols(w);
    const size_t pb = bit_plane_words(h, w) * 8;      // bytes per plane
    const long long gi = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gi >= (long long)n * pb) return;
    const int f = (int)(gi / pb);
    const int rem = (int)(gi - (long long)f * pb);
    const int tile = rem >> 6, r = (rem >> 3) & 7, bi = rem & 7;
    const int ty = tile / tc, tx = tile - ty * tc;
    const int y = ty * 8 + r, x0 = (tx - 1) * 64 + bi * 8;
    unsigned b = 0;
    if (tx > 0 && y < h && x0 < w) {     // (x0 >= 0 for tx > 0; the last tile column starts at or past w)
        const uint8_t *p = img + ((size_t)f * h + y) * w + x0;
        if (x0 + 8 <= w && ((((size_t)p) & 3) == 0)) {
            const uint32_t a = *reinterpret_cast<const uint32_t *>(p), c = *reinterpret_cast<const uint32_t *>(p + 4);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                b |= ((int)((a >> (8 * k)) & 255u) > thr ? 1u : 0u) << k;
                b |= ((int)((c >> (8 * k)) & 255u) > thr ? 1u : 0u) << (4 + k);
            }
        } else {
            for (int k = 0; k < 8 && x0 + k < w; k++) b |= ((int)p[k] > thr ? 1u : 0u) << k;
        }
    }
    reinterpret_cast<uint8_t *>(plane)[gi] = (uint8_t)b;
}

}  // namespace

int build_bitplanes(const uint8_t *img, int n, int h, int w, int thr0, int step, int nplanes, uint32_t *planes, hipStream_t s)
{
    CPE_CHECK_ARG(nplanes >= 1 && nplanes <= 64, "build_bitplanes: 1..64 planes");
    CPE_LAUNCH_BEGIN();
    unsigned long long *pl = reinterpret_cast<unsigned long long *>(planes);
    const int th = (h + 7) >> 3;
    if (nplanes == 1) {
        const long long bytes = (long long)n * bit_plane_words(h, w) * 8;
        CPE_KLAUNCH(k_bitplane1, dim3((unsigned)((bytes + 255) / 256)), dim3(256), 0, s, img, n, h, w, thr0, pl);
        CPE_CHECK_LAUNCH("k_bitplane1");
        return CPE_OK;
    }
    if (w % 16 == 0 && (((size_t)img) & 15) == 0 && thr0 >= 0 && step >= 0 && thr0 + (nplanes - 1) * step <= 255) {
        const long long words = (long long)n * th * 8 * ((w + 63) >> 6);
        CPE_KLAUNCH(k_bitplanes64, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, s, img, n, h, w, thr0, step, nplanes, pl);
        CPE_CHECK_LAUNCH("k_bitplanes64");
        return CPE_OK;
    }
    const long long waves = (long long)n * th * 8 * ((((w + 63) >> 6) + 7) >> 3);
    CPE_KLAUNCH(k_bitplanes, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, img, n * th * 8, h, w, thr0, step, nplanes, pl);
    CPE_CHECK_LAUNCH("k_bitplanes");
    return CPE_OK;
}

// ---- RETR_EXTERNAL: which components lie inside a hole of another one ------------------------------------------------
// cv2.findContours(RETR_EXTERNAL) skips an outer border whose start pixel lies inside the outer border of a component
// found earlier (icvFindNextContour: the last border mark passed on the row is positive), i.e. every component that sits
// in a hole of another one, at any depth.  Equivalent, scan-free form: a component is external iff the background pixel
// west of its raster-first pixel belongs to the OUTER background, the 4-connected background region that reaches the
// border of the window.  This kernel computes that region as a bit mask, one workgroup per frame:
//   out[y][j] bit b = 1  <=>  pixel (64 j + b, y) is background and 4-connected to the window border through background
// by alternating downward / upward sweeps over the rows (lane j owns word j of a row; a row takes what the previous row
// of the sweep has, fills it sideways through runs of background -- carry-ripple fill inside a word, lane exchange across
// words) until a sweep changes nothing.  Typical masks (small blobs, open line fragments) converge in two sweeps; the
// third one only confirms.  Pixels outside the window count as outer background.  w <= 4096 (64 words).
__device__ __forceinline__ unsigned long long pack_nonzero64(const uint8_t *row, int x0, int w)
{
    unsigned long long m = 0;
    if (x0 + 64 <= w && ((((size_t)row) + x0) & 7) == 0) {
        const unsigned long long *p = reinterpret_cast<const unsigned long long *>(row + x0);
#pragma unroll
        for (int k = 0; k < 8; k++) {
            unsigned long long v = p[k];
            v |= v >> 4; v |= v >> 2; v |= v >> 1;
            v &= 0x0101010101010101ull;
            m |= ((v * 0x0102040810204080ull) >> 56) << (8 * k);
        }
    } else {
        for (int b = 0; b < 64 && x0 + b < w; b++) m |= (unsigned long long)(row[x0 + b] != 0) << b;
    }
    return m;
}

// sideways fill of `seed` through the runs of bg, across the words held by the lanes 0 .. WW-1.
// Inside a word: adding the seeds to the run mask ripples a carry from every seed to the end of its run (fill towards the
// high bits); the same on the bit-reversed word fills towards the low bits.  Between words: a filled bit 63 / bit 0 seeds
// the neighbouring word's bit 0 / bit 63; repeat while any lane received a new seed.
__device__ __forceinline__ unsigned long long flood_row(unsigned long long bg, unsigned long long seed, int lane, int WW)
{
    unsigned long long f = seed & bg;
    const unsigned long long rb = __brevll(bg);
    for (;;) {
        f = (((bg + f) ^ bg) & bg) | f;
        const unsigned long long rf = __brevll(f);
        f = __brevll((((rb + rf) ^ rb) & rb) | rf);
        const unsigned long long from_lo = __shfl_up(f, 1, 64), from_hi = __shfl_down(f, 1, 64);
        unsigned long long add = 0;
        if (lane > 0 && lane < WW && (from_lo >> 63) && (bg & 1ull) && !(f & 1ull)) add |= 1ull;
        if (lane + 1 < WW && (from_hi & 1ull) && (bg >> 63) && !(f >> 63)) add |= 1ull << 63;
        if (!__ballot(add != 0ull)) break;
        f |= add;
    }
    return f;
}

// One workgroup per frame, FLOOD_BANDS wavefronts: the window's rows are cut into bands, one per wavefront.  A round is a
// downward and an upward sweep of every band at the same time, each starting from what its neighbour band's boundary row held
// at the last barrier (rows outside the window: all outer background); rounds repeat until one changes nothing anywhere.
// The result is the least fixed point of "background next to outer background (or to the window border) is outer
// background", which does not depend on the order of the updates: the same mask as one wavefront sweeping the whole window
// (the round-2 form: 1.16 ms per launch at 1920x1200, a serial walk of ~1000 rows three times).  The left / right window
// columns seed every row directly, so a sparse mask is nearly done after the first sweep of each band whatever the band above
// knows; what is shadowed from both sides on its own row gets filled from the rows above / below in the next rounds.
constexpr int FLOOD_BANDS = 16;
__global__ __launch_bounds__(64 * FLOOD_BANDS) void k_outside_flood(const uint8_t *__restrict__ mask, int h, int w, FrameState *__restrict__ st,
                                                                   Window win, unsigned long long *__restrict__ bgw_all,
                                                                   unsigned long long *__restrict__ out_all, size_t plane_words,
                                                                   const uint32_t *__restrict__ bits)
{
    // bits (optional): the mask's one-bit plane (build_bitplanes, 1 plane per frame) -- an eighth of the bytes of the first sweep
    __shared__ int s_any[2];
    const size_t f = blockIdx.x;
    const int lane = threadIdx.x & 63, band = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), WW = (w + 63) >> 6;
    const Rect r = window_rect(st, f, win, h, w);
    if (r.x1 < r.x0 || r.y1 < r.y0) return;
    const uint8_t *im = mask + f * (size_t)h * w;
    const int btc = bit_tile_cols(w);
    const unsigned long long *bp = bits ? bit_plane(bits, f, h, w) : nullptr;
    unsigned long long *bgw = bgw_all + f * plane_words, *out = out_all + f * plane_words;
    const int x0 = lane * 64;
    const unsigned long long cmask = lane < WW ? col_mask64(x0, r.x0, r.x1) : 0ull;
    // window columns r.x0 / r.x1 touch the outside on their left / right
    unsigned long long edge = 0;
    if (lane < WW) {
        if (r.x0 >= x0 && r.x0 < x0 + 64) edge |= 1ull << (r.x0 - x0);
        if (r.x1 >= x0 && r.x1 < x0 + 64) edge |= 1ull << (r.x1 - x0);
    }
    const int nrows = r.y1 - r.y0 + 1;
    const int per = (nrows + FLOOD_BANDS - 1) / FLOOD_BANDS;
    const int ya = r.y0 + band * per, yb = min(r.y1, ya + per - 1);      // this wavefront's rows (none: yb < ya)
    const int mine = max(0, yb - ya + 1);
    if (threadIdx.x < 2) s_any[threadIdx.x] = 0;
    // Rows are loaded ahead of their use: the flood of a row only needs the previous row's result (a register), so the
    // next chunk of rows is requested before the current one is worked on.
    constexpr int CHUNK = 8;
    // boundary row of the neighbour band as of the last barrier (L1-bypassing load: another wavefront wrote it)
    auto nb_row = [&](int y) -> unsigned long long {
        if (y < r.y0 || y > r.y1) return ~0ull;                         // outside the window: all outer background
        return lane < WW ? __hip_atomic_load(&out[(size_t)y * WW + lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
    };
    // ---- first sweep (down): pack the background once, seed from the window border; the band above is not known yet
    {
        unsigned long long prev = band == 0 ? ~0ull : 0ull;
        unsigned long long nxt[CHUNK];
        auto load0 = [&](int k0, unsigned long long *dst) {
#pragma unroll
            for (int k = 0; k < CHUNK; k++) {
                const int y = ya + k0 + k;
                unsigned long long m = 0;
                if (lane < WW && k0 + k < mine)
                    m = bp ? bp[bit_word(btc, y, lane)] : pack_nonzero64(im + (size_t)y * w, x0, w);
                dst[k] = ~m & cmask;
            }
        };
        load0(0, nxt);
        for (int k0 = 0; k0 < mine; k0 += CHUNK) {
            unsigned long long bgc[CHUNK];
#pragma unroll
            for (int k = 0; k < CHUNK; k++) bgc[k] = nxt[k];
            if (k0 + CHUNK < mine) load0(k0 + CHUNK, nxt);
#pragma unroll
            for (int k = 0; k < CHUNK; k++) {
                if (k0 + k >= mine) break;
                const int y = ya + k0 + k;
                const unsigned long long bg = bgc[k];
                unsigned long long seed = (prev | edge) & bg;
                if (y == r.y1) seed = bg;      // the row below the window is all outside
                // most rows of a sparse mask: every background pixel has outer background right above it
                const unsigned long long o = __ballot(seed != bg) ? flood_row(bg, seed, lane, WW) : bg;
                if (lane < WW) { bgw[(size_t)y * WW + lane] = bg; out[(size_t)y * WW + lane] = o; }
                prev = o;
            }
        }
    }
    __syncthreads();
    // ---- further sweeps (up, down, up, ...) until a whole round changes nothing in any band.  A row's entry is only
    // rewritten by the wavefront that owns it, in program order, so loading it a chunk early is safe.
    bool converged = false;
    for (int pass = 1; pass < FLOOD_MAX_PASSES; pass++) {
        const bool upw = pass & 1;
        bool any = false;
        unsigned long long prev = mine > 0 ? nb_row(upw ? yb + 1 : ya - 1) : 0ull;
        unsigned long long nb[CHUNK], nc[CHUNK];
        auto load1 = [&](int k0, unsigned long long *db, unsigned long long *dc) {
#pragma unroll
            for (int k = 0; k < CHUNK; k++) {
                const int kk = k0 + k;
                const int y = upw ? yb - kk : ya + kk;
                const bool ok = lane < WW && kk < mine;
                db[k] = ok ? bgw[(size_t)y * WW + lane] : 0ull;
                dc[k] = ok ? out[(size_t)y * WW + lane] : 0ull;
            }
        };
        load1(0, nb, nc);
        for (int k0 = 0; k0 < mine; k0 += CHUNK) {
            unsigned long long bgc[CHUNK], curc[CHUNK];
#pragma unroll
            for (int k = 0; k < CHUNK; k++) { bgc[k] = nb[k]; curc[k] = nc[k]; }
            if (k0 + CHUNK < mine) load1(k0 + CHUNK, nb, nc);
#pragma unroll
            for (int k = 0; k < CHUNK; k++) {
                const int kk = k0 + k;
                if (kk >= mine) break;
                const int y = upw ? yb - kk : ya + kk;
                const unsigned long long bg = bgc[k], cur = curc[k];
                const unsigned long long seed = cur | (prev & bg);
                unsigned long long o = cur;
                if (__ballot(seed != cur)) {
                    o = flood_row(bg, seed, lane, WW);
                    if (lane < WW && o != cur) { out[(size_t)y * WW + lane] = o; any = true; }
                }
                prev = o;
            }
        }
        // a round = an upward and a downward sweep (passes 2q - 1 and 2q); s_any[q & 1] collects its changes
        const int slot = ((pass + 1) >> 1) & 1;
        if (__ballot(any) && lane == 0) atomicOr(&s_any[slot], 1);
        __syncthreads();
        if (!upw) {                                  // end of a round
            const int ch = s_any[slot];
            __syncthreads();
            if (threadIdx.x == 0) s_any[slot] = 0;   // next used two rounds on: the barriers in between order the reset
            if (!ch) { converged = true; break; }
        }
    }
    // a background that still grows after FLOOD_MAX_PASSES alternating sweeps (a spiral thousands of turns deep) would
    // leave components wrongly classified as nested: report the frame instead of altering it silently
    if (!converged && threadIdx.x == 0) set_overflow(st[f], OVF_TRACE);
}

int outside_flood(const uint8_t *mask, int n, int h, int w, FrameState *st, Window win, unsigned long long *bgw,
                  unsigned long long *out, size_t plane_words, hipStream_t s, const uint32_t *bits)
{
    CPE_CHECK_ARG(w <= 4096 && plane_words >= (size_t)h * ((w + 63) >> 6), "outside_flood: frame too wide or scratch too small");
    CPE_LAUNCH_BEGIN();
    CPE_KLAUNCH(k_outside_flood, dim3(n), dim3(64 * FLOOD_BANDS), 0, s, mask, h, w, st, win, bgw, out, plane_words, bits);
    CPE_CHECK_LAUNCH("k_outside_flood");
    return CPE_OK;
}

// ---- the labelling entry points (cpe_dev.h).  Each picks the kernels itself: word-level walks where rows start on 16-byte
// boundaries, reading the one-bit plane of the set where the caller has one, the byte-level kernels elsewhere.
static bool word_rows(const void *img, const int *L, int w) { return w % 16 == 0 && ((size_t)img & 15) == 0 && ((size_t)L & 15) == 0; }
static dim3 word_grid(int n, int h, int w) { return dim3((unsigned)((((w + 63) / 64) * ((h + CCL_STRIP - 1) / CCL_STRIP) + 255) / 256), n); }

// the links of the set img > thr, 8-connected if conn8, else 4-connected (labels outside it untouched); true: the word-level
// kernels made them
static bool links(const uint8_t *img, int n, int h, int w, int thr, int conn8, Window win, int *L, FrameState *st, hipStream_t s)
{
    const size_t N = (size_t)h * w;
    if (word_rows(img, L, w)) {
        const ByteSrc src{img, w, thr, 0};
        CPE_KLAUNCH(k_ccl_init64<ByteSrc>, word_grid(n, h, w), dim3(256), 0, s, src, h, w, conn8, (const FrameState *)st, win, L);
        CPE_KLAUNCH((k_ccl_merge64<ByteSrc, true>), word_grid(n, h, w), dim3(256), 0, s, src, h, w, conn8, (const FrameState *)st, win, L);
        return true;
    }
    CPE_KLAUNCH(k_ccl_init, dim3((n * h + CCL_INIT_ROWS - 1) / CCL_INIT_ROWS), dim3(256), 0, s, img, n * h, h, w, thr, 0, (const FrameState *)st, win, L,
                (int *)nullptr, OUTSIDE_UNTOUCHED);
    CPE_KLAUNCH(k_ccl_merge, dim3((unsigned)((N + CCL_BLK_PX - 1) / CCL_BLK_PX), n), dim3(256), 0, s, img, h, w, thr, 0, conn8, (const FrameState *)st, win, L);
    return false;
}

bool ccl_components_reads_bits(const uint32_t *bits, int w, const int *L) { return bits && w % 16 == 0 && ((size_t)L & 15) == 0; }

int ccl_components(const uint8_t *img, const uint32_t *bits, int n, int h, int w, int thr, Window win, int *L, int *roots,
                   RootList list, FrameState *st, hipStream_t s)
{
    return ccl_components_conn(img, bits, n, h, w, thr, 1, win, L, roots, list, st, s);
}

int ccl_components_conn(const uint8_t *img, const uint32_t *bits, int n, int h, int w, int thr, int conn8, Window win, int *L,
                        int *roots, RootList list, FrameState *st, hipStream_t s)
{
    const size_t N = (size_t)h * w;
    const dim3 gw = word_grid(n, h, w);
    CPE_LAUNCH_BEGIN();
    CPE_KLAUNCH(k_ccl_ctl, dim3((n + 63) / 64), dim3(64), 0, s, st, (int *)nullptr, n, CTL_RESET_ROOTS, list);
    if (ccl_components_reads_bits(bits, w, L)) {
        const BitSrc src{bit_plane(bits, 0, h, w), bit_tile_cols(w), bit_plane_words(h, w)};
        CPE_KLAUNCH(k_ccl_init64<BitSrc>, gw, dim3(256), 0, s, src, h, w, conn8, (const FrameState *)st, win, L);
        CPE_KLAUNCH((k_ccl_merge64<BitSrc, true>), gw, dim3(256), 0, s, src, h, w, conn8, (const FrameState *)st, win, L);
        CPE_KLAUNCH(k_ccl_roots64<BitSrc>, gw, dim3(256), 0, s, src, h, w, st, win, (const int *)L, roots, list);
    } else if (links(img, n, h, w, thr, conn8, win, L, st, s)) {
        CPE_KLAUNCH(k_ccl_roots64<ByteSrc>, gw, dim3(256), 0, s, (ByteSrc{img, w, thr, 0}), h, w, st, win, (const int *)L, roots, list);
    } else {
        CPE_KLAUNCH(k_ccl_roots4, dim3((unsigned)((N + CCL_BLK_PX - 1) / CCL_BLK_PX), n), dim3(256), 0, s, img, h, w, thr, 0, st, win, (const int *)L,
                    roots, list);
    }
    CPE_CHECK_LAUNCH("ccl_components");
    return CPE_OK;
}

int ccl_unions(const uint8_t *mask, int n, int h, int w, Window win, int *L, FrameState *st, hipStream_t s)
{
    CPE_LAUNCH_BEGIN();
    links(mask, n, h, w, 0, 1, win, L, st, s);
    CPE_CHECK_LAUNCH("ccl_unions");
    return CPE_OK;
}

int ccl_label(const uint8_t *img, int n, int h, int w, int *L, const CclPass &p, FrameState *st, hipStream_t s)
{
    const size_t N = (size_t)h * w;
    CPE_LAUNCH_BEGIN();
    if (p.roots) CPE_KLAUNCH(k_ccl_ctl, dim3((n + 63) / 64), dim3(64), 0, s, st, (int *)nullptr, n, CTL_RESET_ROOTS, ROOTS_MAIN);
    CPE_KLAUNCH(k_ccl_init, dim3((n * h + CCL_INIT_ROWS - 1) / CCL_INIT_ROWS), dim3(256), 0, s, img, n * h, h, w, p.thr, p.invert, (const FrameState *)st, p.win, L,
                p.count ? p.cnt : (int *)nullptr, p.outside);
    if (word_rows(img, L, w))
        CPE_KLAUNCH((k_ccl_merge64<ByteSrc, false>), word_grid(n, h, w), dim3(256), 0, s, (ByteSrc{img, w, p.thr, p.invert}), h, w, p.conn8, (const FrameState *)st, p.win, L);
    else
        CPE_KLAUNCH(k_ccl_merge, dim3((unsigned)((N + CCL_BLK_PX - 1) / CCL_BLK_PX), n), dim3(256), 0, s, img, h, w, p.thr, p.invert, p.conn8,
                    (const FrameState *)st, p.win, L);
    if (p.touch) {
        (void)hipMemsetAsync(p.touch, 0, N * n, s);
        const int per = 2 * w + 2 * h;
        CPE_KLAUNCH(k_ccl_touch, dim3((n * per + 255) / 256), dim3(256), 0, s, (const int *)L, n, h, w, (const FrameState *)st, p.win, p.touch);
    }
    CPE_KLAUNCH(k_ccl_finish, dim3((unsigned)((N + CCL_FIN_PX - 1) / CCL_FIN_PX), n), dim3(256), 0, s, img, h, w, p.thr, p.invert, st, p.win, L,
                (const uint8_t *)p.touch, p.count, p.cnt, p.roots, p.nrect, p.outside, ROOTS_MAIN);
    CPE_CHECK_LAUNCH("ccl_label");
    return CPE_OK;
}

// The set {img <= thr} is read as the complement of plane 0 by the merge and the word-level finish.  The init still reads the
// image: the links of OUTSIDE_SWEEP_RUNS need the grey-level buckets.  Rows that do not start on 16-byte boundaries: ccl_label.
int ccl_dark_first(const uint8_t *img, const uint32_t *planes, int nplanes, int n, int h, int w, int thr, int *L, int *roots,
                   int *cnt, FrameState *st, hipStream_t s)
{
    if (!(word_rows(img, L, w) && planes && nplanes >= 1)) {
        CclPass p;
        p.thr = thr; p.invert = 1; p.conn8 = 0; p.win = WIN_SWEEP; p.outside = OUTSIDE_SWEEP_RUNS;
        p.count = COUNT_ALL; p.cnt = cnt; p.roots = roots;
        return ccl_label(img, n, h, w, L, p, st, s);
    }
    CPE_LAUNCH_BEGIN();
    CPE_KLAUNCH(k_ccl_ctl, dim3((n + 63) / 64), dim3(64), 0, s, st, (int *)nullptr, n, CTL_RESET_ROOTS, ROOTS_MAIN);
    CPE_KLAUNCH(k_ccl_init, dim3((n * h + CCL_INIT_ROWS - 1) / CCL_INIT_ROWS), dim3(256), 0, s, img, n * h, h, w, thr, 1, (const FrameState *)st, WIN_SWEEP, L,
                cnt, OUTSIDE_SWEEP_RUNS);
    const dim3 gw = word_grid(n, h, w);
    const NotBitSrc src{BitSrc{bit_plane(planes, 0, h, w), bit_tile_cols(w), bit_plane_words(h, w)}, (size_t)nplanes * bit_plane_words(h, w)};
    CPE_KLAUNCH((k_ccl_merge64<NotBitSrc, false>), gw, dim3(256), 0, s, src, h, w, 0, (const FrameState *)st, WIN_SWEEP, L);
    CPE_KLAUNCH(k_ccl_finish64<NotBitSrc>, gw, dim3(256), 0, s, src, h, w, st, WIN_SWEEP, L, cnt, roots, ROOTS_MAIN);
    CPE_CHECK_LAUNCH("ccl_dark_first");
    return CPE_OK;
}

int ccl_set_sweep_rect(FrameState *st, int *nrect, int n, hipStream_t s)
{
    CPE_LAUNCH_BEGIN();
    CPE_KLAUNCH(k_ccl_ctl, dim3((n + 63) / 64), dim3(64), 0, s, st, nrect, n, CTL_SWEEP_RECT, ROOTS_MAIN);
    CPE_CHECK_LAUNCH("k_ccl_ctl");
    return CPE_OK;
}

}  // namespace cpe
