// Stages a-2, a-4, a-5, a-6 on the GPU:
//   extract_joints (util_cylinder.py:1805-1827), the joint filter of find_cylinder_centroids_and_center
//   (:1913-1920), mask_roi_around_center (:1944-2007), expands_line_roi / expand_line_roi /
//   process_contour_info / create_rotated_line_kernel / get_pca_endpoints (:35-237).
// [ext] OpenCV / numpy-LAPACK semantics restated exactly as in oracle/src/orc_morph.c, orc_masks.c,
// orc_contours.c, orc_draw.c (those are the bit-level specification; parity unpinned vs cv2).
//
// The reference's dominant cost -- two full-frame dilations with a ~100x100 structuring element per
// line fragment -- becomes one workgroup per fragment end point working on the (15 + K)^2 support in LDS.
#include "cpe_dev.h"

namespace cpe {

namespace {

// ---- bit rows, marched: k_open20_joints and k_roi_base --------------------------------------------------------------------
// Both kernels cut the frame into column strips of BR_SPAN pixels and bands of rows; one wave (a workgroup of 64 threads)
// owns one strip of one band and marches down its rows.  A lane owns 16 pixels of the row: one 16-byte load packs them into
// 16 bits, one 16-byte store writes them back as bytes, and a wave's loads and stores of a row are one contiguous run.  What
// a stage needs of the neighbouring pixels along the row comes from the adjacent lanes' input bits by shuffles, once per row:
// the lane then carries its 16 pixels with a halo in one register and every stage is plain bit arithmetic on it.  The first
// and last BR_HALO lanes of a wave only feed their neighbours.  What a stage needs of other rows stays in registers (or,
// for the 18-row delay of the horizontal opening, in a lane-private LDS ring).  No barrier orders anything between waves.
// The one-bit planes leave through an LDS image of a tile row (15 tiles of 64 bytes per plane): every lane writes its 16
// bits of a row, and after 8 rows the wave stores the tiles whole, 16 bytes per lane.
constexpr int BR_HALO = 2, BR_OUT = 64 - 2 * BR_HALO, BR_SPAN = BR_OUT * 16, BR_WORDS = BR_OUT / 4;
constexpr int BR_TILE = BR_WORDS * 32;      // u16 per plane of the tile-row image
inline int br_strips(int w) { return (w + BR_SPAN - 1) / BR_SPAN; }

__device__ __forceinline__ unsigned span32(int a, int b)      // bits a .. b - 1, clipped to the register
{
    a = max(a, 0); b = min(b, 32);
    if (a >= b) return 0u;
    return (b == 32 ? ~0u : (1u << b) - 1u) & ~((1u << a) - 1u);
}
__device__ __forceinline__ unsigned long long span64(int a, int b)
{
    a = max(a, 0); b = min(b, 64);
    if (a >= b) return 0ull;
    return (b == 64 ? ~0ull : (1ull << b) - 1ull) & ~((1ull << a) - 1ull);
}
__device__ __forceinline__ unsigned nz4(unsigned v)           // byte i != 0 -> bit i
{
    v = (((v & 0x7f7f7f7fu) + 0x7f7f7f7fu) | v) & 0x80808080u;
    return ((v >> 7) * 0x10204080u) >> 28;
}
__device__ __forceinline__ unsigned nz16(const uint4 &v) { return nz4(v.x) | (nz4(v.y) << 4) | (nz4(v.z) << 8) | (nz4(v.w) << 12); }
__device__ __forceinline__ unsigned bytes4(unsigned bits)     // bit i -> byte i = 0 / 255
{
    return (((bits & 15u) * 0x00204081u) & 0x01010101u) * 255u;
}
// 16 pixels of a row; al: the row's bytes are 16-byte aligned and whole, otherwise nv (1 .. 16) of them are in the image
__device__ __forceinline__ uint4 load_px16(const uint8_t *p, bool al, int nv)
{
    if (al) return *reinterpret_cast<const uint4 *>(p);
    unsigned v0 = 0, v1 = 0, v2 = 0, v3 = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) {
        if (b < nv) v0 |= (unsigned)p[b] << (8 * b);
        if (b + 4 < nv) v1 |= (unsigned)p[b + 4] << (8 * b);
        if (b + 8 < nv) v2 |= (unsigned)p[b + 8] << (8 * b);
        if (b + 12 < nv) v3 |= (unsigned)p[b + 12] << (8 * b);
    }
    return make_uint4(v0, v1, v2, v3);
}
__device__ __forceinline__ void store_px16(uint8_t *p, unsigned bits, bool al, int nv)
{
    if (al) {
        *reinterpret_cast<uint4 *>(p) = make_uint4(bytes4(bits), bytes4(bits >> 4), bytes4(bits >> 8), bytes4(bits >> 12));
        return;
    }
#pragma unroll
    for (int b = 0; b < 16; b++)
        if (b < nv) p[b] = ((bits >> b) & 1u) ? 255 : 0;
}
// a lane's 16 bits of row y into the tile-row image (lanes BR_HALO .. 63 - BR_HALO)
__device__ __forceinline__ void tile_put(unsigned short *tile, int l, int y, unsigned bits)
{
    const int k = l - BR_HALO;
    if (k >= 0 && k < BR_OUT) tile[(k >> 2) * 32 + (y & 7) * 4 + (k & 3)] = (unsigned short)bits;
}
// tile row ty of a plane from its image: whole tiles, and the zero tile columns where this strip touches them
__device__ __forceinline__ void tile_flush(const unsigned short *tile, unsigned long long *plane, int w, int ty, int s, bool last, int l)
{
    const int tc = bit_tile_cols(w);
    unsigned long long *row = plane + (size_t)ty * tc * 8;
    if (l < BR_OUT) {
        const int j = s * BR_WORDS + (l >> 2);
        if (j + 2 < tc) *reinterpret_cast<uint4 *>(row + (size_t)(j + 1) * 8 + (l & 3) * 2) = *reinterpret_cast<const uint4 *>(tile + l * 8);
    } else {
        const uint4 z = make_uint4(0, 0, 0, 0);
        if (s == 0) *reinterpret_cast<uint4 *>(row + (l & 3) * 2) = z;
        if (last) *reinterpret_cast<uint4 *>(row + (size_t)(tc - 1) * 8 + (l & 3) * 2) = z;
    }
}

// a-2 in one kernel: binary -> open(20x1) -> hmask, open(1x20) -> vmask, joints = hmask & vmask.
// Erosion and dilation both take the in-image pixels of the window [p-10, p+9] (anchor 10 of a 20-tap line; the border
// never erodes and never dilates).
// Horizontal: the lane's window is 64 bits, its 16 pixels with 24 on either side (two lanes' worth); the 20 taps are the
// doubling 1 -> 2 -> 4 -> 8 -> 16 (+4) of shifted copies.  Its result waits 18 rows in the ring for the vertical one.
// Vertical: per column a counter in five bit slices.  The erosion counts the ones that end at the row just read (up to 20:
// row y - 9 is eroded to one where the count is 20); the dilation counts the rows since the erosion's last one (row y - 18
// is one where fewer than 20).  Rows outside the image read as ones and erode to zeros.  A band starts 20 rows early with
// both counters empty, which is exact from its first output row on.
// Where the consumers read words (hb / vb given: line_masks_as_bits) hmask and vmask leave as one-bit planes as well, the
// joints mask only as one (jbits): its bytes have no reader there, and the bytes of hmask / vmask are a debug output that the
// caller may decline (hm, vm null).
constexpr int OB_R = 80, OB_RING = 24, OB_LAG = 18;
template <bool IS_AND> __device__ __forceinline__ unsigned long long window20(unsigned long long v)
{
    // r[p] = AND / OR of v[p - 10 .. p + 9]; exact for p in [10, 54]
    const unsigned long long f = IS_AND ? ~0ull : 0ull;
    auto up = [&](unsigned long long x, int k) { return (x >> k) | (f << (64 - k)); };
    auto op = [](unsigned long long x, unsigned long long y) { return IS_AND ? (x & y) : (x | y); };
    const unsigned long long t1 = op(v, up(v, 1));
    const unsigned long long t2 = op(t1, up(t1, 2));
    const unsigned long long t4 = op(t2, up(t2, 4));
    const unsigned long long t8 = op(t4, up(t4, 8));
    const unsigned long long t20 = op(t8, up(t4, 12));     // taps 0..15 and 12..19
    return (t20 << 10) | (f >> 54);
}
// five bit slices of a per-column counter that stops at 20
struct Count20 {
    unsigned b0, b1, b2, b3, b4;
    __device__ __forceinline__ unsigned full() const { return b4 & (b3 | b2); }      // columns whose count is 20
    // columns of `keep` count one more (up to 20), all others start again at 0
    __device__ __forceinline__ void step(unsigned keep)
    {
        unsigned c = keep & ~full(), t;
        t = b0 & c; b0 ^= c; c = t;
        t = b1 & c; b1 ^= c; c = t;
        t = b2 & c; b2 ^= c; c = t;
        t = b3 & c; b3 ^= c; c = t;
        b4 ^= c;
        b0 &= keep; b1 &= keep; b2 &= keep; b3 &= keep; b4 &= keep;
    }
};
__global__ __launch_bounds__(64) void k_open20_joints(const uint8_t *__restrict__ bin, int h, int w,
                                                      uint8_t *__restrict__ hm, uint8_t *__restrict__ vm,
                                                      uint8_t *__restrict__ jm, uint32_t *__restrict__ jbits,
                                                      unsigned long long *__restrict__ hb, unsigned long long *__restrict__ vb)
{
    // jbits: the joints mask once more as a one-bit plane: its labelling, its RETR_EXTERNAL flood and the border tracer of
    // the joint centroids read an eighth of the bytes
    __shared__ unsigned short s_ring[OB_RING * 64];
    __shared__ __attribute__((aligned(16))) unsigned short s_tile[3 * BR_TILE];
    const int l = threadIdx.x, s = blockIdx.x, yb = blockIdx.y * OB_R, f = blockIdx.z;
    const bool last = s == (int)gridDim.x - 1;
    const int x0 = (s * BR_OUT + l - BR_HALO) * 16;       // the lane's first pixel
    const bool inx = x0 >= 0 && x0 < w;
    const bool out = inx && l >= BR_HALO && l < 64 - BR_HALO;
    const int nv = min(16, w - x0);
    const unsigned ov = span32(0, nv);                                   // the lane's pixels inside the image
    const unsigned long long vw = span64(24 - x0, w - x0 + 24);          // the same of its window: bit i = pixel x0 - 24 + i
    const size_t N = (size_t)h * w;
    const bool al = ((w & 15) == 0) && ((((size_t)bin | (size_t)hm | (size_t)vm | (size_t)jm) & 15) == 0);
    const uint8_t *src = bin + f * N + x0;
    unsigned long long *pj = bit_plane(jbits, f, h, w);
    const size_t pw = bit_plane_words(h, w);
    const int y_end = min(yb + OB_R, (h + 7) & ~7);        // output rows yb .. y_end - 1 (whole tile rows)
    Count20 ce{0u, 0u, 0u, 0u, 0u};                        // ones that end at the row read last
    Count20 cd{0u, 0u, 0xffffu, 0u, 0xffffu};              // rows since the erosion's last one: 20, none in reach
    int wslot = 0, rslot = 0;
    for (int y = yb - 20; y < y_end + OB_LAG; y++) {
        const bool iny = y >= 0 && y < h;
        unsigned xb = 0u;
        if (iny && inx) xb = nz16(load_px16(src + (size_t)y * w, al, nv));
        if (y >= yb && y < y_end) {       // horizontal opening of the band's own rows
            const unsigned p = xb | (__shfl_down(xb, 1) << 16);
            const unsigned q = __shfl_up(p, 2), r = __shfl_down(p, 2);
            unsigned long long win = (unsigned long long)((q & 0xffffu) >> 8) | ((unsigned long long)(q >> 16) << 8) |
                                     ((unsigned long long)xb << 24) | ((unsigned long long)(p >> 16) << 40) |
                                     ((unsigned long long)(r & 0xffu) << 56);
            const unsigned long long e = window20<true>(win | ~vw) & vw;
            const unsigned hres = iny ? (unsigned)((window20<false>(e) & vw) >> 24) & 0xffffu : 0u;
            s_ring[wslot * 64 + l] = (unsigned short)hres;
            wslot = wslot + 1 == OB_RING ? 0 : wslot + 1;
        }
        // vertical: erosion at row y - 9, dilation at row y - 18
        ce.step(iny ? xb : 0xffffu);
        const int ye = y - 9;
        const unsigned er = (ye >= 0 && ye < h) ? ce.full() : 0u;
        cd.step(~er & 0xffffu);
        const int yo = y - OB_LAG;
        if (yo < yb) continue;
        unsigned hbits = 0u, vbits = 0u;
        if (yo < h) {
            hbits = s_ring[rslot * 64 + l];
            vbits = ~cd.full() & ov;
        }
        rslot = rslot + 1 == OB_RING ? 0 : rslot + 1;
        if (out && yo < h && hm) {
            const size_t o = f * N + (size_t)yo * w + x0;
            store_px16(hm + o, hbits, al, nv);
            store_px16(vm + o, vbits, al, nv);
            if (jm) store_px16(jm + o, hbits & vbits, al, nv);
        }
        tile_put(s_tile, l, yo, hbits & vbits);
        if (hb) { tile_put(s_tile + BR_TILE, l, yo, hbits); tile_put(s_tile + 2 * BR_TILE, l, yo, vbits); }
        if ((yo & 7) == 7) {
            __syncthreads();
            tile_flush(s_tile, pj, w, yo >> 3, s, last, l);
            if (hb) {
                tile_flush(s_tile + BR_TILE, hb + f * pw, w, yo >> 3, s, last, l);
                tile_flush(s_tile + 2 * BR_TILE, vb + f * pw, w, yo >> 3, s, last, l);
            }
            __syncthreads();
        }
    }
}

// a-5 tail + a-6 head in one kernel:  roi = open3x3(mask & circle_mask & mask_contour)  (util_cylinder.py:1995-2005),
// base = close3x3(roi) (:150-152); out-of-image pixels never erode / dilate.  The lane's window is its 16 pixels with 4 on
// either side; the four 3x3 passes (erode, dilate, dilate, erode) each keep the row-wise result of their last two rows, so
// row y - 4 of base leaves when row y has been read.  mask_contour is zero outside the region rectangle, so only its pixels
// are read: everything else packs as zero, and a wave whose strip and band lie further than 4 pixels from it only stores
// its zeros.
// The line mask m comes as bytes, or (mb given: line_masks_as_bits) as the one-bit planes k_open20_joints wrote, one per
// frame; roi's bytes are a debug output (null: not written).
// The kernel also seeds the expanded mask: exp = base & mask_contour (the closing is extensive, base may stick out of
// mask_contour), full frame, zeros included -- k_seg_expand only adds 255s to it, and nothing else clears the plane.
constexpr int RB_R = 40, RB_AP = 4;
__global__ __launch_bounds__(64) void k_roi_base(const uint8_t *__restrict__ m, const uint8_t *__restrict__ cm,
                                                 const uint8_t *__restrict__ mc, int h, int w,
                                                 const FrameState *__restrict__ st, uint8_t *__restrict__ roi,
                                                 uint8_t *__restrict__ base, uint8_t *__restrict__ exp,
                                                 uint32_t *__restrict__ bbits, const unsigned long long *__restrict__ mb)
{
    // bbits: `base` as a one-bit plane (cpe_dev.h tiled layout, one plane per frame): the fragments' flood, border tracer
    // and expansion read the plane, and so does their labelling where rows allow the word-level kernels.
    // base (may be null): the same as bytes, for the byte-level labelling kernels only (masks_stage asks ccl.hip)
    __shared__ __attribute__((aligned(16))) unsigned short s_tile[BR_TILE];
    const int l = threadIdx.x, s = blockIdx.x, yb = blockIdx.y * RB_R, f = blockIdx.z;
    const bool last = s == (int)gridDim.x - 1;
    const int c = s * BR_OUT + l - BR_HALO, x0 = c * 16;
    const bool inx = x0 >= 0 && x0 < w;
    const bool out = inx && l >= BR_HALO && l < 64 - BR_HALO;
    const int nv = min(16, w - x0);
    const unsigned vw = span32(4 - x0, min(24, w - x0 + 4));      // in-image pixels of the window: bit i = pixel x0 - 4 + i
    const size_t N = (size_t)h * w;
    const int *rc = st[f].rect;
    const int rx0 = rc[0], ry0 = rc[1], rx1 = rc[0] + rc[2] - 1, ry1 = rc[1] + rc[3] - 1;
    const bool al = ((w & 15) == 0) && ((((size_t)m | (size_t)cm | (size_t)mc | (size_t)roi | (size_t)base | (size_t)exp) & 15) == 0);
    const int y_end = min(yb + RB_R, (h + 7) & ~7);
    const int sx0 = s * BR_SPAN;
    const bool active = st[f].status != CPE_ST_NO_REGION && yb <= ry1 + RB_AP && yb + RB_R - 1 >= ry0 - RB_AP &&
                        sx0 <= rx1 + RB_AP && sx0 + BR_SPAN - 1 >= rx0 - RB_AP;
    const unsigned rm = inx ? span32(rx0 - x0, min(nv, rx1 + 1 - x0)) : 0u;      // the lane's pixels inside the rectangle
    const int ly0 = max(ry0, 0), ly1 = min(ry1, h - 1);
    const unsigned long long *mbf = mb ? mb + f * bit_plane_words(h, w) : nullptr;
    const int btc = bit_tile_cols(w);
    unsigned long long *pb = bit_plane(bbits, f, h, w);
    unsigned he0 = ~0u, he1 = ~0u, d10 = 0u, d11 = 0u, d20 = 0u, d21 = 0u, e40 = ~0u, e41 = ~0u;   // row-wise results of the last two rows
    unsigned cb0 = 0u, cb1 = 0u, cb2 = 0u, cb3 = 0u;                                              // mc != 0 of the last four
    for (int y = active ? yb - RB_AP : yb + RB_AP; y < y_end + RB_AP; y++) {
        unsigned bs = 0u, rs = 0u, cs = 0u;       // base at row y - 4 and mc != 0 there, roi at row y - 2: the lane's 16 pixels
        if (active) {
            // pack (m & cm & mc) != 0 of the rectangle's pixels, and mc != 0 on its own for the seed of exp
            unsigned xb = 0u, cb = 0u;
            if (rm && y >= ly0 && y <= ly1) {
                const size_t o = f * N + (size_t)y * w + x0;
                const uint4 vc = load_px16(mc + o, al, nv), va = load_px16(cm + o, al, nv);
                uint4 v = make_uint4(va.x & vc.x, va.y & vc.y, va.z & vc.z, va.w & vc.w);
                if (m) {
                    const uint4 vm = load_px16(m + o, al, nv);
                    v = make_uint4(v.x & vm.x, v.y & vm.y, v.z & vm.z, v.w & vm.w);
                }
                xb = nz16(v) & rm;
                cb = nz16(vc) & rm;
                // a line-mask byte is 0 or 255: (m & cm & mc) != 0 is the mask's bit and (cm & mc) != 0
                if (mbf) xb &= (unsigned)(mbf[bit_word(btc, y, c >> 2)] >> ((c & 3) * 16));
            }
            const unsigned win = (xb << 4) | (__shfl_up(xb, 1) >> 12) | ((__shfl_down(xb, 1) & 15u) << 20);
            auto in_image = [&](int yy) { return yy >= 0 && yy < h; };
            auto ero3 = [&](unsigned x, int yy) { x |= ~vw; return in_image(yy) ? (x & (x << 1) & (x >> 1)) : ~0u; };
            auto dil3 = [&](unsigned x) { return x | (x << 1) | (x >> 1); };
            // erode -> row y - 1
            const unsigned he = ero3(win, y);
            const unsigned er = in_image(y - 1) ? (he0 & he1 & he & vw) : 0u;
            he0 = he1; he1 = he;
            // dilate -> roi, row y - 2
            const unsigned d1 = dil3(er);
            const unsigned ro = in_image(y - 2) ? ((d10 | d11 | d1) & vw) : 0u;
            d10 = d11; d11 = d1;
            // dilate -> row y - 3
            const unsigned d2 = dil3(ro);
            const unsigned dd = in_image(y - 3) ? ((d20 | d21 | d2) & vw) : 0u;
            d20 = d21; d21 = d2;
            // erode -> base, row y - 4
            const unsigned e4 = ero3(dd, y - 3);
            const unsigned ba = in_image(y - 4) ? (e40 & e41 & e4 & vw) : 0u;
            e40 = e41; e41 = e4;
            bs = (ba >> 4) & 0xffffu; rs = (ro >> 4) & 0xffffu; cs = cb0;
            cb0 = cb1; cb1 = cb2; cb2 = cb3; cb3 = cb;
        }
        const int yo = y - RB_AP, yr = active ? y - 2 : yo;
        if (roi && out && yr >= yb && yr < y_end && yr < h) store_px16(roi + f * N + (size_t)yr * w + x0, rs, al, nv);
        if (yo < yb) continue;
        if (out && yo < h) {
            const size_t o = f * N + (size_t)yo * w + x0;
            store_px16(exp + o, bs & cs, al, nv);
            if (base) store_px16(base + o, bs, al, nv);
        }
        tile_put(s_tile, l, yo, bs);
        if ((yo & 7) == 7) {
            __syncthreads();
            tile_flush(s_tile, pb, w, yo >> 3, s, last, l);
            __syncthreads();
        }
    }
}

// ---- joints: polygon-moment centroids inside the region rectangle, in cv2.findContours order ----------
__global__ __launch_bounds__(64) void k_joint_centroids(const uint32_t *__restrict__ jbits, int h, int w,
                                                        const int *__restrict__ roots, FrameState *__restrict__ st,
                                                        int *__restrict__ jtmp /* n*MAXJ*3 */,
                                                        const unsigned long long *__restrict__ outside, size_t plane_words)
{
    __shared__ unsigned long long s_win[BW_ROWS * 64];   // the tracer's bit window, one column per lane (cpe_dev.h: BitWin)
    const int f = blockIdx.y;
    if (st[f].status != CPE_ST_OK) return;
    const int ncomp = min(st[f].n_roots_p, MAXROOTS);
    for (int k = blockIdx.x * 64 + threadIdx.x; k < ncomp; k += gridDim.x * 64) {
        const int root = roots[(size_t)f * MAXROOTS + k];
        if (!comp_is_external(outside + f * plane_words, w, root, 0)) continue;   // RETR_EXTERNAL (:1817): inside a hole of another blob
        BitWin<64, true> nz{bit_plane(jbits, f, h, w), w, h, s_win + threadIdx.x};   // 64 short borders that start together: wide loads
        StatVisitor sv;
        if (!trace_border(nz, root % w, root / w, false, sv, 4 * (w + h) + 65536)) { set_overflow(st[f], OVF_TRACE); continue; }
        sv.finish();
        double m00, m10, m01;
        moments_from_sums(sv.a00, sv.a10, sv.a01, m00, m10, m01);
        if (m00 == 0) continue;
        int cx = (int)(m10 / m00), cy = (int)(m01 / m00);
        atomicAdd(&st[f].n_joints_all, 1);
        const int *r = st[f].rect;
        if (!(r[0] <= cx && cx < r[0] + r[2] && r[1] <= cy && cy < r[1] + r[3])) continue;
        int q = atomicAdd(&st[f].n_joints, 1);
        if (q >= MAXJ) { set_overflow(st[f], OVF_JOINTS); continue; }
        int *o = jtmp + ((size_t)f * MAXJ + q) * 3;
        o[0] = cx; o[1] = cy; o[2] = root;
    }
}

__global__ __launch_bounds__(256) void k_joint_sort(FrameState *__restrict__ st, const int *__restrict__ jtmp,
                                                    int *__restrict__ joints /* n*MAXJ*2 */)
{
    const int f = blockIdx.x;
    const int nj = min(st[f].n_joints, MAXJ);
    const int *src = jtmp + (size_t)f * MAXJ * 3;
    int *dst = joints + (size_t)f * MAXJ * 2;
    for (int i = threadIdx.x; i < nj; i += 256) {
        int ki = src[3 * i + 2], rank = 0;
        for (int j = 0; j < nj; j++) rank += (src[3 * j + 2] > ki) ? 1 : 0;  // latest discovery first
        dst[2 * rank] = src[3 * i];
        dst[2 * rank + 1] = src[3 * i + 1];
    }
    __syncthreads();
    if (threadIdx.x == 0) st[f].n_joints = nj;
}

// ---- separable fixed-point Gaussian blur on u8 (cv2.GaussianBlur (7,7) and (19,19), sigma 0) ------------
struct Taps { int k[19]; int r; int shift; };

// Both passes in one kernel: a 64x32 tile with an r-pixel apron goes through LDS, the u16 row sums never reach HBM.
// Neither consumer needs the whole plane, so tiles that cannot matter are skipped:
//   BLUR_SPOT (19x19): only `blurred > 240` is ever asked (util_cylinder.py:1958).  The taps sum to 2^16, so the
//     result is <= the largest input: a tile whose apron holds no pixel > 240 is written as 0.
//   BLUR_RECT (7x7): only the box means around the intersection points are read (find_center_point, :1548-1560), and
//     those points lie inside the region rectangle: tiles away from rect +- (half + 1) are left untouched.
constexpr int BT_X = 64, BT_Y = 32;
// one BT_X x BT_Y tile of the 7 x 7 blur (workgroup-wide, 256 threads; ends with the stores, no barrier after them).
// The window (columns gx0 - 4 .. gx0 + BT_X + 3, dword aligned) goes to LDS with dword loads where the tile and its apron lie
// inside the frame and the rows are 4-byte aligned, byte by byte with reflect101 otherwise.  Row sums: a thread makes 8
// neighbouring sums from 4 dwords of the window (v_alignbyte_b32 + two v_dot4_u32_u8 per sum, as blur19_tile_spot does) and
// stores them as one 16-byte LDS write; the window is in registers by then, so the row sums take its place in LDS.  Column
// pass: a thread makes 4 neighbouring columns of 2 neighbouring rows from 8 eight-byte reads and stores a dword per row.
constexpr int B7_R = 3, B7_IH = BT_Y + 2 * B7_R, B7_QW = (BT_X + 8) / 4;
constexpr int B7_LDS_WORDS = B7_IH * BT_X / 2;     // u16 row sums of the window's rows (>= B7_IH * B7_QW window dwords)
static_assert(B7_IH * B7_QW <= B7_LDS_WORDS && BT_X == 64 && BT_Y == 32, "blur_tile's thread maps");
template <int R>
__device__ __forceinline__ void blur_tile(const uint8_t *__restrict__ im, int h, int w, int gx0, int gy0, const Taps &t,
                                          uint8_t *__restrict__ out, uint32_t *s_buf /* B7_LDS_WORDS */)
{
    static_assert(R == B7_R, "the 7 x 7 tile");
    constexpr int IH = B7_IH, QW = B7_QW, TASKS = IH * (BT_X / 8), PER = (TASKS + 255) / 256;
    const int tid = threadIdx.x;
    const int ax0 = gx0 - 4, ay0 = gy0 - R;
    if (ax0 >= 0 && ax0 + 4 * QW <= w && ay0 >= 0 && ay0 + IH <= h && (w & 3) == 0 && (((size_t)im) & 3) == 0) {
        for (int i = tid; i < IH * QW; i += 256) {
            const int ry = i / QW, q = i - ry * QW;
            s_buf[i] = *reinterpret_cast<const uint32_t *>(im + (size_t)(ay0 + ry) * w + ax0 + 4 * q);
        }
    } else {
        uint8_t *s_in8 = reinterpret_cast<uint8_t *>(s_buf);
        for (int i = tid; i < IH * QW * 4; i += 256) {
            const int ry = i / (4 * QW), b = i - ry * 4 * QW;
            s_in8[i] = im[(size_t)reflect101(ay0 + ry, h) * w + reflect101(ax0 + b, w)];
        }
    }
    __syncthreads();
    // tile column c is window byte c + 4: the sum of column c0 + o reads window bytes c0 + o + 1 .. c0 + o + 7
    uint32_t d[PER][4];
#pragma unroll
    for (int u = 0; u < PER; u++) {
        const int it = tid + 256 * u;
        if (it < TASKS) {
            const int ry = it >> 3, c0 = (it & 7) * 8;
#pragma unroll
            for (int k = 0; k < 4; k++) d[u][k] = s_buf[ry * QW + (c0 >> 2) + k];
        }
    }
    __syncthreads();
    const uint32_t T0 = (uint32_t)t.k[0] | ((uint32_t)t.k[1] << 8) | ((uint32_t)t.k[2] << 16) | ((uint32_t)t.k[3] << 24);
    const uint32_t T1 = (uint32_t)t.k[4] | ((uint32_t)t.k[5] << 8) | ((uint32_t)t.k[6] << 16);
#pragma unroll
    for (int u = 0; u < PER; u++) {
        const int it = tid + 256 * u;
        if (it < TASKS) {
            uint32_t hs[8];
#pragma unroll
            for (int o = 0; o < 8; o++) {
                const int sb = o + 1, i0 = sb >> 2, i1 = (sb + 4) >> 2, sh = sb & 3;
                const uint32_t a0 = sh ? __builtin_amdgcn_alignbyte(d[u][i0 + 1], d[u][i0], sh) : d[u][i0];
                const uint32_t a1 = sh ? __builtin_amdgcn_alignbyte(d[u][i1 < 3 ? i1 + 1 : 3], d[u][i1], sh) : d[u][i1];
                hs[o] = __builtin_amdgcn_udot4(a1, T1, __builtin_amdgcn_udot4(a0, T0, 0u, false), false);
            }
            // s_h[ry * BT_X + c0 + o] as u16: 8 of them are 16 aligned bytes
            reinterpret_cast<uint4 *>(s_buf)[it] = make_uint4(hs[0] | (hs[1] << 16), hs[2] | (hs[3] << 16), hs[4] | (hs[5] << 16), hs[6] | (hs[7] << 16));
        }
    }
    __syncthreads();
    const int cg = tid & 15, ry = (tid >> 4) * 2;      // columns 4 cg .. 4 cg + 3 of rows ry, ry + 1
    uint32_t acc[2][4] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};
#pragma unroll
    for (int j = 0; j < 2 * R + 2; j++) {
        const uint2 p = reinterpret_cast<const uint2 *>(s_buf)[(ry + j) * (BT_X / 4) + cg];
        const uint32_t e[4] = {p.x & 0xFFFFu, p.x >> 16, p.y & 0xFFFFu, p.y >> 16};
#pragma unroll
        for (int c = 0; c < 4; c++) {
            if (j <= 2 * R) acc[0][c] += (uint32_t)t.k[j] * e[c];
            if (j >= 1) acc[1][c] += (uint32_t)t.k[j - 1] * e[c];
        }
    }
    const uint32_t rnd = 1u << (t.shift - 1);
    const int gx = gx0 + 4 * cg;
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const int gy = gy0 + ry + q;
        if (gy >= h) continue;
        uint8_t *o = out + (size_t)gy * w + gx;
        uint32_t b[4];
#pragma unroll
        for (int c = 0; c < 4; c++) b[c] = ((acc[q][c] + rnd) >> t.shift) & 255u;
        if (gx + 4 <= w && (((size_t)o) & 3) == 0) *reinterpret_cast<uint32_t *>(o) = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
        else {
#pragma unroll
            for (int c = 0; c < 4; c++) if (gx + c < w) o[c] = (uint8_t)b[c];
        }
    }
}

// BLUR_RECT (7 x 7): one workgroup per tile, tiles away from the region rectangle are left untouched
template <int R>
__global__ __launch_bounds__(256) void k_blur_fused(const uint8_t *__restrict__ src, int h, int w, int tiles_x, int tiles_y, Taps t,
                                                    const FrameState *__restrict__ st, uint8_t *__restrict__ dst)
{
    __shared__ uint4 s_buf[B7_LDS_WORDS / 4];
    const int tiles = tiles_x * tiles_y;
    const int f = blockIdx.x / tiles, tt = blockIdx.x - f * tiles;
    const int gx0 = (tt % tiles_x) * BT_X, gy0 = (tt / tiles_x) * BT_Y;
    const size_t N = (size_t)h * w;
    const FrameState &S = st[f];
    if (S.status != CPE_ST_OK) return;
    int half = (int)(S.r0 / 5.0);
    if (half < 3) half = 3;
    if (half > 10) half = half + 5;
    half = max(half, (int)(S.r0 / 4.5));   // the planar script's window (util_plane.py:1280)
    const int m = half + 1;
    if (gx0 > S.rect[0] + S.rect[2] + m || gx0 + BT_X < S.rect[0] - m || gy0 > S.rect[1] + S.rect[3] + m ||
        gy0 + BT_Y < S.rect[1] - m)
        return;
    blur_tile<R>(src + f * N, h, w, gx0, gy0, t, dst + f * N, reinterpret_cast<uint32_t *>(s_buf));
}

// BLUR_SPOT (19 x 19) in two steps.  k_spot_scan reads the frame once (16-byte loads, a band of BT_Y rows per workgroup) and
// flags the tiles that hold a pixel > 240; their bounding box (+ 16 px) becomes st[].srect, the window of the spot
// labelling.  k_blur19_spot (again a band per workgroup) writes zeros over every tile with no flagged tile among its 3 x 3
// neighbours -- the taps sum to 2^16, so the blur is <= the largest input of its 19 x 19 window and cannot exceed 240
// there -- and looks at the others (blur19_tile_spot).  One read and one write of the frame instead of 1.6 reads through
// LDS per tile.  The blurred plane is only ever asked `> 240` (util_cylinder.py:1958): where that cannot hold it is 0.
__global__ __launch_bounds__(256) void k_spot_scan(const uint8_t *__restrict__ gray, int h, int w, int tiles_x, int tiles_y,
                                                   FrameState *__restrict__ st, uint8_t *__restrict__ flags, size_t flag_stride)
{
    __shared__ int s_f[128];
    const int f = blockIdx.x / tiles_y, ty = blockIdx.x - f * tiles_y, tid = threadIdx.x;
    const int gy0 = ty * BT_Y, rows = min(BT_Y, h - gy0);
    if (tid < 128) s_f[tid] = 0;
    __syncthreads();
    const uint8_t *im = gray + (size_t)f * h * w + (size_t)gy0 * w;
    if ((w & 15) == 0 && (((size_t)im) & 15) == 0) {
        const int cw = w >> 4;                     // the rows of a band are contiguous: chunk i = (row i / cw, 16 columns from 16 (i % cw))
        // a byte > 240 <=> (byte + 15) carries into bit 8 of its own 9-bit field: test the two byte pairs apart
        auto gt = [](uint32_t d) { return (((d & 0x00FF00FFu) + 0x000F000Fu) | (((d >> 8) & 0x00FF00FFu) + 0x000F000Fu)) & 0x01000100u; };
        for (int i = tid; i < rows * cw; i += 256) {
            const uint4 v = reinterpret_cast<const uint4 *>(im)[i];
            if (gt(v.x) | gt(v.y) | gt(v.z) | gt(v.w)) s_f[((i % cw) * 16) / BT_X] = 1;
        }
    } else {
        for (int i = tid; i < rows * w; i += 256)
            if (im[i] > 240) s_f[(i % w) / BT_X] = 1;
    }
    __syncthreads();
    uint8_t *fl = flags + f * flag_stride + (size_t)ty * tiles_x;
    for (int tx = tid; tx < tiles_x; tx += 256) {
        fl[tx] = (uint8_t)s_f[tx];
        if (s_f[tx]) {
            FrameState &S = st[f];
            atomicMin(&S.srect[0], max(tx * BT_X - 16, 0)); atomicMin(&S.srect[1], max(gy0 - 16, 0));
            atomicMax(&S.srect[2], min(tx * BT_X + BT_X + 15, w - 1)); atomicMax(&S.srect[3], min(gy0 + BT_Y + 15, h - 1));
        }
    }
}

// One live tile of the 19 x 19 blur.  Row sums first: a thread makes 8 neighbouring sums of a row from 8 dwords of the LDS
// window (v_alignbyte_b32 picks the four bytes that start at any byte, v_dot4_u32_u8 multiplies them with four taps: 10
// instructions per sum instead of 19 byte reads and 19 multiply-adds).  The column pass is a weighted mean of row sums
// (its taps add up to 256): if no row sum of the tile's rows exceeds 240 * 256 no blurred value exceeds 240, and the tile
// keeps the zeros it already holds -- the case of nearly every live tile (the dots where two laser lines cross are > 240
// but only ~5 px wide; it takes the saturated spot to lift a 19-tap mean over 240).  Returns after the stores, no barrier.
__device__ __forceinline__ void blur19_tile_spot(const uint8_t *__restrict__ im, int h, int w, int gx0, int gy0, const Taps &t,
                                                 uint8_t *__restrict__ out, uint32_t *s_in32, uint16_t *s_h, int *s_max)
{
    constexpr int R = 9, IH = BT_Y + 2 * R, QW = (BT_X + 24) / 4;   // LDS window: columns gx0 - 12 .. gx0 + BT_X + 11 (dword aligned)
    const int tid = threadIdx.x;
    const int ax0 = gx0 - 12, ay0 = gy0 - R;
    if (tid == 0) *s_max = 0;
    if (ax0 >= 0 && ax0 + 4 * QW <= w && ay0 >= 0 && ay0 + IH <= h && (w & 3) == 0 && (((size_t)im) & 3) == 0) {
        for (int i = tid; i < IH * QW; i += 256) {
            const int ry = i / QW, q = i - ry * QW;
            s_in32[i] = *reinterpret_cast<const uint32_t *>(im + (size_t)(ay0 + ry) * w + ax0 + 4 * q);
        }
    } else {
        uint8_t *s_in8 = reinterpret_cast<uint8_t *>(s_in32);
        for (int i = tid; i < IH * QW * 4; i += 256) {
            const int ry = i / (4 * QW), b = i - ry * 4 * QW;
            s_in8[i] = im[(size_t)reflect101(ay0 + ry, h) * w + reflect101(ax0 + b, w)];
        }
    }
    __syncthreads();
    uint32_t T[5];
#pragma unroll
    for (int q = 0; q < 5; q++)
        T[q] = (uint32_t)t.k[4 * q] | ((uint32_t)t.k[4 * q + 1] << 8) | ((uint32_t)t.k[4 * q + 2] << 16) | ((q < 4 ? (uint32_t)t.k[4 * q + 3] : 0u) << 24);
    int mx = 0;
    for (int it = tid; it < IH * (BT_X / 8); it += 256) {
        const int ry = it / (BT_X / 8), c0 = (it - ry * (BT_X / 8)) * 8;
        const uint32_t *dp = s_in32 + ry * QW + (c0 >> 2);   // tile column c is window byte c + 3 .. the sum of column c0 + o reads bytes c0 + o + 3 .. + 21
        uint32_t d[8];
#pragma unroll
        for (int k = 0; k < 8; k++) d[k] = dp[k];
#pragma unroll
        for (int o = 0; o < 8; o++) {
            const int sb = o + 3, idx = sb >> 2, sh = sb & 3;
            uint32_t acc = 0;
#pragma unroll
            for (int q = 0; q < 5; q++)
                acc = __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(d[idx + q + 1], d[idx + q], sh), T[q], acc, false);
            s_h[ry * BT_X + c0 + o] = (uint16_t)acc;
            mx = max(mx, (int)acc);
        }
    }
    for (int off = 32; off >= 1; off >>= 1) mx = max(mx, __shfl_xor(mx, off, 64));
    if ((tid & 63) == 0) atomicMax(s_max, mx);
    __syncthreads();
    if (*s_max <= 240 * 256) return;               // (uniform) every blurred value of the tile is <= 240: it stays 0
    for (int i = tid; i < BT_Y * BT_X; i += 256) {
        int ry = i / BT_X, rx = i - ry * BT_X;
        const uint16_t *p = &s_h[ry * BT_X + rx];
        int sacc = 0;
#pragma unroll
        for (int j = 0; j <= 2 * R; j++) sacc += t.k[j] * (int)p[j * BT_X];
        if (gy0 + ry < h && gx0 + rx < w)
            out[(size_t)(gy0 + ry) * w + gx0 + rx] = (uint8_t)((sacc + (1 << (t.shift - 1))) >> t.shift);
    }
}

__global__ __launch_bounds__(256) void k_blur19_spot(const uint8_t *__restrict__ src, int h, int w, int tiles_x, int tiles_y, Taps t,
                                                     const uint8_t *__restrict__ flags, size_t flag_stride, uint8_t *__restrict__ dst)
{
    constexpr int R = 9, IH = BT_Y + 2 * R, QW = (BT_X + 24) / 4;
    __shared__ uint32_t s_in32[IH * QW];
    __shared__ uint16_t s_h[IH * BT_X];
    __shared__ uint8_t s_live[128];
    __shared__ int s_max;
    const int f = blockIdx.x / tiles_y, ty = blockIdx.x - f * tiles_y, tid = threadIdx.x;
    const int gy0 = ty * BT_Y, rows = min(BT_Y, h - gy0);
    const size_t N = (size_t)h * w;
    const uint8_t *fl = flags + f * flag_stride;
    for (int tx = tid; tx < tiles_x; tx += 256) {
        int any = 0;
        for (int yy = max(ty - 1, 0); yy <= min(ty + 1, tiles_y - 1); yy++)
            for (int xx = max(tx - 1, 0); xx <= min(tx + 1, tiles_x - 1); xx++) any |= fl[(size_t)yy * tiles_x + xx];
        s_live[tx] = (uint8_t)any;
    }
    // zeros over the whole band; the few tiles whose blur can exceed 240 are written again below
    uint8_t *out = dst + f * N + (size_t)gy0 * w;
    if ((w & 15) == 0 && (((size_t)out) & 15) == 0) {
        for (int i = tid; i < rows * (w >> 4); i += 256) reinterpret_cast<uint4 *>(out)[i] = make_uint4(0, 0, 0, 0);
    } else {
        for (int i = tid; i < rows * w; i += 256) out[i] = 0;
    }
    __syncthreads();                               // (waits for this wavefront's zero stores: the stores below come after them)
    for (int tx = 0; tx < tiles_x; tx++) {
        if (!s_live[tx]) continue;                 // (uniform)
        blur19_tile_spot(src + f * N, h, w, tx * BT_X, gy0, t, dst + f * N, s_in32, s_h, &s_max);
        __syncthreads();
    }
}

// ---- saturated spot -> minEnclosingCircle -> ellipse erased from a 255 plane -----------------------
__global__ __launch_bounds__(64) void k_spot_area(const uint8_t *__restrict__ g19, int h, int w,
                                                  const int *__restrict__ roots, FrameState *__restrict__ st,
                                                  unsigned long long *__restrict__ best)
{
    const int f = blockIdx.y;
    const size_t N = (size_t)h * w;
    const int ncomp = min(st[f].n_roots_s, MAXROOTS);   // (runs beside the region stage: no look at st[].status here)
    for (int k = blockIdx.x * 64 + threadIdx.x; k < ncomp; k += gridDim.x * 64) {
        const int root = roots[(size_t)f * MAXROOTS + k];
        ThreshPred nz{g19 + f * N, w, h, 240};
        StatVisitor sv;
        if (!trace_border(nz, root % w, root / w, false, sv, 8 * (w + h) + (1 << 20))) { set_overflow(st[f], OVF_TRACE); continue; }
        sv.finish();
        long long a2 = sv.a00 < 0 ? -sv.a00 : sv.a00;
        // max(contours, key=contourArea): first maximum in list order = latest discovered among equals; area 0 counts
        unsigned long long key = ((unsigned long long)(a2 + 1) << 24) | (unsigned long long)(root & 0xFFFFFF);
        atomicMax(&best[f], key);
    }
}

struct VertVisitor {
    int *v;
    int cap, n = 0;
    __device__ __forceinline__ void point(int x, int y, bool vertex)
    {
        if (!vertex) return;
        if (n < cap) { v[2 * n] = x; v[2 * n + 1] = y; }
        n++;
    }
    __device__ __forceinline__ bool stop() const { return false; }
};

__device__ __forceinline__ float normf2(float x, float y) { return (float)sqrt((double)x * x + (double)y * y); }
constexpr float MEC_EPS = 1.0e-4f;

__device__ void circle3(const float *px, const float *py, float &cx_, float &cy_, float &r_)
{
    float v1x = px[1] - px[0], v1y = py[1] - py[0];
    float v2x = px[2] - px[0], v2y = py[2] - py[0];
    float m1x = (px[0] + px[1]) / 2.0f, m1y = (py[0] + py[1]) / 2.0f;
    float c1 = m1x * v1x + m1y * v1y;
    float m2x = (px[0] + px[2]) / 2.0f, m2y = (py[0] + py[2]) / 2.0f;
    float c2 = m2x * v2x + m2y * v2y;
    float det = v1x * v2y - v1y * v2x;
    if (fabsf(det) <= MEC_EPS) {
        float d1 = (px[0] - px[1]) * (px[0] - px[1]) + (py[0] - py[1]) * (py[0] - py[1]);
        float d2 = (px[0] - px[2]) * (px[0] - px[2]) + (py[0] - py[2]) * (py[0] - py[2]);
        float d3 = (px[1] - px[2]) * (px[1] - px[2]) + (py[1] - py[2]) * (py[1] - py[2]);
        float mx = d1 > d2 ? d1 : d2;
        mx = mx > d3 ? mx : d3;
        r_ = sqrtf(mx) * 0.5f + MEC_EPS;
        if (d1 >= d2 && d1 >= d3) { cx_ = (px[0] + px[1]) * 0.5f; cy_ = (py[0] + py[1]) * 0.5f; }
        else if (d2 >= d1 && d2 >= d3) { cx_ = (px[0] + px[2]) * 0.5f; cy_ = (py[0] + py[2]) * 0.5f; }
        else { cx_ = (px[1] + px[2]) * 0.5f; cy_ = (py[1] + py[2]) * 0.5f; }
        return;
    }
    float cx = (c1 * v2y - c2 * v1y) / det;
    float cy = (v1x * c2 - v2x * c1) / det;
    cx_ = cx; cy_ = cy;
    cx -= px[0]; cy -= py[0];
    r_ = (float)sqrt((double)(cx * cx + cy * cy)) + MEC_EPS;
}

__device__ void mec_third(const int *p, int i, int j, float &cx, float &cy, float &r)
{
    cx = (float)(p[2 * j] + p[2 * i]) / 2.0f;
    cy = (float)(p[2 * j + 1] + p[2 * i + 1]) / 2.0f;
    r = normf2((float)(p[2 * j] - p[2 * i]), (float)(p[2 * j + 1] - p[2 * i + 1])) / 2.0f + MEC_EPS;
    for (int k = 0; k < j; k++) {
        float dx = cx - (float)p[2 * k], dy = cy - (float)p[2 * k + 1];
        if (normf2(dx, dy) < r) continue;
        float fx[3] = {(float)p[2 * i], (float)p[2 * j], (float)p[2 * k]};
        float fy[3] = {(float)p[2 * i + 1], (float)p[2 * j + 1], (float)p[2 * k + 1]};
        float ncx, ncy, nr = 0;
        circle3(fx, fy, ncx, ncy, nr);
        if (nr > 0) { r = nr; cx = ncx; cy = ncy; }
    }
}
__device__ void mec_second(const int *p, int i, float &cx, float &cy, float &r)
{
    cx = (float)(p[0] + p[2 * i]) / 2.0f;
    cy = (float)(p[1] + p[2 * i + 1]) / 2.0f;
    r = normf2((float)(p[0] - p[2 * i]), (float)(p[1] - p[2 * i + 1])) / 2.0f + MEC_EPS;
    for (int j = 1; j < i; j++) {
        float dx = cx - (float)p[2 * j], dy = cy - (float)p[2 * j + 1];
        if (normf2(dx, dy) < r) continue;
        float ncx, ncy, nr = 0;
        mec_third(p, i, j, ncx, ncy, nr);
        if (nr > 0) { r = nr; cx = ncx; cy = ncy; }
    }
}
__device__ void min_enclosing_circle(const int *p, int n, float &cx, float &cy, float &r)
{
    cx = cy = r = 0;
    if (n == 0) return;
    if (n == 1) { cx = (float)p[0]; cy = (float)p[1]; r = MEC_EPS; return; }
    if (n == 2) {
        cx = ((float)p[0] + (float)p[2]) / 2.0f;
        cy = ((float)p[1] + (float)p[3]) / 2.0f;
        double dx = p[0] - p[2], dy = p[1] - p[3];
        r = (float)(sqrt(dx * dx + dy * dy) / 2.0) + MEC_EPS;
        return;
    }
    cx = (float)(p[0] + p[2]) / 2.0f;
    cy = (float)(p[1] + p[3]) / 2.0f;
    r = normf2((float)(p[0] - p[2]), (float)(p[1] - p[3])) / 2.0f + MEC_EPS;
    for (int i = 2; i < n; i++) {
        float dx = (float)p[2 * i] - cx, dy = (float)p[2 * i + 1] - cy;
        float d = normf2(dx, dy);
        if (d < r) continue;
        float ncx, ncy, nr = 0;
        mec_second(p, i, ncx, ncy, nr);
        if (nr > 0) { r = nr; cx = ncx; cy = ncy; }
    }
}

constexpr int XY_SHIFT = 16;
constexpr int XY_ONE = 1 << XY_SHIFT;

__device__ __forceinline__ void putz(uint8_t *img, int h, int w, int x, int y)
{
    if (x >= 0 && x < w && y >= 0 && y < h) img[(size_t)y * w + x] = 0;
}

__device__ void line2z(uint8_t *img, int h, int w, long long p1x, long long p1y, long long p2x, long long p2y)
{
    long long dx = p2x - p1x, dy = p2y - p1y;
    long long j = dx < 0 ? -1 : 0, ax = (dx ^ j) - j;
    long long i = dy < 0 ? -1 : 0, ay = (dy ^ i) - i;
    long long x_step, y_step;
    int ecount;
    if (ax > ay) {
        dy = (dy ^ j) - j;
        p1x ^= p2x & j; p2x ^= p1x & j; p1x ^= p2x & j;
        p1y ^= p2y & j; p2y ^= p1y & j; p1y ^= p2y & j;
        x_step = XY_ONE;
        y_step = dy * (1 << XY_SHIFT) / (ax | 1);
        ecount = (int)((p2x - p1x) >> XY_SHIFT);
    } else {
        dx = (dx ^ i) - i;
        p1x ^= p2x & i; p2x ^= p1x & i; p1x ^= p2x & i;
        p1y ^= p2y & i; p2y ^= p1y & i; p1y ^= p2y & i;
        x_step = dx * (1 << XY_SHIFT) / (ay | 1);
        y_step = XY_ONE;
        ecount = (int)((p2y - p1y) >> XY_SHIFT);
    }
    (void)x_step; (void)y_step;
    p1x += (XY_ONE >> 1);
    p1y += (XY_ONE >> 1);
    putz(img, h, w, (int)((p2x + (XY_ONE >> 1)) >> XY_SHIFT), (int)((p2y + (XY_ONE >> 1)) >> XY_SHIFT));
    if (ax > ay) {
        p1x >>= XY_SHIFT;
        while (ecount >= 0) {
            putz(img, h, w, (int)p1x, (int)(p1y >> XY_SHIFT));
            p1x++;
            p1y += y_step;
            ecount--;
        }
    } else {
        p1y >>= XY_SHIFT;
        while (ecount >= 0) {
            putz(img, h, w, (int)(p1x >> XY_SHIFT), (int)p1y);
            p1x += x_step;
            p1y++;
            ecount--;
        }
    }
}

// FillConvexPoly(shift = 16, colour 0), the scan-line half: sink(y, x1, x2) receives every row span (x1 <= x2, clipped to
// the image) in order of y.  OpenCV also draws the polygon's edges (Line2 from vertex to vertex): poly_edges_z below.
template <class Sink>
__device__ void convex_poly_rows(int h, int w, const long long *vx, const long long *vy, int npts, Sink sink)
{
    const int shift = XY_SHIFT;
    struct { int idx, di; long long x, dx; int ye; } edge[2];
    int delta = 1 << shift >> 1;
    int i, y, imin = 0, edges = npts;
    long long xmin, xmax, ymin, ymax;
    const int delta1 = XY_ONE >> 1, delta2 = XY_ONE >> 1;
    xmin = xmax = vx[0];
    ymin = ymax = vy[0];
    for (i = 0; i < npts; i++) {
        long long px = vx[i], py = vy[i];
        if (py < ymin) { ymin = py; imin = i; }
        if (py > ymax) ymax = py;
        if (px > xmax) xmax = px;
        if (px < xmin) xmin = px;
    }
    xmin = (xmin + delta) >> shift;
    xmax = (xmax + delta) >> shift;
    ymin = (ymin + delta) >> shift;
    ymax = (ymax + delta) >> shift;
    if (npts < 3 || (int)xmax < 0 || (int)ymax < 0 || (int)xmin >= w || (int)ymin >= h) return;
    if (ymax > h - 1) ymax = h - 1;
    edge[0].idx = edge[1].idx = imin;
    edge[0].ye = edge[1].ye = y = (int)ymin;
    edge[0].di = 1;
    edge[1].di = npts - 1;
    edge[0].x = edge[1].x = -XY_ONE;
    edge[0].dx = edge[1].dx = 0;
    do {
        for (i = 0; i < 2; i++) {
            if (y >= edge[i].ye) {
                int idx0 = edge[i].idx, di = edge[i].di;
                int idx = idx0 + di;
                if (idx >= npts) idx -= npts;
                int ty = 0;
                for (; edges-- > 0;) {
                    ty = (int)((vy[idx] + delta) >> shift);
                    if (ty > y) {
                        long long xs = vx[idx0], xe = vx[idx];
                        edge[i].ye = ty;
                        edge[i].dx = ((xe - xs) * 2 + (ty - y)) / (2 * (ty - y));
                        edge[i].x = xs;
                        edge[i].idx = idx;
                        break;
                    }
                    idx0 = idx;
                    idx += di;
                    if (idx >= npts) idx -= npts;
                }
            }
        }
        if (edges < 0) break;
        if (y >= 0) {
            int left = 0, right = 1;
            if (edge[0].x > edge[1].x) { left = 1; right = 0; }
            int xx1 = (int)((edge[left].x + delta1) >> XY_SHIFT);
            int xx2 = (int)((edge[right].x + delta2) >> XY_SHIFT);
            if (xx2 >= 0 && xx1 < w) {
                if (xx1 < 0) xx1 = 0;
                if (xx2 >= w) xx2 = w - 1;
                sink(y, xx1, xx2);
            }
        }
        edge[0].x += edge[0].dx;
        edge[1].x += edge[1].dx;
    } while (++y <= (int)ymax);
}

// cv2.circle(img, (cx, cy), radius, 0, thickness=-1): the midpoint spans of OpenCV's Circle() (as in k_discs)
__device__ void circle_fill_z(uint8_t *im, int h, int w, int cx, int cy, int radius)
{
    int err = 0, dx = radius, dy = 0, plus = 1, minus = (radius << 1) - 1;
    while (dx >= dy) {
        int ys[4] = {cy - dy, cy + dy, cy - dx, cy + dx};
        int xa[4] = {cx - dx, cx - dx, cx - dy, cx - dy};
        int xb[4] = {cx + dx, cx + dx, cx + dy, cx + dy};
        for (int q = 0; q < 4; q++) {
            if (ys[q] < 0 || ys[q] >= h) continue;
            int x1 = max(xa[q], 0), x2 = min(xb[q], w - 1);
            for (int x = x1; x <= x2; x++) im[(size_t)ys[q] * w + x] = 0;
        }
        dy++;
        err += plus;
        plus += 2;
        int mask = (err <= 0) - 1;
        err -= minus & mask;
        dx += mask;
        minus -= mask & 2;
    }
}

// cv2.ellipse(img, (cx, cy), (a, b), 0, 0, 360, 0, -1): ellipse2Poly with the angle step OpenCV derives from the axes
// (at most 360 / 5 + 2 vertices), rounded to 16 fractional bits as EllipseEx does; the polygon is then filled
constexpr int ELL_MAXV = 80;
__device__ int ellipse_vertices(int cx, int cy, int a, int b, long long *vx, long long *vy)
{
    long long ccx = (long long)cx << XY_SHIFT, ccy = (long long)cy << XY_SHIFT;
    long long aw = llabs((long long)a << XY_SHIFT), ah = llabs((long long)b << XY_SHIFT);
    int delta = (int)(((aw > ah ? aw : ah) + (XY_ONE >> 1)) >> XY_SHIFT);
    delta = delta < 3 ? 90 : delta < 10 ? 30 : delta < 15 ? 18 : 5;
    int nv = 0;
    long long prevx = -1, prevy = -1;
    bool have_prev = false;
    for (int i = 0; i < 360 + delta; i += delta) {
        int ang = i > 360 ? 360 : i;
        double sx = (double)(float)sin((450 - ang) * 0.017453292519943295769236907684886);
        double sy = (double)(float)sin(ang * 0.017453292519943295769236907684886);
        if ((450 - ang) % 90 == 0) { int q = ((450 - ang) / 90) % 4; sx = q == 0 ? 0 : q == 1 ? 1 : q == 2 ? 0 : -1; }
        if (ang % 90 == 0) { int q = (ang / 90) % 4; sy = q == 0 ? 0 : q == 1 ? 1 : q == 2 ? 0 : -1; }
        double x = (double)aw * sx, y = (double)ah * sy;
        double ptx = (double)ccx + x, pty = (double)ccy + y;
        long long qx = (long long)(int)rint(ptx / XY_ONE) << XY_SHIFT, qy = (long long)(int)rint(pty / XY_ONE) << XY_SHIFT;
        qx += (int)rint(ptx - (double)qx);
        qy += (int)rint(pty - (double)qy);
        if (!have_prev || qx != prevx || qy != prevy) {
            vx[nv] = qx; vy[nv] = qy; nv++;
            prevx = qx; prevy = qy; have_prev = true;
        }
    }
    if (nv == 1) { vx[0] = vx[1] = ccx; vy[0] = vy[1] = ccy; nv = 2; }
    return nv;
}

// one wavefront per frame: contour of the largest saturated blob -> circle -> ellipse erased from cm (pre-set to 255).
// Lane 0 follows the border, runs minEnclosingCircle and makes the ellipse's vertices and row spans (a few hundred
// sequential steps, all in LDS: no per-lane scratch); the pixels -- the polygon's edges, one lane per edge, and its rows,
// 64 pixels per store -- are written by the whole wavefront.
constexpr int SPOT_ROWS = 1024;   // row spans kept in LDS; a taller ellipse is filled by lane 0 alone
__global__ __launch_bounds__(64) void k_spot_ellipse(const uint8_t *__restrict__ g19, int n, int h, int w,
                                                     const unsigned long long *__restrict__ best, FrameState *__restrict__ st,
                                                     int *__restrict__ verts /* n*MAXV*2 */, uint8_t *__restrict__ cm, int planar)
{
    const int f = blockIdx.x, lane = threadIdx.x;
    FrameState &S = st[f];
    __shared__ long long s_vx[ELL_MAXV], s_vy[ELL_MAXV];
    __shared__ int s_nv, s_rows, s_y0;
    __shared__ int2 s_span[SPOT_ROWS];
    const size_t N = (size_t)h * w;
    uint8_t *img = cm + f * N;
    if (lane == 0) {
        s_nv = 0; s_rows = 0; s_y0 = 0;
        if (best[f] == 0) S.spot_fail = 1;
        else {
            const int root = (int)(best[f] & 0xFFFFFF);
            ThreshPred nz{g19 + f * N, w, h, 240};
            VertVisitor vv{verts + (size_t)f * MAXV * 2, MAXV};
            trace_border(nz, root % w, root / w, false, vv, 8 * (w + h) + (1 << 20));
            if (vv.n > MAXV) { set_overflow(S, OVF_VERTS); vv.n = MAXV; }
            float cx, cy, rad;
            min_enclosing_circle(vv.v, vv.n, cx, cy, rad);
            int icx = (int)cx, icy = (int)cy;
            int cr0 = (int)rad;
            int cr = rad < 30 ? cr0 + 20 : cr0 + 5;
            int minor = cr + 20 > 1 ? cr + 20 : 1;
            int a = (int)rint((cr + 40) / 2.0), b = (int)rint(minor / 2.0);
            if (planar) { a = cr0; b = cr0; circle_fill_z(img, h, w, icx, icy, cr0); }   // util_plane.py:2733-2792: plain circle
            else {
                const int nv = ellipse_vertices(icx, icy, a, b, s_vx, s_vy);
                s_nv = nv;
                int rows = 0, y0 = 0;
                convex_poly_rows(h, w, s_vx, s_vy, nv, [&](int y, int x1, int x2) {
                    if (rows == 0) y0 = y;
                    if (rows < SPOT_ROWS) s_span[rows] = make_int2(x1, x2);
                    else for (int x = x1; x <= x2; x++) img[(size_t)y * w + x] = 0;
                    rows++;
                });
                s_rows = rows < SPOT_ROWS ? rows : SPOT_ROWS; s_y0 = y0;
            }
            S.r0 = cr0;
            S.spot[0] = icx; S.spot[1] = icy; S.spot[2] = a; S.spot[3] = b;
        }
    }
    __syncthreads();
    const int nv = s_nv;
    for (int e = lane; e < nv; e += 64) {          // FillConvexPoly draws every edge (vertex e-1 -> vertex e) with Line2
        const int p = e == 0 ? nv - 1 : e - 1;
        line2z(img, h, w, s_vx[p], s_vy[p], s_vx[e], s_vy[e]);
    }
    const int rows = s_rows, y0 = s_y0;
    for (int r = 0; r < rows; r++) {
        const int2 sp = s_span[r];
        uint8_t *rowp = img + (size_t)(y0 + r) * w;
        for (int x = sp.x + lane; x <= sp.y; x += 64) rowp[x] = 0;
    }
}

// ---- line-fragment expansion ------------------------------------------------------------------------

__device__ __forceinline__ double sign1(double a, double b) { return b >= 0 ? fabs(a) : -fabs(a); }

// numpy.linalg.eig of a symmetric 2x2 as LAPACK dgeev (dlanv2) orders and signs it
__device__ void eig2_lapack(double a, double b, double c, double d, double *w, double *V)
{
    double cs, sn;
    if (c == 0) {
        cs = 1; sn = 0;
    } else if (b == 0) {
        cs = 0; sn = 1;
        double t = d; d = a; a = t; b = -c; c = 0;
    } else if ((a - d) == 0 && sign1(1, b) != sign1(1, c)) {
        cs = 1; sn = 0;
    } else {
        double temp = a - d, p = 0.5 * temp;
        double bcmax = fmax(fabs(b), fabs(c));
        double bcmis = fmin(fabs(b), fabs(c)) * sign1(1, b) * sign1(1, c);
        double scale = fmax(fabs(p), bcmax);
        double z = (p / scale) * p + (bcmax / scale) * bcmis;
        if (z >= 4.0 * 2.220446049250313e-16) {
            z = p + sign1(sqrt(scale) * sqrt(z), p);
            a = d + z;
            d = d - (bcmax / z) * bcmis;
            double tau = hypot(c, z);
            cs = z / tau;
            sn = c / tau;
            b = b - c;
            c = 0;
        } else {
            double sigma = b + c;
            double tau = hypot(sigma, temp);
            cs = sqrt(0.5 * (1 + fabs(sigma) / tau));
            sn = -(p / (tau * cs)) * sign1(1, sigma);
            double aa = a * cs + b * sn, bb = -a * sn + b * cs, cc = c * cs + d * sn, dd = -c * sn + d * cs;
            a = aa * cs + cc * sn; b = bb * cs + dd * sn; c = -aa * sn + cc * cs; d = -bb * sn + dd * cs;
            temp = 0.5 * (a + d);
            a = temp; d = temp;
        }
    }
    w[0] = a; w[1] = d;
    double v1x = cs, v1y = sn;
    double x0 = (a != d) ? -b / (a - d) : 0.0, x1 = 1.0;
    double v2x = cs * x0 - sn * x1, v2y = sn * x0 + cs * x1;
    double n2 = sqrt(v2x * v2x + v2y * v2y);
    v2x /= n2; v2y /= n2;
    V[0] = v1x; V[1] = v2x; V[2] = v1y; V[3] = v2y;
}

struct SegVisitor {
    float *pts;  // maxv x 2
    int maxv;
    int n = 0;
    __device__ __forceinline__ void point(int x, int y, bool vertex)
    {
        if (!vertex) return;
        if (n < maxv) { pts[2 * n] = (float)x; pts[2 * n + 1] = (float)y; }
        n++;
    }
    // expand_line_roi skips contours with more than max_pixels vertices (util_cylinder.py:169): no need to finish those
    __device__ __forceinline__ bool stop() const { return n > maxv; }
};

// one thread per fragment: CHAIN_APPROX_SIMPLE vertices (MINV..MAXVS: 5..200 for the cylinder script, 8..700 for the planar
// one, expand_line_roi's min_pixels / max_pixels) -> PCA end points, angle, length
constexpr int SEG_LPW = 4;
template <int MINV, int MAXVS>
__global__ __launch_bounds__(64) void k_seg_trace(const uint32_t *__restrict__ base_bits, int h, int w, int which,
                                                  const int *__restrict__ roots, RootList list, FrameState *__restrict__ st,
                                                  SegRec *__restrict__ segs /* n*MAXSEG */,
                                                  const unsigned long long *__restrict__ outside, size_t plane_words)
{
    const int f = blockIdx.y;
    if (st[f].status != CPE_ST_OK) return;
    __shared__ unsigned long long s_win[BW_ROWS * SEG_LPW];   // windows for the lanes that trace only
    __shared__ float s_pts[SEG_LPW][2 * MAXVS];
    const int ncomp = min(*root_counter(st[f], list), MAXROOTS);
    // Few, long borders: a wavefront steps at the pace of its slowest lane, and with 64 borders in flight nearly every
    // step waits for some lane's window refill (one memory round trip).  SEG_LPW borders per wavefront keep most steps
    // LDS-only; the other lanes idle.
    if (threadIdx.x >= SEG_LPW) return;
    for (int k = blockIdx.x * SEG_LPW + threadIdx.x; k < ncomp; k += gridDim.x * SEG_LPW) {
    const int root = roots[(size_t)f * MAXROOTS + k];
    if (!comp_is_external(outside + f * plane_words, w, root, window_rect(st, f, WIN_REGION, h, w).x0)) continue;   // RETR_EXTERNAL (:161)
    BitWin<SEG_LPW> nz{bit_plane(base_bits, f, h, w), w, h, s_win + threadIdx.x};
    float *pts = s_pts[threadIdx.x];     // the border's vertices live in LDS: 1.6 KB (5.6 KB planar) per lane were scratch
    SegVisitor sv{pts, MAXVS};
    if (!trace_border(nz, root % w, root / w, false, sv, 8 * (w + h) + (1 << 20))) { set_overflow(st[f], OVF_TRACE); continue; }
    const int n = sv.n;
    if (n < MINV || n > MAXVS) continue;
    // get_pca_endpoints
    float mx = 0, my = 0;
    for (int i = 0; i < n; i++) { mx += pts[2 * i]; my += pts[2 * i + 1]; }
    mx = mx / (float)n; my = my / (float)n;
    double ax = 0, ay = 0;
    for (int i = 0; i < n; i++) { ax += (double)(pts[2 * i] - mx); ay += (double)(pts[2 * i + 1] - my); }
    ax /= n; ay /= n;
    double sxx = 0, sxy = 0, syy = 0;
    for (int i = 0; i < n; i++) {
        double dx = (double)(pts[2 * i] - mx) - ax, dy = (double)(pts[2 * i + 1] - my) - ay;
        sxx += dx * dx; sxy += dx * dy; syy += dy * dy;
    }
    double fct = 1.0 / (n - 1);
    sxx *= fct; sxy *= fct; syy *= fct;
    double wv[2], V[4];
    eig2_lapack(sxx, sxy, sxy, syy, wv, V);
    int kk = wv[1] > wv[0] ? 1 : 0;
    double ux = V[0 + kk], uy = V[2 + kk];
    int imin = 0, imax = 0;
    double pmin = 0, pmax = 0;
    for (int i = 0; i < n; i++) {
        double pr = (double)(pts[2 * i] - mx) * ux + (double)(pts[2 * i + 1] - my) * uy;
        if (i == 0 || pr < pmin) { pmin = pr; imin = i; }
        if (i == 0 || pr > pmax) { pmax = pr; imax = i; }
    }
    float p1x = pts[2 * imin], p1y = pts[2 * imin + 1], p2x = pts[2 * imax], p2y = pts[2 * imax + 1];
    float dx = p2x - p1x, dy = p2y - p1y;
    float length = (float)hypot((double)dx, (double)dy);
    if (length < 1e-8) continue;
    float at = (float)atan2((double)dy, (double)dx);
    float deg = at * (float)(180.0 / 3.14159265358979323846);
    int q = atomicAdd(&st[f].n_seg[which], 1);
    if (q >= MAXSEG) { set_overflow(st[f], OVF_SEGS); continue; }
    SegRec &r = segs[(size_t)f * MAXSEG + q];
    r.p1x = p1x; r.p1y = p1y; r.p2x = p2x; r.p2y = p2y; r.angle = -deg; r.len = length; r.valid = 1;
    }
}

// median angle (np.median of float32) and maximum length per frame
__global__ __launch_bounds__(256) void k_seg_global(FrameState *__restrict__ st, int which, const SegRec *__restrict__ segs)
{
    const int f = blockIdx.x, t = threadIdx.x;
    __shared__ float s_lo, s_hi;
    __shared__ unsigned int s_len;
    const int nv = min(st[f].n_seg[which], MAXSEG);
    const SegRec *S = segs + (size_t)f * MAXSEG;
    if (t == 0) { s_lo = 0; s_hi = 0; s_len = 0; }
    __syncthreads();
    const int k_hi = nv / 2, k_lo = (nv & 1) ? nv / 2 : nv / 2 - 1;
    for (int i = t; i < nv; i += 256) {
        float ai = S[i].angle;
        int rank = 0;
        for (int j = 0; j < nv; j++) {
            float aj = S[j].angle;
            rank += (aj < ai || (aj == ai && j < i)) ? 1 : 0;
        }
        if (rank == k_lo) s_lo = ai;
        if (rank == k_hi) s_hi = ai;
        atomicMax(&s_len, __float_as_uint(S[i].len));  // lengths are positive: uint order == float order
    }
    __syncthreads();
    if (t == 0) {
        st[f].gang[which] = (nv & 1) ? s_hi : (float)(((double)s_lo + (double)s_hi) / 2.0);
        st[f].glen[which] = __uint_as_float(s_len);
    }
}

// one workgroup per fragment: the 15x15 patch of the mask around each end point (read from base's one-bit plane) dilated by
// the rotated line kernel (reflected, as cv2.dilate does), eroded 3x3.  exp holds base & mask_contour already (k_roi_base);
// every pixel the erosion keeps is stored as 255 & mask_contour where that is not zero -- ((expansion | base) ? 255 : 0) &
// mask_contour without a plane in between.  Workgroups whose supports overlap store the same value to the same byte: no
// read-modify-write.
// The line kernel is built once per fragment: warpAffine's X0 / Y0 per row and adelta / bdelta per column go into tables
// (4 ks f64 evaluations), the ks^2 membership test is integer only.  The support of an end point -- (15 + ks + 2)^2 with a
// 1-px margin for the erosion -- lives in LDS as rows of EXP_WW 64-pixel words, bit 0 = column bx1: the dilation ORs a patch
// row's 15 bits, shifted, into one or two words per kernel offset, the erosion is shifts and ANDs of three rows.
constexpr int EXP_MAXKS = 176;       // cylinder script: kernel 91 + r0
constexpr int EXP_MAXKS_PLANE = 208;  // planar script: fixed 201
constexpr int EXP_NT = 256, EXP_WW = 4, EXP_MAXOFF = 4096;
template <int MAXKS>
__global__ __launch_bounds__(EXP_NT) void k_seg_expand(const uint32_t *__restrict__ base_bits, const uint8_t *__restrict__ mc, int h, int w,
                                                       int which, FrameState *__restrict__ st, const SegRec *__restrict__ segs,
                                                       uint8_t *__restrict__ exp, int fixed_ks)
{
    constexpr int EXP_REG = 15 + MAXKS + 2;
    static_assert(EXP_REG <= 64 * EXP_WW, "a support row must fit EXP_WW words");
    __shared__ unsigned long long dil[EXP_REG * EXP_WW];
    __shared__ short koff[EXP_MAXOFF][2];
    __shared__ int tX0[MAXKS], tY0[MAXKS], tA[MAXKS], tB[MAXKS];
    __shared__ unsigned long long vc[EXP_WW];     // the support's columns that lie inside the image
    __shared__ unsigned prow[15];                 // the patch, one 15-bit row each (bit 0 = column x1)
    __shared__ int s_nk;
    const int f = blockIdx.y, t = threadIdx.x;
    FrameState &S = st[f];
    if (S.status != CPE_ST_OK) return;
    const int nseg = min(S.n_seg[which], MAXSEG);
    const size_t N = (size_t)h * w;
    const unsigned long long *bp = bit_plane(base_bits, f, h, w);
    const int btc = bit_tile_cols(w);
    const uint8_t *mcf = mc + f * N;
    uint8_t *ex = exp + f * N;
    for (int seg = blockIdx.x; seg < nseg; seg += gridDim.x) {   // fragments in turns
    const SegRec r = segs[(size_t)f * MAXSEG + seg];
    const float glen = S.glen[which], gang = S.gang[which];
    if ((double)r.len > 0.8 * (double)glen) continue;
    const int ks = fixed_ks > 0 ? fixed_ks : 91 + S.r0;
    if (ks > MAXKS) { if (t == 0) set_overflow(S, OVF_KERNEL); return; }
    __syncthreads();   // the previous fragment's readers of the tables, koff and dil are done
    const float ak = fabsf(r.angle - gang) > 5.0f ? gang : r.angle;
    const int a = ks / 2, half = 7;
    if (t == 0) s_nk = 0;
    // rotated line kernel: getRotationMatrix2D + warpAffine(INTER_NEAREST) of the centre row
    const int c = ks / 2;
    {
        double ar = (double)ak * 3.1415926535897932384626433832795 / 180.0;
        double alpha = cos(ar), beta = sin(ar);
        double M[6] = {alpha, beta, (1 - alpha) * c - beta * c, -beta, alpha, beta * c + (1 - alpha) * c};
        double D = M[0] * M[4] - M[1] * M[3];
        D = D != 0 ? 1. / D : 0;
        double A11 = M[4] * D, A22 = M[0] * D;
        double iM[6];
        iM[0] = A11; iM[1] = M[1] * (-D); iM[3] = M[3] * (-D); iM[4] = A22;
        double b1 = -iM[0] * M[2] - iM[1] * M[5];
        double b2 = -iM[3] * M[2] - iM[4] * M[5];
        iM[2] = b1; iM[5] = b2;
        for (int i = t; i < ks; i += EXP_NT) {      // i: a row y for X0 / Y0, a column x for adelta / bdelta
            tX0[i] = (int)rint((iM[1] * i + iM[2]) * 1024) + 512;
            tY0[i] = (int)rint((iM[4] * i + iM[5]) * 1024) + 512;
            tA[i] = (int)rint(iM[0] * i * 1024);
            tB[i] = (int)rint(iM[3] * i * 1024);
        }
    }
    __syncthreads();
    for (int y = t >> 6; y < ks; y += EXP_NT / 64) {
        const int X0 = tX0[y], Y0 = tY0[y];
        for (int x = t & 63; x < ks; x += 64) {
            const int X = (X0 + tA[x]) >> 10, Y = (Y0 + tB[x]) >> 10;
            if (X >= 0 && X < ks && Y == c) {
                int q = atomicAdd(&s_nk, 1);
                if (q < EXP_MAXOFF) { koff[q][0] = (short)(x - a); koff[q][1] = (short)(y - a); }
            }
        }
    }
    __syncthreads();
    const int nk = min(s_nk, EXP_MAXOFF);
    if (s_nk > EXP_MAXOFF && t == 0) set_overflow(S, OVF_EXPAND);
    for (int e = 0; e < 2; e++) {   // the fragment's two end points
    const int cx = (int)rint((double)(e ? r.p2x : r.p1x)), cy = (int)rint((double)(e ? r.p2y : r.p1y));
    const int x1 = max(cx - half, 0), x2 = min(cx + half + 1, w), y1 = max(cy - half, 0), y2 = min(cy + half + 1, h);
    if (x2 <= x1 || y2 <= y1) continue;      // no patch
    // support box (global coords) with a 1-px margin for the erosion: the dilation sets local columns 1 .. bw - 2 and rows
    // 1 .. bh - 2 only, so a margin pixel never survives the erosion and nothing outside the box is ever asked for
    const int bx1 = x1 - a - 1, by1 = y1 - a - 1;
    const int bh = (y2 - y1) + 2 * a + 2;
    if (e) __syncthreads();   // the first end point's readers of dil / prow / vc are done
    for (int i = t; i < bh * EXP_WW; i += EXP_NT) dil[i] = 0ull;
    if (t < 15) {
        const int y = y1 + t;
        unsigned m = 0u;
        if (y < y2) {
            const int j = x1 >> 6, sh = x1 & 63;
            unsigned long long v = bp[bit_word(btc, y, j)] >> sh;
            if (sh) v |= bp[bit_word(btc, y, j + 1)] << (64 - sh);      // j + 1 may be the plane's zero column
            m = (unsigned)v & ((1u << (x2 - x1)) - 1u);
        }
        prow[t] = m;
    } else if (t >= 16 && t < 16 + EXP_WW) {
        const int wd = t - 16;
        const int lo = min(max(-bx1 - 64 * wd, 0), 64), hi = min(max(w - bx1 - 64 * wd, 0), 64);   // bits [lo, hi) of the word
        unsigned long long v = 0ull;
        if (hi > lo) v = (hi == 64 ? ~0ull : ((1ull << hi) - 1ull)) & ~((1ull << lo) - 1ull);
        vc[wd] = v;
    }
    __syncthreads();
    // dilation: pixel p - k for every patch pixel p and kernel offset k, inside the image
    for (int i = t; i < nk * 15; i += EXP_NT) {
        const int k = i / 15, pr = i - k * 15;
        const unsigned long long m = prow[pr];
        const int yy = y1 + pr - koff[k][1];
        if (!m || yy < 0 || yy >= h) continue;
        const int sh = a + 1 - koff[k][0];            // local column of the patch's first one: 1 .. 2 a + 1
        const int wd = sh >> 6, b = sh & 63;
        unsigned long long *row = dil + (yy - by1) * EXP_WW;
        const unsigned long long lo = (m << b) & vc[wd];
        if (lo) atomicOr(&row[wd], lo);
        if (b > 49) {
            const unsigned long long hi = (m >> (64 - b)) & vc[wd + 1];
            if (hi) atomicOr(&row[wd + 1], hi);
        }
    }
    __syncthreads();
    // 3x3 erosion on words, 16 pixels per step: a neighbour outside the image is the neutral element (cv2.erode)
    for (int i = t; i < (bh - 2) * EXP_WW * 4; i += EXP_NT) {
        const int ly = 1 + (i >> 4), wd = (i >> 2) & 3, off = (i & 3) * 16;
        const int gy = by1 + ly;
        if (gy < 0 || gy >= h || !((dil[ly * EXP_WW + wd] >> off) & 0xffffull)) continue;
        unsigned long long acc = vc[wd];
#pragma unroll
        for (int dr = -1; dr <= 1; dr++) {
            if (gy + dr < 0 || gy + dr >= h) continue;
            const unsigned long long *row = dil + (ly + dr) * EXP_WW;
            const unsigned long long xb = row[wd] | ~vc[wd];
            const unsigned long long xa = wd > 0 ? (row[wd - 1] | ~vc[wd - 1]) : 0ull;             // local column -1: only beside the margin
            const unsigned long long xc = wd + 1 < EXP_WW ? (row[wd + 1] | ~vc[wd + 1]) : 0ull;   // column 256: never reached
            acc &= xb & ((xb >> 1) | (xc << 63)) & ((xb << 1) | (xa >> 63));
        }
        unsigned bits = (unsigned)(acc >> off) & 0xffffu;
        const size_t o = (size_t)gy * w + (bx1 + wd * 64 + off);
        while (bits) {
            const int b = __ffs(bits) - 1;
            bits &= bits - 1u;
            const uint8_t cv = mcf[o + b];
            if (cv) ex[o + b] = 255 & cv;
        }
    }
    }
    }
}

// the three chains meet: the region stage's verdict comes first (a frame without a region never looked for its spot
// in the sequential order: mask_roi_around_center is not reached, util_cylinder.py:1900 raises before)
__global__ void k_masks_reset(FrameState *st, int n)
{
    int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n) return;
    FrameState &S = st[f];
    S.n_joints = 0; S.n_joints_all = 0; S.n_seg[0] = 0; S.n_seg[1] = 0;
    S.gang[0] = S.gang[1] = 0; S.glen[0] = S.glen[1] = 0;
    if (S.status == CPE_ST_NO_REGION) { S.r0 = 0; S.spot[0] = S.spot[1] = S.spot[2] = S.spot[3] = 0; }
    else if (S.status == CPE_ST_OK && S.spot_fail) S.status = CPE_ST_NO_SPOT;
}

inline unsigned grid1(size_t total) { return (unsigned)((total + 255) / 256); }

// true: every reader of the joints mask takes its one-bit plane (ccl_components, outside_flood, the centroid tracer), so the
// buffer of its bytes is free and holds hmask and vmask as one-bit planes for k_roi_base: n frames of hmask, then n of vmask
inline bool line_masks_as_bits(const MaskBuffers &B, int w) { return ccl_components_reads_bits(B.jbits, w, B.lab_p); }
inline unsigned long long *line_mask_bits(const MaskBuffers &B, int which, int n, int h, int w)
{
    return reinterpret_cast<unsigned long long *>(B.joints_mask) + (size_t)which * n * bit_plane_words(h, w);
}

}  // namespace


// cv2.GaussianBlur(img,(7,7),0) for indexing_data (util_cylinder.py:1433)
// indexing_data on a colour frame (util_cylinder.py:1433-1435): cv2.GaussianBlur(img, (7, 7), 0) channel by channel, then
// cv2.cvtColor(BGR2GRAY) of the blurred image.  Same tiles and the same skip rule as the grey blur; bgr: u8[n,h,w,3].
__global__ __launch_bounds__(256) void k_blur7_bgr(const uint8_t *__restrict__ bgr, int h, int w, int tiles_x, int tiles_y, Taps t,
                                                   const FrameState *__restrict__ st, uint8_t *__restrict__ dst)
{
    constexpr int R = 3, IW = BT_X + 2 * R, IH = BT_Y + 2 * R, PER = BT_X * BT_Y / 256;
    __shared__ uint8_t s_in[IH * IW];
    __shared__ uint16_t s_h[IH * BT_X];
    const int tid = threadIdx.x;
    const int tiles = tiles_x * tiles_y;
    const int f = blockIdx.x / tiles, tt = blockIdx.x - f * tiles;
    const int gx0 = (tt % tiles_x) * BT_X, gy0 = (tt / tiles_x) * BT_Y;
    const size_t N = (size_t)h * w;
    const FrameState &S = st[f];
    if (S.status != CPE_ST_OK) return;
    int half = (int)(S.r0 / 5.0);
    if (half < 3) half = 3;
    if (half > 10) half = half + 5;
    half = max(half, (int)(S.r0 / 4.5));
    const int m = half + 1;
    if (gx0 > S.rect[0] + S.rect[2] + m || gx0 + BT_X < S.rect[0] - m || gy0 > S.rect[1] + S.rect[3] + m || gy0 + BT_Y < S.rect[1] - m)
        return;
    const uint8_t *im = bgr + f * N * 3;
    uint32_t ch[PER][3];
    for (int c = 0; c < 3; c++) {
        for (int i = tid; i < IH * IW; i += 256) {
            int ry = i / IW, rx = i - ry * IW;
            s_in[i] = im[((size_t)reflect101(gy0 - R + ry, h) * w + reflect101(gx0 - R + rx, w)) * 3 + c];
        }
        __syncthreads();
        for (int i = tid; i < IH * BT_X; i += 256) {
            int ry = i / BT_X, rx = i - ry * BT_X;
            const uint8_t *p = &s_in[ry * IW + rx];
            int sacc = 0;
#pragma unroll
            for (int j = 0; j <= 2 * R; j++) sacc += t.k[j] * p[j];
            s_h[i] = (uint16_t)sacc;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < PER; q++) {
            const int i = tid + q * 256;
            int ry = i / BT_X, rx = i - ry * BT_X;
            const uint16_t *p = &s_h[ry * BT_X + rx];
            int sacc = 0;
#pragma unroll
            for (int j = 0; j <= 2 * R; j++) sacc += t.k[j] * (int)p[j * BT_X];
            ch[q][c] = (uint32_t)((sacc + (1 << (t.shift - 1))) >> t.shift);
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < PER; q++) {
        const int i = tid + q * 256;
        int ry = i / BT_X, rx = i - ry * BT_X;
        if (gy0 + ry < h && gx0 + rx < w)
            dst[f * N + (size_t)(gy0 + ry) * w + gx0 + rx] = (uint8_t)((ch[q][0] * 3735u + ch[q][1] * 19235u + ch[q][2] * 9798u + 16384u) >> 15);
    }
}

int blur7_bgr(const uint8_t *bgr, int n, int h, int w, const FrameState *st, uint8_t *dst, hipStream_t s)
{
    Taps t7 = {{2, 7, 14, 18, 14, 7, 2}, 3, 12};
    CPE_LAUNCH_BEGIN();
    const int tiles_x = (w + BT_X - 1) / BT_X, tiles_y = (h + BT_Y - 1) / BT_Y;
    CPE_KLAUNCH(k_blur7_bgr, dim3((unsigned)(n * tiles_x * tiles_y)), dim3(256), 0, s, bgr, h, w, tiles_x, tiles_y, t7, st, dst);
    CPE_CHECK_LAUNCH("blur7_bgr");
    return CPE_OK;
}

int blur7_u8(const uint8_t *src, int n, int h, int w, const FrameState *st, uint8_t *dst, hipStream_t s)
{
    Taps t7 = {{2, 7, 14, 18, 14, 7, 2}, 3, 12};
    CPE_LAUNCH_BEGIN();
    const int tiles_x = (w + BT_X - 1) / BT_X, tiles_y = (h + BT_Y - 1) / BT_Y;
    CPE_KLAUNCH((k_blur_fused<3>), dim3((unsigned)(n * tiles_x * tiles_y)), dim3(256), 0, s, src, h, w, tiles_x, tiles_y, t7,
                st, dst);
    CPE_CHECK_LAUNCH("blur7_u8");
    return CPE_OK;
}

// a-2: hmask, vmask, joints mask and its components (no dependence on the region stage: own stream)
int joints_mask_stage(int n, int h, int w, const MaskBuffers &B, FrameState *st, hipStream_t s)
{
    CPE_LAUNCH_BEGIN();
    // word-level consumers: hmask / vmask leave as one-bit planes in the joints-mask buffer, whose bytes nobody reads then
    const bool as_bits = line_masks_as_bits(B, w);
    CPE_CHECK_ARG(!as_bits || 2 * bit_plane_words(h, w) * 8 <= (size_t)h * w, "joints_mask_stage: frame too small for its line-mask planes");
    unsigned long long *hb = as_bits ? line_mask_bits(B, 0, n, h, w) : nullptr, *vb = as_bits ? line_mask_bits(B, 1, n, h, w) : nullptr;
    uint8_t *hm = as_bits && B.skip_debug ? nullptr : B.hmask, *vm = as_bits && B.skip_debug ? nullptr : B.vmask;
    uint8_t *jm = as_bits ? nullptr : B.joints_mask;
    // one wave per column strip, band of rows and frame
    CPE_CHECK_ARG(n <= 65535 && (h + OB_R - 1) / OB_R <= 65535, "joints_mask_stage: too many frames or rows for one launch");
    CPE_KLAUNCH(k_open20_joints, dim3((unsigned)br_strips(w), (unsigned)((h + OB_R - 1) / OB_R), (unsigned)n), dim3(64), 0, s,
                (const uint8_t *)B.binary, h, w, hm, vm, jm, B.jbits, hb, vb);
    CPE_CHECK_LAUNCH("joints_mask_stage");
    int rc;
    if ((rc = ccl_components(B.joints_mask, B.jbits, n, h, w, 0, WIN_FRAME, B.lab_p, B.roots_p, ROOTS_JOINTS, st, s)) != CPE_OK) return rc;
    // RETR_EXTERNAL (:1817): outer background of the joints mask (whole frame), on this chain, beside the region stage
    const size_t fl_words = (size_t)h * ((w + 63) / 64);
    return outside_flood(B.joints_mask, n, h, w, st, WIN_FRAME, B.fl_j, B.fl_j + (size_t)n * fl_words, fl_words, s, B.jbits);
}

// a-5 head: saturated spot -> circle_mask, r0 (depends on the grey frame only: own stream)
int spot_stage(const uint8_t *gray, int n, int h, int w, const MaskBuffers &B, FrameState *st, hipStream_t s, int planar)
{
    const size_t total = (size_t)h * w * n;
    int rc;
    CPE_LAUNCH_BEGIN();
    // (B.best_s and st[].srect were reset by k_state_init)
    Taps t19 = {{1, 1, 3, 5, 10, 15, 20, 27, 30, 32, 30, 27, 20, 15, 10, 5, 3, 1, 1}, 9, 16};
    {
        const int tiles_x = (w + BT_X - 1) / BT_X, tiles_y = (h + BT_Y - 1) / BT_Y;
        CPE_CHECK_ARG(tiles_x <= 128 && (size_t)tiles_x * tiles_y <= (size_t)MAXROOTS * sizeof(int), "spot_stage: frame too large");
        // tile flags: in the root list of the spot labelling, which is written after the blur has read them
        uint8_t *flags = reinterpret_cast<uint8_t *>(B.roots_s);
        const size_t fstride = (size_t)MAXROOTS * sizeof(int);
        CPE_KLAUNCH(k_spot_scan, dim3((unsigned)(n * tiles_y)), dim3(256), 0, s, gray, h, w, tiles_x, tiles_y, st, flags, fstride);
        CPE_KLAUNCH(k_blur19_spot, dim3((unsigned)(n * tiles_y)), dim3(256), 0, s, gray, h, w, tiles_x, tiles_y, t19,
                    (const uint8_t *)flags, fstride, B.g19);
    }
    // labelling of blurred > 240 inside st[].srect (WIN_SPOT): the only place it can hold
    if ((rc = ccl_components(B.g19, nullptr, n, h, w, 240, WIN_SPOT, B.lab_s, B.roots_s, ROOTS_SPOT, st, s)) != CPE_OK) return rc;
    CPE_KLAUNCH(k_spot_area, dim3(4, n), dim3(64), 0, s, B.g19, h, w, B.roots_s, st, B.best_s);
    (void)hipMemsetAsync(B.cm, 255, total, s);
    CPE_KLAUNCH(k_spot_ellipse, dim3(n), dim3(64), 0, s, B.g19, n, h, w, B.best_s, st, B.verts, B.cm, planar);
    CPE_CHECK_LAUNCH("spot_stage");
    return CPE_OK;
}

// a-2/a-4 (joint centroids inside rect), a-5 (roi masks), a-6 (expansion).  Needs st[].rect and mc, the joints
// components and the spot.
int masks_stage(const uint8_t *gray, int n, int h, int w, const MaskBuffers &B, FrameState *st, hipStream_t s,
                const RegionSide *side, int planar, hipStream_t sj)
{
    int rc;
    CPE_LAUNCH_BEGIN();
    CPE_KLAUNCH(k_masks_reset, dim3((n + 63) / 64), dim3(64), 0, s, st, n);
    // scratch of the RETR_EXTERNAL tests: u64 planes carved from the one-bit planes the region stage is done with
    // (planes 0 and 1 hold the fragment masks below; a u64 plane of h * ceil(w/64) words fits one bit plane)
    const size_t fl_words = bit_plane_words(h, w);          // u64 words per frame of one flood plane = of one bit plane
    auto fl_plane = [&](int k) { return bit_plane(B.bits, (size_t)(2 + k) * n, h, w); };
    // joints (their outer-background mask comes from the joints chain).  Only the lines kernel reads them: with helper
    // streams they are collected on `sj` beside the two fragment chains instead of in front of them
    const bool jside = side && sj != s;
    if (jside) { (void)hipEventRecord(side->clahe_done, s); (void)hipStreamWaitEvent(sj, side->clahe_done, 0); }
    {
        hipStream_t q = jside ? sj : s;
        CPE_KLAUNCH(k_joint_centroids, dim3(frame_waves(n, 16, MAXROOTS / 64), n), dim3(64), 0, q, (const uint32_t *)B.jbits, h, w, B.roots_p, st, B.jtmp,
                    (const unsigned long long *)(B.fl_j + (size_t)n * h * ((w + 63) / 64)), (size_t)h * ((w + 63) / 64));
        CPE_KLAUNCH(k_joint_sort, dim3(n), dim3(256), 0, q, st, B.jtmp, B.joints);
    }
    // a-5 tail, a-6 and the labelling of the expanded masks, once per line direction.  The two directions share
    // nothing but their inputs: the vertical one runs on the helper stream (if any) with the spot chain's label plane.
    const dim3 rb_grid((unsigned)br_strips(w), (unsigned)((h + RB_R - 1) / RB_R), (unsigned)n);
    CPE_CHECK_ARG(n <= 65535 && rb_grid.y <= 65535, "masks_stage: too many frames or rows for one launch");
    if (side) { (void)hipEventRecord(side->clahe_done, s); (void)hipStreamWaitEvent(side->s, side->clahe_done, 0); }
    for (int which = 0; which < 2; which++) {
        hipStream_t q = (which && side) ? side->s : s;
        const bool as_bits = line_masks_as_bits(B, w);
        const uint8_t *lm = as_bits ? nullptr : (which ? B.vmask : B.hmask);
        const unsigned long long *lmb = as_bits ? line_mask_bits(B, which, n, h, w) : nullptr;
        uint8_t *roi = as_bits && B.skip_debug ? nullptr : (which ? B.roi_v : B.roi_h);
        uint8_t *exp = which ? B.exp_v : B.exp_h;
        int *lab = which ? B.lab_s : B.lab, *roots = which ? B.roots_s : B.roots;
        const RootList list = which ? ROOTS_SPOT : ROOTS_MAIN;
        uint32_t *bits = reinterpret_cast<uint32_t *>(bit_plane(B.bits, which ? (size_t)n : 0, h, w));
        SegRec *segs = B.segs + (size_t)which * n * MAXSEG;
        // roi = open3x3(mask & circle_mask & mask_contour), base = close3x3(roi) as a one-bit plane, exp = base & mask_contour.
        // base's bytes are only written where the labelling will read them (the byte-level kernels)
        uint8_t *base = ccl_components_reads_bits(bits, w, lab) ? nullptr : (which ? B.base_v : B.base_h);
        CPE_KLAUNCH(k_roi_base, rb_grid, dim3(64), 0, q, lm, (const uint8_t *)B.cm, (const uint8_t *)B.mc,
                    h, w, (const FrameState *)st, roi, base, exp, bits, lmb);
        if ((rc = ccl_components(base, bits, n, h, w, 0, WIN_REGION, lab, roots, list, st, q)) != CPE_OK) return rc;
        unsigned long long *fl_bg = fl_plane(2 + 2 * which), *fl_out = fl_plane(3 + 2 * which);
        if ((rc = outside_flood(base, n, h, w, st, WIN_REGION, fl_bg, fl_out, fl_words, q, bits)) != CPE_OK) return rc;
        if (planar) CPE_KLAUNCH((k_seg_trace<8, 700>), dim3(frame_waves(n, 32, 512), n), dim3(64), 0, q, (const uint32_t *)bits, h, w, which, (const int *)roots, list, st, segs, (const unsigned long long *)fl_out, fl_words);
        else CPE_KLAUNCH((k_seg_trace<5, 200>), dim3(frame_waves(n, 32, 512), n), dim3(64), 0, q, (const uint32_t *)bits, h, w, which, (const int *)roots, list, st, segs, (const unsigned long long *)fl_out, fl_words);
        CPE_KLAUNCH(k_seg_global, dim3(n), dim3(256), 0, q, st, which, (const SegRec *)segs);
        // the expansion adds its pixels to the seed k_roi_base left in exp
        if (planar) CPE_KLAUNCH(k_seg_expand<EXP_MAXKS_PLANE>, dim3(frame_waves(n, 32, 256), n), dim3(EXP_NT), 0, q, (const uint32_t *)bits, (const uint8_t *)B.mc, h, w, which, st, (const SegRec *)segs, exp, 201);
        else CPE_KLAUNCH(k_seg_expand<EXP_MAXKS>, dim3(frame_waves(n, 32, 256), n), dim3(EXP_NT), 0, q, (const uint32_t *)bits, (const uint8_t *)B.mc, h, w, which, st, (const SegRec *)segs, exp, 0);
        CPE_CHECK_LAUNCH("masks_stage expand");
        // cv2.connectedComponents of the expanded mask: unions only, k_lines resolves the joints' labels
        if ((rc = ccl_unions(exp, n, h, w, WIN_REGION, which ? B.lab_v : B.lab_h, st, q)) != CPE_OK) return rc;
    }
    if (side) { (void)hipEventRecord(side->traced, side->s); (void)hipStreamWaitEvent(s, side->traced, 0); }
    return CPE_OK;
}

}  // namespace cpe
