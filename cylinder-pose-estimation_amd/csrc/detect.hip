// detect_grid for a batch of grey frames: orchestration of the image half of the hot path and its C ABI.
//   reference: python_grid_detection_cylinder.py:68-112 (detect_grid) and
//              util_cylinder.color_and_expand_lines (:2014-2060)
// Stage order (the reference's 1..6, with independent stages hoisted):
//   preprocess -> hmask/vmask/joints mask -> region (blob hull + rect) -> joints in rect, spot ellipse,
//   roi masks, fragment expansion -> labels of the expanded masks -> blur7 -> lines / indexing kernel.
// Everything stays in HBM between the u8 frame read and the point-table write; all scratch lives in the
// caller-supplied workspace (cpe_detect_workspace_bytes), laid out plane-major so that every kernel
// streams [n, h, w] planes with fully coalesced accesses.
#include "workspace.h"
#include <ctype.h>
#include <mutex>
#include <stdlib.h>

namespace cpe {

namespace {

// per-frame state of a call, and the accumulators the three chains start from (one launch in front of the fork instead of a
// reset kernel at the head of every chain)
__global__ void k_state_init(FrameState *st, int n, unsigned long long *best, unsigned long long *best_s, int *nrect)
{
    int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n) return;
    FrameState z = {};
    z.srect[0] = INT_MAX; z.srect[1] = INT_MAX; z.srect[2] = -1; z.srect[3] = -1;   // spot window: empty until k_spot_scan finds a tile
    st[f] = z;
    if (best) { best[f] = 0; best_s[f] = 0; }                                      // largest-contour keys (region / spot)
    if (nrect) { nrect[16 * f] = INT_MAX; nrect[16 * f + 1] = INT_MAX; nrect[16 * f + 2] = -1; nrect[16 * f + 3] = -1; }   // CLAHE's bounding box
}

__global__ void k_finish(const FrameState *st, int n, int *status, int *n_pts)
{
    int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n) return;
    int s = st[f].status;
    if (st[f].overflow) s = CPE_ST_OVERFLOW;
    status[f] = s;
    if (s != CPE_ST_OK) n_pts[f] = 0;
}

// Helper streams for the independent chains of a call: one set (three streams, their events) per device AND caller stream,
// so two host threads -- or one thread with chunks in flight on several streams (FramePipeline(lanes=2)) -- neither share
// nor serialise their side chains.  Created on first use, kept for the life of the process (at most SIDE_SETS caller
// streams per device get their own set; further ones share the last).  CPE_SERIAL=1 keeps everything on the caller's stream.
struct SideStreams {
    std::mutex mu;      // held by a caller from its fork to its join (cpe_detect_grid_batch_ex)
    bool ok = false;
    hipStream_t key = nullptr;
    bool used = false;
    hipStream_t s1 = nullptr, s2 = nullptr, s3 = nullptr;
    hipEvent_t fork = nullptr, join1 = nullptr, join2 = nullptr, e3a = nullptr, e3b = nullptr, e3c = nullptr, e3d = nullptr;
};
constexpr int SIDE_SETS = 4;
SideStreams &side_streams(hipStream_t caller)
{
    static SideStreams sets[32][SIDE_SETS];
    static std::mutex mu;
    static SideStreams none;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 32) return none;
    const char *e = getenv("CPE_SERIAL");   // looked at on every call: a profiling pass can switch the overlap off
    if (e && e[0] == '1') return none;
    std::lock_guard<std::mutex> lk(mu);
    int slot = SIDE_SETS - 1;
    for (int k = 0; k < SIDE_SETS; k++) {
        if (sets[dev][k].used && sets[dev][k].key == caller) { slot = k; break; }
        if (!sets[dev][k].used) { slot = k; break; }
    }
    SideStreams &X = sets[dev][slot];
    if (!X.used) {
        X.used = true;
        X.key = caller;
        bool good = hipStreamCreateWithFlags(&X.s1, hipStreamNonBlocking) == hipSuccess &&
                    hipStreamCreateWithFlags(&X.s2, hipStreamNonBlocking) == hipSuccess &&
                    hipStreamCreateWithFlags(&X.s3, hipStreamNonBlocking) == hipSuccess &&
                    hipEventCreateWithFlags(&X.e3a, hipEventDisableTiming) == hipSuccess &&
                    hipEventCreateWithFlags(&X.e3b, hipEventDisableTiming) == hipSuccess &&
                    hipEventCreateWithFlags(&X.e3c, hipEventDisableTiming) == hipSuccess &&
                    hipEventCreateWithFlags(&X.e3d, hipEventDisableTiming) == hipSuccess &&
                    hipEventCreateWithFlags(&X.fork, hipEventDisableTiming) == hipSuccess &&
                    hipEventCreateWithFlags(&X.join1, hipEventDisableTiming) == hipSuccess &&
                    hipEventCreateWithFlags(&X.join2, hipEventDisableTiming) == hipSuccess;
        X.ok = good;
        if (!good) (void)hipGetLastError();
    }
    return X;
}

// the region stage's buffers inside the workspace (cpe_detect_grid_batch*, cpe_debug_blob_region, cpe_debug_clahe_planes)
RegionBuffers region_buffers(const Workspace &W, int h, int w)
{
    RegionBuffers R;
    R.cl = W.at<uint8_t>(WS_CLAHE); R.ext = W.at<uint8_t>(WS_DISCS); R.mc = W.at<uint8_t>(WS_MASK_CONTOUR); R.touch = W.at<uint8_t>(WS_TOUCH);
    R.lab = W.at<int>(WS_LABELS); R.cnt = W.at<int>(WS_LABELS_AUX); R.roots = W.at<int>(WS_ROOTS); R.nrect = W.at<int>(WS_NRECT);
    R.lab2 = W.at<int>(WS_BRIGHT_NODES); R.cnt2 = W.at<int>(WS_BRIGHT_COUNTS); R.sw = W.at<int>(WS_SWEEP); R.bk = W.at<int>(WS_BUCKET_PIXELS);
    R.hl = W.at<int2>(WS_LIST_DARK); R.bl = W.at<int2>(WS_LIST_BRIGHT); R.tl = W.at<int2>(WS_LIST_TRACE);
    R.bits = W.at<uint32_t>(WS_BITS); R.pool = W.at<uint32_t>(WS_POOL); R.blob_ch = W.at<unsigned short>(WS_BLOB_CH);
    R.maxch = region_maxch(h, w); R.maxdf = region_maxdf(h, w); R.gmid = W.at<double>(WS_GMID);
    R.hist = W.at<unsigned int>(WS_HIST); R.lut = W.at<uint8_t>(WS_LUT);
    R.blobs = W.at<BlobRec>(WS_BLOBS); R.blob_d = W.at<int>(WS_BLOB_D); R.order = W.at<int>(WS_ORDER); R.dists = W.at<double>(WS_DISTS);
    R.groups = W.at<Group>(WS_GROUPS); R.best = W.at<unsigned long long>(WS_BEST); R.lohi = W.at<int>(WS_LOHI); R.hull = W.at<int>(WS_HULL);
    return R;
}

// the masks stage's buffers inside the workspace (cpe_detect_grid_batch*, cpe_debug_masks); R: region_buffers of the same call
MaskBuffers mask_buffers(const Workspace &W, const RegionBuffers &R)
{
    MaskBuffers M;
    M.binary = W.at<uint8_t>(WS_BINARY); M.hmask = W.at<uint8_t>(WS_HMASK); M.vmask = W.at<uint8_t>(WS_VMASK);
    M.joints_mask = W.at<uint8_t>(WS_JOINTS_MASK);
    M.g19 = W.at<uint8_t>(WS_BLUR19); M.cm = W.at<uint8_t>(WS_CM); M.mc = R.mc; M.roi_h = W.at<uint8_t>(WS_ROI_H);
    M.roi_v = W.at<uint8_t>(WS_ROI_V); M.base_h = W.at<uint8_t>(WS_BASE_H); M.base_v = W.at<uint8_t>(WS_BASE_V);
    M.exp_h = W.at<uint8_t>(WS_EXP_H); M.exp_v = W.at<uint8_t>(WS_EXP_V); M.touch = R.touch; M.bits = R.bits;
    M.lab = R.lab; M.roots = R.roots; M.jtmp = W.at<int>(WS_JTMP); M.joints = W.at<int>(WS_JOINTS); M.verts = W.at<int>(WS_VERTS);
    M.best = R.best; M.segs = W.at<SegRec>(WS_SEGS);
    M.lab_p = W.at<int>(WS_LABELS_JOINTS); M.lab_s = W.at<int>(WS_LABELS_SPOT);
    M.roots_p = W.at<int>(WS_ROOTS_JOINTS); M.roots_s = W.at<int>(WS_ROOTS_SPOT); M.best_s = W.at<unsigned long long>(WS_BEST_SPOT);
    M.fl_j = W.at<unsigned long long>(WS_FLJ); M.jbits = W.at<uint32_t>(WS_JOINT_BITS);
    M.lab_h = nullptr; M.lab_v = nullptr;   // WS_LABELS / WS_LABELS_AUX, set by the caller once the region stage is done with them
    return M;
}

}  // namespace
}  // namespace cpe

using namespace cpe;

extern "C" size_t cpe_detect_workspace_bytes(int32_t n, int32_t h, int32_t w)
{
    if (n <= 0 || h <= 0 || w <= 0) return 0;
    return make_layout(n, h, w).total;
}

extern "C" int32_t cpe_detect_workspace_plane(int32_t n, int32_t h, int32_t w, int32_t plane, size_t *offset,
                                              size_t *bytes_per_frame)
{
    CPE_CHECK_ARG(n > 0 && h > 0 && w > 0 && plane >= 0 && plane < CPE_PLANE_COUNT && offset && bytes_per_frame,
                  "cpe_detect_workspace_plane: bad argument");
    const Layout L = make_layout(n, h, w);
    const WsId id = ws_public(plane);
    *offset = L.off[id];
    *bytes_per_frame = L.bytes_per_frame[id];
    return CPE_OK;
}

// One row of the workspace's table of buffers (CPE_WS_TABLE) for an (n, h, w) call: host code only (tests, debugging).
extern "C" int32_t cpe_debug_workspace_buffer(int32_t n, int32_t h, int32_t w, int32_t index, char *name_out, size_t name_cap,
                                              size_t *offset, size_t *bytes_per_frame, int32_t *overlay, int32_t *side,
                                              int32_t *public_plane)
{
    CPE_CHECK_ARG(n > 0 && h > 0 && w > 0 && index >= 0 && index < WS_COUNT && name_out && name_cap > 0 && offset && bytes_per_frame &&
                  overlay && side && public_plane, "cpe_debug_workspace_buffer: bad argument");
    const Layout L = make_layout(n, h, w);
    const WsRow &r = WS_ROWS[index];
    size_t k = 0;
    for (; r.name[k] && k + 1 < name_cap; k++) name_out[k] = (char)tolower(r.name[k]);
    name_out[k] = 0;
    *offset = L.off[index]; *bytes_per_frame = L.bytes_per_frame[index];
    *overlay = r.overlay; *side = r.side; *public_plane = r.public_plane;
    return CPE_OK;
}

// One row of the state record's table of fields (CPE_STATE_FIELDS, cpe_dev.h): host code only (tests, debugging).
extern "C" int32_t cpe_debug_state_field(int32_t index, char *name_out, size_t name_cap, int32_t *words, int32_t *is_float)
{
    constexpr int32_t rows = sizeof(STATE_FIELDS) / sizeof(STATE_FIELDS[0]);
    CPE_CHECK_ARG(index >= 0 && index < rows && name_out && name_cap > 0 && words && is_float, "cpe_debug_state_field: bad argument");
    const StateField &r = STATE_FIELDS[index];
    size_t k = 0;
    for (; r.name[k] && k + 1 < name_cap; k++) name_out[k] = r.name[k];
    name_out[k] = 0;
    *words = r.words; *is_float = r.is_float;
    return CPE_OK;
}

extern "C" int32_t cpe_detect_grid_batch(const uint8_t *gray, int32_t n, int32_t h, int32_t w, void *ws, size_t ws_bytes,
                                         double *xy, int32_t *id, int32_t *n_pts, double *center, int32_t *status,
                                         void *stream)
{
    return cpe_detect_grid_batch_ex(gray, n, h, w, nullptr, ws, ws_bytes, xy, id, n_pts, center, status, stream);
}

namespace cpe { namespace {
// L channel of cv2.cvtColor(BGR2LAB) of a colour frame (util_cylinder.py:1840-1841), [ext] OpenCV 4.5.5 RGB2Lab_b: sRGB gamma
// table per channel, Y row of sRGB -> XYZ (D65) in 12-bit fixed point, cube-root table folded into LY (tools/gen_lab_lut.py
// colour).  R = G = B gives region.hip's c_lab_l.
__constant__ uint16_t c_gamma[256] = { 0, 1, 1, 2, 2, 3, 4, 4, 5, 6, 6, 7, 8, 8, 9, 10, 11, 11, 12, 13, 14, 15, 16, 17, 19, 20, 21, 22, 24, 25, 26, 28, 29, 31, 33, 34, 36, 38, 40, 41, 43, 45, 47, 49, 51, 54, 56, 58, 60, 63, 65, 68, 70, 73, 75, 78, 81, 83, 86, 89, 92, 95, 98, 101, 105, 108, 111, 115, 118, 121, 125, 129, 132, 136, 140, 144, 147, 151, 155, 160, 164, 168, 172, 176, 181, 185, 190, 194, 199, 204, 209, 213, 218, 223, 228, 233, 239, 244, 249, 255, 260, 265, 271, 277, 282, 288, 294, 300, 306, 312, 318, 324, 331, 337, 343, 350, 356, 363, 370, 376, 383, 390, 397, 404, 411, 418, 426, 433, 440, 448, 455, 463, 471, 478, 486, 494, 502, 510, 518, 527, 535, 543, 552, 560, 569, 578, 586, 595, 604, 613, 622, 631, 641, 650, 659, 669, 678, 688, 698, 707, 717, 727, 737, 747, 757, 768, 778, 788, 799, 809, 820, 831, 842, 852, 863, 875, 886, 897, 908, 920, 931, 943, 954, 966, 978, 990, 1002, 1014, 1026, 1038, 1050, 1063, 1075, 1088, 1101, 1113, 1126, 1139, 1152, 1165, 1178, 1192, 1205, 1218, 1232, 1245, 1259, 1273, 1287, 1301, 1315, 1329, 1343, 1357, 1372, 1386, 1401, 1415, 1430, 1445, 1460, 1475, 1490, 1505, 1521, 1536, 1551, 1567, 1583, 1598, 1614, 1630, 1646, 1662, 1678, 1695, 1711, 1728, 1744, 1761, 1778, 1794, 1811, 1828, 1846, 1863, 1880, 1897, 1915, 1933, 1950, 1968, 1986, 2004, 2022, 2040 };
__constant__ uint8_t c_ly[2041] = { 0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11, 12, 14, 15, 16, 17, 18, 19, 20, 21, 23, 24, 25, 26, 27, 27, 28, 29, 30, 31, 32, 33, 33, 34, 35, 36, 36, 37, 38, 38, 39, 40, 40, 41, 42, 42, 43, 43, 44, 45, 45, 46, 46, 47, 47, 48, 48, 49, 50, 50, 51, 51, 52, 52, 53, 53, 54, 54, 54, 55, 55, 56, 56, 57, 57, 58, 58, 58, 59, 59, 60, 60, 61, 61, 61, 62, 62, 63, 63, 63, 64, 64, 65, 65, 65, 66, 66, 66, 67, 67, 68, 68, 68, 69, 69, 69, 70, 70, 70, 71, 71, 71, 72, 72, 72, 73, 73, 73, 74, 74, 74, 75, 75, 75, 76, 76, 76, 77, 77, 77, 77, 78, 78, 78, 79, 79, 79, 80, 80, 80, 80, 81, 81, 81, 82, 82, 82, 82, 83, 83, 83, 83, 84, 84, 84, 85, 85, 85, 85, 86, 86, 86, 86, 87, 87, 87, 87, 88, 88, 88, 88, 89, 89, 89, 89, 90, 90, 90, 90, 91, 91, 91, 91, 92, 92, 92, 92, 93, 93, 93, 93, 94, 94, 94, 94, 95, 95, 95, 95, 95, 96, 96, 96, 96, 97, 97, 97, 97, 97, 98, 98, 98, 98, 99, 99, 99, 99, 99, 100, 100, 100, 100, 101, 101, 101, 101, 101, 102, 102, 102, 102, 102, 103, 103, 103, 103, 103, 104, 104, 104, 104, 104, 105, 105, 105, 105, 105, 106, 106, 106, 106, 106, 107, 107, 107, 107, 107, 108, 108, 108, 108, 108, 109, 109, 109, 109, 109, 109, 110, 110, 110, 110, 110, 111, 111, 111, 111, 111, 112, 112, 112, 112, 112, 112, 113, 113, 113, 113, 113, 114, 114, 114, 114, 114, 114, 115, 115, 115, 115, 115, 115, 116, 116, 116, 116, 116, 116, 117, 117, 117, 117, 117, 117, 118, 118, 118, 118, 118, 119, 119, 119, 119, 119, 119, 119, 120, 120, 120, 120, 120, 120, 121, 121, 121, 121, 121, 121, 122, 122, 122, 122, 122, 122, 123, 123, 123, 123, 123, 123, 124, 124, 124, 124, 124, 124, 124, 125, 125, 125, 125, 125, 125, 126, 126, 126, 126, 126, 126, 126, 127, 127, 127, 127, 127, 127, 128, 128, 128, 128, 128, 128, 128, 129, 129, 129, 129, 129, 129, 129, 130, 130, 130, 130, 130, 130, 130, 131, 131, 131, 131, 131, 131, 131, 132, 132, 132, 132, 132, 132, 132, 133, 133, 133, 133, 133, 133, 133, 134, 134, 134, 134, 134, 134, 134, 135, 135, 135, 135, 135, 135, 135, 135, 136, 136, 136, 136, 136, 136, 136, 137, 137, 137, 137, 137, 137, 137, 138, 138, 138, 138, 138, 138, 138, 138, 139, 139, 139, 139, 139, 139, 139, 139, 140, 140, 140, 140, 140, 140, 140, 141, 141, 141, 141, 141, 141, 141, 141, 142, 142, 142, 142, 142, 142, 142, 142, 143, 143, 143, 143, 143, 143, 143, 143, 144, 144, 144, 144, 144, 144, 144, 144, 145, 145, 145, 145, 145, 145, 145, 145, 146, 146, 146, 146, 146, 146, 146, 146, 147, 147, 147, 147, 147, 147, 147, 147, 147, 148, 148, 148, 148, 148, 148, 148, 148, 149, 149, 149, 149, 149, 149, 149, 149, 149, 150, 150, 150, 150, 150, 150, 150, 150, 151, 151, 151, 151, 151, 151, 151, 151, 151, 152, 152, 152, 152, 152, 152, 152, 152, 152, 153, 153, 153, 153, 153, 153, 153, 153, 154, 154, 154, 154, 154, 154, 154, 154, 154, 155, 155, 155, 155, 155, 155, 155, 155, 155, 156, 156, 156, 156, 156, 156, 156, 156, 156, 156, 157, 157, 157, 157, 157, 157, 157, 157, 157, 158, 158, 158, 158, 158, 158, 158, 158, 158, 159, 159, 159, 159, 159, 159, 159, 159, 159, 159, 160, 160, 160, 160, 160, 160, 160, 160, 160, 161, 161, 161, 161, 161, 161, 161, 161, 161, 161, 162, 162, 162, 162, 162, 162, 162, 162, 162, 163, 163, 163, 163, 163, 163, 163, 163, 163, 163, 164, 164, 164, 164, 164, 164, 164, 164, 164, 164, 165, 165, 165, 165, 165, 165, 165, 165, 165, 165, 166, 166, 166, 166, 166, 166, 166, 166, 166, 166, 167, 167, 167, 167, 167, 167, 167, 167, 167, 167, 168, 168, 168, 168, 168, 168, 168, 168, 168, 168, 168, 169, 169, 169, 169, 169, 169, 169, 169, 169, 169, 170, 170, 170, 170, 170, 170, 170, 170, 170, 170, 170, 171, 171, 171, 171, 171, 171, 171, 171, 171, 171, 172, 172, 172, 172, 172, 172, 172, 172, 172, 172, 172, 173, 173, 173, 173, 173, 173, 173, 173, 173, 173, 173, 174, 174, 174, 174, 174, 174, 174, 174, 174, 174, 174, 175, 175, 175, 175, 175, 175, 175, 175, 175, 175, 176, 176, 176, 176, 176, 176, 176, 176, 176, 176, 176, 176, 177, 177, 177, 177, 177, 177, 177, 177, 177, 177, 177, 178, 178, 178, 178, 178, 178, 178, 178, 178, 178, 178, 179, 179, 179, 179, 179, 179, 179, 179, 179, 179, 179, 180, 180, 180, 180, 180, 180, 180, 180, 180, 180, 180, 180, 181, 181, 181, 181, 181, 181, 181, 181, 181, 181, 181, 181, 182, 182, 182, 182, 182, 182, 182, 182, 182, 182, 182, 183, 183, 183, 183, 183, 183, 183, 183, 183, 183, 183, 183, 184, 184, 184, 184, 184, 184, 184, 184, 184, 184, 184, 184, 185, 185, 185, 185, 185, 185, 185, 185, 185, 185, 185, 185, 186, 186, 186, 186, 186, 186, 186, 186, 186, 186, 186, 186, 187, 187, 187, 187, 187, 187, 187, 187, 187, 187, 187, 187, 187, 188, 188, 188, 188, 188, 188, 188, 188, 188, 188, 188, 188, 189, 189, 189, 189, 189, 189, 189, 189, 189, 189, 189, 189, 190, 190, 190, 190, 190, 190, 190, 190, 190, 190, 190, 190, 190, 191, 191, 191, 191, 191, 191, 191, 191, 191, 191, 191, 191, 191, 192, 192, 192, 192, 192, 192, 192, 192, 192, 192, 192, 192, 193, 193, 193, 193, 193, 193, 193, 193, 193, 193, 193, 193, 193, 194, 194, 194, 194, 194, 194, 194, 194, 194, 194, 194, 194, 194, 195, 195, 195, 195, 195, 195, 195, 195, 195, 195, 195, 195, 195, 196, 196, 196, 196, 196, 196, 196, 196, 196, 196, 196, 196, 196, 196, 197, 197, 197, 197, 197, 197, 197, 197, 197, 197, 197, 197, 197, 198, 198, 198, 198, 198, 198, 198, 198, 198, 198, 198, 198, 198, 199, 199, 199, 199, 199, 199, 199, 199, 199, 199, 199, 199, 199, 199, 200, 200, 200, 200, 200, 200, 200, 200, 200, 200, 200, 200, 200, 200, 201, 201, 201, 201, 201, 201, 201, 201, 201, 201, 201, 201, 201, 202, 202, 202, 202, 202, 202, 202, 202, 202, 202, 202, 202, 202, 202, 203, 203, 203, 203, 203, 203, 203, 203, 203, 203, 203, 203, 203, 203, 204, 204, 204, 204, 204, 204, 204, 204, 204, 204, 204, 204, 204, 204, 204, 205, 205, 205, 205, 205, 205, 205, 205, 205, 205, 205, 205, 205, 205, 206, 206, 206, 206, 206, 206, 206, 206, 206, 206, 206, 206, 206, 206, 207, 207, 207, 207, 207, 207, 207, 207, 207, 207, 207, 207, 207, 207, 207, 208, 208, 208, 208, 208, 208, 208, 208, 208, 208, 208, 208, 208, 208, 209, 209, 209, 209, 209, 209, 209, 209, 209, 209, 209, 209, 209, 209, 209, 210, 210, 210, 210, 210, 210, 210, 210, 210, 210, 210, 210, 210, 210, 210, 211, 211, 211, 211, 211, 211, 211, 211, 211, 211, 211, 211, 211, 211, 211, 212, 212, 212, 212, 212, 212, 212, 212, 212, 212, 212, 212, 212, 212, 212, 213, 213, 213, 213, 213, 213, 213, 213, 213, 213, 213, 213, 213, 213, 213, 214, 214, 214, 214, 214, 214, 214, 214, 214, 214, 214, 214, 214, 214, 214, 215, 215, 215, 215, 215, 215, 215, 215, 215, 215, 215, 215, 215, 215, 215, 215, 216, 216, 216, 216, 216, 216, 216, 216, 216, 216, 216, 216, 216, 216, 216, 217, 217, 217, 217, 217, 217, 217, 217, 217, 217, 217, 217, 217, 217, 217, 217, 218, 218, 218, 218, 218, 218, 218, 218, 218, 218, 218, 218, 218, 218, 218, 218, 219, 219, 219, 219, 219, 219, 219, 219, 219, 219, 219, 219, 219, 219, 219, 219, 220, 220, 220, 220, 220, 220, 220, 220, 220, 220, 220, 220, 220, 220, 220, 220, 221, 221, 221, 221, 221, 221, 221, 221, 221, 221, 221, 221, 221, 221, 221, 221, 222, 222, 222, 222, 222, 222, 222, 222, 222, 222, 222, 222, 222, 222, 222, 222, 223, 223, 223, 223, 223, 223, 223, 223, 223, 223, 223, 223, 223, 223, 223, 223, 223, 224, 224, 224, 224, 224, 224, 224, 224, 224, 224, 224, 224, 224, 224, 224, 224, 225, 225, 225, 225, 225, 225, 225, 225, 225, 225, 225, 225, 225, 225, 225, 225, 225, 226, 226, 226, 226, 226, 226, 226, 226, 226, 226, 226, 226, 226, 226, 226, 226, 226, 227, 227, 227, 227, 227, 227, 227, 227, 227, 227, 227, 227, 227, 227, 227, 227, 227, 228, 228, 228, 228, 228, 228, 228, 228, 228, 228, 228, 228, 228, 228, 228, 228, 228, 229, 229, 229, 229, 229, 229, 229, 229, 229, 229, 229, 229, 229, 229, 229, 229, 229, 230, 230, 230, 230, 230, 230, 230, 230, 230, 230, 230, 230, 230, 230, 230, 230, 230, 231, 231, 231, 231, 231, 231, 231, 231, 231, 231, 231, 231, 231, 231, 231, 231, 231, 231, 232, 232, 232, 232, 232, 232, 232, 232, 232, 232, 232, 232, 232, 232, 232, 232, 232, 233, 233, 233, 233, 233, 233, 233, 233, 233, 233, 233, 233, 233, 233, 233, 233, 233, 233, 234, 234, 234, 234, 234, 234, 234, 234, 234, 234, 234, 234, 234, 234, 234, 234, 234, 234, 235, 235, 235, 235, 235, 235, 235, 235, 235, 235, 235, 235, 235, 235, 235, 235, 235, 235, 236, 236, 236, 236, 236, 236, 236, 236, 236, 236, 236, 236, 236, 236, 236, 236, 236, 236, 237, 237, 237, 237, 237, 237, 237, 237, 237, 237, 237, 237, 237, 237, 237, 237, 237, 237, 238, 238, 238, 238, 238, 238, 238, 238, 238, 238, 238, 238, 238, 238, 238, 238, 238, 238, 239, 239, 239, 239, 239, 239, 239, 239, 239, 239, 239, 239, 239, 239, 239, 239, 239, 239, 239, 240, 240, 240, 240, 240, 240, 240, 240, 240, 240, 240, 240, 240, 240, 240, 240, 240, 240, 241, 241, 241, 241, 241, 241, 241, 241, 241, 241, 241, 241, 241, 241, 241, 241, 241, 241, 241, 242, 242, 242, 242, 242, 242, 242, 242, 242, 242, 242, 242, 242, 242, 242, 242, 242, 242, 242, 243, 243, 243, 243, 243, 243, 243, 243, 243, 243, 243, 243, 243, 243, 243, 243, 243, 243, 243, 244, 244, 244, 244, 244, 244, 244, 244, 244, 244, 244, 244, 244, 244, 244, 244, 244, 244, 244, 245, 245, 245, 245, 245, 245, 245, 245, 245, 245, 245, 245, 245, 245, 245, 245, 245, 245, 245, 245, 246, 246, 246, 246, 246, 246, 246, 246, 246, 246, 246, 246, 246, 246, 246, 246, 246, 246, 246, 247, 247, 247, 247, 247, 247, 247, 247, 247, 247, 247, 247, 247, 247, 247, 247, 247, 247, 247, 248, 248, 248, 248, 248, 248, 248, 248, 248, 248, 248, 248, 248, 248, 248, 248, 248, 248, 248, 248, 249, 249, 249, 249, 249, 249, 249, 249, 249, 249, 249, 249, 249, 249, 249, 249, 249, 249, 249, 249, 250, 250, 250, 250, 250, 250, 250, 250, 250, 250, 250, 250, 250, 250, 250, 250, 250, 250, 250, 250, 251, 251, 251, 251, 251, 251, 251, 251, 251, 251, 251, 251, 251, 251, 251, 251, 251, 251, 251, 251, 252, 252, 252, 252, 252, 252, 252, 252, 252, 252, 252, 252, 252, 252, 252, 252, 252, 252, 252, 252, 253, 253, 253, 253, 253, 253, 253, 253, 253, 253, 253, 253, 253, 253, 253, 253, 253, 253, 253, 253, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255 };
__global__ __launch_bounds__(256) void k_bgr2labl(const uint8_t *__restrict__ bgr, size_t npx, uint8_t *__restrict__ L)
{
    __shared__ uint16_t s_g[256];
    __shared__ uint8_t s_ly[2048];
    s_g[threadIdx.x] = c_gamma[threadIdx.x];
    for (int i = threadIdx.x; i < 2041; i += 256) s_ly[i] = c_ly[i];
    __syncthreads();
    for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < npx; p += (size_t)gridDim.x * 256) {
        const int B = s_g[bgr[3 * p]], G = s_g[bgr[3 * p + 1]], R = s_g[bgr[3 * p + 2]];
        L[p] = s_ly[(R * 871 + G * 2929 + B * 296 + (1 << 11)) >> 12];
    }
}
__global__ __launch_bounds__(256) void k_bgr2gray(const uint8_t *__restrict__ bgr, size_t npx, uint8_t *__restrict__ gray);
__global__ __launch_bounds__(256) void k_bgr2gray_any(const uint8_t *__restrict__ bgr, size_t npx, uint8_t *__restrict__ gray,
                                                      uint8_t *__restrict__ any);
} }

// the call behind both entry points: grey frames (bgr == null) or true-colour frames (gray == null; the grey plane and the
// L plane are made in the workspace first)
static int32_t detect_impl(const uint8_t *gray, const uint8_t *bgr, int32_t n, int32_t h, int32_t w, const CpeDetectParams *params,
                           void *ws, size_t ws_bytes, double *xy, int32_t *id, int32_t *n_pts,
                           double *center, int32_t *status, void *stream)
{
    CpeDetectParams prm = {0, 7, 1.0, CPE_TARGET_CYLINDER, 0};
    if (params) prm = *params;
    CPE_CHECK_ARG(prm.subpixel == 0 || (prm.subpixel_window >= 1 && prm.subpixel_window <= 13 && prm.subpixel_step > 0),
                  "cpe_detect_grid_batch_ex: bad sub-pixel parameters");
    CPE_CHECK_ARG(prm.target == CPE_TARGET_CYLINDER || prm.target == CPE_TARGET_PLANE, "cpe_detect_grid_batch_ex: unknown target %d", prm.target);
    CPE_CHECK_ARG(!(prm.target == CPE_TARGET_PLANE && prm.subpixel), "cpe_detect_grid_batch_ex: no sub-pixel refinement for the planar target");
    CPE_CHECK_ARG((prm.flags & ~CPE_DETECT_SKIP_DEBUG_PLANES) == 0, "cpe_detect_grid_batch_ex: unknown flags 0x%x", (unsigned)prm.flags);
    const int planar = prm.target == CPE_TARGET_PLANE ? 1 : 0;
    CPE_CHECK_ARG((gray || bgr) && xy && id && n_pts && center && status, "cpe_detect_grid_batch: null pointer");
    CPE_CHECK_ARG(!(bgr && prm.subpixel), "cpe_detect_grid_bgr_batch_ex: colour frames: no sub-pixel refinement");
    CPE_CHECK_ARG(n >= 0 && h >= 64 && w >= 64 && h <= MAX_DIM && w <= MAX_DIM,
                  "cpe_detect_grid_batch: need n>=0 and 64 <= h,w <= 4096 (got %d,%d,%d)", n, h, w);
    if (n == 0) return CPE_OK;
    Workspace W;
    if (int32_t rc = W.open(ws, ws_bytes, n, h, w, "cpe_detect_grid_batch", CPE_ERR_WORKSPACE)) return rc;
    hipStream_t s = (hipStream_t)stream;
    FrameState *st = W.state();
    // colour input: the grey plane lives in the workspace; the L plane borrows the disc plane of the region stage, which is
    // first written (cleared) after CLAHE has read L.  The planar target reads no L plane: its region stage thresholds the
    // any-channel plane instead (get_convex_hull of util_plane.py), kept in the CLAHE plane, which that target never uses.
    uint8_t *lplane = bgr && !planar ? W.at<uint8_t>(WS_DISCS) : nullptr;
    uint8_t *anyplane = bgr && planar ? W.at<uint8_t>(WS_CLAHE) : nullptr;
    uint8_t *const grayin = W.at<uint8_t>(WS_GRAYIN), *const g7 = W.at<uint8_t>(WS_BLUR7);
    if (bgr) gray = grayin;
    RegionBuffers R = region_buffers(W, h, w);
    MaskBuffers M = mask_buffers(W, R);
    M.skip_debug = (prm.flags & CPE_DETECT_SKIP_DEBUG_PLANES) != 0;
    // three chains that only meet in masks_stage: ridge mask -> line masks -> joints (stream 1), saturated spot
    // (stream 2), region (the caller's stream).  The side chains are mostly ALU / latency bound and fill the CUs the
    // region stage's serial kernels leave idle.  The helper streams and their events are per device and shared by all
    // callers: the enqueue below (fork .. join, host side only, microseconds per kernel) runs under the device's mutex,
    // so two host threads never interleave their forks and joins.
    SideStreams &X = side_streams(s);
    std::unique_lock<std::mutex> lk(X.mu, std::defer_lock);
    if (X.ok) lk.lock();
    bool forked = false;
    auto enqueue = [&]() -> int {
        int rc;
        CPE_LAUNCH_BEGIN();
        CPE_KLAUNCH(k_state_init, dim3((n + 63) / 64), dim3(64), 0, s, st, n, R.best, M.best_s, R.nrect);
        CPE_CHECK_LAUNCH("k_state_init");
        if (bgr && planar) {   // BGR2GRAY and the any-channel threshold of get_convex_hull, from one read of the frame
            const size_t npx = (size_t)n * h * w;
            CPE_KLAUNCH(k_bgr2gray_any, dim3((unsigned)(((npx + 3) / 4 + 255) / 256)), dim3(256), 0, s, bgr, npx, grayin, anyplane);
            CPE_CHECK_LAUNCH("colour planes");
        } else if (bgr) {      // BGR2GRAY (load_and_preprocess_image, mask_roi_around_center) and the L channel of BGR2LAB (detect_largest_blob)
            const size_t npx = (size_t)n * h * w;
            CPE_KLAUNCH(k_bgr2gray, dim3((unsigned)(((npx + 3) / 4 + 255) / 256)), dim3(256), 0, s, bgr, npx, grayin);
            CPE_KLAUNCH(k_bgr2labl, dim3((unsigned)std::min<size_t>((npx + 255) / 256, 1 << 16)), dim3(256), 0, s, bgr, npx, lplane);
            CPE_CHECK_LAUNCH("colour planes");
        }
        if (X.ok) {
            CPE_CHECK_HIP(hipEventRecord(X.fork, s));
            CPE_CHECK_HIP(hipStreamWaitEvent(X.s1, X.fork, 0));
            CPE_CHECK_HIP(hipStreamWaitEvent(X.s2, X.fork, 0));
            forked = true;
        }
        hipStream_t s1 = X.ok ? X.s1 : s, s2 = X.ok ? X.s2 : s;
        if ((rc = cpe_preprocess_batch(gray, n, h, w, M.binary, (void *)s1)) != CPE_OK) return rc;
        if ((rc = joints_mask_stage(n, h, w, M, st, s1)) != CPE_OK) return rc;
        if ((rc = spot_stage(gray, n, h, w, M, st, s2, planar)) != CPE_OK) return rc;
        if (X.ok) {   // ends of the joints and the spot chain (nothing more is enqueued on s1 / s2 before the join below)
            CPE_CHECK_HIP(hipEventRecord(X.join1, X.s1));
            CPE_CHECK_HIP(hipEventRecord(X.join2, X.s2));
        }
        RegionSide rside = {X.s3, X.e3a, X.e3b, X.e3c, X.e3d, X.join1, X.join2};
        if (planar) { if ((rc = region_stage_plane(bgr ? anyplane : gray, n, h, w, R, st, s)) != CPE_OK) return rc; }
        else if ((rc = region_stage(gray, n, h, w, 4.5, R, st, s, X.ok ? &rside : nullptr, lplane, nullptr)) != CPE_OK) return rc;
        if (X.ok) {
            CPE_CHECK_HIP(hipStreamWaitEvent(s, X.join1, 0));
            CPE_CHECK_HIP(hipStreamWaitEvent(s, X.join2, 0));
            forked = false;
        }
        M.lab_h = W.at<int>(WS_LABELS); M.lab_v = W.at<int>(WS_LABELS_AUX);
        // the 7x7 blur of the indexing step only needs the region rectangle, and only the lines kernel reads the joints: both
        // run on the (now idle) spot stream beside the fragment chains of the masks stage
        if (X.ok) {
            CPE_CHECK_HIP(hipEventRecord(X.fork, s));
            CPE_CHECK_HIP(hipStreamWaitEvent(X.s2, X.fork, 0));
            forked = true;
            if ((rc = bgr ? blur7_bgr(bgr, n, h, w, st, g7, X.s2) : blur7_u8(gray, n, h, w, st, g7, X.s2)) != CPE_OK) return rc;
        }
        if ((rc = masks_stage(gray, n, h, w, M, st, s, X.ok ? &rside : nullptr, planar, X.ok ? X.s2 : s)) != CPE_OK) return rc;   // joints: on s2 too
        if (X.ok) {
            CPE_CHECK_HIP(hipEventRecord(X.join2, X.s2));
            CPE_CHECK_HIP(hipStreamWaitEvent(s, X.join2, 0));
            forked = false;
        }
        else if ((rc = bgr ? blur7_bgr(bgr, n, h, w, st, g7, s) : blur7_u8(gray, n, h, w, st, g7, s)) != CPE_OK) return rc;
        if ((rc = lines_stage(M.lab_h, M.lab_v, M.exp_h, M.exp_v, g7, n, h, w, M.joints, st, W.at<void>(WS_LINES), xy, id,
                              n_pts, center, gray, prm.subpixel, prm.subpixel_window, prm.subpixel_step, W.at<float>(WS_SUBPIX),
                              std::max(h, w) + 128, s, planar)) != CPE_OK)
            return rc;
        CPE_LAUNCH_BEGIN();
        CPE_KLAUNCH(k_finish, dim3((n + 63) / 64), dim3(64), 0, s, st, n, status, n_pts);
        CPE_CHECK_LAUNCH("k_finish");
        return CPE_OK;
    };
    const int rc = enqueue();
    if (X.ok && (forked || rc != CPE_OK)) {
        // an error between fork and join: whatever already runs on the helper streams still uses the caller's buffers,
        // so the caller's stream is made to wait for all of them before the error is reported
        hipStream_t hs[3] = {X.s1, X.s2, X.s3};
        hipEvent_t he[3] = {X.join1, X.join2, X.e3a};
        for (int k = 0; k < 3; k++)
            if (hipEventRecord(he[k], hs[k]) == hipSuccess) (void)hipStreamWaitEvent(s, he[k], 0);
        (void)hipGetLastError();
    }
    return rc;
}

extern "C" int32_t cpe_detect_grid_batch_ex(const uint8_t *gray, int32_t n, int32_t h, int32_t w, const CpeDetectParams *params,
                                            void *ws, size_t ws_bytes, double *xy, int32_t *id, int32_t *n_pts,
                                            double *center, int32_t *status, void *stream)
{
    CPE_CHECK_ARG(gray, "cpe_detect_grid_batch: null pointer");
    return detect_impl(gray, nullptr, n, h, w, params, ws, ws_bytes, xy, id, n_pts, center, status, stream);
}

extern "C" int32_t cpe_detect_grid_bgr_batch_ex(const uint8_t *bgr, int32_t n, int32_t h, int32_t w, const CpeDetectParams *params,
                                                void *ws, size_t ws_bytes, double *xy, int32_t *id, int32_t *n_pts,
                                                double *center, int32_t *status, void *stream)
{
    CPE_CHECK_ARG(bgr && (((uintptr_t)bgr) & 3) == 0, "cpe_detect_grid_bgr_batch_ex: bgr must be a 4-byte aligned device pointer");
    return detect_impl(nullptr, bgr, n, h, w, params, ws, ws_bytes, xy, id, n_pts, center, status, stream);
}

extern "C" int32_t cpe_detect_line_tables(const void *ws, size_t ws_bytes, int32_t n, int32_t h, int32_t w, int32_t frame,
                                          double *eq, int32_t *npts, double *pts, int32_t *n_lines, void *stream)
{
    CPE_CHECK_ARG(ws && eq && npts && pts && n_lines && n > 0 && frame >= 0 && frame < n && h >= 64 && w >= 64,
                  "cpe_detect_line_tables: bad argument");
    static_assert(CPE_MAXL == MAXL, "cpe.h and cpe_dev.h disagree on the line capacity");
    Workspace W;
    if (int32_t rc = W.open(ws, ws_bytes, n, h, w, "cpe_detect_line_tables")) return rc;
    return lines_export(W.at<const uint8_t>(WS_LINES), frame, eq, npts, pts, n_lines, (hipStream_t)stream);
}

extern "C" int32_t cpe_detect_results_sizes(const void *ws, size_t ws_bytes, int32_t n, int32_t h, int32_t w, const int32_t *n_pts,
                                            const int32_t *status, int64_t *offsets, void *stream)
{
    CPE_CHECK_ARG(ws && n_pts && status && offsets && n > 0 && h >= 64 && w >= 64 && ((uintptr_t)n_pts & 3) == 0 &&
                  ((uintptr_t)status & 3) == 0 && ((uintptr_t)offsets & 7) == 0, "cpe_detect_results_sizes: bad argument");
    Workspace W;
    if (int32_t rc = W.open(ws, ws_bytes, n, h, w, "cpe_detect_results_sizes")) return rc;
    static_assert(sizeof(long long) == sizeof(int64_t), "offsets are 64-bit");
    return results_sizes(W.at<const uint8_t>(WS_LINES), n, n_pts, (long long *)offsets, (hipStream_t)stream);
}

extern "C" int32_t cpe_detect_results_pack(const void *ws, size_t ws_bytes, int32_t n, int32_t h, int32_t w, const double *xy,
                                           const int32_t *id, const int32_t *n_pts, const double *center, const int32_t *status,
                                           const int64_t *offsets, void *payload, size_t payload_bytes, void *stream)
{
    CPE_CHECK_ARG(ws && xy && id && n_pts && center && status && offsets && payload && n > 0 && h >= 64 && w >= 64,
                  "cpe_detect_results_pack: bad argument");
    CPE_CHECK_ARG((((uintptr_t)xy | (uintptr_t)id | (uintptr_t)center | (uintptr_t)offsets | (uintptr_t)payload) & 7) == 0 &&
                  (((uintptr_t)n_pts | (uintptr_t)status) & 3) == 0, "cpe_detect_results_pack: a buffer is not aligned (8 bytes; n_pts, status: 4)");
    Workspace W;
    if (int32_t rc = W.open(ws, ws_bytes, n, h, w, "cpe_detect_results_pack")) return rc;
    return results_pack(W.at<const uint8_t>(WS_LINES), n, xy, id, n_pts, center, status, (const long long *)offsets, payload,
                        payload_bytes, (hipStream_t)stream);
}

// BGR2GRAY of the entry point for colour input (load_and_preprocess_image, util_cylinder.py:1781-1789)
namespace cpe { namespace {
__global__ __launch_bounds__(256) void k_bgr2gray(const uint8_t *__restrict__ bgr, size_t npx, uint8_t *__restrict__ gray)
{
    // 4 pixels (12 bytes in, 1 dword out) per thread; cv2.cvtColor 8-bit: (B*3735 + G*19235 + R*9798 + 2^14) >> 15
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t p0 = q * 4;
    if (p0 >= npx) return;
    if (p0 + 4 <= npx) {
        const uint32_t *src = (const uint32_t *)(bgr + p0 * 3);     // p0 * 3 is a multiple of 12
        const uint32_t a = src[0], b = src[1], c = src[2];
        const uint32_t px[4][3] = {{a & 255, (a >> 8) & 255, (a >> 16) & 255}, {a >> 24, b & 255, (b >> 8) & 255},
                                   {(b >> 16) & 255, b >> 24, c & 255}, {(c >> 8) & 255, (c >> 16) & 255, c >> 24}};
        uint32_t out = 0;
        for (int k = 0; k < 4; k++) out |= ((px[k][0] * 3735u + px[k][1] * 19235u + px[k][2] * 9798u + 16384u) >> 15) << (8 * k);
        *(uint32_t *)(gray + p0) = out;
    } else {
        for (size_t p = p0; p < npx; p++)
            gray[p] = (uint8_t)((bgr[3 * p] * 3735u + bgr[3 * p + 1] * 19235u + bgr[3 * p + 2] * 9798u + 16384u) >> 15);
    }
}
} }

// the planar target's colour frames: BGR2GRAY as k_bgr2gray, and beside it the mask get_convex_hull thresholds
// (util_plane.py:2590-2689): cv2.threshold(img, 127, 255, THRESH_BINARY) per channel, then BGR2GRAY of that 0/255 image,
// which is non-zero exactly where some channel is above 127 -- written as 0 / 255 (the region stage thresholds it at 127)
namespace cpe { namespace {
__global__ __launch_bounds__(256) void k_bgr2gray_any(const uint8_t *__restrict__ bgr, size_t npx, uint8_t *__restrict__ gray,
                                                      uint8_t *__restrict__ any)
{
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t p0 = q * 4;
    if (p0 >= npx) return;
    if (p0 + 4 <= npx) {
        const uint32_t *src = (const uint32_t *)(bgr + p0 * 3);     // p0 * 3 is a multiple of 12
        const uint32_t a = src[0], b = src[1], c = src[2];
        const uint32_t px[4][3] = {{a & 255, (a >> 8) & 255, (a >> 16) & 255}, {a >> 24, b & 255, (b >> 8) & 255},
                                   {(b >> 16) & 255, b >> 24, c & 255}, {(c >> 8) & 255, (c >> 16) & 255, c >> 24}};
        uint32_t out = 0, m = 0;
        for (int k = 0; k < 4; k++) {
            out |= ((px[k][0] * 3735u + px[k][1] * 19235u + px[k][2] * 9798u + 16384u) >> 15) << (8 * k);
            if (max(px[k][0], max(px[k][1], px[k][2])) > 127u) m |= 255u << (8 * k);
        }
        *(uint32_t *)(gray + p0) = out;
        *(uint32_t *)(any + p0) = m;
    } else {
        for (size_t p = p0; p < npx; p++) {
            const uint32_t B = bgr[3 * p], G = bgr[3 * p + 1], R = bgr[3 * p + 2];
            gray[p] = (uint8_t)((B * 3735u + G * 19235u + R * 9798u + 16384u) >> 15);
            any[p] = max(B, max(G, R)) > 127u ? 255 : 0;
        }
    }
}
} }

extern "C" int32_t cpe_bgr2gray_batch(const uint8_t *bgr, int32_t n, int32_t h, int32_t w, uint8_t *gray, void *stream)
{
    CPE_CHECK_ARG(bgr && gray && n >= 0 && h > 0 && w > 0, "cpe_bgr2gray_batch: bad argument");
    CPE_CHECK_ARG(((uintptr_t)bgr & 3) == 0 && ((uintptr_t)gray & 3) == 0, "cpe_bgr2gray_batch: buffers must be 4-byte aligned");
    if (n == 0) return CPE_OK;
    const size_t npx = (size_t)n * h * w;
    const size_t quads = (npx + 3) / 4;
    CPE_LAUNCH_BEGIN();
    CPE_KLAUNCH(k_bgr2gray, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, bgr, npx, gray);
    CPE_CHECK_LAUNCH("k_bgr2gray");
    return CPE_OK;
}

// cv2.findContours(mask, RETR_EXTERNAL, .) reduced to what its callers keep of the hierarchy: the raster-first pixels of the
// components that do NOT lie inside a hole of another component (tests of the RETR_EXTERNAL rule, util_cylinder.py:161,1817)
namespace cpe { namespace {
__global__ __launch_bounds__(256) void k_list_external(const int *__restrict__ roots, const FrameState *__restrict__ st, int w,
                                                       const unsigned long long *__restrict__ outside, size_t plane_words,
                                                       int *__restrict__ first_px, int cap, int *__restrict__ count)
{
    const int f = blockIdx.y;
    const int ncomp = min(st[f].n_roots, MAXROOTS);
    for (int k = blockIdx.x * 256 + threadIdx.x; k < ncomp; k += gridDim.x * 256) {
        const int root = roots[(size_t)f * MAXROOTS + k];
        if (!comp_is_external(outside + f * plane_words, w, root, 0)) continue;
        const int q = atomicAdd(&count[f], 1);
        if (q < cap) first_px[(size_t)f * cap + q] = root;
    }
}
} }

extern "C" int32_t cpe_debug_external_components(const uint8_t *mask, int32_t n, int32_t h, int32_t w, void *ws, size_t ws_bytes,
                                                 int32_t *first_px, int32_t cap, int32_t *count, void *stream)
{
    CPE_CHECK_ARG(mask && ws && first_px && count && n > 0 && h >= 64 && w >= 64 && w <= MAX_DIM && cap > 0, "cpe_debug_external_components: bad argument");
    Workspace W;
    if (int32_t rc = W.open(ws, ws_bytes, n, h, w, "cpe_debug_external_components")) return rc;
    hipStream_t s = (hipStream_t)stream;
    FrameState *st = W.state();
    int *roots = W.at<int>(WS_ROOTS);
    int rc;
    CPE_LAUNCH_BEGIN();
    CPE_KLAUNCH(k_state_init, dim3((n + 63) / 64), dim3(64), 0, s, st, n, (unsigned long long *)nullptr, (unsigned long long *)nullptr, (int *)nullptr);
    CPE_CHECK_HIP(hipMemsetAsync(count, 0, (size_t)n * sizeof(int), s));
    if ((rc = ccl_components(mask, nullptr, n, h, w, 0, WIN_FRAME, W.at<int>(WS_LABELS), roots, ROOTS_MAIN, st, s)) != CPE_OK) return rc;
    const size_t fl_words = bit_plane_words(h, w);   // u64 words per frame of a flood plane (>= h * ceil(w / 64))
    unsigned long long *bgw = bit_plane(W.at<uint32_t>(WS_BITS), 0, h, w);
    unsigned long long *out = bit_plane(W.at<uint32_t>(WS_BITS), n, h, w);
    if ((rc = outside_flood(mask, n, h, w, st, WIN_FRAME, bgw, out, fl_words, s, nullptr)) != CPE_OK) return rc;
    CPE_KLAUNCH(k_list_external, dim3(32, n), dim3(256), 0, s, (const int *)roots, (const FrameState *)st, w, (const unsigned long long *)out, fl_words,
                first_px, cap, count);
    CPE_CHECK_LAUNCH("k_list_external");
    return CPE_OK;
}

// Stand-alone labelling pass over the workspace's label planes (profiling / tests): labels of
// {(img > thr) != invert} land in the CPE_PLANE_LABELS plane.
extern "C" int32_t cpe_debug_ccl(const uint8_t *img, int32_t n, int32_t h, int32_t w, int32_t thr, int32_t invert,
                                 int32_t conn8, int32_t count_mode, int32_t want_bbox, int32_t want_roots, void *ws,
                                 size_t ws_bytes, void *stream)
{
    CPE_CHECK_ARG(img && ws && n > 0 && h >= 64 && w >= 64, "cpe_debug_ccl: bad argument");
    Workspace W;
    if (int32_t rc = W.open(ws, ws_bytes, n, h, w, "cpe_debug_ccl")) return rc;
    hipStream_t s = (hipStream_t)stream;
    FrameState *st = W.state();
    CclPass p;
    p.thr = thr; p.invert = invert; p.conn8 = conn8; p.win = (want_bbox >> 1) & 1 ? WIN_SWEEP : WIN_FRAME;
    p.count = (CclCount)count_mode; p.cnt = W.at<int>(WS_LABELS_AUX);
    p.touch = invert ? W.at<uint8_t>(WS_TOUCH) : nullptr;   // the background sets: holes only
    p.roots = want_roots ? W.at<int>(WS_ROOTS) : nullptr;
    p.nrect = (want_bbox & 1) ? W.at<int>(WS_NRECT) : nullptr;
    return ccl_label(img, n, h, w, W.at<int>(WS_LABELS), p, st, s);
}

namespace cpe { namespace {
__global__ void k_debug_rect(FrameState *st, int n, const int *rect)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f < n) for (int k = 0; k < 4; k++) st[f].crect[k] = rect[4 * f + k];
}
__global__ void k_debug_n_roots(const FrameState *st, int n, int *n_roots)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f < n) n_roots[f] = st[f].n_roots;
}
} }

// The first labelling of the blob sweep's dark forest on a given image (tests): the set img <= thr inside rect (i32[n,4] x0, y0,
// x1, y1), with the sweep's pre-linked runs outside it.  path 0: the general pass (ccl_label); 1: the passes the region stage
// runs (ccl_dark_first, reading the one-bit plane of img > thr).  Labels and counts (-1 where not written) go to
// lab / cnt i32[n,h,w], the root list to roots i32[n,CPE_MAXROOTS_DEBUG] and its length to n_roots i32[n].
static_assert(CPE_MAXROOTS_DEBUG == cpe::MAXROOTS, "cpe.h and cpe_dev.h disagree on the root-list capacity");
extern "C" int32_t cpe_debug_dark_labels(const uint8_t *img, int32_t n, int32_t h, int32_t w, int32_t thr, const int32_t *rect,
                                         int32_t path, void *ws, size_t ws_bytes, int32_t *lab, int32_t *cnt, int32_t *roots,
                                         int32_t *n_roots, void *stream)
{
    CPE_CHECK_ARG(img && rect && ws && lab && cnt && roots && n_roots && n > 0 && h >= 64 && w >= 64 && (path == 0 || path == 1) &&
                  thr >= 0 && thr + 160 <= 255,
                  "cpe_debug_dark_labels: bad argument");
    Workspace W;
    if (int32_t rc = W.open(ws, ws_bytes, n, h, w, "cpe_debug_dark_labels")) return rc;
    hipStream_t s = (hipStream_t)stream;
    FrameState *st = W.state();
    int *lb = W.at<int>(WS_LABELS), *cb = W.at<int>(WS_LABELS_AUX), *rb = W.at<int>(WS_ROOTS);
    uint32_t *bits = W.at<uint32_t>(WS_BITS);
    const size_t N = (size_t)h * w;
    CPE_LAUNCH_BEGIN();
    CPE_KLAUNCH(k_state_init, dim3((n + 63) / 64), dim3(64), 0, s, st, n, (unsigned long long *)nullptr, (unsigned long long *)nullptr, (int *)nullptr);
    CPE_KLAUNCH(k_debug_rect, dim3((n + 63) / 64), dim3(64), 0, s, st, n, (const int *)rect);
    (void)hipMemsetAsync(lb, 0xff, N * n * sizeof(int), s);
    (void)hipMemsetAsync(cb, 0xff, N * n * sizeof(int), s);
    CPE_CHECK_LAUNCH("cpe_debug_dark_labels");
    int rc;
    if (path == 0) {
        CclPass p;
        p.thr = thr; p.invert = 1; p.conn8 = 0; p.win = WIN_SWEEP; p.outside = OUTSIDE_SWEEP_RUNS;
        p.count = COUNT_ALL; p.cnt = cb; p.roots = rb;
        rc = ccl_label(img, n, h, w, lb, p, st, s);
    } else if ((rc = build_bitplanes(img, n, h, w, thr, 10, 17, bits, s)) == CPE_OK)   // the stack of planes the region stage keeps
        rc = ccl_dark_first(img, bits, 17, n, h, w, thr, lb, rb, cb, st, s);
    if (rc != CPE_OK) return rc;
    (void)hipMemcpyAsync(lab, lb, N * n * sizeof(int), hipMemcpyDeviceToDevice, s);
    (void)hipMemcpyAsync(cnt, cb, N * n * sizeof(int), hipMemcpyDeviceToDevice, s);
    (void)hipMemcpyAsync(roots, rb, (size_t)n * MAXROOTS * sizeof(int), hipMemcpyDeviceToDevice, s);
    CPE_KLAUNCH(k_debug_n_roots, dim3((n + 63) / 64), dim3(64), 0, s, (const FrameState *)st, n, n_roots);
    CPE_CHECK_LAUNCH("cpe_debug_dark_labels");
    return CPE_OK;
}

// The component list of the set img > thr (tests): ccl_components with the connectivity, the window and the source of the
// set as arguments, so that the word-level passes (k_ccl_init64 / k_ccl_merge64 / k_ccl_roots64) can be driven through
// everything they are written for.  rect (may be null: the whole frame) i32[n,4] x0, y0, x1, y1; bits != 0: the set is read
// from its one-bit plane, built here.  lab i32[n,h,w]: the label plane as the passes leave it (union-find links; -1 where
// they wrote nothing), roots i32[n,CPE_MAXROOTS_DEBUG], n_roots i32[n].
extern "C" int32_t cpe_debug_ccl_tiles(const uint8_t *img, int32_t n, int32_t h, int32_t w, int32_t thr, int32_t conn8,
                                       int32_t bits, const int32_t *rect, void *ws, size_t ws_bytes, int32_t *lab, int32_t *roots,
                                       int32_t *n_roots, void *stream)
{
    CPE_CHECK_ARG(img && ws && lab && roots && n_roots && n > 0 && h >= 1 && w >= 16 && thr >= 0 && thr <= 255,
                  "cpe_debug_ccl_tiles: bad argument");
    Workspace W;
    if (int32_t rc = W.open(ws, ws_bytes, n, h, w, "cpe_debug_ccl_tiles")) return rc;
    hipStream_t s = (hipStream_t)stream;
    FrameState *st = W.state();
    int *lb = W.at<int>(WS_LABELS), *rb = W.at<int>(WS_ROOTS);
    uint32_t *planes = W.at<uint32_t>(WS_BITS);
    const size_t N = (size_t)h * w;
    CPE_LAUNCH_BEGIN();
    CPE_KLAUNCH(k_state_init, dim3((n + 63) / 64), dim3(64), 0, s, st, n, (unsigned long long *)nullptr, (unsigned long long *)nullptr, (int *)nullptr);
    if (rect) CPE_KLAUNCH(k_debug_rect, dim3((n + 63) / 64), dim3(64), 0, s, st, n, (const int *)rect);
    (void)hipMemsetAsync(lb, 0xff, N * n * sizeof(int), s);
    CPE_CHECK_LAUNCH("cpe_debug_ccl_tiles");
    int rc;
    if (bits && (rc = build_bitplanes(img, n, h, w, thr, 0, 1, planes, s)) != CPE_OK) return rc;
    if ((rc = ccl_components_conn(img, bits ? planes : nullptr, n, h, w, thr, conn8 ? 1 : 0, rect ? WIN_SWEEP : WIN_FRAME, lb, rb, ROOTS_MAIN,
                                  st, s)) != CPE_OK) return rc;
    (void)hipMemcpyAsync(lab, lb, N * n * sizeof(int), hipMemcpyDeviceToDevice, s);
    (void)hipMemcpyAsync(roots, rb, (size_t)n * MAXROOTS * sizeof(int), hipMemcpyDeviceToDevice, s);
    CPE_KLAUNCH(k_debug_n_roots, dim3((n + 63) / 64), dim3(64), 0, s, (const FrameState *)st, n, n_roots);
    CPE_CHECK_LAUNCH("cpe_debug_ccl_tiles");
    return CPE_OK;
}

// The region stage of the cylinder target on a given sweep image (tests): region_stage as the product runs it, serially, with
// an identity CLAHE table in place of LAB-L + CLAHE, and its blob records and key points copied out (RegionProbe).
extern "C" int32_t cpe_debug_blob_region(const uint8_t *img, int32_t n, int32_t h, int32_t w, void *ws, size_t ws_bytes,
                                         float *kp, int32_t kp_cap, int32_t *n_kp, double *blobs, int32_t blob_cap,
                                         int32_t *n_blobs, void *stream)
{
    CPE_CHECK_ARG(img && ws && kp && n_kp && blobs && n_blobs && n > 0 && h >= 64 && w >= 64 && h <= MAX_DIM && w <= MAX_DIM &&
                  kp_cap > 0 && blob_cap > 0, "cpe_debug_blob_region: bad argument");
    Workspace W;
    if (int32_t rc = W.open(ws, ws_bytes, n, h, w, "cpe_debug_blob_region")) return rc;
    hipStream_t s = (hipStream_t)stream;
    FrameState *st = W.state();
    RegionBuffers R = region_buffers(W, h, w);
    RegionProbe probe = {1, blobs, blob_cap, n_blobs, kp, kp_cap, n_kp};
    CPE_LAUNCH_BEGIN();
    CPE_KLAUNCH(k_state_init, dim3((n + 63) / 64), dim3(64), 0, s, st, n, R.best, W.at<unsigned long long>(WS_BEST_SPOT), R.nrect);
    CPE_CHECK_LAUNCH("k_state_init");
    return region_stage(img, n, h, w, 4.5, R, st, s, nullptr, nullptr, &probe);
}

// LAB-L + CLAHE of grey frames and the 17 threshold planes, as the region stage makes them (tests)
extern "C" int32_t cpe_debug_clahe_planes(const uint8_t *gray, int32_t n, int32_t h, int32_t w, int32_t fused, void *ws, size_t ws_bytes,
                                          uint8_t *cl, uint32_t *planes, int32_t *buckets, int32_t *box, void *stream)
{
    CPE_CHECK_ARG(gray && ws && cl && planes && buckets && box && n > 0 && h >= 64 && w >= 64 && h <= MAX_DIM && w <= MAX_DIM,
                  "cpe_debug_clahe_planes: bad argument");
    Workspace W;
    if (int32_t rc = W.open(ws, ws_bytes, n, h, w, "cpe_debug_clahe_planes")) return rc;
    hipStream_t s = (hipStream_t)stream;
    FrameState *st = W.state();
    RegionBuffers R = region_buffers(W, h, w);
    CPE_LAUNCH_BEGIN();
    CPE_KLAUNCH(k_state_init, dim3((n + 63) / 64), dim3(64), 0, s, st, n, R.best, W.at<unsigned long long>(WS_BEST_SPOT), R.nrect);
    CPE_CHECK_LAUNCH("k_state_init");
    return clahe_front_probe(gray, n, h, w, fused, 1, R, s, cl, planes, buckets, box);
}

// The same for true-colour frames: the L plane as detect_impl makes it (k_bgr2labl into the disc plane), then CLAHE without
// the grey LAB-L table (tests)
extern "C" int32_t cpe_debug_clahe_planes_bgr(const uint8_t *bgr, int32_t n, int32_t h, int32_t w, int32_t fused, void *ws,
                                              size_t ws_bytes, uint8_t *L, uint8_t *cl, uint32_t *planes, int32_t *buckets,
                                              int32_t *box, void *stream)
{
    CPE_CHECK_ARG(bgr && ws && L && cl && planes && buckets && box && n > 0 && h >= 64 && w >= 64 && h <= MAX_DIM && w <= MAX_DIM,
                  "cpe_debug_clahe_planes_bgr: bad argument");
    Workspace W;
    if (int32_t rc = W.open(ws, ws_bytes, n, h, w, "cpe_debug_clahe_planes_bgr")) return rc;
    hipStream_t s = (hipStream_t)stream;
    FrameState *st = W.state();
    RegionBuffers R = region_buffers(W, h, w);
    uint8_t *lplane = W.at<uint8_t>(WS_DISCS);
    const size_t npx = (size_t)n * h * w;
    CPE_LAUNCH_BEGIN();
    CPE_KLAUNCH(k_state_init, dim3((n + 63) / 64), dim3(64), 0, s, st, n, R.best, W.at<unsigned long long>(WS_BEST_SPOT), R.nrect);
    CPE_KLAUNCH(k_bgr2labl, dim3((unsigned)std::min<size_t>((npx + 255) / 256, 1 << 16)), dim3(256), 0, s, bgr, npx, lplane);
    CPE_CHECK_LAUNCH("cpe_debug_clahe_planes_bgr");
    (void)hipMemcpyAsync(L, lplane, npx, hipMemcpyDeviceToDevice, s);
    return clahe_front_probe(lplane, n, h, w, fused, 0, R, s, cl, planes, buckets, box);
}

// The hull stage on a given image (tests): largest external contour -> convex hull -> filled polygon -> boundingRect, through
// region_hull as the product calls it.  mode 0: the cylinder target's tail, img a disc-union image (non-zero = set) -- what
// region_stage does once its discs are drawn, the one-component shortcut included; mode 1: region_stage_plane on grey frames.
extern "C" int32_t cpe_debug_region_hull(const uint8_t *img, int32_t n, int32_t h, int32_t w, int32_t mode, void *ws, size_t ws_bytes,
                                         void *stream)
{
    CPE_CHECK_ARG(img && ws && n > 0 && h >= 64 && w >= 64 && h <= MAX_DIM && w <= MAX_DIM && (mode == 0 || mode == 1),
                  "cpe_debug_region_hull: bad argument");
    Workspace W;
    if (int32_t rc = W.open(ws, ws_bytes, n, h, w, "cpe_debug_region_hull")) return rc;
    hipStream_t s = (hipStream_t)stream;
    FrameState *st = W.state();
    RegionBuffers R = region_buffers(W, h, w);
    int rc;
    CPE_LAUNCH_BEGIN();
    CPE_KLAUNCH(k_state_init, dim3((n + 63) / 64), dim3(64), 0, s, st, n, R.best, W.at<unsigned long long>(WS_BEST_SPOT), R.nrect);
    CPE_CHECK_LAUNCH("k_state_init");
    if (mode == 1) return region_stage_plane(img, n, h, w, R, st, s);
    CPE_CHECK_HIP(hipMemsetAsync(R.mc, 0, (size_t)n * h * w, s));
    // the union's one-bit plane, which the product draws directly (k_disc_bands) or builds from its byte image; the labelling
    // reads the plane where ccl_components_reads_bits holds and the caller's bytes elsewhere
    if ((rc = build_bitplanes(img, n, h, w, 0, 0, 1, R.bits, s)) != CPE_OK) return rc;
    return region_hull(img, n, h, w, 0, true, 1, R.mc, R, st, s);
}

namespace cpe { namespace {
// the region stage's verdict as the caller gives it: what masks_stage reads of that stage besides mask_contour
__global__ void k_debug_region(FrameState *st, int n, const int *rect, const int *status)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n) return;
    for (int k = 0; k < 4; k++) st[f].rect[k] = rect[4 * f + k];
    st[f].status = status[f];
}
} }

// The masks stage on given inputs (tests): what detect_impl runs between the pre-process and the lines stage, in the same
// order, serially on `stream`, with binary, mask_contour, rect and the region status taken from the caller.
extern "C" int32_t cpe_debug_masks(const uint8_t *binary, const uint8_t *gray, const uint8_t *mask_contour, const int32_t *rect,
                                   const int32_t *region_status, int32_t n, int32_t h, int32_t w, int32_t target, void *ws,
                                   size_t ws_bytes, void *stream)
{
    CPE_CHECK_ARG(binary && gray && mask_contour && rect && region_status && ws && n > 0 && h >= 64 && w >= 64 && h <= MAX_DIM &&
                  w <= MAX_DIM && (target == CPE_TARGET_CYLINDER || target == CPE_TARGET_PLANE), "cpe_debug_masks: bad argument");
    Workspace W;
    if (int32_t rc = W.open(ws, ws_bytes, n, h, w, "cpe_debug_masks")) return rc;
    const int planar = target == CPE_TARGET_PLANE ? 1 : 0;
    hipStream_t s = (hipStream_t)stream;
    FrameState *st = W.state();
    RegionBuffers R = region_buffers(W, h, w);
    MaskBuffers M = mask_buffers(W, R);
    const size_t total = (size_t)n * h * w;
    int rc;
    CPE_LAUNCH_BEGIN();
    CPE_KLAUNCH(k_state_init, dim3((n + 63) / 64), dim3(64), 0, s, st, n, R.best, M.best_s, R.nrect);
    CPE_CHECK_HIP(hipMemcpyAsync(M.binary, binary, total, hipMemcpyDeviceToDevice, s));
    CPE_CHECK_HIP(hipMemcpyAsync(R.mc, mask_contour, total, hipMemcpyDeviceToDevice, s));
    CPE_KLAUNCH(k_debug_region, dim3((n + 63) / 64), dim3(64), 0, s, st, n, (const int *)rect, (const int *)region_status);
    CPE_CHECK_LAUNCH("cpe_debug_masks");
    if ((rc = joints_mask_stage(n, h, w, M, st, s)) != CPE_OK) return rc;
    if ((rc = spot_stage(gray, n, h, w, M, st, s, planar)) != CPE_OK) return rc;
    M.lab_h = W.at<int>(WS_LABELS); M.lab_v = W.at<int>(WS_LABELS_AUX);
    if ((rc = masks_stage(gray, n, h, w, M, st, s, nullptr, planar, s)) != CPE_OK) return rc;
    return blur7_u8(gray, n, h, w, st, W.at<uint8_t>(WS_BLUR7), s);
}

namespace cpe { namespace {
// what the lines stage reads of the stages in front of it, as the caller gives it
__global__ void k_debug_lines_state(FrameState *st, int n, const int *rect, const int *r0, const int *n_joints, const int *status)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n) return;
    for (int k = 0; k < 4; k++) st[f].rect[k] = rect[4 * f + k];
    st[f].r0 = r0[f];
    st[f].n_joints = min(max(n_joints[f], 0), MAXJ);
    st[f].status = status[f];
}
// every pixel its own root: a mask pixel outside the labelling window (the product's masks have none, a caller's may) then
// resolves to itself in k_lines instead of following whatever the plane held
__global__ __launch_bounds__(256) void k_debug_singletons(int *__restrict__ lab_h, int *__restrict__ lab_v, size_t N, size_t total)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int v = (int)(i % N);
        lab_h[i] = v; lab_v[i] = v;
    }
}
} }

// The lines stage on given inputs (tests): the label planes of the expanded masks as masks_stage makes them, then lines_stage
// as detect_impl calls it, serially on `stream`.
extern "C" int32_t cpe_debug_lines(const uint8_t *exp_h, const uint8_t *exp_v, const int32_t *joints, const int32_t *n_joints,
                                   const int32_t *rect, const int32_t *r0, const int32_t *stage_status, const uint8_t *g7,
                                   const uint8_t *gray, int32_t n, int32_t h, int32_t w, const CpeDetectParams *params, void *ws,
                                   size_t ws_bytes, double *xy, int32_t *id, int32_t *n_pts, double *center, int32_t *status,
                                   void *stream)
{
    CpeDetectParams prm = {0, 7, 1.0, CPE_TARGET_CYLINDER, 0};
    if (params) prm = *params;
    CPE_CHECK_ARG(exp_h && exp_v && joints && n_joints && rect && r0 && stage_status && g7 && gray && ws && xy && id && n_pts &&
                  center && status && n > 0 && h >= 64 && w >= 64 && h <= MAX_DIM && w <= MAX_DIM, "cpe_debug_lines: bad argument");
    CPE_CHECK_ARG(prm.subpixel == 0 || (prm.subpixel_window >= 1 && prm.subpixel_window <= 13 && prm.subpixel_step > 0),
                  "cpe_debug_lines: bad sub-pixel parameters");
    CPE_CHECK_ARG((prm.target == CPE_TARGET_CYLINDER || prm.target == CPE_TARGET_PLANE) && prm.flags == 0 &&
                  !(prm.target == CPE_TARGET_PLANE && prm.subpixel), "cpe_debug_lines: bad target, flags, or sub-pixel refinement of the planar target");
    Workspace W;
    if (int32_t rc = W.open(ws, ws_bytes, n, h, w, "cpe_debug_lines")) return rc;
    const int planar = prm.target == CPE_TARGET_PLANE ? 1 : 0;
    hipStream_t s = (hipStream_t)stream;
    FrameState *st = W.state();
    RegionBuffers R = region_buffers(W, h, w);
    MaskBuffers M = mask_buffers(W, R);
    M.lab_h = W.at<int>(WS_LABELS); M.lab_v = W.at<int>(WS_LABELS_AUX);
    uint8_t *const b7 = W.at<uint8_t>(WS_BLUR7);
    const size_t N = (size_t)h * w, total = N * n;
    int rc;
    CPE_LAUNCH_BEGIN();
    CPE_KLAUNCH(k_state_init, dim3((n + 63) / 64), dim3(64), 0, s, st, n, R.best, M.best_s, R.nrect);
    CPE_KLAUNCH(k_debug_lines_state, dim3((n + 63) / 64), dim3(64), 0, s, st, n, (const int *)rect, (const int *)r0, (const int *)n_joints,
                (const int *)stage_status);
    CPE_CHECK_HIP(hipMemcpyAsync(M.exp_h, exp_h, total, hipMemcpyDeviceToDevice, s));
    CPE_CHECK_HIP(hipMemcpyAsync(M.exp_v, exp_v, total, hipMemcpyDeviceToDevice, s));
    CPE_CHECK_HIP(hipMemcpyAsync(b7, g7, total, hipMemcpyDeviceToDevice, s));
    CPE_CHECK_HIP(hipMemcpyAsync(M.joints, joints, (size_t)n * MAXJ * 2 * sizeof(int), hipMemcpyDeviceToDevice, s));
    CPE_KLAUNCH(k_debug_singletons, dim3((unsigned)std::min<size_t>((total + 255) / 256, 1 << 16)), dim3(256), 0, s, M.lab_h, M.lab_v, N, total);
    CPE_CHECK_LAUNCH("cpe_debug_lines");
    if ((rc = ccl_unions(M.exp_h, n, h, w, WIN_REGION, M.lab_h, st, s)) != CPE_OK) return rc;
    if ((rc = ccl_unions(M.exp_v, n, h, w, WIN_REGION, M.lab_v, st, s)) != CPE_OK) return rc;
    if ((rc = lines_stage(M.lab_h, M.lab_v, M.exp_h, M.exp_v, b7, n, h, w, M.joints, st, W.at<void>(WS_LINES), xy, id, n_pts, center,
                          gray, prm.subpixel, prm.subpixel_window, prm.subpixel_step, W.at<float>(WS_SUBPIX), std::max(h, w) + 128, s,
                          planar)) != CPE_OK)
        return rc;
    CPE_LAUNCH_BEGIN();
    CPE_KLAUNCH(k_finish, dim3((n + 63) / 64), dim3(64), 0, s, st, n, status, n_pts);
    CPE_CHECK_LAUNCH("k_finish");
    return CPE_OK;
}
